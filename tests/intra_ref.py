"""Intra sample prediction of one transform block (H.265 8.4.4.2.1 - 8.4.4.2.6) in plain Python / numpy on int64: reference
sample availability and substitution (8.4.4.2.2), the filtering of the reference samples (8.4.4.2.3: the size / mode rule,
[1 2 1], the bilinear filter with its two conditions), planar (8.4.4.2.4), DC (8.4.4.2.5) and the angular modes with the
inverse-angle projection and the edge filters of modes 10 / 26 (8.4.4.2.6).  Written from the standard; it shares nothing
with oracle/oracle_recon.c or the kernels.

predict() takes one decode-order record (residual_ref.Picture.records()) and the reconstruction-stage planes of its picture
and returns the predicted block and a dict of events: which branches the block took.  The availability of the neighbouring
samples comes from the record (its derivation is held by test_avail.py); everything else is computed here.

The reference samples of a block are kept in ONE line of 4 nT + 1 samples in the order of the substitution process: index 0
is p[-1][2 nT - 1] (the lowest sample left of and below the block), index 2 nT is the corner p[-1][-1], index 4 nT is
p[2 nT - 1][-1] (the last sample above and right of it)."""
import numpy as np

import residual_ref as rr

INTRA_PRED_ANGLE = {2: 32, 3: 26, 4: 21, 5: 17, 6: 13, 7: 9, 8: 5, 9: 2, 10: 0, 11: -2, 12: -5, 13: -9, 14: -13, 15: -17, 16: -21,
                    17: -26, 18: -32, 19: -26, 20: -21, 21: -17, 22: -13, 23: -9, 24: -5, 25: -2, 26: 0, 27: 2, 28: 5, 29: 9, 30: 13,
                    31: 17, 32: 21, 33: 26, 34: 32}                                                       # Table 8-5
INV_ANGLE = {11: -4096, 12: -1638, 13: -910, 14: -630, 15: -482, 16: -390, 17: -315, 18: -256, 19: -315, 20: -390, 21: -482,
             22: -630, 23: -910, 24: -1638, 25: -4096}                                                     # Table 8-6
SEGMENTS = ("BL", "L", "TL", "T", "TR")


def _segment(i, nT):
    return "BL" if i < nT else "L" if i < 2 * nT else "TL" if i == 2 * nT else "T" if i <= 3 * nT else "TR"


def reference_line(rec, plane, bit_depth, ev):
    """8.4.4.2.2: the 4 nT + 1 reference samples after substitution"""
    nT, x0, y0 = 1 << rec["log2"], rec["x"], rec["y"]
    n = 4 * nT + 1
    avail = np.zeros(n, bool)
    line = np.zeros(n, np.int64)
    # left column, y = 0 .. avail_left - 1 and nT .. nT + avail_bottom_left - 1 -> index 2 nT - 1 - y
    for first, count in ((0, rec["avail_left"]), (nT, rec["avail_bottom_left"])):
        if count:
            ys = np.arange(first, first + count)
            avail[2 * nT - 1 - ys] = True
            line[2 * nT - 1 - ys] = plane[y0 + ys, x0 - 1]
    if rec["avail_tl"]:
        avail[2 * nT] = True
        line[2 * nT] = plane[y0 - 1, x0 - 1]
    for first, count in ((0, rec["avail_top"]), (nT, rec["avail_top_right"])):
        if count:
            xs = np.arange(first, first + count)
            avail[2 * nT + 1 + xs] = True
            line[2 * nT + 1 + xs] = plane[y0 - 1, x0 + xs]
    sources = set()
    if not avail.any():
        line[:] = 1 << (bit_depth - 1)
        sources.add("default")
    elif not avail.all():
        idx = np.flatnonzero(avail)
        if not avail[0]:  # search upwards from p[-1][2 nT - 1] for the first available sample
            line[:idx[0]] = line[idx[0]]
            sources.add(_segment(int(idx[0]), nT))
        # every other missing sample takes the sample before it: the nearest available one below its index
        missing = np.flatnonzero(~avail)
        missing = missing[missing > idx[0]]
        if missing.size:
            src = idx[np.searchsorted(idx, missing) - 1]
            line[missing] = line[src]
            sources.update(_segment(int(s), nT) for s in np.unique(src))
    ev["sources"] = sources
    return line


def _pattern(rec):
    """the availability patterns of the census the record belongs to"""
    nT = 1 << rec["log2"]
    L, BL, T, TR, TL = rec["avail_left"], rec["avail_bottom_left"], rec["avail_top"], rec["avail_top_right"], rec["avail_tl"]
    out = set()
    if not (L or BL or T or TR or TL):
        out.add("nothing")
    if L == nT and T == 0 and not TL and TR == 0:
        out.add("top_missing_only")
    if T == nT and L == 0 and not TL and BL == 0:
        out.add("left_missing_only")
    if L == nT and BL == nT and T == nT and TR == nT and TL:
        out.add("complete")
    out.add("bl_none" if BL == 0 else "bl_full" if BL == nT else "bl_partial")
    out.add("tr_none" if TR == 0 else "tr_full" if TR == nT else "tr_partial")
    if T == 0 and TR:
        out.add("top_missing_tr_present")
    if not TL and L and T:
        out.add("corner_missing_only")
    if L == 0 and rec["x"] > 0:
        out.add("left_missing_inside")
    return out


def filter_rule(mode, nT):
    """8.4.4.2.3: filterFlag by size and mode"""
    if mode == 1 or nT == 4:
        return False
    return min(abs(mode - 26), abs(mode - 10)) > {8: 7, 16: 1, 32: 0}[nT]


def smooth_121(line):
    out = line.copy()
    out[1:-1] = (line[:-2] + 2 * line[1:-1] + line[2:] + 2) >> 2
    return out


def smooth_bilinear(line, nT):
    """8.4.4.2.3 with biIntFlag (nT = 32): both arms interpolated between the corner and their far ends"""
    n = 2 * nT
    k = np.arange(1, n)  # distance from the corner
    out = line.copy()
    out[n + k] = ((64 - k) * line[n] + k * line[2 * n] + 32) >> 6
    out[n - k] = ((64 - k) * line[n] + k * line[0] + 32) >> 6
    return out


def predict_from_line(line, mode, nT, cidx, bit_depth, edge_filters):
    """8.4.4.2.4 - 8.4.4.2.6 from the (filtered) reference line; (pred[y, x], edge event or None, clipped at 0, at max)"""
    log2 = nT.bit_length() - 1
    c = 2 * nT
    left = line[c - 1::-1]   # left[y] = p[-1][y], y = 0 .. 2 nT - 1
    top = line[c + 1:]       # top[x] = p[x][-1]
    corner = line[c]
    mx = (1 << bit_depth) - 1
    edge, lo, hi = None, False, False
    if mode == 0:
        x = np.arange(nT)[None, :]
        y = np.arange(nT)[:, None]
        pred = ((nT - 1 - x) * left[:nT, None] + (x + 1) * top[nT] + (nT - 1 - y) * top[None, :nT] + (y + 1) * left[nT] + nT) >> (log2 + 1)
        return pred, edge, lo, hi
    if mode == 1:
        dc = (int(top[:nT].sum()) + int(left[:nT].sum()) + nT) >> (log2 + 1)
        pred = np.full((nT, nT), dc, np.int64)
        if cidx == 0 and nT < 32:
            edge = "dc"
            pred[0, :] = (top[:nT] + 3 * dc + 2) >> 2
            pred[:, 0] = (left[:nT] + 3 * dc + 2) >> 2
            pred[0, 0] = (left[0] + 2 * dc + top[0] + 2) >> 2
        return pred, edge, lo, hi
    angle = INTRA_PRED_ANGLE[mode]
    vertical = mode >= 18
    main, side = (top, left) if vertical else (left, top)  # the arm the block is projected onto, and the other one
    # ref[r], r = -nT .. 2 nT, stored at r + nT
    ref = np.zeros(3 * nT + 1, np.int64)
    ref[nT] = corner
    ref[nT + 1:2 * nT + 1] = main[:nT]
    last = (nT * angle) >> 5
    if angle < 0:
        if last < -1:
            inv = INV_ANGLE[mode]
            for r in range(last, 0):
                v = (r * inv + 128) >> 8      # ref[r] = p[-1][-1 + v] resp. p[-1 + v][-1]
                ref[nT + r] = corner if v == 0 else side[v - 1]
    else:
        ref[2 * nT + 1:] = main[nT:]
    k = np.arange(1, nT + 1)
    i_idx, i_fact = (k * angle) >> 5, (k * angle) & 31
    pos = np.arange(nT)[None, :] + i_idx[:, None] + 1 + nT  # [distance from the main arm, position along it]
    f = i_fact[:, None]
    pred = np.where(f != 0, ((32 - f) * ref[pos] + f * ref[np.minimum(pos + 1, 3 * nT)] + 16) >> 5, ref[pos])
    if mode in (10, 26) and cidx == 0 and nT < 32:
        if edge_filters:
            edge = "v" if vertical else "h"
            raw = main[0] + ((side[:nT] - corner) >> 1)
            lo, hi = bool((raw < 0).any()), bool((raw > mx).any())
            pred[:, 0] = np.clip(raw, 0, mx)
        else:
            edge = "suppressed"
    return (pred if vertical else pred.T), edge, lo, hi


def predict(rec, planes, pic):
    """(predicted block [y, x] as int64, events) of one record; pic: residual_ref.Picture (bit depth, chroma format, flags)"""
    nT, mode, cidx, bd = 1 << rec["log2"], rec["mode"], rec["cidx"], pic.bit_depth
    assert not rec["pcm"] and 0 <= mode <= 34
    ev = dict(mode=mode, patterns=_pattern(rec))
    line = reference_line(rec, planes[cidx], bd, ev)
    ev["smoothing"] = "none"
    ev["strong"] = None
    used = line
    if (cidx == 0 or pic.chroma_format == 3) and filter_rule(mode, nT):
        if pic.flags & rr.PIC_NO_INTRA_SMOOTHING:
            ev["smoothing"] = "off_by_flag"
        else:
            bil = False
            if (pic.flags & rr.PIC_STRONG_INTRA) and cidx == 0 and nT == 32:
                lim = 1 << (bd - 5)
                s_top = abs(int(line[64] + line[128] - 2 * line[96]))    # p[-1][-1] + p[63][-1] - 2 p[31][-1]
                s_left = abs(int(line[64] + line[0] - 2 * line[32]))     # p[-1][-1] + p[-1][63] - 2 p[-1][31]
                bil = s_top < lim and s_left < lim
                ev["strong"] = dict(decision=bil, top_ok=s_top < lim, left_ok=s_left < lim, at_limit=any(s in (lim - 1, lim) for s in (s_top, s_left)),
                                    constant=bool((line == line[0]).all()))
            used = smooth_bilinear(line, nT) if bil else smooth_121(line)
            ev["smoothing"] = "bilinear" if bil else "121"
    edge_filters = not rr.bypass_unit_of_rdpcm_picture(rec, pic.flags)  # (the flag that also makes the unit's levels run sums)
    pred, ev["edge"], ev["edge_clip_lo"], ev["edge_clip_hi"] = predict_from_line(used, mode, nT, cidx, bd, edge_filters)
    if ev["edge"] is None and mode in (1, 10, 26):
        ev["edge"] = "not_chroma" if cidx else "not_32"
    if ev["strong"] and ev["strong"]["decision"]:
        other, _, _, _ = predict_from_line(smooth_121(line), mode, nT, cidx, bd, edge_filters)
        ev["strong"]["visible"] = not np.array_equal(other, pred)
    return pred, ev


def res_scale(rec, pic):
    """ResScaleVal of a chroma record (hm_stream.h: chroma records of a cross-component picture carry it in place of QpY)"""
    return rec["qpy"] if (pic.flags & rr.PIC_CROSS_COMPONENT) and rec["cidx"] and not rec["pcm"] else 0


def observable(rec, pic, carry=None):
    """whether the block's samples can be computed from its record and its neighbours: without a residual the picture holds the
    prediction itself; with one residual_ref restates the unit - transforms, skip and bypass (residual), implicit RDPCM
    (unit_residual), PCM (pcm_block).  A chroma block with a cross-component term needs the luma residual of its transform unit:
    observable where the walk carries it along (carry: a residual_ref.LumaCarry fed by expected_block in decode order)."""
    if res_scale(rec, pic) != 0:
        return carry is not None
    return True


def expected_block(rec, planes, pic, carry=None, quirks=rr.REFERENCE, pcm_bits=None):
    """(expected samples of an observable block, events); events["rail_lo" / "rail_hi"]: clip(pred + residual) acted;
    events["tools"]: the events of residual_ref's range-extension tools (own / ccp / pcm, each a dict or None, and luma: the events
    of the luma block under a cross-component term).  carry: see observable(); with it every record of the picture must pass
    through here in decode order.  pcm_bits: (luma, chroma) PCM bit depths where the caller knows them."""
    tools = dict(own=None, ccp=None, pcm=None, luma=None)
    if rec["pcm"]:
        v, tools["pcm"] = rr.pcm_block(rec, pic.bit_depth, None if pcm_bits is None else pcm_bits[1 if rec["cidx"] else 0])
        if carry is not None and rec["cidx"] == 0:
            carry.keep(rec, None, None)
        return v, dict(mode=None, rail_lo=False, rail_hi=False, tools=tools)
    pred, ev = predict(rec, planes, pic)
    ev["rail_lo"] = ev["rail_hi"] = False
    ev["tools"] = tools
    r = None
    if rec["cbf"]:
        r, tools["own"] = rr.unit_residual(rec, pic.bit_depth, pic.scaling, pic.flags, quirks)
    if carry is not None and rec["cidx"] == 0:
        carry.keep(rec, r, tools["own"])
    scale = res_scale(rec, pic)
    if scale != 0:
        assert pic.chroma_format == 3 and carry is not None
        r_luma, tools["luma"] = carry.luma_of(rec)
        r, tools["ccp"] = rr.cross_component(r, tools["own"], r_luma, scale, pic.bit_depth, pic.bit_depth_c, quirks)
    if r is not None:
        s = pred + r
        mx = (1 << pic.bit_depth) - 1
        ev["rail_lo"], ev["rail_hi"] = bool((s < 0).any()), bool((s > mx).any())
        pred = np.clip(s, 0, mx)
    return pred, ev
