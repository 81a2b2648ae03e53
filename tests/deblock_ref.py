"""The deblocking filter (8.7.2 of the standard) of one intra picture in plain numpy on int64: all vertical edges of a whole
plane first, then all horizontal edges on the result - the order of the standard's text and of the reference decoder, not the
shifted 8x8 windows of filters.hip.  Written from the standard and from reading the reference decoder (deblock.cc,
fallback-postfilter.h, x86_new/x86_dbk.cc); it shares nothing with oracle/oracle_recon.c or the kernels.  All units of one
direction of one plane are independent of each other (edges lie on the 8-sample grid, a filter reads four and writes three
samples on each side), so they are computed at once, as arrays over the units.

Inputs: the reconstruction-stage planes and residual_ref.Picture(blob in decode order).  The picture's intra-only: every
transform-block edge has bS 2, every other grid position bS 0 (8.7.2.4).

Where the reference decoder observably departs from the standard the model follows the reference, each departure behind a
switch of `Quirks` ("Deblocking, decision by decision"):

  pcmf_luma           In a picture with (pcm_enabled && pcm_loop_filter_disabled) || transquant_bypass_enabled the reference's
                      luma path (deblock.cc:755-783) sets no_p / no_q to "this side is NEITHER pcm NOR bypass" - pcm_flag alone,
                      without pcm_loop_filter_disabled - and hands them to a filter that modifies a side when its flag is
                      FALSE (fallback-postfilter.h:85-127).  A segment that touches a PCM / bypass unit therefore has exactly
                      its PCM / bypass sides filtered; a segment between ordinary units goes to the accelerated function,
                      which for 8-bit samples in the default build is the SSE kernel that ignores the flags and filters both
                      sides ("simd"), and otherwise the same scalar function, which then filters nothing ("scalar").
                      "off": 8.7.2.5.7 - nDp = 0 for pcm_loop_filter_disabled PCM and for bypass, nothing else.
  vchroma_p_for_both  fallback-postfilter.h:158-164: a vertical chroma edge writes q0 under the P side's flag.
  segment_params      deblock.cc:737-752, 1712-1716: QpY (luma) and the slice's offsets are those of the first 4-line unit
                      of an 8-sample segment.  Not observable: a luma segment lies inside one 8x8 block on either side
                      (one coding unit: one QpY, one slice), a chroma segment inside one CTB (one slice), and chroma QpC is
                      taken per unit.  The census holds the count at zero.
"""
import numpy as np

import residual_ref as rr

# Table 8-12: beta' and tc' from Q
BETA_PRIME = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 65, 2)), np.int64)
TC_PRIME = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], np.int64)
assert len(BETA_PRIME) == 52 and len(TC_PRIME) == 54
# Table 8-10: QpC from qPi for ChromaArrayType 1 (qPi < 30: qPi; > 43: qPi - 6)
QPC_30_43 = np.array([29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37], np.int64)


def table_8_10(qpi):
    qpi = np.asarray(qpi, np.int64)
    return np.where(qpi < 30, qpi, np.where(qpi > 43, qpi - 6, QPC_30_43[np.clip(qpi - 30, 0, 13)]))


class Quirks:
    def __init__(self, pcmf_luma="simd", vchroma_p_for_both=True, segment_params=True):
        assert pcmf_luma in ("simd", "scalar", "off")
        self.pcmf_luma, self.vchroma_p_for_both, self.segment_params = pcmf_luma, vchroma_p_for_both, segment_params


class Maps:
    """what 8.7.2 needs of the picture per 4x4 luma block [y4, x4], from the luma records, the CTB table and the slice table"""

    def __init__(self, P):
        assert P.crop == (0, 0, 0, 0), "pictures with a conformance window: the planes handed out are cropped"
        assert P.width % 8 == 0 and P.height % 8 == 0
        W4, H4 = P.width // 4, P.height // 4
        self.tu_left, self.tu_top = np.zeros((H4, W4), bool), np.zeros((H4, W4), bool)
        self.qpy = np.full((H4, W4), -999, np.int64)
        self.pcm, self.bypass = np.zeros((H4, W4), bool), np.zeros((H4, W4), bool)
        covered = 0
        for rec in P.records():
            if rec["cidx"]:
                continue
            n, x4, y4 = (1 << rec["log2"]) // 4, rec["x"] // 4, rec["y"] // 4
            self.tu_left[y4:y4 + n, x4] = True
            self.tu_top[y4, x4:x4 + n] = True
            self.qpy[y4:y4 + n, x4:x4 + n] = rec["qpy"]
            self.pcm[y4:y4 + n, x4:x4 + n] = rec["pcm"]
            self.bypass[y4:y4 + n, x4:x4 + n] = rec["bypass"]
            covered += n * n
        assert covered == W4 * H4, "the luma records do not tile the picture"
        ctbs, slices = P.ctbs(), P.slices()
        shift = P.log2_ctb - 2
        ctb_of = (np.arange(H4)[:, None] >> shift) * P.ctb_w + (np.arange(W4)[None, :] >> shift)
        self.ctb_flags = ctbs["flags"][ctb_of].astype(np.int64)
        self.slice = ctbs["slice_idx"][ctb_of].astype(np.int64)
        self.off = (self.ctb_flags & rr.CTB_DEBLOCK_OFF) != 0
        assert np.array_equal(self.off, slices["deblocking_disabled"][self.slice] != 0)
        self.beta_offset = slices["beta_offset_div2"].astype(np.int64)[self.slice] * 2   # slice_beta_offset_div2 << 1
        self.tc_offset = slices["tc_offset_div2"].astype(np.int64)[self.slice] * 2
        self.lf_across_slices = slices["lf_across_slices"][self.slice] != 0
        ctb4 = 1 << shift
        at_ctb_x = (np.arange(W4) % ctb4 == 0)[None, :]
        at_ctb_y = (np.arange(H4) % ctb4 == 0)[:, None]
        # 8.7.2.3: filterEdgeFlag - the picture's left / top edge, and the left / top edge of a slice or tile that the loop filters do not
        # cross (the parser's answer per CTB: HM_CTB_DEBLOCK_LEFT / TOP); 8.7.2: nothing in a slice with slice_deblocking_filter_disabled
        self.allowed_v = ~self.off & (~at_ctb_x | ((self.ctb_flags & rr.CTB_DEBLOCK_LEFT) != 0)) & (np.arange(W4) > 0)[None, :]
        self.allowed_h = ~self.off & (~at_ctb_y | ((self.ctb_flags & rr.CTB_DEBLOCK_TOP) != 0)) & (np.arange(H4) > 0)[:, None]
        # 8.7.2.4: an intra picture - bS 2 on transform-block edges, 0 elsewhere
        self.bs_v = 2 * (self.tu_left & self.allowed_v).astype(np.int64)
        self.bs_h = 2 * (self.tu_top & self.allowed_h).astype(np.int64)


def _clip3(lo, hi, v):
    return np.minimum(np.maximum(v, lo), hi)


def _edges_of_one_direction(A, c, vertical, M, P, quirks):
    """filter all edges of one direction of plane c in place (A: int64); returns the event record of every 4-line unit on the
    8-sample grid (bS 0 included).  Written for vertical edges; horizontal ones run on the transposed plane and maps."""
    t = (lambda a: a) if vertical else (lambda a: a.T)
    A = t(A)
    sw, sh = ((1 if P.chroma_format == 3 else 2), (2 if P.chroma_format == 1 else 1)) if c else (1, 1)
    if not vertical:
        sw, sh = sh, sw
    bd = P.bit_depth_c if c else P.bit_depth
    maxv = (1 << bd) - 1
    Hc, Wc = A.shape
    xc = np.tile(np.arange(8, Wc, 8), len(range(0, Hc, 4)))
    yc = np.repeat(np.arange(0, Hc, 4), len(range(8, Wc, 8)))
    ev = dict(plane=np.full(len(xc), c), vertical=np.full(len(xc), vertical), x=xc if vertical else yc, y=yc if vertical else xc)
    if not len(xc):
        return None
    x4, y4 = xc * sw // 4, yc * sh // 4
    y4s = (yc // 8 * 8) * sh // 4 if quirks.segment_params else y4   # the first unit of the 8-sample segment
    bS = t(M.bs_v if vertical else M.bs_h)[y4, x4]
    qpy, slc, off = t(M.qpy), t(M.slice), t(M.off)
    pcm, byp = t(M.pcm), t(M.bypass)
    yq = y4s if c == 0 else y4
    QpQ, QpP = qpy[yq, x4], qpy[yq, x4 - 1]
    tc_off, beta_off = t(M.tc_offset)[y4s, x4], t(M.beta_offset)[y4s, x4]
    ev.update(bS=bS, QpP=QpP, QpQ=QpQ, slice_p=slc[y4, x4 - 1], slice_q=slc[y4, x4], off_p=off[y4, x4 - 1], off_q=off[y4, x4],
              beta_offset=beta_off, tc_offset=tc_off, beta_offset_p=t(M.beta_offset)[y4, x4 - 1], tc_offset_p=t(M.tc_offset)[y4, x4 - 1],
              tu_edge=t(M.tu_left if vertical else M.tu_top)[y4, x4], allowed=t(M.allowed_v if vertical else M.allowed_h)[y4, x4],
              lf_across_slices=t(M.lf_across_slices)[y4, x4],
              segment_differs=(slc[y4s, x4] != slc[y4, x4]) | ((qpy[y4s, x4] != qpy[y4, x4]) | (qpy[y4s, x4 - 1] != qpy[y4, x4 - 1]) if c == 0 else False),
              pcm_p=pcm[y4, x4 - 1], pcm_q=pcm[y4, x4], bypass_p=byp[y4, x4 - 1], bypass_q=byp[y4, x4])
    # the window of filters.hip that holds the unit: [8k - 4, 8k + 4) along the edge, cut at the plane's borders
    o = (yc + 4) // 8 * 8 - 4
    ev["window"] = np.where(o < 0, 1, np.where(o + 8 > Hc, 2, 0))   # 0 interior, 1 first half missing (top / left), 2 second half missing (bottom / right)
    rows = (yc[:, None] + np.arange(4))[:, :, None]
    pi, qi = (xc[:, None] - 1 - np.arange(4))[:, None, :], (xc[:, None] + np.arange(4))[:, None, :]
    p, q = A[rows, pi], A[rows, qi]   # [unit, line k, sample i]: p_i,k / q_i,k
    before = (p.copy(), q.copy())
    # 8.7.2.5.7: nDp / nDq = 0
    lossless_p = (P.pcm_loop_filter_disabled != 0) & pcm[y4, x4 - 1] | byp[y4, x4 - 1]
    lossless_q = (P.pcm_loop_filter_disabled != 0) & pcm[y4, x4] | byp[y4, x4]
    filterP, filterQ = ~lossless_p, ~lossless_q
    pcmf = bool(P.flags & rr.PIC_PCMF)
    on = bS > 0

    if c == 0:
        # ---- 8.7.2.5.3: the decisions ----
        qPL = (QpQ + QpP + 1) >> 1
        Qb, Qt = qPL + beta_off, qPL + 2 * (bS - 1) + tc_off
        beta = BETA_PRIME[np.clip(Qb, 0, 51)] * (1 << (bd - 8))
        tc = TC_PRIME[np.clip(Qt, 0, 53)] * (1 << (bd - 8))
        p0, p1, p2, p3 = (p[:, :, i] for i in range(4))
        q0, q1, q2, q3 = (q[:, :, i] for i in range(4))
        dpk, dqk = np.abs(p2 - 2 * p1 + p0), np.abs(q2 - 2 * q1 + q0)
        dp0, dp3, dq0, dq3 = dpk[:, 0], dpk[:, 3], dqk[:, 0], dqk[:, 3]
        dpq0, dpq3, dp, dq = dp0 + dq0, dp3 + dq3, dp0 + dp3, dq0 + dq3
        d = dpq0 + dpq3
        filtered = on & (d < beta)
        tc25 = (5 * tc + 1) >> 1
        preds = np.stack([2 * dpq0 < (beta >> 2), np.abs(p3[:, 0] - p0[:, 0]) + np.abs(q0[:, 0] - q3[:, 0]) < (beta >> 3), np.abs(p0[:, 0] - q0[:, 0]) < tc25,
                          2 * dpq3 < (beta >> 2), np.abs(p3[:, 3] - p0[:, 3]) + np.abs(q0[:, 3] - q3[:, 3]) < (beta >> 3), np.abs(p0[:, 3] - q0[:, 3]) < tc25], 1)
        strong = filtered & preds.all(1)
        normal = filtered & ~strong
        side = (beta + (beta >> 1)) >> 3
        dEp, dEq = filtered & (dp < side), filtered & (dq < side)
        if pcmf and quirks.pcmf_luma != "off":
            special_p, special_q = pcm[y4, x4 - 1] | byp[y4, x4 - 1], pcm[y4, x4] | byp[y4, x4]
            # (both units of the 8-sample segment: an 8x8 block on either side, so they hold the same answers - asserted)
            y4o = y4 ^ 1
            assert np.array_equal(special_p, (pcm | byp)[y4o, x4 - 1]) and np.array_equal(special_q, (pcm | byp)[y4o, x4])
            ordinary = ~special_p & ~special_q
            both = bd == 8 and quirks.pcmf_luma == "simd"
            filterP, filterQ = np.where(ordinary, both, special_p), np.where(ordinary, both, special_q)
        # ---- 8.7.2.5.7, strong: six positions, each within 2 tc of its sample ----
        tc2 = (2 * tc)[:, None]
        raw_s = [(p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (p2 + p1 + p0 + q0 + 2) >> 2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3,
                 (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, (p0 + q0 + q1 + q2 + 2) >> 2, (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3]
        old_s = [p0, p1, p2, q0, q1, q2]
        new_s = [_clip3(o_ - tc2, o_ + tc2, r_) for o_, r_ in zip(old_s, raw_s)]
        wr_s = [strong & (filterP if k < 3 else filterQ) for k in range(6)]
        ev["strong_lo"] = np.stack([(w[:, None] & (r_ < o_ - tc2)).any(1) for w, o_, r_ in zip(wr_s, old_s, raw_s)], 1)
        ev["strong_hi"] = np.stack([(w[:, None] & (r_ > o_ + tc2)).any(1) for w, o_, r_ in zip(wr_s, old_s, raw_s)], 1)
        # ---- normal ----
        term = 9 * (q0 - p0) - 3 * (q1 - p1) + 8
        delta0 = term >> 4
        line = normal[:, None] & (np.abs(delta0) < 10 * tc[:, None])
        delta = _clip3(-tc[:, None], tc[:, None], delta0)
        tch = (tc >> 1)[:, None]
        raw_dp, raw_dq = (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1
        Dp, Dq = _clip3(-tch, tch, raw_dp), _clip3(-tch, tch, raw_dq)
        w_p0, w_q0 = line & filterP[:, None], line & filterQ[:, None]
        w_p1, w_q1 = w_p0 & dEp[:, None], w_q0 & dEq[:, None]
        raw_n = [p0 + delta, p1 + Dp, q0 - delta, q1 + Dq]
        wr_n = [w_p0, w_p1, w_q0, w_q1]
        ev.update(delta_lo=((w_p0 | w_q0) & (delta0 < -tc[:, None])).any(1), delta_hi=((w_p0 | w_q0) & (delta0 > tc[:, None])).any(1),
                  dp_lo=(w_p1 & (raw_dp < -tch)).any(1), dp_hi=(w_p1 & (raw_dp > tch)).any(1),
                  dq_lo=(w_q1 & (raw_dq < -tch)).any(1), dq_hi=(w_q1 & (raw_dq > tch)).any(1),
                  res_lo=np.any([(w & (r_ < 0)).any(1) for w, r_ in zip(wr_n, raw_n)], 0), res_hi=np.any([(w & (r_ > maxv)).any(1) for w, r_ in zip(wr_n, raw_n)], 0),
                  lines_skipped=(normal[:, None] & ~line).sum(1), lines_filtered=line.sum(1),
                  peak=np.where(normal, np.abs(term).max(1), 0), peak_strong=np.where(strong, np.abs(term).max(1), 0))
        pn, qn = p.copy(), q.copy()
        for k in range(3):
            pn[:, :, k] = np.where(wr_s[k][:, None], new_s[k], pn[:, :, k])
            qn[:, :, k] = np.where(wr_s[3 + k][:, None], new_s[3 + k], qn[:, :, k])
        pn[:, :, 0] = np.where(w_p0, np.clip(raw_n[0], 0, maxv), pn[:, :, 0])
        pn[:, :, 1] = np.where(w_p1, np.clip(raw_n[1], 0, maxv), pn[:, :, 1])
        qn[:, :, 0] = np.where(w_q0, np.clip(raw_n[2], 0, maxv), qn[:, :, 0])
        qn[:, :, 1] = np.where(w_q1, np.clip(raw_n[3], 0, maxv), qn[:, :, 1])
        ev.update(Q_beta=Qb, Q_tc=Qt, beta=beta, tc=tc, d=d, dE=np.where(strong, 2, np.where(normal, 1, 0)), dEp=dEp, dEq=dEq, preds=preds,
                  filterP=filterP & on, filterQ=filterQ & on)
    else:
        # ---- 8.7.2.5.5: chroma edges, bS 2 only ----
        cQpPicOffset = P.cb_qp_offset if c == 1 else P.cr_qp_offset
        qPi = ((QpQ + QpP + 1) >> 1) + cQpPicOffset
        QpC = table_8_10(qPi) if P.chroma_format == 1 else np.minimum(qPi, 51)
        Qt = QpC + 2 * (bS - 1) + tc_off
        tc = np.where(bS == 2, TC_PRIME[np.clip(Qt, 0, 53)] * (1 << (bd - 8)), 0)
        p0, p1, q0, q1 = p[:, :, 0], p[:, :, 1], q[:, :, 0], q[:, :, 1]
        raw = (((q0 - p0) << 2) + p1 - q1 + 4) >> 3
        delta = _clip3(-tc[:, None], tc[:, None], raw)
        if vertical and quirks.vchroma_p_for_both:
            filterQ = filterP
        w_p, w_q = (on & filterP)[:, None], (on & filterQ)[:, None]
        pn, qn = p.copy(), q.copy()
        pn[:, :, 0] = np.where(w_p, np.clip(p0 + delta, 0, maxv), p0)
        qn[:, :, 0] = np.where(w_q, np.clip(q0 - delta, 0, maxv), q0)
        ev.update(qPi=qPi, QpC=QpC, Q_tc=Qt, tc=tc, beta=np.zeros_like(tc), dE=np.where(on, 1, 0), filterP=filterP & on, filterQ=filterQ & on,
                  lossless_p=lossless_p, lossless_q=lossless_q,
                  delta_lo=((w_p | w_q) & (raw < -tc[:, None])).any(1), delta_hi=((w_p | w_q) & (raw > tc[:, None])).any(1),
                  res_lo=((w_p & (p0 + delta < 0)) | (w_q & (q0 - delta < 0))).any(1), res_hi=((w_p & (p0 + delta > maxv)) | (w_q & (q0 - delta > maxv))).any(1))
    A[rows, pi], A[rows, qi] = pn, qn
    ev["changed"] = (pn != before[0]).any((1, 2)) | (qn != before[1]).any((1, 2))
    return ev


def deblock(planes, P, quirks=None):
    """(deblocked planes as int64 arrays, events): events is a list of dicts of arrays, one per (plane, direction) with at least
    one grid position, each array with one entry per 4-line unit"""
    quirks = quirks or Quirks()
    M = Maps(P)
    out, events = [], []
    for c, plane in enumerate(planes):
        A = np.array(plane, np.int64)
        assert A.shape == ((P.height, P.width) if c == 0 else (P.height // (2 if P.chroma_format == 1 else 1), P.width // (1 if P.chroma_format == 3 else 2)))
        after_v = None
        for vertical in (True, False):
            ev = _edges_of_one_direction(A, c, vertical, M, P, quirks)
            if ev is None:
                continue
            if vertical:
                after_v = A != np.asarray(plane, np.int64)
            elif after_v is not None:
                # a horizontal unit that READS a sample its vertical edge changed (the crossing of filters.hip's windows)
                ev["reads_filtered"] = np.array([after_v[y - 4:y + 4, x:x + 4].any() for x, y in zip(ev["x"], ev["y"])], bool) & (ev["bS"] > 0)
            events.append(ev)
        out.append(A)
    return out, events


def describe(ev, k):
    """the event record of unit k of one (plane, direction)"""
    keys = ("bS", "QpP", "QpQ", "beta", "tc", "dE", "dEp", "dEq", "filterP", "filterQ", "QpC", "d")
    return (f"plane {int(ev['plane'][k])} {'vertical' if ev['vertical'][k] else 'horizontal'} edge, unit at (x,y)=({int(ev['x'][k])},{int(ev['y'][k])}) " +
            " ".join(f"{n} {int(ev[n][k])}" for n in keys if n in ev) +
            (" filter " + ("none", "normal", "strong")[int(ev["dE"][k])] if ev["plane"][k] == 0 else " filter chroma"))


def units_at(events, c, y, x):
    """the records of the units whose samples (four on either side of the edge) hold sample (y, x) of plane c"""
    out = []
    for ev in events:
        if ev["plane"][0] != c:
            continue
        along, across = (ev["y"], ev["x"]) if ev["vertical"][0] else (ev["x"], ev["y"])
        a, b = (y, x) if ev["vertical"][0] else (x, y)
        for k in np.flatnonzero((along <= a) & (a < along + 4) & (across - 4 <= b) & (b < across + 4)):
            out.append(describe(ev, k))
    return out
