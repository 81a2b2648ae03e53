"""Sample adaptive offset (8.7.3 of the standard) of one intra picture in plain numpy on int64, every sample of a plane at once.
Written from the standard's text and from reading the reference decoder (sao.cc); it shares nothing with oracle/oracle_recon.c,
filters.hip or hevc_parse.cpp, and it does not read the parser's neighbour answers (hm_ctb.sao_nb_mask, sao_nb_mask_c, sao_ring_c) nor
HM_CTB_LOSSLESS.

Inputs: the planes SAO reads (deblocking stage, or reconstruction stage for SAO alone) UNCROPPED, residual_ref.Picture(blob in decode
order) and the stream's bytes.  Of the blob it takes the SAO parameters of every CTB (hm_ctb.sao[3]: SaoOffsetVal as delivered, already
scaled), the slices' flags and addresses (hm_slice), the CTB -> slice table and the PCM / bypass flags of the luma records.  The tile
structure is NOT taken from the parser: the stream's PPS is read here, with a bit reader of its own, and colBd / rowBd / TileId /
CtbAddrRsToTs follow (6-3), (6-4), (6-5), (6-9).

The arithmetic as 8.7.3 words it: bandTable[(k + sao_band_position) & 31] = k + 1, bandShift = bitDepth - 5; edgeIdx = 2 + sign(a) +
sign(b) with 0, 1, 2 remapped to 1, 2, 0; the clip to [0, (1 << bitDepth) - 1]; every sample reads the INPUT picture; a sample of a PCM
unit under pcm_loop_filter_disabled or of a bypass unit is not modified; a neighbour sample is unavailable (edgeIdx 0) when it lies
outside the picture, in an earlier slice while the current sample's slice has slice_loop_filter_across_slices_enabled_flag 0, in a later
slice that has the flag 0, or in another tile with loop_filter_across_tiles_enabled_flag 0.  "Earlier" is the standard's MinTbAddrZs
order: the position in decoding order.

Where the reference decoder observably departs from this text the model follows the reference, each departure behind a switch of
`Quirks` ("SAO, sample by sample"):

  chroma_slice_lookup     Q13, sao.cc:289: "the slice of the current CTB", whose address the neighbour's is compared with, is looked up at
                          the CTB's position in samples of the COMPONENT: for sub-sampled chroma at CTB (x >> 1, y >> 1 or y).  The flag
                          of the current sample's slice and both tile ids are the right ones (sao.cc:389, 403).  With it comes sao.cc:366:
                          only the samples of the (cut) CTB's outer ring are tested - without the wrong address a test of an inner
                          sample cannot fail, with it it could, so the restriction belongs to the switch.
  pps_fast_path           sao.cc:323: with pps_loop_filter_across_slices_enabled_flag, no tiles and no PCM / bypass unit in the CTB the
                          edge offset goes down a path that tests the picture's borders alone:
                          slice_loop_filter_across_slices_enabled_flag is never looked at.
  slice_order_by_address  sao.cc:388, 395: "earlier" / "later" compare SliceAddrRS, the raster address of the slice's first CTB, not the
                          decoding order.  The two differ only with tiles: a slice that starts in a lower CTB row of the left tile is
                          decoded before the first slice of the tile to its right and has the larger address.
"""
import numpy as np

import hevcutil

NAL_PPS = 34
HPOS = np.array([[-1, 1], [0, 0], [-1, 1], [1, -1]], np.int64)   # Table 8-13: hPos[k], vPos[k] per SaoEoClass
VPOS = np.array([[0, 0], [-1, 1], [-1, 1], [-1, 1]], np.int64)
OK, PICTURE_EDGE, EARLIER_SLICE, LATER_SLICE, TILE_BORDER = 0, 1, 2, 3, 4
REASONS = ("ok", "picture_edge", "earlier_slice", "later_slice", "tile_border")


class Quirks:
    NAMES = ("chroma_slice_lookup", "pps_fast_path", "slice_order_by_address")

    def __init__(self, chroma_slice_lookup=True, pps_fast_path=True, slice_order_by_address=True):
        self.chroma_slice_lookup, self.pps_fast_path, self.slice_order_by_address = chroma_slice_lookup, pps_fast_path, slice_order_by_address

    def without(self, name):
        q = Quirks(self.chroma_slice_lookup, self.pps_fast_path, self.slice_order_by_address)
        assert name in self.NAMES
        setattr(q, name, False)
        return q


# ---- the stream's PPS ------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, nal):
        body, out, zeros = nal[2:], bytearray(), 0  # (two bytes of NAL header; 7.4.2: emulation_prevention_three_byte removed)
        for b in body:
            if zeros >= 2 and b == 3:
                zeros = 0
                continue
            out.append(b)
            zeros = zeros + 1 if b == 0 else 0
        self.b, self.p = bytes(out), 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.b[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)


def read_pps(data):
    """7.3.2.3.1 up to pps_loop_filter_across_slices_enabled_flag, of the stream's one PPS"""
    nals = [n for n in hevcutil.split_nals(data) if (n[0] >> 1) & 0x3F == NAL_PPS]
    assert len(nals) == 1
    r = _Bits(nals[0])
    r.ue(), r.ue()                      # pps_pic_parameter_set_id, pps_seq_parameter_set_id
    r.u(1), r.u(1), r.u(3), r.u(1), r.u(1)  # dependent_slice_segments_enabled, output_flag_present, num_extra_slice_header_bits, sign_data_hiding, cabac_init_present
    r.ue(), r.ue(), r.se()              # num_ref_idx_l0 / l1_default_active_minus1, init_qp_minus26
    r.u(1), r.u(1)                      # constrained_intra_pred, transform_skip_enabled
    if r.u(1):                          # cu_qp_delta_enabled_flag
        r.ue()                          # diff_cu_qp_delta_depth
    r.se(), r.se()                      # pps_cb_qp_offset, pps_cr_qp_offset
    r.u(1), r.u(1), r.u(1), r.u(1)      # pps_slice_chroma_qp_offsets_present, weighted_pred, weighted_bipred, transquant_bypass_enabled
    pps = dict(tiles_enabled=r.u(1), cols=1, rows=1, uniform=1, col_widths=[], row_heights=[], lf_across_tiles=1)
    r.u(1)                              # entropy_coding_sync_enabled_flag
    if pps["tiles_enabled"]:
        pps["cols"], pps["rows"] = r.ue() + 1, r.ue() + 1
        pps["uniform"] = r.u(1)
        if not pps["uniform"]:
            pps["col_widths"] = [r.ue() + 1 for _ in range(pps["cols"] - 1)]
            pps["row_heights"] = [r.ue() + 1 for _ in range(pps["rows"] - 1)]
        pps["lf_across_tiles"] = r.u(1)
    pps["lf_across_slices"] = r.u(1)
    return pps


class Tiles:
    """colBd / rowBd (6-3, 6-4), TileId per CTB in raster order (6-9) and CtbAddrRsToTs (6-5)"""

    def __init__(self, pps, ctb_w, ctb_h):
        def sizes(n, total, explicit):
            if pps["uniform"]:
                return [(i + 1) * total // n - i * total // n for i in range(n)]
            return list(explicit) + [total - sum(explicit)]
        col_w, row_h = sizes(pps["cols"], ctb_w, pps["col_widths"]), sizes(pps["rows"], ctb_h, pps["row_heights"])
        assert min(col_w) > 0 and min(row_h) > 0
        self.colBd, self.rowBd = np.concatenate([[0], np.cumsum(col_w)]), np.concatenate([[0], np.cumsum(row_h)])
        tx = np.searchsorted(self.colBd[1:], np.arange(ctb_w), side="right")
        ty = np.searchsorted(self.rowBd[1:], np.arange(ctb_h), side="right")
        self.tile_id = (ty[:, None] * pps["cols"] + tx[None, :]).ravel()
        col_w, row_h = np.array(col_w, np.int64), np.array(row_h, np.int64)
        before_rows = (ctb_w * self.rowBd[:-1])[ty][:, None]                 # the tile rows above
        before_cols = row_h[ty][:, None] * self.colBd[:-1][tx][None, :]     # the tiles to the left in this tile row
        inside = (np.arange(ctb_h) - self.rowBd[:-1][ty])[:, None] * col_w[tx][None, :] + (np.arange(ctb_w) - self.colBd[:-1][tx])[None, :]
        self.rs_to_ts = (before_rows + before_cols + inside).ravel()
        assert np.array_equal(np.sort(self.rs_to_ts), np.arange(ctb_w * ctb_h))


class Layout:
    """what 8.7.3 needs of the picture per CTB (raster order) and per 4x4 luma block"""

    def __init__(self, P, data):
        self.pps = read_pps(data)
        T = self.tiles = Tiles(self.pps, P.ctb_w, P.ctb_h)
        ctbs, slices = P.ctbs(), P.slices()
        sidx = ctbs["slice_idx"].astype(np.int64)
        self.slice_addr = slices["slice_addr"].astype(np.int64)[sidx]
        self.decode_pos = T.rs_to_ts[self.slice_addr]   # of the slice's first CTB: the slices' decoding order
        self.lf = slices["lf_across_slices"][sidx] != 0
        self.on = (slices["sao_luma"][sidx] != 0, slices["sao_chroma"][sidx] != 0)
        self.tile = T.tile_id
        self.sao = ctbs["sao"]
        W4, H4 = (P.width + 3) // 4, (P.height + 3) // 4
        self.pcm, self.bypass = np.zeros((H4, W4), bool), np.zeros((H4, W4), bool)
        for rec in P.records():
            if rec["cidx"] == 0 and (rec["pcm"] or rec["bypass"]):
                n, x4, y4 = (1 << rec["log2"]) // 4, rec["x"] // 4, rec["y"] // 4
                self.pcm[y4:y4 + n, x4:x4 + n] = rec["pcm"]
                self.bypass[y4:y4 + n, x4:x4 + n] = rec["bypass"]
        self.kept = (self.pcm & bool(P.pcm_loop_filter_disabled)) | self.bypass   # samples SAO does not modify
        s = P.log2_ctb - 2
        special = self.pcm | self.bypass
        self.ctb_special = np.zeros(P.ctb_w * P.ctb_h, bool)                       # the CTB holds a PCM or a bypass unit (sao.cc:309)
        yy, xx = np.nonzero(special)
        self.ctb_special[(yy >> s) * P.ctb_w + (xx >> s)] = True


def _plane(A, c, P, L, q, in_place, record):
    """(SAO of plane c as int64, the event record of every sample as whole-plane arrays)"""
    H, W = A.shape
    sw, sh = ((1 if P.chroma_format == 3 else 2), (2 if P.chroma_format == 1 else 1)) if c else (1, 1)
    csw, csh = sw - 1, sh - 1
    l2w, l2h = P.log2_ctb - csw, P.log2_ctb - csh
    bd = P.bit_depth_c if c else P.bit_depth
    maxv = (1 << bd) - 1
    y, x = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    cx, cy = x >> l2w, y >> l2h
    ctb = cy * P.ctb_w + cx + np.zeros((H, W), np.int64)
    n_ctb = P.ctb_w * P.ctb_h
    par = L.sao[:, c]
    on = L.on[1 if c else 0][ctb]
    typ = np.where(on, par["type"].astype(np.int64)[ctb], 0)
    kept = L.kept[(y * sh) >> 2, (x * sw) >> 2]
    special = (L.pcm | L.bypass)[(y * sh) >> 2, (x * sw) >> 2]
    val5 = np.zeros((n_ctb, 5), np.int64)
    val5[:, 1:] = par["offset"]                                  # SaoOffsetVal[0] = 0, [i + 1] = the offsets as delivered
    # ---- 8.7.3.2, band offset ----
    bp = par["band_position"].astype(np.int64)
    table = np.zeros((n_ctb, 32), np.int64)
    for k in range(4):
        table[np.arange(n_ctb), (k + bp) & 31] = k + 1
    band = A >> (bd - 5)
    band_idx = table[ctb, band]
    raw_band = A + val5[ctb, band_idx]
    # ---- 8.7.3.2, edge offset ----
    cls = par["eo_class"].astype(np.int64)[ctb]
    i, j = x - (cx << l2w), y - (cy << l2h)
    ring = (i == 0) | (j == 0) | (i == np.minimum(1 << l2w, W - (cx << l2w)) - 1) | (j == np.minimum(1 << l2h, H - (cy << l2h)) - 1)
    ctb_q13 = (cy >> csh) * P.ctb_w + (cx >> csw) + np.zeros((H, W), np.int64)  # where sao.cc:289 looks "the current slice" up
    tiles_stop = L.pps["tiles_enabled"] and not L.pps["lf_across_tiles"]

    def judge(nb, quirks, ring_only=True):
        """why a sample may not use a neighbour sample that lies in CTB nb (inside the picture)"""
        key = L.slice_addr if quirks.slice_order_by_address else L.decode_pos
        cur = key[ctb_q13 if quirks.chroma_slice_lookup else ctb]
        earlier = (key[nb] < cur) & ~L.lf[ctb]
        later = (key[nb] > cur) & ~L.lf[nb]
        tile = (L.tile[nb] != L.tile[ctb]) if tiles_stop else np.zeros((H, W), bool)
        r = np.where(earlier, EARLIER_SLICE, np.where(later, LATER_SLICE, np.where(tile, TILE_BORDER, OK)))
        if quirks.chroma_slice_lookup and ring_only:
            r = np.where(ring, r, OK)
        if quirks.pps_fast_path and L.pps["lf_across_slices"] and not L.pps["tiles_enabled"]:
            r = np.where(L.ctb_special[ctb], r, OK)
        return r

    pos = lambda m: m[(y * sh) >> 2, (x * sw) >> 2]
    ev = dict(type=typ, on=on, eo_class=cls, band=band, band_idx=band_idx, band_position=bp[ctb], kept=kept, special=special, ctb=ctb,
              ring=ring, before=A, on_luma=L.on[0][ctb], on_chroma=L.on[1][ctb], pcm=pos(L.pcm), bypass=pos(L.bypass),
              cut_right=((cx + 1) << l2w) > W, cut_bottom=((cy + 1) << l2h) > H,
              cb_cr_differ=(L.sao[:, 1]["offset"] != L.sao[:, 2]["offset"]).any(1)[ctb] if c else np.zeros((H, W), bool),
              own_ctb_blocked=judge(ctb, q, ring_only=False) != OK)  # (sub-sampled chroma under Q13 alone: every ring sample of the CTB with a neighbour inside it is stopped)
    nbv, avail_all = [], np.ones((H, W), bool)
    variants = {name: np.zeros((H, W), bool) for name in Quirks.NAMES}
    for k in range(2):
        xS, yS = x + HPOS[cls, k], y + VPOS[cls, k]
        outside = (xS < 0) | (yS < 0) | (xS >= W) | (yS >= H)
        xc, yc = np.clip(xS, 0, W - 1), np.clip(yS, 0, H - 1)
        dxc, dyc = (xc >> l2w) - cx, (yc >> l2h) - cy
        nb = ctb + dyc * P.ctb_w + dxc
        reason = np.where(outside, PICTURE_EDGE, judge(nb, q))
        avail_all &= reason == OK
        nbv.append((yc, xc))
        ev["ab"[k] + "_reason"] = reason
        ev["ab"[k] + "_dx"], ev["ab"[k] + "_dy"] = dxc, dyc
        if not record:
            continue
        for name in Quirks.NAMES:  # what the answer would be with one switch off: the samples each quirk decides
            if getattr(q, name):
                variants[name] |= ~outside & ((judge(nb, q.without(name)) == OK) != (reason == OK))
        # the CTBs beside a diagonal neighbour CTB (classes 2 and 3)
        diagonal = ~outside & (dxc != 0) & (dyc != 0)
        side_h, side_v = judge(ctb + dxc, q), judge(ctb + dyc * P.ctb_w, q)
        ev["ab"[k] + "_outside_x"], ev["ab"[k] + "_outside_y"] = (xS < 0) * -1 + (xS >= W) * 1, (yS < 0) * -1 + (yS >= H) * 1
        ev["ab"[k] + "_diag_blocked_sides_ok"] = diagonal & (reason != OK) & (side_h == OK) & (side_v == OK)
        ev["ab"[k] + "_diag_ok_side_blocked"] = diagonal & (reason == OK) & ((side_h != OK) | (side_v != OK))
        ev["ab"[k] + "_own_ctb_blocked"] = ~outside & (dxc == 0) & (dyc == 0) & (reason != OK)
        ev["ab"[k] + "_kept"] = kept[yc, xc] & ~outside
        ev["ab"[k] + "_other_slice_used"] = ~outside & (reason == OK) & (L.slice_addr[nb] != L.slice_addr[ctb]) & \
            np.where(L.decode_pos[nb] < L.decode_pos[ctb], ~L.lf[ctb], ~L.lf[nb])
    for name in Quirks.NAMES:
        ev["decided_by_" + name] = variants[name]

    def edge(src_a):
        a, b = src_a[nbv[0]], A[nbv[1]]
        idx = 2 + np.sign(A - a) + np.sign(A - b)
        idx = np.where(idx == 2, 0, np.where(idx < 2, idx + 1, idx))  # (8-xxx): edgeIdx 0, 1, 2 -> 1, 2, 0
        idx = np.where(avail_all, idx, 0)
        return idx, A + val5[ctb, idx]

    edge_idx, raw_edge = edge(A)
    raw = np.where(typ == 1, raw_band, np.where(typ == 2, raw_edge, A))
    out = np.where(kept, A, np.clip(raw, 0, maxv))
    ev.update(edge_idx=edge_idx, available=avail_all, raw=raw, after=out)
    if not (record or in_place):
        return out, ev
    # the deliberately wrong in-place variant: neighbour a - the one that precedes the sample in raster order in every class - read after SAO
    _, raw_wrong = edge(out)
    wrong = np.where(kept | (typ != 2), out, np.clip(raw_wrong, 0, maxv))
    ev["in_place_would_differ"] = wrong != out
    return (wrong if in_place else out), ev


def planes_shape(P):
    cw, ch = (P.width if P.chroma_format == 3 else P.width // 2), (P.height // 2 if P.chroma_format == 1 else P.height)
    return [(P.height, P.width)] + ([] if P.chroma_format == 0 else [(ch, cw), (ch, cw)])


def sao(planes, P, data, quirks=None, in_place=False, record=True):
    """(the planes after SAO as int64 arrays, [event record of plane c]): planes are the whole coded picture, no conformance window applied.
    record=False: only what describe() prints of a sample - not the census' records (what each quirk decides, the CTBs beside a diagonal one, the in-place variant)"""
    quirks = quirks or Quirks()
    L = Layout(P, data)
    out, events = [], []
    assert [tuple(np.shape(p)) for p in planes] == planes_shape(P), "the planes are not those of the whole coded picture"
    for c, plane in enumerate(planes):
        o, ev = _plane(np.array(plane, np.int64), c, P, L, quirks, in_place, record)
        ev["plane"] = c
        out.append(o)
        events.append(ev)
    return out, events


def describe(ev, y, x):
    """the event record of sample (y, x) of one plane"""
    g = lambda n: int(ev[n][y, x])
    kind = ("off", "band", "edge")[g("type")]
    s = f"plane {ev['plane']} CTB {g('ctb')} SAO {kind} input {g('before')} model {g('after')}"
    if not g("on"):
        s += " (slice flag 0)"
    if g("kept"):
        s += " kept (PCM / bypass)"
    if kind == "band":
        s += f" band {g('band')} position {g('band_position')} bandIdx {g('band_idx')} unclipped {g('raw')}"
    if kind == "edge":
        s += (f" class {g('eo_class')} a: {REASONS[g('a_reason')]} (CTB {g('a_dx'):+d},{g('a_dy'):+d}) b: {REASONS[g('b_reason')]} (CTB {g('b_dx'):+d},{g('b_dy'):+d}) "
              f"edgeIdx {g('edge_idx')} unclipped {g('raw')} ring {g('ring')}")
    return s
