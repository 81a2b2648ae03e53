"""An exact restatement of the residual arithmetic of one transform block - dequantisation (8.6.3 / 8.6.4.1), the inverse
transforms (8.6.4.2), transform skip and transquant bypass - in plain numpy on int64, where none of the sums can overflow.
Written from the standard and from the SCALAR code of the reference decoder (transform.cc:386-545, fallback-dct.cc); it
shares nothing with oracle/oracle_recon.c or the kernels.  Where the reference's arithmetic differs from the standard's
unbounded integers the difference is written out:

  * the flat product level * (levelScale << qP / 6) + offset is an `int` in the reference (transform.cc:496-502): it is
    taken modulo 2^32 here, explicitly (wrap32) - quirk Q3;
  * with scaling lists the product is 64 bits wide (transform.cc:507-545): no wrap;
  * the 4x4 DST clips its second stage to 16 bits, the DCTs do not (fallback-dct.cc:311-449 against :592-733) - quirk Q4.
    With bit depths up to 12 the DST's second stage cannot leave 16 bits: its largest value is 242 * 32768 >> 8 = 30976
    (242 = the largest sum of |weights| over a column of the DST matrix), so that clip never acts - residual() asserts it.
    The DCT's second stage does leave 16 bits at 10 and 12 bit (event "stage2_beyond_int16").

The range-extension residual tools follow behind residual(): implicit RDPCM (unit_residual), cross-component prediction
(cross_component, with LumaCarry for the luma residual of the current transform unit) and PCM (pcm_block); the reference's
deviations there sit behind the switches of Quirks.

The records are those of a command stream in decode order (include/hm_stream.h: hm_tu, 16 bytes)."""
import struct

import numpy as np

LEVEL_SCALE = (40, 45, 51, 57, 64, 72)                       # (8-309)
DST = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)  # (8-320)

# transMatrix (8-321 .. 8-324): the first 16 columns of the 32 rows as the standard prints them; the other 16 follow from
# the symmetry of the cosines (even rows symmetric, odd rows antisymmetric)
_COLS_0_15 = """
64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64
90 90 88 85 82 78 73 67 61 54 46 38 31 22 13 4
90 87 80 70 57 43 25 9 -9 -25 -43 -57 -70 -80 -87 -90
90 82 67 46 22 -4 -31 -54 -73 -85 -90 -88 -78 -61 -38 -13
89 75 50 18 -18 -50 -75 -89 -89 -75 -50 -18 18 50 75 89
88 67 31 -13 -54 -82 -90 -78 -46 -4 38 73 90 85 61 22
87 57 9 -43 -80 -90 -70 -25 25 70 90 80 43 -9 -57 -87
85 46 -13 -67 -90 -73 -22 38 82 88 54 -4 -61 -90 -78 -31
83 36 -36 -83 -83 -36 36 83 83 36 -36 -83 -83 -36 36 83
82 22 -54 -90 -61 13 78 85 31 -46 -90 -67 4 73 88 38
80 9 -70 -87 -25 57 90 43 -43 -90 -57 25 87 70 -9 -80
78 -4 -82 -73 13 85 67 -22 -88 -61 31 90 54 -38 -90 -46
75 -18 -89 -50 50 89 18 -75 -75 18 89 50 -50 -89 -18 75
73 -31 -90 -22 78 67 -38 -90 -13 82 61 -46 -88 -4 85 54
70 -43 -87 9 90 25 -80 -57 57 80 -25 -90 -9 87 43 -70
67 -54 -78 38 85 -22 -90 4 90 13 -88 -31 82 46 -73 -61
64 -64 -64 64 64 -64 -64 64 64 -64 -64 64 64 -64 -64 64
61 -73 -46 82 31 -88 -13 90 -4 -90 22 85 -38 -78 54 67
57 -80 -25 90 -9 -87 43 70 -70 -43 87 9 -90 25 80 -57
54 -85 -4 88 -46 -61 82 13 -90 38 67 -78 -22 90 -31 -73
50 -89 18 75 -75 -18 89 -50 -50 89 -18 -75 75 18 -89 50
46 -90 38 54 -90 31 61 -88 22 67 -85 13 73 -82 4 78
43 -90 57 25 -87 70 9 -80 80 -9 -70 87 -25 -57 90 -43
38 -88 73 -4 -67 90 -46 -31 85 -78 13 61 -90 54 22 -82
36 -83 83 -36 -36 83 -83 36 36 -83 83 -36 -36 83 -83 36
31 -78 90 -61 4 54 -88 82 -38 -22 73 -90 67 -13 -46 85
25 -70 90 -80 43 9 -57 87 -87 57 -9 -43 80 -90 70 -25
22 -61 85 -90 73 -38 -4 46 -78 90 -82 54 -13 -31 67 -88
18 -50 75 -89 89 -75 50 -18 -18 50 -75 89 -89 75 -50 18
13 -38 61 -78 88 -90 85 -73 54 -31 4 22 -46 67 -82 90
9 -25 43 -57 70 -80 87 -90 90 -87 80 -70 57 -43 25 -9
4 -13 22 -31 38 -46 54 -61 67 -73 78 -82 85 -88 90 -90
"""


def _trans_matrix():
    left = np.array([[int(v) for v in line.split()] for line in _COLS_0_15.strip().splitlines()], np.int64)
    assert left.shape == (32, 16)
    sign = np.where(np.arange(32) % 2 == 0, 1, -1)[:, None]
    m = np.concatenate([left, sign * left[:, ::-1]], axis=1)
    # what the table must be: round(64 * sqrt(2) * c(k) cos((2 n + 1) k pi / 64)) up to the standard's hand-tuned entries
    k, n = np.arange(32)[:, None], np.arange(32)[None, :]
    ideal = 64 * np.sqrt(2) * np.where(k == 0, np.sqrt(0.5), 1.0) * np.cos((2 * n + 1) * k * np.pi / 64)
    assert np.abs(m - ideal).max() < 2.0
    return m


TRANS = _trans_matrix()


def wrap32(v):
    """an int64 value as the reference's 32-bit `int` holds it (two's complement)"""
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def clip16(v):
    return np.clip(v, -32768, 32767)


# ---- reading a command stream (decode order: hm_tu) ---------------------------------------------------------------------
PIC_SCALING_LIST, PIC_SPLIT_CHAINS, PIC_TS_ROTATION, PIC_IMPLICIT_RDPCM, PIC_CROSS_COMPONENT = 0x100, 0x1000, 0x2000, 0x4000, 0x10000
PIC_STRONG_INTRA, PIC_NO_INTRA_SMOOTHING = 0x1, 0x8000
TU_CBF, TU_TSKIP, TU_AVAIL_TL, MODE_BYPASS, MODE_PCM = 0x20, 0x40, 0x80, 0x40, 0x80


PIC_TILES, PIC_LF_ACROSS_TILES, PIC_PCMF = 0x40, 0x80, 0x200
CTB_DEBLOCK_LEFT, CTB_DEBLOCK_TOP, CTB_DEBLOCK_OFF = 0x01, 0x02, 0x08
SLICE_DTYPE = np.dtype([("slice_addr", "<u4"), ("beta_offset_div2", "i1"), ("tc_offset_div2", "i1"), ("deblocking_disabled", "u1"), ("sao_luma", "u1"),
                        ("sao_chroma", "u1"), ("lf_across_slices", "u1"), ("slice_qp", "i1"), ("reserved", "u1")])
SAO_DTYPE = np.dtype([("type", "u1"), ("eo_class", "u1"), ("band_position", "u1"), ("offset", "i1", (4,)), ("reserved", "u1")])  # hm_sao: offsets already scaled
CTB_DTYPE = np.dtype(dict(names=["tu_first", "tu_count", "slice_idx", "flags", "sao"], formats=["<u4", "<u2", "<u2", "u1", (SAO_DTYPE, (3,))], offsets=[0, 4, 6, 8, 12],
                          itemsize=52))


def scaling_offset(log2, cidx):  # HM_SCALING_OFFSET
    return {2: 16 * cidx, 3: 48 + 64 * cidx, 4: 240 + 256 * cidx, 5: 1008}[log2]


class Picture:
    """header fields and the records of a blob parsed in decode order"""

    def __init__(self, blob):
        self.blob = blob
        self.width, self.height = struct.unpack_from("<HH", blob, 8)
        self.crop = struct.unpack_from("<4H", blob, 12)
        self.chroma_format, self.bit_depth, self.bit_depth_c, self.log2_ctb, self.log2_min_tb, self.log2_min_cb = struct.unpack_from("<6B", blob, 20)
        self.sao_scale_y, self.sao_scale_c = struct.unpack_from("<2B", blob, 26)  # log2_sao_offset_scale_luma / chroma (hm_sao.offset holds them applied)
        self.ctb_w, self.ctb_h = struct.unpack_from("<HH", blob, 28)
        self.cb_qp_offset, self.cr_qp_offset, self.pcm_loop_filter_disabled = struct.unpack_from("<bbB", blob, 32)
        self.flags = struct.unpack_from("<I", blob, 36)[0]
        assert not self.flags & PIC_SPLIT_CHAINS, "parse with record_order = decode order"
        self.n_slices, self.n_ctbs, self.n_tus, self.n_coeffs = struct.unpack_from("<4I", blob, 0x2C)
        self.off_slices, self.off_ctbs, self.off_tus, self.off_coeffs, self.off_scaling = struct.unpack_from("<5I", blob, 0x3C)
        self.scaling = np.frombuffer(blob, np.uint8, 1008 + 1024, self.off_scaling).astype(np.int64) if self.flags & PIC_SCALING_LIST else None
        self.coeffs = np.frombuffer(blob, np.dtype([("pos", "<u2"), ("value", "<i2")]), self.n_coeffs, self.off_coeffs)

    def slices(self):
        """hm_slice[n_slices] as a structured array"""
        return np.frombuffer(self.blob, SLICE_DTYPE, self.n_slices, self.off_slices)

    def ctbs(self):
        """the fields of hm_ctb[n_ctbs] that the loop filters read, as a structured array"""
        return np.frombuffer(self.blob, CTB_DTYPE, self.n_ctbs, self.off_ctbs)

    def records(self, ctb=None):
        """the records of all CTBs (or of one) in decode order: dicts with the block's position in its plane"""
        sw = 1 if self.chroma_format == 3 else 2
        sh = 2 if self.chroma_format == 1 else 1
        for a in (range(self.n_ctbs) if ctb is None else [ctb]):
            tu_first, tu_count = struct.unpack_from("<IH", self.blob, self.off_ctbs + 52 * a)
            for t in range(tu_first, tu_first + tu_count):
                x, y, info, pm, qp, qpy, n, first, a_l, a_bl, a_t, a_tr = struct.unpack_from("<BBBBBbHI4B", self.blob, self.off_tus + 16 * t)
                cidx = (info >> 3) & 3
                cx, cy = (a % self.ctb_w) << self.log2_ctb, (a // self.ctb_w) << self.log2_ctb
                if cidx:
                    cx, cy = cx // sw, cy // sh
                yield dict(x=cx + x, y=cy + y, log2=info & 7, cidx=cidx, cbf=bool(info & TU_CBF), tskip=bool(info & TU_TSKIP),
                           mode=pm & 0x3F, bypass=bool(pm & MODE_BYPASS), pcm=bool(pm & MODE_PCM), qp=qp, qpy=qpy,
                           levels=self.coeffs[first:first + n], avail_left=a_l, avail_bottom_left=a_bl, avail_top=a_t, avail_top_right=a_tr,
                           avail_tl=bool(info & TU_AVAIL_TL))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def dequantise(rec, bit_depth, scaling, events):
    """TransCoeffLevel -> d (8.6.4.1 with the reference's integer widths): an nT x nT int64 array, d[y, x]"""
    nT, log2 = 1 << rec["log2"], rec["log2"]
    pos = rec["levels"]["pos"].astype(np.int64)
    level = rec["levels"]["value"].astype(np.int64)
    qP = rec["qp"]
    scale = LEVEL_SCALE[qP % 6] << (qP // 6)
    if scaling is None:
        # m = 16 folded into the shift: bdShift - 4 (transform.cc:486-506)
        bd_shift = bit_depth + log2 - 5 - 4
        exact = level * scale + (1 << (bd_shift - 1))
        prod = wrap32(exact)                       # Q3: the reference's int
        events["wrap"] = bool((prod != exact).any())
        v = prod >> bd_shift
    else:
        bd_shift = bit_depth + log2 - 5
        m = scaling[scaling_offset(log2, rec["cidx"]) + pos]
        fact = wrap32(m * LEVEL_SCALE[qP % 6] << (qP // 6))  # (an int in the reference; at most 255 * 72 << 12 < 2^31)
        v = (level * fact + (1 << (bd_shift - 1))) >> bd_shift
        events["wrap"] = False
    events["clip_hi"] = bool((v > 32767).any())
    events["clip_lo"] = bool((v < -32768).any())
    d = np.zeros(nT * nT, np.int64)
    d[pos] = clip16(v)
    return d.reshape(nT, nT)


def residual(rec, bit_depth, scaling=None, pic_flags=0):
    """(residual[y, x] as int64, events) of a record with a residual.  Not for implicit-RDPCM blocks (unit_residual), PCM
    (pcm_block) or the cross-component term of a chroma block (cross_component)."""
    assert rec["cbf"] and not rec["pcm"]
    nT, log2 = 1 << rec["log2"], rec["log2"]
    pos = rec["levels"]["pos"].astype(np.int64)
    ev = dict(wrap=False, clip_hi=False, clip_lo=False, stage1_clip=False, stage2_beyond_int16=False, kind="")
    ev["dc_only"] = bool(len(pos) and (pos == 0).all())
    ev["top_left_only"] = bool(len(pos) and ((pos % nT < 4) & (pos // nT < 4)).all())
    ev["last_group"] = bool(((pos % nT >= nT - 4)).any() and ((pos // nT >= nT - 4)).any())
    rotate = bool(pic_flags & PIC_TS_ROTATION) and nT == 4
    if rec["bypass"]:  # 8.6.2: the levels are the residual
        ev["kind"] = "bypass"
        r = np.zeros(nT * nT, np.int64)
        r[pos] = rec["levels"]["value"].astype(np.int64)
        r = r.reshape(nT, nT)
        return (r[::-1, ::-1] if rotate else r), ev
    d = dequantise(rec, bit_depth, scaling, ev)
    bd_shift = 20 - bit_depth
    if rec["tskip"]:  # 8.6.4.2: r = rotated d << tsShift, tsShift = 5 + log2 (extended_precision_processing off)
        ev["kind"] = "tskip"
        if rotate:
            d = d[::-1, ::-1]
        r = wrap32(d << (5 + log2))  # (|d| << 10 stays far inside 32 bits: written for completeness)
        r = (r + (1 << (bd_shift - 1))) >> bd_shift
        return r, ev
    if nT == 4 and rec["cidx"] == 0:
        ev["kind"] = "dst"
        M = DST
    else:
        ev["kind"] = "dct"
        M = TRANS[np.arange(nT) * (32 // nT)][:, :nT]  # rows 0, 32 / nT, ...: the nT-point matrix (8.6.4.2)
    # stage 1, columns: e[y, x] = sum_j M[j, y] d[j, x]; g = Clip3(coeffMin, coeffMax, (e + 64) >> 7)
    e = M.T @ d
    g = (e + 64) >> 7
    ev["stage1_clip"] = bool(((g > 32767) | (g < -32768)).any())
    g = clip16(g)
    # stage 2, rows: r[y, x] = sum_j M[j, x] g[y, j]; (r + (1 << (bdShift - 1))) >> bdShift
    r = ((g @ M) + (1 << (bd_shift - 1))) >> bd_shift
    beyond = bool(((r > 32767) | (r < -32768)).any())
    if ev["kind"] == "dst":
        assert not beyond, "the DST's second stage left 16 bits: impossible up to 12 bit (see the module's text)"
        r = clip16(r)  # Q4 (never acts)
    else:
        ev["stage2_beyond_int16"] = beyond
    return r, ev


# ---- the range-extension residual tools: implicit RDPCM, cross-component prediction, PCM ------------------------------------
# Written from 7.3.8.12, 8.6.2, 8.6.6, 8.6.8 and 8.4.4.1 of the standard (v2 and later) and, where the reference does something
# else, from its scalar code (transform.cc:251-285, 427-466, 566-643; fallback-dct.cc:173-299; slice.cc:3774-3805, 4462-4504).
#
# Which inverse transforms the reference takes in a cross-component picture: ALL blocks that are neither skipped nor bypassed,
# luma and chroma alike, go through its "explicit" variants (transform.cc:658-663 -> 288-336: transform_idst_4x4 /
# transform_idct_NxN into an int32 buffer, fallback-dct.cc:511-550, 737-878).  They clip the first stage to 16 bits like the
# adding variants and leave the second stage unclipped - for the DCT that is what residual() does anyway (Q4), for the DST the
# missing clip is one that never acts (residual() asserts it), so residual() restates both.
class Quirks:
    """the reference's deviations from the standard's unbounded integers in these tools, each behind a switch (all on: the
    reference).
      res16            8-bit 4x4 transform-skip residuals - the block's own values, its RDPCM run sums and, for chroma, the sum
                       with the cross-component term - are stored through int16 (transform.cc:577-607: residual_luma16,
                       rdpcm_h16 / rdpcm_v16, cross_comp_pred16)
      shift_pair_int32 (rY << BitDepthC) >> BitDepthY is taken in a 32-bit int (transform.cc:264-265): it wraps for
                       |rY| >= 2^(31 - BitDepthC)"""

    def __init__(self, res16=True, shift_pair_int32=True):
        self.res16, self.shift_pair_int32 = res16, shift_pair_int32


REFERENCE = Quirks()
RES_SCALE_VALUES = (-8, -4, -2, -1, 1, 2, 4, 8)  # 7.4.9.12: (1 << (log2_res_scale_abs_plus1 - 1)) * (1 - 2 * sign)


def int16_store(v):
    """an int64 value as an int16_t holds it"""
    return ((np.asarray(v, np.int64) + 32768) & 0xFFFF) - 32768


def bypass_unit_of_rdpcm_picture(rec, pic_flags):
    """implicit_rdpcm_enabled_flag && cu_transquant_bypass_flag: the ONE flag that both turns the levels of a mode 10 / 26 block
    into run sums (8.6.2) and suppresses the boundary filters of those two modes (8.4.4.2.6: disableIntraBoundaryFilter;
    intrapred.cc:323-326) - intra_ref.predict reads it here"""
    return bool(pic_flags & PIC_IMPLICIT_RDPCM) and rec["bypass"]


def rdpcm_direction(rec, pic_flags):
    """None, "h" (mode 10: along rows) or "v" (mode 26: along columns) - slice.cc:3774-3779; intra pictures: implicit only"""
    if not rec["cbf"] or rec["pcm"] or rec["mode"] not in (10, 26):
        return None
    if bypass_unit_of_rdpcm_picture(rec, pic_flags) or (bool(pic_flags & PIC_IMPLICIT_RDPCM) and rec["tskip"]):
        return "v" if rec["mode"] == 26 else "h"
    return None


def unit_residual(rec, bit_depth, scaling=None, pic_flags=0, quirks=REFERENCE):
    """(the block's OWN residual [y, x] as int64 - before any cross-component term -, events) of a record with levels, implicit
    RDPCM included.  events beyond those of residual(): rdpcm (None / "h" / "v"), rotated (the 4x4 rotation acted on this
    block), run_beyond_int16 (an RDPCM run sum left -32768 .. 32767), res16 (the block takes the reference's 16-bit arm),
    res16_acts (the int16 store changed a value)."""
    assert rec["cbf"] and not rec["pcm"]
    nT, log2 = 1 << rec["log2"], rec["log2"]
    direction = rdpcm_direction(rec, pic_flags)
    skipping = rec["bypass"] or rec["tskip"]
    if direction is None:
        r, ev = residual(rec, bit_depth, scaling, pic_flags)
    else:
        # 8.6.2 / 8.6.6 + 8.6.8: the rotation acts on the array of levels / scaled coefficients FIRST (transform.cc:446-448,
        # 574-576), a transform-skip element is rounded on its own, ((d << tsShift) + rnd) >> bdShift, and only then do the
        # elements accumulate along the direction of the prediction (fallback-dct.cc:173-255)
        pos = rec["levels"]["pos"].astype(np.int64)
        ev = dict(wrap=False, clip_hi=False, clip_lo=False, stage1_clip=False, stage2_beyond_int16=False)
        ev["dc_only"] = bool(len(pos) and (pos == 0).all())
        ev["top_left_only"] = bool(len(pos) and ((pos % nT < 4) & (pos // nT < 4)).all())
        ev["last_group"] = bool(((pos % nT >= nT - 4)).any() and ((pos // nT >= nT - 4)).any())
        if rec["bypass"]:
            ev["kind"] = "bypass"
            e = np.zeros(nT * nT, np.int64)
            e[pos] = rec["levels"]["value"].astype(np.int64)
            e = e.reshape(nT, nT)
        else:
            ev["kind"] = "tskip"
            e = dequantise(rec, bit_depth, scaling, ev)
        if (pic_flags & PIC_TS_ROTATION) and nT == 4:
            e = e[::-1, ::-1]
        if not rec["bypass"]:
            bd_shift = 20 - bit_depth
            e = (wrap32(e << (5 + log2)) + (1 << (bd_shift - 1))) >> bd_shift
        r = np.cumsum(e, axis=1 if direction == "h" else 0)
    ev["rdpcm"] = direction
    ev["rotated"] = bool(skipping and (pic_flags & PIC_TS_ROTATION) and nT == 4)
    ev["run_beyond_int16"] = bool(direction is not None and ((r > 32767) | (r < -32768)).any())
    ev["res16"] = bool(rec["tskip"] and not rec["bypass"] and bit_depth == 8 and nT == 4)
    ev["res16_acts"] = False
    if ev["res16"] and quirks.res16:
        t = int16_store(r)
        ev["res16_acts"] = bool((t != r).any())
        r = t
    return r, ev


def luma_kind(ev):
    """the kind of a luma block as the census of the cross-component term names it"""
    return ev["kind"] + ("_rdpcm" if ev["rdpcm"] else "")


def cross_component(own, own_ev, r_luma, scale, bit_depth_y, bit_depth_c, quirks=REFERENCE):
    """7.3.8.12 / 8.6.6: (own + ((ResScaleVal * ((rY << BitDepthC) >> BitDepthY)) >> 3), events).  own: the chroma block's own
    residual, or None for a block without levels (slice.cc:3797-3805: the term alone); own_ev: its events or None.  The shift pair
    is the reference's int32 one (quirk shift_pair_int32); >> 3 is an arithmetic shift: it rounds a negative product towards minus
    infinity.  Events: scale, neg_odd (the >> 3 acted on a negative product that is no multiple of 8: a division would round
    otherwise), wrap (the shift pair wrapped), res16_acts (the 16-bit arm's store of the sum changed a value)."""
    assert scale in RES_SCALE_VALUES
    r_luma = np.asarray(r_luma, np.int64)
    exact = (r_luma << bit_depth_c) >> bit_depth_y
    taken = (wrap32(r_luma << bit_depth_c) >> bit_depth_y) if quirks.shift_pair_int32 else exact
    prod = scale * taken
    term = prod >> 3
    ev = dict(scale=scale, neg_odd=bool(((prod < 0) & (prod & 7 != 0)).any()), wrap=bool((wrap32(r_luma << bit_depth_c) != (r_luma << bit_depth_c)).any()),
              res16_acts=False)
    r = term if own is None else own + term
    if own_ev is not None and own_ev["res16"] and quirks.res16:  # cross_comp_pred16: the sum goes back into the int16 buffer
        t = int16_store(r)
        ev["res16_acts"] = bool((t != r).any())
        r = t
    return r, ev


class LumaCarry:
    """tctx->residual_luma while a picture's records are walked in decode order: the residual of the luma block of the current
    transform unit.  In 4:4:4 - the one format with cross-component prediction - the chroma records of a unit follow its luma record
    and have its position and size."""

    def __init__(self):
        self.rec = self.r = self.ev = None

    def keep(self, rec, r, ev):
        """after a luma record: r / ev of unit_residual, or None where the block has no levels"""
        self.rec, self.r, self.ev = rec, r, ev

    def luma_of(self, rec):
        """(residual, events) of the luma block under a chroma record with a non-zero ResScaleVal; asserts what the syntax
        promises: 7.3.8.12 sends a scale only behind a luma block with cbf_luma, and never (the product's parser refuses it, Q17)
        behind an 8-bit 4x4 transform-skip luma block, whose residual the reference keeps in another buffer (transform.cc:581)"""
        L = self.rec
        assert L is not None and L["cidx"] == 0 and (L["x"], L["y"], L["log2"]) == (rec["x"], rec["y"], rec["log2"]), "a scale without its luma block"
        assert L["cbf"] and self.r is not None, "a scale behind a luma block without cbf (7.3.8.12)"
        assert not self.ev["res16"], "Q17: a scale behind an 8-bit 4x4 transform-skip luma block"
        return self.r, self.ev


def pcm_block(rec, bit_depth, pcm_bits=None):
    """8.4.4.1 (v2+: 8.4.4.1 "decoding process for PCM samples"): recSamples = pcm_sample << (BitDepth - PcmBitDepth), nT x nT in
    raster order.  The record holds the shifted values; with pcm_bits known the shift is restated: every value is a multiple of
    1 << shift and at most ((1 << pcm_bits) - 1) << shift.  (samples [y, x] as int64, events)"""
    assert rec["pcm"]
    nT = 1 << rec["log2"]
    assert len(rec["levels"]) == nT * nT and (rec["levels"]["pos"] == np.arange(nT * nT)).all()
    v = rec["levels"]["value"].astype(np.int64).reshape(nT, nT)
    assert v.min() >= 0 and v.max() < (1 << bit_depth)
    ev = dict(size=nT, zero=bool((v == 0).any()), top=False, shift=None)
    if pcm_bits is not None:
        assert 1 <= pcm_bits <= bit_depth
        shift = bit_depth - pcm_bits
        top = ((1 << pcm_bits) - 1) << shift
        assert (v % (1 << shift) == 0).all() and v.max() <= top, "PCM samples: not pcm_sample << (BitDepth - PcmBitDepth)"
        ev.update(top=bool((v == top).any()), shift=shift)
    return v, ev
