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

Not restated here (the sweep against the reference decoder holds them): implicit RDPCM, cross-component prediction, PCM.

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
    """(residual[y, x] as int64, events) of a record with a residual.  Not for implicit-RDPCM blocks, PCM or chroma blocks
    with a cross-component term."""
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
