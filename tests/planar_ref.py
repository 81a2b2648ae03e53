"""planar_ref.py - TEST INFRASTRUCTURE: the reference's conversion to a planar YCbCr target, restated in numpy.

Every operation a planar chain can hold is restated from the reference's source (file:line per function) on numpy arrays -
float32 arrays with one IEEE operation per step, integer arithmetic in int32 - or taken from the oracle where the oracle
already has it (bilinear up-sampling, the depth changes).  The chain to run comes from oracle/pipeline_search.py, never from
the product.  Planes are plain 2-D arrays (uint8, or uint16 for more than 8 bits) of exactly the plane's size.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pipeline_search as ps  # noqa: E402

import orc  # noqa: E402

F = np.float32
HM_OUT_YCBCR = {1: 0x101, 2: 0x102, 3: 0x103}
HM_OUT_YCBCR_8BIT = 0x200

# the operations hm_colour_convert_planar runs (the issue's section 2)
INSIDE = {
    "Op_YCbCr_to_RGB<uint8_t>", "Op_YCbCr_to_RGB<uint16_t>", "Op_RGB_to_YCbCr<uint8_t>", "Op_RGB_to_YCbCr<uint16_t>", "Op_mono_to_YCbCr420",
    "Op_to_sdr_planes", "Op_to_hdr_planes", "Op_drop_alpha_plane",
    "Op_YCbCr420_bilinear_to_YCbCr444<uint8_t>", "Op_YCbCr420_bilinear_to_YCbCr444<uint16_t>",
    "Op_YCbCr422_bilinear_to_YCbCr444<uint8_t>", "Op_YCbCr422_bilinear_to_YCbCr444<uint16_t>",
    "Op_YCbCr444_to_YCbCr420_average<uint8_t>", "Op_YCbCr444_to_YCbCr420_average<uint16_t>",
    "Op_YCbCr444_to_YCbCr422_average<uint8_t>", "Op_YCbCr444_to_YCbCr422_average<uint16_t>",
}


def chain_for(chroma, has_alpha, bits, nclx, target_chroma, hdr8=False, forced_bilinear=False, target_colorspace=ps.CS_YCBCR):
    """nclx: None or (matrix, primaries, transfer, full_range) -> list of op names, [] or None (no chain)"""
    n = ps.Nclx(nclx[0], nclx[1], nclx[2], bool(nclx[3])) if nclx else None
    opts = ps.Options(ps.DOWN_AVERAGE, ps.UP_BILINEAR, bool(forced_bilinear))
    return ps.chain(ps.CS_MONO if chroma == 0 else ps.CS_YCBCR, chroma, bool(has_alpha), bits, n, target_colorspace, target_chroma,
                    8 if hdr8 else 0, opts)


def chroma_size(chroma, w, h):
    return (w if chroma == 3 else (w + 1) // 2), ((h + 1) // 2 if chroma == 1 else h)


def dtype_of(bits):
    return np.uint16 if bits > 8 else np.uint8


def clip_f_u16(fx, maxi):
    """common_utils.h:64-70: (long)(fx + 0.5f), clamped"""
    x = (fx.astype(F) + F(0.5)).astype(np.int64)  # the conversion truncates toward zero
    return np.clip(x, 0, maxi)


def kr_kb(matrix):
    """nclx.cc:85-138 for the matrices that do not derive from the primaries"""
    table = {1: (0.2126, 0.0722), 4: (0.30, 0.11), 5: (0.299, 0.114), 6: (0.299, 0.114), 7: (0.212, 0.087), 9: (0.2627, 0.0593), 10: (0.2627, 0.0593)}
    assert matrix not in (12, 13)
    kr, kb = table.get(matrix, (0.0, 0.0))
    return F(kr), F(kb)


def ycbcr_to_rgb_coefficients(has_nclx, matrix):
    """nclx.cc:141-171 -> r_cr, g_cb, g_cr, b_cb"""
    d = (F(1.402), F(-0.344136), F(-0.714136), F(1.772))
    if not has_nclx:
        return d
    kr, kb = kr_kb(matrix)
    if kr == 0 and kb == 0:
        return d
    one, two = F(1), F(2)
    return (two * (-kr + one), two * kb * (-kb + one) / (kb + kr - one), two * kr * (-kr + one) / (kb + kr - one), two * (-kb + one))


def rgb_to_ycbcr_coefficients(matrix):
    """nclx.cc:175-218 -> 3 x 3"""
    kr, kb = kr_kb(matrix)
    if kr == 0 and kb == 0:
        return [[F(0.299), F(0.587), F(0.114)], [F(-0.168735), F(-0.331264), F(0.5)], [F(0.5), F(-0.418688), F(-0.081312)]]
    one, two = F(1), F(2)
    return [[kr, one - kr - kb, kb],
            [-kr / (one - kb) / two, -(one - kr - kb) / (one - kb) / two, F(0.5)],
            [F(0.5), -(one - kr - kb) / (one - kr) / two, -kb / (one - kr) / two]]


def op_ycbcr_to_rgb(y, cb, cr, bits, chroma, seen):
    """Op_YCbCr_to_RGB<Pixel> (yuv2rgb.cc:79-254).  seen = (has_nclx, matrix, primaries, full_range) of the image the op is
    handed.  Chroma is read nearest neighbour: cx = x >> shiftH, cy = y >> shiftV (:200-203)."""
    h, w = y.shape
    half, full_max, off = 1 << (bits - 1), (1 << bits) - 1, F(16 << (bits - 8))
    ys, xs = np.arange(h) >> (1 if chroma == 1 else 0), np.arange(w) >> (0 if chroma == 3 else 1)
    u, v = cb[np.ix_(ys, xs)], cr[np.ix_(ys, xs)]
    matrix, full_range = (seen[1], bool(seen[3])) if seen[0] else (2, True)
    dt = dtype_of(bits)
    if matrix == 0:
        if full_range:
            return v.astype(dt), y.astype(dt), u.astype(dt)
        conv = lambda p, k: clip_f_u16((p.astype(F) - off) * F(k), full_max).astype(dt)  # noqa: E731
        return conv(v, 1.1429), conv(y, 1.1689), conv(u, 1.1429)
    if matrix == 8:
        yv, c1, c2 = y.astype(np.int32), u.astype(np.int32) - half, v.astype(np.int32) - half
        c8 = lambda a: np.clip(a, 0, 255).astype(dt)  # noqa: E731
        return c8(yv - c1 + c2), c8(yv + c1), c8(yv - c1 - c2)
    r_cr, g_cb, g_cr, b_cb = ycbcr_to_rgb_coefficients(seen[0], matrix)
    yv = y.astype(F)
    fcb = (u.astype(np.int32) - half).astype(F)
    fcr = (v.astype(np.int32) - half).astype(F)
    if not full_range:
        yv = (yv - off) * F(1.1689)
        fcb = fcb * F(1.1429)
        fcr = fcr * F(1.1429)
    r = clip_f_u16(yv + r_cr * fcr, full_max)
    g = clip_f_u16((yv + g_cb * fcb) + g_cr * fcr, full_max)
    b = clip_f_u16(yv + b_cb * fcb, full_max)
    return r.astype(dt), g.astype(dt), b.astype(dt)


def op_rgb_to_ycbcr(r, g, b, bits, target_chroma, target):
    """Op_RGB_to_YCbCr<Pixel> (rgb2yuv.cc:88-275).  target = (matrix, primaries, full_range) of the TARGET state (:175-180)."""
    h, w = r.shape
    matrix, full_range = target[0], bool(target[2])
    half, full_max, off = F(1 << (bits - 1)), (1 << bits) - 1, F(16 << (bits - 8))
    dt = dtype_of(bits)
    sub_h, sub_v = (1 if target_chroma == 3 else 2), (2 if target_chroma == 1 else 1)
    xs, ys = np.arange(0, w, sub_h), np.arange(0, h, sub_v)
    c = rgb_to_ycbcr_coefficients(matrix)
    fr, fg, fb = r.astype(F), g.astype(F), b.astype(F)
    if matrix == 0:  # :196-203, 222-230: G is luma; chroma takes the box's top-left sample, no averaging
        if full_range:
            return g.astype(dt), b[np.ix_(ys, xs)].astype(dt), r[np.ix_(ys, xs)].astype(dt)
        yo = clip_f_u16(((fg * F(219.0)) / F(256)) + off, full_max)
        cbo = clip_f_u16(((fb[np.ix_(ys, xs)] * F(224.0)) / F(256)) + off, full_max)
        cro = clip_f_u16(((fr[np.ix_(ys, xs)] * F(224.0)) / F(256)) + off, full_max)
        return yo.astype(dt), cbo.astype(dt), cro.astype(dt)
    v = (fr * c[0][0] + fg * c[0][1]) + fb * c[0][2]
    if not full_range:
        v = ((v * F(219)) / F(256)) + off
    yo = clip_f_u16(v, full_max)
    ar, ag, ab = fr[np.ix_(ys, xs)], fg[np.ix_(ys, xs)], fb[np.ix_(ys, xs)]
    if sub_h > 1 or sub_v > 1:  # :236-256: x2 only moves for 4:2:0 ("do not center for 4:2:2"), y2 only for 4:2:0
        x2 = np.where((xs + 1 < w) & (sub_h == 2) & (sub_v == 2), xs + 1, xs)
        y2 = np.where((ys + 1 < h) & (sub_v == 2), ys + 1, ys)

        def box(p):
            a = p[np.ix_(ys, xs)]
            a = a + p[np.ix_(ys, x2)]
            a = a + p[np.ix_(y2, xs)]
            a = a + p[np.ix_(y2, x2)]
            return a * F(0.25)
        ar, ag, ab = box(fr), box(fg), box(fb)
    fcb = (ar * c[1][0] + ag * c[1][1]) + ab * c[1][2]
    fcr = (ar * c[2][0] + ag * c[2][1]) + ab * c[2][2]
    if not full_range:
        fcb = (fcb * F(224)) / F(256)
        fcr = (fcr * F(224)) / F(256)
    return yo.astype(dt), clip_f_u16(fcb + half, full_max).astype(dt), clip_f_u16(fcr + half, full_max).astype(dt)


def op_average_420(p):
    """Op_YCbCr444_to_YCbCr420_average on one chroma plane (chroma_sampling.cc:172-221)"""
    h, w = p.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    s = p.astype(np.int32)
    out = np.zeros((ch, cw), np.int32)
    he, we = h & ~1, w & ~1
    out[:he // 2, :we // 2] = (s[0:he:2, 0:we:2] + s[0:he:2, 1:we:2] + s[1:he:2, 0:we:2] + s[1:he:2, 1:we:2] + 2) // 4
    if h & 1:
        out[ch - 1, :we // 2] = (s[h - 1, 0:we:2] + s[h - 1, 1:we:2] + 1) // 2
    if w & 1:
        out[:he // 2, cw - 1] = (s[0:he:2, w - 1] + s[1:he:2, w - 1] + 1) // 2
    if (w & 1) and (h & 1):
        out[ch - 1, cw - 1] = s[h - 1, w - 1]
    return out.astype(p.dtype)


def op_average_422(p):
    """Op_YCbCr444_to_YCbCr422_average on one chroma plane (chroma_sampling.cc:396-420) -> (plane, undefined): with an odd
    width the border loop runs to height - 1 only, so the last sample of the last row is never written (undefined = its
    (row, column), else None); the copied sample stands there in this restatement."""
    h, w = p.shape
    cw = (w + 1) // 2
    s = p.astype(np.int32)
    out = np.zeros((h, cw), np.int32)
    we = w & ~1
    out[:, :we // 2] = (s[:, 0:we:2] + s[:, 1:we:2] + 1) // 2
    undefined = None
    if w & 1:
        out[:, cw - 1] = s[:, w - 1]
        undefined = (h - 1, cw - 1)
    return out.astype(p.dtype), undefined


def _padded(p):
    """2-D array -> libheif-style (buffer, stride) for the oracle's plane functions"""
    h, w = p.shape
    bps = p.dtype.itemsize
    buf, stride = orc.alloc_plane(w, h, bps)
    buf[:h, :w * bps] = np.ascontiguousarray(p).view(np.uint8).reshape(h, w * bps)
    return buf, stride


def _unpadded(plane, w, h, bits):
    buf, _ = plane
    bps = 2 if bits > 8 else 1
    return np.ascontiguousarray(buf[:h, :w * bps]).view(dtype_of(bits)).reshape(h, w).copy()


def op_bilinear(p, w, h, bits, chroma):
    return _unpadded(orc.upsample_bilinear(_padded(p), w, h, bits, chroma), w, h, bits)


def op_to_sdr(p, bits):
    h, w = p.shape
    return _unpadded(orc.to_sdr(_padded(p), w, h, bits), w, h, 8)


def op_to_hdr(p, bits):
    h, w = p.shape
    return _unpadded(orc.to_hdr(_padded(p), w, h, bits), w, h, bits)


def run_chain(chain, planes, bits, chroma, nclx, target_chroma, target_bits, forced_bilinear=False):
    """planes: {"y", "cb", "cr", "a"} (cb / cr absent for 4:0:0, "a" optional, of the picture's depth); nclx: None or (matrix,
    primaries, transfer, full_range).  -> (planes, bits, chroma, undefined) with undefined = [(plane name, row, column)] the
    reference leaves unwritten.  forced_bilinear: the request's only_use_preferred_chroma_algorithm."""
    P = dict(planes)
    h, w = P["y"].shape
    seen = (1, nclx[0], nclx[1], nclx[3]) if nclx else (0, 0, 0, 0)
    m, pr = (nclx[0], nclx[1]) if nclx else (2, 2)
    state = (1, 6 if m == 2 else m, 1 if pr == 2 else pr, nclx[3] if nclx else 1)
    target = (state[1], state[2], state[3])
    undefined = []
    for name in chain:
        if name == "Op_drop_alpha_plane":
            P.pop("a", None)
        elif name == "Op_mono_to_YCbCr420":  # monochrome.cc:52-156
            cw, ch = chroma_size(1, w, h)
            P["cb"] = np.full((ch, cw), 128 << (bits - 8), dtype_of(bits))
            P["cr"] = P["cb"].copy()
            chroma = 1
            state = (1, 6, 1, 1)
        elif name == "Op_to_sdr_planes":  # hdr_sdr.cc:138-200: every plane, alpha included
            P = {k: op_to_sdr(v, bits) for k, v in P.items()}
            bits = 8
        elif name == "Op_to_hdr_planes":  # hdr_sdr.cc:52-105
            P = {k: op_to_hdr(v, target_bits) for k, v in P.items()}
            bits = target_bits
        elif "bilinear_to_YCbCr444" in name:
            P["cb"], P["cr"] = op_bilinear(P["cb"], w, h, bits, chroma), op_bilinear(P["cr"], w, h, bits, chroma)
            chroma = 3
        elif "to_YCbCr420_average" in name:
            P["cb"], P["cr"] = op_average_420(P["cb"]), op_average_420(P["cr"])
            chroma = 1
        elif "to_YCbCr422_average" in name:
            (P["cb"], u), (P["cr"], _) = op_average_422(P["cb"]), op_average_422(P["cr"])
            if u:
                undefined += [("cb",) + u, ("cr",) + u]
            chroma = 2
        elif name.startswith("Op_YCbCr_to_RGB<"):
            P["y"], P["cb"], P["cr"] = op_ycbcr_to_rgb(P["y"], P["cb"], P["cr"], bits, chroma, seen)  # (R, G, B under the names y, cb, cr)
            chroma = 3
        elif name.startswith("Op_RGB_to_YCbCr<"):
            # the op's target is its STEP's output state (colorconversion.cc:447): with only_use_preferred_chroma_algorithm it
            # stays at 4:4:4 (rgb2yuv.cc:62-77) and the averaging op follows
            chroma = 3 if forced_bilinear else target_chroma
            P["y"], P["cb"], P["cr"] = op_rgb_to_ycbcr(P["y"], P["cb"], P["cr"], bits, chroma, target)
        else:
            raise AssertionError(f"operation outside the planar set: {name}")
        seen = state
    return P, bits, chroma, undefined
