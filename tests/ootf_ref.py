"""numpy model of the OOTF step (hm_device_ootf, include/heif_mi355x.h) on top of light_ref / tone_ref / alpha_ref, written from the
header's text and Rec. ITU-R BT.2100: the system gamma of Table 5 (notes 5e and 5f), the HLG inverse OETF, the two tables in float64
with the C library's functions (Python's math module calls them), rounded once to float32, the luminance weights from the H.273
chromaticities, and the step itself in float32 with every operation rounded on its own - the scene luminance in FRONT of the gamut
matrix, its 10-bit HLG code by a count of thresholds, one common factor per pixel.  finish() is tone_ref.finish with the step in
front of the matrix."""
import math

import numpy as np

import light_ref
import tone_ref

F = np.float32
STEPS = 1024
TOP = float(STEPS - 1)


def gamma(display_peak, gamma_arg=0.0):
    """the system gamma, float64: gamma_arg as it is when non-zero, else BT.2100 Table 5 note 5e inside 400 .. 2000 cd/m2, note 5f outside"""
    L, g = float(F(display_peak)), float(F(gamma_arg))
    if g != 0.0:
        return g
    if 400.0 <= L <= 2000.0:
        return 1.2 + 0.42 * math.log10(L / 1000.0)
    return 1.2 * math.pow(1.111, math.log2(L / 1000.0))


def hlg(e):
    """F of transfer 18, the inverse OETF: code value e in [0, 1] -> scene light, float64"""
    a = 0.17883277
    b = 1.0 - 4.0 * a
    c = 0.5 - a * math.log(4.0 * a)
    return e * e / 3.0 if e <= 0.5 else (math.exp((e - c) / a) + b) / 12.0


def tables(gain, display_peak, gamma_arg=0.0):
    """(thr, sg) as the kernels hold them, float32: thr[0] = 0, thr[i] = (float)(g F((i - 0.5) / 1023)); sg[k] = (float)pow(F(k / 1023),
    gamma - 1), sg[0] = sg[1]"""
    g, gm = float(F(gain)), gamma(display_peak, gamma_arg)
    thr = np.array([0.0] + [g * hlg((i - 0.5) / TOP) for i in range(1, STEPS)], np.float64).astype(F)
    sg = np.array([0.0] + [math.pow(hlg(k / TOP), gm - 1.0) for k in range(1, STEPS)], np.float64).astype(F)
    sg[0] = sg[1]
    return thr, sg


def luma(primaries):
    """the Y row of the primaries' RGB -> XYZ matrix, each entry rounded once to float32"""
    return light_ref.to_xyz(primaries)[1].astype(F)


def step(y, thr, sg, r):
    """the step on linear scene light r (.. x 3, float32) -> (r', k)"""
    assert r.dtype == F and thr.dtype == F and sg.dtype == F and y.dtype == F
    ys = (y[0] * r[..., 0] + y[1] * r[..., 1]) + y[2] * r[..., 2]
    assert ys.dtype == F
    k = np.searchsorted(thr[1:], ys, side="right").astype(np.int64)
    k[np.isnan(ys)] = 0
    out = r * sg[k][..., None]
    assert out.dtype == F
    return out, k


def finish(r, alpha, resampled, enc, m, ootf, tone, dtype, scale, bias):
    """tone_ref.finish with the OOTF step - ootf: (y, thr, sg), or None - in front of the matrix"""
    if ootf is not None:
        r = step(ootf[0], ootf[1], ootf[2], r)[0]
    return tone_ref.finish(r, alpha, resampled, enc, m, tone, dtype, scale, bias)


def render_alpha(pixels, bits, mode, background, view, taps, dtype, scale, bias, lin, enc, m, ootf, tone):
    """alpha_ref.render beside a light step, with the OOTF step on the alpha step's r_c; returns the destination's values and r_c"""
    import alpha_ref
    import view_filters_ref
    x, S, Sa, moved_alpha, summed = alpha_ref.sums(pixels, bits, lin, view, taps)
    b = [lin[v] for v in background] if mode == alpha_ref.MATTE else None
    r = alpha_ref.rule(mode, x, S, Sa, summed, float((1 << bits) - 1), b)
    integer = dtype in (np.uint8, np.uint16)
    sc, bi = np.asarray(scale, F), np.asarray(bias, F)
    none = np.zeros(r.shape[:2] + (0,), F)
    colour = finish(r, none, summed, enc, m, ootf, tone, F if not integer else dtype, scale, bias)
    if mode != alpha_ref.MATTE:
        if summed:
            a_out = view_filters_ref.to_integer(Sa, 255 if dtype == np.uint8 else 65535) if integer else Sa * sc[3] + bi[3]
        else:
            a_out = moved_alpha.astype(np.int64) if integer else moved_alpha.astype(F) * sc[3] + bi[3]
        colour = np.concatenate([colour, a_out[..., None]], axis=2)
    with np.errstate(over="ignore"):
        return colour.astype(dtype), r


def arms(y, thr, r):
    """the census of k: pixels with k == 0, 1 <= k <= 511 (the square-law part), 512 <= k <= 1022, k == 1023"""
    k = step(y, thr, np.ones(STEPS, F), r)[1]
    return int((k == 0).sum()), int(((k >= 1) & (k <= 511)).sum()), int(((k >= 512) & (k <= 1022)).sum()), int((k == 1023).sum())
