"""numpy model of the tone step (hm_device_tone, include/heif_mi355x.h) on top of light_ref, written from the formulas of Report
ITU-R BT.2390 (the EETF, both black levels at 0: no black lift) and SMPTE ST 2084: the two tables in float64, rounded once to
float32, and the step itself in float32 with every operation rounded on its own - the norm max(R, G, B) behind the gamut matrix, its
11-bit PQ code by a count of thresholds, one common factor per pixel.  finish() is light_ref.finish with the step between the
matrix and the finish, and with the 8-bit finish (the codes of an 8-bit threshold table whatever the depth of the samples)."""
import numpy as np

import light_ref

F = np.float32
STEPS = 2048
TOP = float(STEPS - 1)


def eotf(e):
    """ST 2084: code value e in [0, 1] -> light, 1.0 = 10000 cd/m2"""
    return light_ref.to_light(16, e)


def pq(y):
    """the inverse: light y (1.0 = 10000 cd/m2) -> code value"""
    p = np.power(np.asarray(y, np.float64), light_ref.M1)
    return np.power((light_ref.C1 + light_ref.C2 * p) / (1.0 + light_ref.C3 * p), light_ref.M2)


def knee(src_peak, dst_peak):
    """(Pw, maxLum, KS)"""
    pw = float(pq(src_peak / 10000.0))
    max_lum = float(pq(dst_peak / 10000.0)) / pw
    return pw, max_lum, 1.5 * max_lum - 0.5


def thresholds(gain, unit_nits):
    """thr[0] = 0, thr[i] = (float)(g (10000 / U) EOTF((i - 0.5) / 2047)): float64"""
    g = float(F(gain))
    i = np.arange(STEPS, dtype=np.float64)
    t = g * (10000.0 / float(unit_nits)) * eotf(np.maximum(i - 0.5, 0.0) / TOP)
    t[0] = 0.0
    return t


def mapped_codes(src_peak, dst_peak):
    """(E2 Pw, curved): the PQ code value the curve maps code k / 2047 to (float64; the code itself where the ratio is 1 by
    definition) and whether entry k lies on the curve"""
    pw, max_lum, ks = knee(src_peak, dst_peak)
    e = np.arange(STEPS, dtype=np.float64) / TOP
    e1 = np.minimum(e / pw, 1.0)
    curved = ~((max_lum >= 1.0) | (e1 < ks))
    curved[0] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (e1 - ks) / (1.0 - ks)
        e2 = (2 * t**3 - 3 * t**2 + 1) * ks + (t**3 - 2 * t**2 + t) * (1.0 - ks) + (-2 * t**3 + 3 * t**2) * max_lum
    return np.where(curved, e2 * pw, e), curved


def gains(src_peak, dst_peak, unit_nits, out_unit_nits):
    """sg[k] = ratio U / Uo: float64"""
    out, curved = mapped_codes(src_peak, dst_peak)
    e = np.arange(STEPS, dtype=np.float64) / TOP
    ratio = np.ones(STEPS)
    ratio[curved] = eotf(out[curved]) / eotf(e[curved])
    return ratio * float(unit_nits) / float(out_unit_nits)


def tables(gain, src_peak, dst_peak, unit_nits, out_unit_nits):
    """(thr, sg) as the kernels hold them: float32"""
    return thresholds(gain, unit_nits).astype(F), gains(src_peak, dst_peak, unit_nits, out_unit_nits).astype(F)


def peak_of(has_clli, max_cll, has_mdcv, mdcv_max):
    """the image's own peak (src_peak == 0)"""
    if has_clli and max_cll != 0:
        return float(min(max_cll, 10000))  # (PQ codes no light above 10000 cd/m2)
    if has_mdcv and 50000 <= mdcv_max <= 100000000:
        return float(F(mdcv_max * 0.0001))
    return 1000.0


def step(thr, sg, r):
    """the step on linear light r (.. x 3, float32) -> (r', k)"""
    assert r.dtype == F and thr.dtype == F and sg.dtype == F
    n = np.fmax(np.fmax(r[..., 0], r[..., 1]), r[..., 2])
    k = np.searchsorted(thr[1:], n, side="right").astype(np.int64)
    out = r * sg[k][..., None]
    assert out.dtype == F
    return out, k


def finish(r, alpha, resampled, enc, m, tone, dtype, scale, bias):
    """light_ref.finish with the tone step - tone: (thr, sg) float32 tables, or None - between the matrix and the finish.  enc is the
    table of the codes that are stored: under the 8-bit finish the 8-bit one, with dtype np.uint8 or a float type."""
    if m is not None:
        r = light_ref.gamut(m, r)
    if tone is not None:
        r = step(tone[0], tone[1], r)[0]
    return light_ref.finish(r, alpha, resampled, enc, None, dtype, scale, bias)


def arms(thr, r, m, src_peak, dst_peak, gain, unit_nits):
    """the census of the norm: the fraction of pixels below the knee, between knee and src_peak, and above src_peak"""
    if m is not None:
        r = light_ref.gamut(m, r)
    n = np.fmax(np.fmax(r[..., 0], r[..., 1]), r[..., 2])
    k = np.searchsorted(thr[1:], n, side="right")
    pw, _, ks = knee(src_peak, dst_peak)
    e1 = k / TOP / pw
    below, above = e1 < ks, k / TOP > pw
    return float(below.mean()), float((~below & ~above).mean()), float(above.mean())
