"""numpy model of the light statistics (hm_light_stats, include/heif_mi355x.h "Light statistics") on top of light_ref, ootf_ref and
tone_ref, written from the header's text: every pixel of the rectangle through lin[] (one table, or three - one per channel), the OOTF
step, the gamut matrix, the norm max(R, G, B) and its count of thresholds in the tone step's thr[] (tone_ref.thresholds, the search of
tone_ref.step); then the histogram, the largest norm, and the host arithmetic behind them - code_nits, percentile, average - in
float64 with the C library's pow (numpy's float64 power calls it), rounded once to float32 where the header says so."""
import math

import numpy as np

import light_ref
import ootf_ref
import tone_ref

F = np.float32
BINS = 2048
TOP = float(BINS - 1)


def eotf(e):
    """ST 2084 at one code value e in [0, 1], float64, with the C library's pow (math.pow calls it; numpy's power need not agree
    with it in the last bit): 1.0 = 10000 cd/m2"""
    m1, m2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
    c1, c2, c3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
    p = math.pow(e, 1.0 / m2)
    return math.pow(max(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1)


def code_nits(k, edge):
    """10000 EOTF(x / 2047): x = k, or for edge 1 the upper edge of bin k, min(k + 0.5, 2047); float64"""
    x = min(k + 0.5, TOP) if edge else float(k)
    return 10000.0 * eotf(x / TOP)


def percentile(hist, pixels, fraction):
    """(code, nits): the smallest k whose cumulative count reaches rank = min(max(ceil(fraction pixels), 1), pixels), and the float32
    upper edge of its bin"""
    rank = min(max(int(math.ceil(fraction * float(pixels))), 1), int(pixels))
    below = 0
    for k in range(BINS):
        below += int(hist[k])
        if below >= rank:
            break
    return k, float(F(code_nits(k, 1)))


def average(hist, pixels):
    """the sum over k, in increasing k, of hist[k] code_nits(k, 0) in float64, over pixels, rounded once to float32"""
    s = 0.0
    for k in range(BINS):
        s += float(hist[k]) * code_nits(k, 0)
    return float(F(s / float(pixels)))


def norms(pixels, bits, lin, m, ootf, crop):
    """N of every pixel of the rectangle (float32): pixels h x w x 3|4 code values (alpha ignored); lin: one float32 table of 1 << bits
    entries or three of them (3 x (1 << bits): red, green, blue); m: 9 float32 values or None; ootf: (y, thr, sg) or None; crop: (x, y,
    w, h) or None"""
    if crop is not None:
        x, y, w, h = crop
        pixels = pixels[y:y + h, x:x + w]
    peak = (1 << bits) - 1
    v = np.minimum(pixels[..., :3].astype(np.int64), peak)
    lin = np.asarray(lin, F)
    if lin.ndim == 2:
        r = np.stack([lin[c][v[..., c]] for c in range(3)], axis=-1)
    else:
        r = lin[v]
    assert r.dtype == F
    if ootf is not None:
        r = ootf_ref.step(ootf[0], ootf[1], ootf[2], r)[0]
    if m is not None:
        r = light_ref.gamut(m, r)
    return np.fmax(np.fmax(r[..., 0], r[..., 1]), r[..., 2])


def stats(pixels, bits, lin, m, ootf, thr, crop, unit_nits=10000.0, gain=1.0):
    """the statistic as a dict: pixels, hist (uint32[2048]), max_norm (float32), max_code, max_nits, average_nits (float32 values as
    Python floats).  thr: the tone step's float32 thresholds for the light step's gain and unit_nits."""
    assert thr.dtype == F and thr.shape == (BINS,)
    n = norms(pixels, bits, lin, m, ootf, crop)
    assert n.dtype == F
    k = np.searchsorted(thr[1:], n, side="right").astype(np.int64)  # (tone_ref.step's search)
    k[np.isnan(n) | (n < 0)] = 0
    hist = np.bincount(k.ravel(), minlength=BINS).astype(np.uint32)
    count = int(n.size)
    pos = n[n > 0]
    max_norm = F(pos.max()) if pos.size else F(0.0)
    g = float(F(gain))
    return dict(pixels=count, hist=hist, max_norm=max_norm, max_code=int(np.flatnonzero(hist)[-1]),
                max_nits=float(F(float(max_norm) * float(F(unit_nits)) / g)), average_nits=average(hist, count))


def of_struct(s):
    """a capi.LightStatsC as the same dict"""
    return dict(pixels=int(s.pixels), hist=np.ctypeslib.as_array(s.hist).astype(np.uint32), max_norm=F(s.max_norm), max_code=int(s.max_code),
                max_nits=float(s.max_nits), average_nits=float(s.average_nits))


def same(got, exp, what=""):
    """equality of two such dicts, everything exact: the histogram, the count, max_norm by its bit pattern, the rest by value"""
    assert got["pixels"] == exp["pixels"], (what, got["pixels"], exp["pixels"])
    if not np.array_equal(got["hist"], exp["hist"]):
        bad = np.flatnonzero(got["hist"] != exp["hist"])
        raise AssertionError(f"{what}: {bad.size} bins differ, first bin {bad[0]}: got {got['hist'][bad[0]]}, expected {exp['hist'][bad[0]]}")
    assert F(got["max_norm"]).view(np.uint32) == F(exp["max_norm"]).view(np.uint32), (what, got["max_norm"], exp["max_norm"])
    assert got["max_code"] == exp["max_code"], (what, got["max_code"], exp["max_code"])
    assert F(got["max_nits"]).view(np.uint32) == F(exp["max_nits"]).view(np.uint32), (what, got["max_nits"], exp["max_nits"])
    assert F(got["average_nits"]).view(np.uint32) == F(exp["average_nits"]).view(np.uint32), (what, got["average_nits"], exp["average_nits"])
