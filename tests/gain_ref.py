"""numpy model of the gain step (hm_device_gain, include/heif_mi355x.h "Gain") on top of light_ref and tone_ref, written from the
header's text: the weight and the tables in float64, rounded once to float32; the geometry (a whole factor per axis, the map's crop);
the map's view sums over tab_c[code] (horizontal first, tap 0 first, every operation rounded; the tap weights are handed in - the tests
take them from hm_view_filter_taps); and the update r = ((r + kb) * M) - ka in float32, three rounded operations, before the gamut
matrix.  finish() is tone_ref.finish: matrix, tone step, the light step's finish."""
import math

import numpy as np

import light_ref
import tone_ref
import view_ref

F = np.float32
TRIANGLE, NEAREST = view_ref.TRIANGLE, view_ref.NEAREST
FIELDS = ("min", "max", "gamma", "base_offset", "alternate_offset")


def weight(headroom, hb, ha):
    """wgt = min(max((Hd - Hb) / (Ha - Hb), 0), 1), Hd = (double)(float)headroom; +inf allowed"""
    hd = float(F(headroom))
    assert hd >= 0.0 and ha != hb
    if math.isinf(hd):
        return 1.0 if ha > hb else 0.0
    return min(max((hd - hb) / (ha - hb), 0.0), 1.0)


def table(wgt, lo, hi, gamma, bits):
    """tab[v] = (float)exp2(wgt (min + (max - min) u)), u = v / mpeak, raised to 1 / gamma unless gamma is 1"""
    n = 1 << bits
    u = np.arange(n, dtype=np.float64) / float(n - 1)
    if gamma != 1.0:
        u = np.power(u, 1.0 / gamma)
    return np.exp2(wgt * (lo + (hi - lo) * u)).astype(F)


def channels(params):
    """1 when the three parameter sets are equal, else 3; params: {field: [three doubles]}"""
    return 1 if all(params[f][0] == params[f][1] == params[f][2] for f in FIELDS) else 3


def tables(params, headroom, hb, ha, bits):
    """the nch tables of a parameter set"""
    w = weight(headroom, hb, ha)
    return [table(w, params["min"][c], params["max"][c], params["gamma"][c], bits) for c in range(channels(params))]


def offsets(params, gain):
    """(kb, ka): (float)(g * offset_c), g = (double)(float)gain"""
    g = float(F(gain))
    return (np.array([g * v for v in params["base_offset"]]).astype(F), np.array([g * v for v in params["alternate_offset"]]).astype(F))


def factor(full, part):
    """s = (W + MW - 1) / MW with MW == (W + s - 1) / s, or None"""
    if part < 1 or part > full:
        return None
    s = (full + part - 1) // part
    return s if (full + s - 1) // s == part else None


def map_crop(size, map_size, crop):
    """the map's crop (x / sx, y / sy, (w + sx - 1) / sx, (h + sy - 1) / sy) of the base's crop (None: the whole image)"""
    sx, sy = factor(size[0], map_size[0]), factor(size[1], map_size[1])
    assert sx and sy, (size, map_size)
    x, y, w, h = crop if crop else (0, 0, size[0], size[1])
    assert x % sx == 0 and y % sy == 0
    return x // sx, y // sy, (w + sx - 1) // sx, (h + sy - 1) // sy


def map_sums(gmap, mbits, tabs, view, base_size, taps):
    """M (oh x ow x 3, float32): the view sums over tab_c[min(code, mpeak)] of the map's crop - HM_VIEW_TRIANGLE whatever the view's
    filter, the moved sample under HM_VIEW_NEAREST.  gmap: mh x mw codes; view: None or (crop, size, filter) of the BASE."""
    crop, size, filt = view if view else (None, None, NEAREST)
    mx, my, mw, mh = map_crop(base_size, (gmap.shape[1], gmap.shape[0]), crop)
    x, y, w, h = crop if crop else (0, 0, base_size[0], base_size[1])
    ow, oh = size if size else (w, h)
    codes = np.minimum(gmap[my:my + mh, mx:mx + mw].astype(np.int64), (1 << mbits) - 1)
    a = np.stack([t[codes] for t in tabs], axis=2)
    assert a.dtype == F
    if size is not None and filt == NEAREST:
        m = a[(np.arange(oh) * mh // oh)[:, None], (np.arange(ow) * mw // ow)[None, :]]
    else:
        t = light_ref._axis(a, mw, ow, 1, TRIANGLE, taps)  # horizontal first
        m = light_ref._axis(t, mh, oh, 0, TRIANGLE, taps)
    return np.repeat(m, 3, axis=2) if m.shape[2] == 1 else m


def update(r, m, kb, ka):
    """r_c = fsub(fmul(fadd(r_c, kb_c), M_c), ka_c)"""
    assert r.dtype == F and m.dtype == F and kb.dtype == F and ka.dtype == F
    out = ((r + kb) * m) - ka
    assert out.dtype == F
    return out


def render(pixels, bits, lin, gmap, mbits, tabs, kb, ka, view, taps, enc, matrix, tone, dtype, scale, bias):
    """the destination's values (oh x ow x c) of base `pixels` (h x w x c codes) and map `gmap` under the light, gain and tone steps"""
    r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, view, taps)
    m = map_sums(gmap, mbits, tabs, view, (pixels.shape[1], pixels.shape[0]), taps)
    return tone_ref.finish(update(r, m, kb, ka), alpha, resampled, enc, matrix, tone, dtype, scale, bias)
