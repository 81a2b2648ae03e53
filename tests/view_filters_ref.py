"""numpy restatement of the cubic and Lanczos-3 filters of a view (hm_device_view, include/heif_mi355x.h), beside tests/view_ref.py:
the tap table in float64 - support a = 1 / 2 / 3 for triangle / cubic / Lanczos-3, the window lo .. hi, the kernel function, the
weights summed with i increasing, divided by the total and converted to float32 -, the sums in float32 tap by tap (multiply and add
rounded separately), horizontal pass first.  What the new filters leave as it was comes from view_ref (to_float, the NEAREST rule, the
triangle's table); to_integer is restated because the sums can now be negative."""
import math

import numpy as np

import view_ref

TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
SUPPORT = {TRIANGLE: 1.0, CUBIC: 2.0, LANCZOS3: 3.0}
MAX_REDUCTION = {TRIANGLE: 256, CUBIC: 128, LANCZOS3: 85}
F = np.float32
PI = 3.14159265358979323846


def kernel(filt, x):
    """k(x), in float64 (Python floats), every operation rounded on its own"""
    x = abs(x)
    if filt == CUBIC:  # Keys, a = -0.5
        if x < 1.0:
            return (1.5 * x - 2.5) * x * x + 1.0
        if x < 2.0:
            return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
        return 0.0
    if filt == LANCZOS3:
        if x == 0.0:
            return 1.0
        if x >= 3.0:
            return 0.0
        p = PI * x
        q = p / 3.0
        return (math.sin(p) / p) * (math.sin(q) / q)
    return max(0.0, 1.0 - x)


def taps_total(n, m, j, filt):
    """(first source index, float32 weights, the normalising total) of output index j on an axis of n -> m"""
    a = SUPPORT[filt]
    s = n / m
    fs = max(s, 1.0)
    c = (j + 0.5) * s
    lo = max(0, int(c - a * fs + 0.5))  # (int(): towards zero, as the C conversion)
    hi = min(n, int(c + a * fs + 0.5))
    w = [kernel(filt, (i + 0.5 - c) / fs) for i in range(lo, hi)]
    total = 0.0
    for x in w:  # in increasing i
        total += x
    return lo, np.array([x / total for x in w], np.float64).astype(F), total


def taps(n, m, j, filt):
    if filt == NEAREST:
        return view_ref.taps(n, m, j, NEAREST)
    return taps_total(n, m, j, filt)[:2]


def _axis(src, n, m, axis, filt):
    """the sequential float32 sum over the taps of one axis of `src` (float32), giving m entries on that axis"""
    src = np.moveaxis(src, axis, 0)
    out = np.zeros((m,) + src.shape[1:], F)
    for j in range(m):
        first, w = taps(n, m, j, filt)
        t = np.zeros(src.shape[1:], F)
        for i, wi in enumerate(w):
            t = t + wi * src[first + i]
            assert t.dtype == F
        out[j] = t
    return np.moveaxis(out, 0, axis)


def resample(pixels, crop, size, filt):
    """pixels: h x w x c unsigned samples; crop: (x, y, w, h) or None; size: (w, h).  The float32 sums r (oh x ow x c), neither
    rounded nor clamped: they overshoot 0 and the peak at hard edges."""
    if filt == NEAREST or size is None:
        return view_ref.resample(pixels, crop, size, NEAREST)
    x, y, n_w, n_h = crop if crop else (0, 0, pixels.shape[1], pixels.shape[0])
    assert 0 <= x and 0 <= y and n_w > 0 and n_h > 0 and x + n_w <= pixels.shape[1] and y + n_h <= pixels.shape[0]
    ow, oh = size
    t = _axis(pixels[y:y + n_h, x:x + n_w].astype(F), n_w, ow, 1, filt)  # horizontal first
    return _axis(t, n_h, oh, 0, filt)


def to_integer(r, peak):
    """an integer destination: min(max((int)(r + 0.5f), 0), peak); the conversion is towards zero, also for a negative r + 0.5f"""
    v = np.trunc(r.astype(F) + F(0.5)).astype(np.int64)
    return np.clip(v, 0, peak)


to_float = view_ref.to_float
