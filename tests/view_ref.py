"""numpy restatement of a view (hm_device_view, include/heif_mi355x.h): the tap table in float64 exactly as the header states it,
the sums in float32 tap by tap (multiply and add rounded separately), horizontal pass first, and the NEAREST index rule."""
import numpy as np

TRIANGLE, NEAREST = 0, 1
F = np.float32


def taps(n, m, j, filt=TRIANGLE):
    """(first source index, float32 weights) of output index j on an axis of n -> m"""
    if filt == NEAREST:
        return j * n // m, np.ones(1, F)
    s = n / m
    fs = max(s, 1.0)
    c = (j + 0.5) * s
    lo = max(0, int(c - fs + 0.5))  # (int(): towards zero, as the C conversion)
    hi = min(n, int(c + fs + 0.5))
    w = [max(0.0, 1.0 - abs((i + 0.5 - c) / fs)) for i in range(lo, hi)]
    total = 0.0
    for x in w:  # in increasing i
        total += x
    return lo, np.array([x / total for x in w], np.float64).astype(F)


def _axis(src, n, m, axis):
    """the sequential float32 sum over the taps of one axis of `src` (float32), giving m entries on that axis"""
    src = np.moveaxis(src, axis, 0)
    out = np.zeros((m,) + src.shape[1:], F)
    for j in range(m):
        first, w = taps(n, m, j)
        t = np.zeros(src.shape[1:], F)
        for i, wi in enumerate(w):
            t = t + wi * src[first + i]
            assert t.dtype == F
        out[j] = t
    return np.moveaxis(out, 0, axis)


def resample(pixels, crop, size, filt=TRIANGLE):
    """pixels: h x w x c unsigned samples; crop: (x, y, w, h) or None; size: (w, h) or None (the crop alone).
    TRIANGLE: the float32 sums r (oh x ow x c), not rounded; NEAREST or the crop alone: the samples moved (the input's dtype)."""
    x, y, n_w, n_h = crop if crop else (0, 0, pixels.shape[1], pixels.shape[0])
    assert 0 <= x and 0 <= y and n_w > 0 and n_h > 0 and x + n_w <= pixels.shape[1] and y + n_h <= pixels.shape[0]
    rect = pixels[y:y + n_h, x:x + n_w]
    if size is None:
        return rect.copy()
    ow, oh = size
    if filt == NEAREST:
        ys = np.array([k * n_h // oh for k in range(oh)])
        xs = np.array([j * n_w // ow for j in range(ow)])
        return rect[ys][:, xs].copy()
    t = _axis(rect.astype(F), n_w, ow, 1)  # horizontal first
    return _axis(t, n_h, oh, 0)


def to_integer(r, peak):
    """an integer destination: min(max((int)(r + 0.5f), 0), peak)"""
    v = (r.astype(F) + F(0.5)).astype(np.int64)  # (towards zero; r is never negative)
    return np.clip(v, 0, peak)


def to_float(r, scale, bias):
    """a float destination: r * scale[c] + bias[c] in float32, each step rounded (r: float32 sums or moved samples)"""
    c = r.shape[2]
    v = r.astype(F) * np.asarray(scale[:c], F) + np.asarray(bias[:c], F)
    assert v.dtype == F
    return v
