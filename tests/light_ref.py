"""numpy model of the light step (hm_device_light, include/heif_mi355x.h), written from the standards: the transfer functions of
ITU-T H.273 codes 1 / 6 / 14 / 15 (BT.709), 4, 5, 8, 13 (IEC 61966-2-1 sRGB), 16 (SMPTE ST 2084 PQ) and 18 (ITU-R BT.2100 HLG, the
inverse OETF) in float64, the tables made of them, the RGB -> RGB matrix from the H.273 chromaticities (BT.2087 publishes the
2020 -> 709 one), and the pixel pipeline in float32 with every operation rounded on its own: table lookup, the sums of a view
(horizontal first, tap 0 first; the tap weights are handed in - the tests take them from hm_view_filter_taps), the matrix, and the
finish (linear floats, or the count of thresholds reached)."""
import numpy as np

import view_filters_ref
import view_ref

F = np.float32
LINEAR = 8
TRANSFERS = (1, 4, 5, 6, 8, 13, 14, 15, 16, 18)
PRIMARIES = (1, 5, 6, 7, 9, 12)
NEAREST = view_ref.NEAREST

# BT.709's constants as the solution of the two conditions that make the pieces meet in value and slope (H.273 prints 1.099 and 0.018)
ALPHA, BETA = 1.09929682680944, 0.018053968510807
# ST 2084
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
# BT.2100 HLG
HLG_A = 0.17883277
HLG_B = 1.0 - 4.0 * HLG_A
HLG_C = 0.5 - HLG_A * np.log(4.0 * HLG_A)

# H.273 table 2: x, y of red, green, blue; the white of all of these is D65
CHROMATICITIES = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),
                  5: ((0.640, 0.330), (0.290, 0.600), (0.150, 0.060)),
                  6: ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070)),
                  7: ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070)),
                  9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),
                  12: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}
D65 = (0.3127, 0.3290)


def to_light(transfer, e):
    """F_t: code value e in [0, 1] -> light, float64"""
    e = np.asarray(e, np.float64)
    if transfer in (1, 6, 14, 15):
        return np.where(e < 4.5 * BETA, e / 4.5, np.power((e + (ALPHA - 1.0)) / ALPHA, 1.0 / 0.45))
    if transfer == 4:
        return np.power(e, 2.2)
    if transfer == 5:
        return np.power(e, 2.8)
    if transfer == 8:
        return e.copy()
    if transfer == 13:
        return np.where(e <= 0.04045, e / 12.92, np.power((e + 0.055) / 1.055, 2.4))
    if transfer == 16:
        p = np.power(e, 1.0 / M2)
        return np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)
    if transfer == 18:
        return np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)
    raise ValueError(f"transfer {transfer}")


def table(transfer, bits, gain, encode):
    """lin[c] = (float)(g F(c / peak)), or enc[c] = (float)(g F((c - 0.5) / peak)) with entry 0 (never looked at) at 0; g = (double)gain"""
    n = 1 << bits
    peak = float(n - 1)
    g = float(F(gain))
    c = np.arange(n, dtype=np.float64)
    if not encode:
        return (g * to_light(transfer, c / peak)).astype(F)
    t = (g * to_light(transfer, np.maximum(c - 0.5, 0.0) / peak)).astype(F)
    t[0] = 0.0
    return t


def to_xyz(primaries):
    """RGB -> XYZ of a set of primaries: the columns are the primaries' XYZ, scaled so that R = G = B = 1 is the white"""
    P = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in CHROMATICITIES[primaries]], np.float64).T
    W = np.array([D65[0] / D65[1], 1.0, (1.0 - D65[0] - D65[1]) / D65[1]], np.float64)
    return P * np.linalg.solve(P, W)


def matrix(from_primaries, to_primaries):
    """(to -> XYZ)^-1 (from -> XYZ), float64"""
    if from_primaries == to_primaries:
        return np.eye(3)
    return np.linalg.solve(to_xyz(to_primaries), to_xyz(from_primaries))


def gamut(m, rgb):
    """R' = (m0 R + m1 G) + m2 B in float32, every operation rounded; m: 9 float32 values, row-major"""
    m = np.asarray(m, F).reshape(3, 3)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    out = np.stack([(m[k, 0] * R + m[k, 1] * G) + m[k, 2] * B for k in range(3)], axis=-1)
    assert out.dtype == F
    return out


def encode(enc, r):
    """|{c in 1 .. peak : enc[c] <= r}|"""
    return np.searchsorted(enc[1:], r, side="right").astype(np.int64)


def _axis(src, n, m, axis, filt, taps):
    src = np.moveaxis(src, axis, 0)
    out = np.zeros((m,) + src.shape[1:], F)
    for j in range(m):
        first, w = taps(n, m, j, filt)
        t = np.zeros(src.shape[1:], F)
        for i, wi in enumerate(w):
            t = t + F(wi) * src[first + i]
            assert t.dtype == F
        out[j] = t
    return np.moveaxis(out, 0, axis)


def light_sums(pixels, bits, lin, view, taps):
    """(r, alpha, resampled): linear light of the colour channels (oh x ow x 3, float32) before the matrix - the sums of a resampling
    view, or lin[] of the samples that are moved -, the alpha channel beside it (oh x ow x 0 or 1: float32 sums, or moved samples),
    and whether the view resampled.  view: None or (crop, size, filter); taps(n, m, j, filter) -> (first, weights)."""
    peak = (1 << bits) - 1
    crop, size, filt = view if view else (None, None, NEAREST)
    if size is None or filt == NEAREST:
        moved = view_ref.resample(pixels, crop, size, NEAREST)
        return lin[np.minimum(moved[..., :3].astype(np.int64), peak)], moved[..., 3:], False
    x, y, n_w, n_h = crop if crop else (0, 0, pixels.shape[1], pixels.shape[0])
    rect = pixels[y:y + n_h, x:x + n_w]
    a = np.concatenate([lin[np.minimum(rect[..., :3].astype(np.int64), peak)], rect[..., 3:].astype(F)], axis=2)
    assert a.dtype == F
    t = _axis(a, n_w, size[0], 1, filt, taps)  # horizontal first
    t = _axis(t, n_h, size[1], 0, filt, taps)
    return t[..., :3], t[..., 3:], True


def finish(r, alpha, resampled, enc, m, dtype, scale, bias):
    """The destination's values (oh x ow x c, of `dtype`: np.uint8 / np.uint16 / np.float16 / np.float32) of light_sums' result.
    enc: the float32 threshold table (None: linear light); m: 9 float32 values or None."""
    c = 3 + alpha.shape[2]
    integer = dtype in (np.uint8, np.uint16)
    sc, bi = np.asarray(scale[:c], F), np.asarray(bias[:c], F)
    if m is not None:
        r = gamut(m, r)
    if enc is None:
        assert not integer
        colour = r * sc[:3] + bi[:3]
    else:
        code = encode(enc, r)
        colour = code if integer else code.astype(F) * sc[:3] + bi[:3]
    if c == 4:  # not light: finished as without a light step
        if integer:
            a_out = view_filters_ref.to_integer(alpha, 255 if dtype == np.uint8 else 65535) if resampled else alpha
        else:
            a_out = alpha.astype(F) * sc[3:] + bi[3:]
        colour = np.concatenate([colour, a_out], axis=2)
    if not integer:
        assert colour.dtype == F
    return colour.astype(dtype)


def render(pixels, bits, lin, enc, m, view, taps, dtype, scale, bias):
    """light_sums, then finish"""
    r, alpha, resampled = light_sums(pixels, bits, lin, view, taps)
    return finish(r, alpha, resampled, enc, m, dtype, scale, bias)
