"""numpy model of the alpha step (hm_device_alpha, include/heif_mi355x.h), written from the header's text on top of view_ref /
light_ref / tone_ref: per source pixel a = (float)vA, x_c = (float)v_c (with a light step lin[min(v_c, peak)]) and p_c = x_c * a;
under a resampling view the sums of "Views" over p_c and a (horizontal first, tap 0 first; the tap weights are handed in - the tests
take them from hm_view_filter_taps), otherwise S_c = p_c and S_a = a of the pixel that is moved; then the mode's rule - STRAIGHT
S_c / S_a where S_a > 0 (without sums: x_c itself), PREMULTIPLIED S_c / P, MATTE S_c / P + b_c * (1 - clamp(S_a / P, 0, 1)) - and the
finish: without a light step rounding half up and clamping (integers) or r * scale + bias (floats), with one the gamut matrix, the
tone step and the light step's finish.  Everything is float32, every operation rounded on its own; numpy's float32 division is
correctly rounded, like __fdiv_rn."""
import numpy as np

import light_ref
import tone_ref
import view_filters_ref
import view_ref

F = np.float32
STRAIGHT, PREMULTIPLIED, MATTE = 1, 2, 3
NEAREST = view_ref.NEAREST


def sums(pixels, bits, lin, view, taps):
    """(x, S, S_a, moved_alpha, summed) of h x w x 4 unsigned samples: x the colour as floats of the pixels that are moved (None when
    summed), S (oh x ow x 3) and S_a (oh x ow) the sums - or the product and alpha of the pixel that is moved -, moved_alpha the alpha
    samples that are moved (None when summed).  lin: the light step's table or None; view: None or (crop, size, filter);
    taps(n, m, j, filter) -> (first, weights)."""
    assert pixels.shape[2] == 4
    peak = (1 << bits) - 1

    def colour(v):
        return lin[np.minimum(v.astype(np.int64), peak)] if lin is not None else v.astype(F)
    crop, size, filt = view if view else (None, None, NEAREST)
    if size is None or filt == NEAREST:
        moved = view_ref.resample(pixels, crop, size, NEAREST)
        x, a = colour(moved[..., :3]), moved[..., 3].astype(F)
        p = x * a[..., None]
        assert p.dtype == F
        return x, p, a, moved[..., 3], False
    cx, cy, n_w, n_h = crop if crop else (0, 0, pixels.shape[1], pixels.shape[0])
    rect = pixels[cy:cy + n_h, cx:cx + n_w]
    a = rect[..., 3].astype(F)
    pa = np.concatenate([colour(rect[..., :3]) * a[..., None], a[..., None]], axis=2)
    assert pa.dtype == F
    t = light_ref._axis(pa, n_w, size[0], 1, filt, taps)  # horizontal first
    t = light_ref._axis(t, n_h, size[1], 0, filt, taps)
    return None, t[..., :3], t[..., 3], None, True


def rule(mode, x, S, Sa, summed, P, b):
    """r (oh x ow x 3, float32) of the mode's rule; b: the background as three float32 values (MATTE)"""
    P = F(P)
    if mode == STRAIGHT:
        if not summed:
            return x
        with np.errstate(divide="ignore", invalid="ignore"):
            q = S / Sa[..., None]
        r = np.where(Sa[..., None] > 0, q, F(0.0))
    elif mode == PREMULTIPLIED:
        r = S / P
    else:
        cov = np.minimum(np.maximum(Sa / P, F(0.0)), F(1.0))
        r = S / P + np.asarray(b, F) * (F(1.0) - cov)[..., None]
    assert r.dtype == F
    return r


def render(pixels, bits, mode, background, view, taps, dtype, scale, bias, lin=None, enc=None, m=None, tone=None):
    """The destination's values (oh x ow x 3 for MATTE, x 4 otherwise; of `dtype`: np.uint8 / np.uint16 / np.float16 / np.float32).
    lin: the light step's table (None: no light step), enc: its threshold table (None: linear light), m: 9 float32 values or None,
    tone: (thr, sg) or None.  Also returns (S, S_a) for the tests' assertions on the model."""
    x, S, Sa, moved_alpha, summed = sums(pixels, bits, lin, view, taps)
    P = float((1 << bits) - 1)
    b = None
    if mode == MATTE:
        b = [lin[v] if lin is not None else F(v) for v in background]
    r = rule(mode, x, S, Sa, summed, P, b)
    integer = dtype in (np.uint8, np.uint16)
    full = 255 if dtype == np.uint8 else 65535
    sc, bi = np.asarray(scale, F), np.asarray(bias, F)
    if lin is None:
        if mode == STRAIGHT and not summed:  # the samples themselves
            colour = r.astype(np.int64) if integer else r * sc[:3] + bi[:3]
        else:
            colour = view_filters_ref.to_integer(r, full) if integer else r * sc[:3] + bi[:3]
    else:  # r takes the place of the resampled light
        none = np.zeros(r.shape[:2] + (0,), F)
        colour = tone_ref.finish(r, none, summed, enc, m, tone, F if not integer else dtype, scale, bias)
    if mode != MATTE:
        if summed:
            a_out = view_filters_ref.to_integer(Sa, full) if integer else Sa * sc[3] + bi[3]
        else:
            a_out = moved_alpha.astype(np.int64) if integer else moved_alpha.astype(F) * sc[3] + bi[3]
        colour = np.concatenate([colour, a_out[..., None]], axis=2)
    if not integer:
        assert colour.dtype == F
    with np.errstate(over="ignore"):  # (a float16 destination: beyond 65504 is inf, on the device too)
        return colour.astype(dtype), S, Sa
