"""numpy restatement of a planar view (a view, hm_device_view, into hm_device_planes: include/heif_mi355x.h): the geometry per plane,
each plane through view_filters_ref.resample as an h x w x 1 image of its own, the final store with the plane's own peak and the
msb_aligned shift, the affine map of the float dtypes, and the packing of HM_DEV_PLANES_SEMI."""
import numpy as np

import view_filters_ref as vf

SEPARATE, SEMI = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = vf.TRIANGLE, vf.NEAREST, vf.CUBIC, vf.LANCZOS3
F = np.float32


def sub(chroma):
    """(sx, sy) of a chroma format (0 4:0:0, 1 4:2:0, 2 4:2:2, 3 4:4:4)"""
    return (2 if chroma in (1, 2) else 1), (2 if chroma == 1 else 1)


def geometry(chroma, W, H, crop, size):
    """crop: (x, y, w, h) or None (the whole image); size: (ow, oh) or None (the crop's own).  -> (crops, outs): per plane Y, Cb, Cr, A
    the crop (x, y, w, h) inside that plane and the size (w, h) written; all zero for Cb / Cr of 4:0:0.  ValueError("x") / ("y"): an
    origin that is no multiple of the sub-sampling; ("crop"): a rectangle that is empty or not inside the image."""
    x, y, w, h = crop if crop else (0, 0, W, H)
    if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > W or y + h > H:
        raise ValueError("crop")
    ow, oh = size if size else (w, h)
    sx, sy = sub(chroma)
    if x % sx:
        raise ValueError("x")
    if y % sy:
        raise ValueError("y")
    luma, none = ((x, y, w, h), (ow, oh)), ((0, 0, 0, 0), (0, 0))
    chr_ = ((x // sx, y // sy, (w + sx - 1) // sx, (h + sy - 1) // sy), ((ow + sx - 1) // sx, (oh + sy - 1) // sy)) if chroma else none
    planes = [luma, chr_, chr_, luma]
    return [p[0] for p in planes], [p[1] for p in planes]


def within_limits(crops, outs, filt, chroma):
    """the reduction limit of the filter, per plane and axis"""
    most = vf.MAX_REDUCTION.get(filt, 256)
    for c in (0, 1) if chroma else (0,):
        for n, m in ((crops[c][2], outs[c][0]), (crops[c][3], outs[c][1])):
            if m < 1 or m > 32768 or n > most * m:
                return False
    return True


def plane_view(plane, crop, out, filt, crop_only):
    """one plane (2-D unsigned samples) as an image of its own: the float32 sums r, or - the crop alone, NEAREST - the samples moved"""
    r = vf.resample(plane[:, :, None], crop, None if crop_only else out, filt)
    return r[:, :, 0]


def store(r, c, dtype, scale, bias, bits, msb, moved):
    """the elements of component c (0 Y, 1 Cb, 2 Cr, 3 alpha) of a plane of `bits` bits"""
    if dtype in (F16, F32):
        v = r.astype(F) * F(scale[c]) + F(bias[c])
        assert v.dtype == F
        return v.astype(np.float16) if dtype == F16 else v
    shift = 16 - bits if msb else 0
    if moved:
        return (r.astype(np.uint32) << shift).astype(NP[dtype])
    return (vf.to_integer(r, (1 << bits) - 1).astype(np.uint32) << shift).astype(NP[dtype])


def sums(host, crop, size, filt, want_alpha):
    """per source plane Y, Cb, Cr, A: (float32 sums or moved samples, moved?) - None where the plane does not exist or is not asked for"""
    crops, outs = geometry(host["chroma"], host["w"], host["h"], crop, size)
    moved = size is None or filt == NEAREST
    src = list(host["planes"]) + [None] * (3 - len(host["planes"])) + [host["alpha"] if want_alpha else None]
    return [None if p is None else plane_view(p, crops[c], outs[c], filt, size is None) for c, p in enumerate(src)], moved


def images_from(r, moved, host, layout, dtype, scale, bias, msb):
    """what plane[0 .. 3] must hold, from the sums of `sums`: 2-D arrays of elements (the interleaved plane: rows of Cb, Cr pairs),
    None where no plane is written"""
    out = [store(r[0], 0, dtype, scale, bias, host["bits"], msb, moved), None, None, None]
    if host["chroma"] != 0:
        cb, cr = (store(r[c], c, dtype, scale, bias, host["bits"], msb, moved) for c in (1, 2))
        if layout == SEMI:
            out[1] = np.stack([cb, cr], axis=2).reshape(cb.shape[0], cb.shape[1] * 2)
        else:
            out[1], out[2] = cb, cr
    if r[3] is not None:
        out[3] = store(r[3], 3, dtype, scale, bias, host["alpha_bits"], msb, moved)
    return out


def dest_images(host, layout, dtype, scale, bias, msb, want_alpha, crop, size, filt):
    """host: dict(w, h, chroma, bits, planes [Y, Cb, Cr], alpha, alpha_bits) as tests/test_device_planes_gpu.py's host_decode gives it"""
    r, moved = sums(host, crop, size, filt, want_alpha)
    return images_from(r, moved, host, layout, dtype, scale, bias, msb)
