"""GPU: planar YCbCr in caller-owned device memory (hm_decode_item_to_device_planes, hm_decode_frames_to_device_planes,
hm_pipeline_submit_to_device_planes, hm_planes_to_tensor and the Python decode_to_planes family).  Everything is bit-exact: the
reference of every case is the same item decoded by hm_decode_item to host memory with the same params (which the other GPU tests
hold to the reference decoder); floats are restated in float32 numpy, multiply and add rounded separately, float16 is numpy's
astype.  Every plane sits in a buffer of its own between two guard regions, pre-filled with 0xA5, and the WHOLE buffer is compared
with its expected image: the samples, and 0xA5 in the guards, the pitch padding and - after a refused call - everywhere."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import moovwriter
import synthutil

pytestmark = pytest.mark.gpu
SEPARATE, SEMI = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
ELEM = {U8: 1, U16: 2, F16: 2, F32: 4}
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
YCBCR = {1: 0x101, 2: 0x102, 3: 0x103}
YCBCR_8BIT = 0x200
GUARD = 512
ALPHA_URN = "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"
ONE, ZERO = [1.0] * 4, [0.0] * 4


def affine(peak):
    """per-component scale / bias on samples of `peak`: all four differ, chroma is centred"""
    return [1.0 / peak, 2.0 / peak, 1.5 / peak, 0.5 / peak], [0.0625, -1.0, -0.75, 0.25]


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def inputs():
    """name -> (file bytes, host threads)"""
    files = {}
    full = synthutil.picture(48000, width=200, height=136, qp=30, vui=1, full_range=1, matrix=6)
    files["420_8"] = heifwriter.write_heic([full], (200, 136))
    files["420_8_clap_odd"] = heifwriter.write_heic([full], (200, 136), transforms=[("clap", (121, 1, 77, 1, 7, 2, -5, 2))])
    p422 = synthutil.picture(48001, width=160, height=96, chroma_format=2, bit_depth=10, full_range=0, matrix=1, primaries=1)
    files["422_10"] = heifwriter.write_heic([p422], (160, 96), chroma_format=2, bit_depth=10)
    p444 = synthutil.picture(48002, width=72, height=40, chroma_format=3)
    files["444_8"] = heifwriter.write_heic([p444], (72, 40), chroma_format=3)
    mono = synthutil.picture(48003, width=64, height=64, chroma_format=0)
    files["400_8"] = heifwriter.write_heic([mono], (64, 64), chroma_format=0)
    tiles = [synthutil.picture(48100 + t, width=64, height=64) for t in range(8)]
    # (three tile rows of two: a fourth row of 64 x 64 tiles would begin below a canvas of 171 rows, which the file format forbids)
    files["grid_cropped"] = heifwriter.write_heic(tiles[:6], (64, 64), grid=(3, 2, 117, 171))
    alpha = synthutil.picture(48201, width=48, height=32)
    files["444_8_alpha"] = heifwriter.write_heic([synthutil.picture(48200, width=96, height=64, chroma_format=3)], (96, 64), chroma_format=3,
                                                 aux=[(alpha, (48, 32), ALPHA_URN, 1, 8)])
    files["420_8_alpha"] = heifwriter.write_heic([synthutil.picture(48202, width=96, height=64)], (96, 64), aux=[(alpha, (48, 32), ALPHA_URN)])
    alpha10 = synthutil.picture(48203, width=48, height=32, bit_depth=10)
    files["420_8_alpha10"] = heifwriter.write_heic([synthutil.picture(48202, width=96, height=64)], (96, 64), aux=[(alpha10, (48, 32), ALPHA_URN, 1, 10)])
    mtiles = [synthutil.picture(48300 + t, width=64, height=64, chroma_format=0) for t in range(4)]
    files["grid_400"] = heifwriter.write_heic(mtiles, (64, 64), grid=(2, 2, 120, 100), chroma_format=0)
    return {n: (d, 2) for n, d in files.items()}


def host_decode(capi, L, data, fmt=0, to_8bit=0, threads=2, item=0, alpha_bits=8):
    """hm_decode_item to host memory: dict(w, h, chroma, bits, planes [Y, Cb, Cr] of the plane sizes, alpha or None, meta)"""
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, to_8bit)
        d = capi.Decoded()
        rc = L.hm_decode_item(fh, item or L.hm_file_primary_item(fh), C.byref(prm), C.byref(d))
        assert rc == 0, L.hm_last_error().decode()
        dt = np.uint16 if d.bit_depth > 8 else np.uint8
        planes = []
        for c in range(3):
            if not d.plane[c]:
                continue
            pw, ph = d.plane_width[c], d.plane_height[c]
            raw = np.ctypeslib.as_array(d.plane[c], shape=(ph, d.stride[c]))
            planes.append(np.ascontiguousarray(raw[:, :pw * dt().itemsize]).view(dt).copy())
        alpha = None
        if d.alpha:
            adt = np.uint16 if alpha_bits > 8 else np.uint8
            raw = np.ctypeslib.as_array(d.alpha, shape=(d.height, d.alpha_stride))
            alpha = np.ascontiguousarray(raw[:, :d.width * adt().itemsize]).view(adt).copy()
        meta = {k: getattr(d, k) for k in "width height bit_depth chroma out_format has_nclx primaries transfer matrix full_range has_alpha warnings".split()}
        meta["plane_size"] = [(d.plane_width[c], d.plane_height[c]) for c in range(3)]
        res = dict(w=d.width, h=d.height, chroma=d.chroma, bits=d.bit_depth, planes=planes, alpha=alpha, alpha_bits=alpha_bits if alpha is not None else 0, meta=meta)
        L.hm_decoded_free(C.byref(d))
        return res
    finally:
        L.hm_file_close(fh)


class Guarded:
    """`need` bytes of device memory between two guards, everything pre-filled with 0xA5"""

    def __init__(self, need, offset=0):
        import torch
        self.size = GUARD + offset + need + GUARD
        self.t = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.start = GUARD + offset
        self.ptr = self.t.data_ptr() + self.start
        assert self.t.data_ptr() % 256 == 0

    def host(self):
        return self.t.cpu().numpy()


def convert(v, c, dtype, scale, bias, shift):
    """samples of component c (0 Y, 1 Cb, 2 Cr, 3 alpha) as the destination's elements"""
    if dtype in (F16, F32):
        r = v.astype(np.float32) * np.float32(scale[c]) + np.float32(bias[c])
        assert r.dtype == np.float32
        return r.astype(np.float16) if dtype == F16 else r
    return (v.astype(np.uint32) << shift).astype(NP[dtype])


def dest_images(host, layout, dtype, scale, bias, msb, want_alpha):
    """what plane[0 .. 3] must hold: 2-D arrays of elements (the interleaved plane: rows of Cb, Cr pairs), None where no plane is written"""
    shift = 16 - host["bits"] if msb else 0
    P = host["planes"]
    out = [convert(P[0], 0, dtype, scale, bias, shift), None, None, None]
    if host["chroma"] != 0:
        cb, cr = convert(P[1], 1, dtype, scale, bias, shift), convert(P[2], 2, dtype, scale, bias, shift)
        if layout == SEMI:
            out[1] = np.stack([cb, cr], axis=2).reshape(cb.shape[0], cb.shape[1] * 2)
        else:
            out[1], out[2] = cb, cr
    if want_alpha:
        out[3] = convert(host["alpha"], 3, dtype, scale, bias, 16 - host["alpha_bits"] if msb else 0)
    return out


def make_planes(capi, L, host, layout, dtype, scale, bias, pad, off, msb=0, want_alpha=False, shrink=None):
    """(hm_device_planes, guarded buffers per plane (None: no plane), pitches in use)"""
    d = capi.DevicePlanes()
    d.layout, d.dtype, d.msb_aligned = layout, dtype, msb
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    shapes = [None if im is None else im.shape for im in dest_images(host, layout, F32, ONE, ZERO, 0, want_alpha)]
    pitches = [0] * 4
    for c, shape in enumerate(shapes):
        if shape is None:
            continue
        tight = shape[1] * ELEM[dtype]
        # pad 1: 21 elements more (no 16-byte store is possible on every row); pad 2: 64 bytes more
        pitches[c] = tight if not pad else tight + (21 * ELEM[dtype] if pad == 1 else 64)
        d.plane[c].row_pitch = pitches[c] if pad else 0
    if want_alpha:
        d.plane[3].ptr = 1 << 20  # (hm_device_planes_bytes only asks whether it is given)
    need = (C.c_int64 * 4)()
    total = L.hm_device_planes_bytes(host["chroma"], host["bits"], host["w"], host["h"], C.byref(d), C.byref(need))
    assert total > 0, L.hm_last_error().decode()
    bufs = [None] * 4
    for c, shape in enumerate(shapes):
        if shape is None:
            continue
        assert need[c] == pitches[c] * (shape[0] - 1) + shape[1] * ELEM[dtype]
        bufs[c] = Guarded(need[c], off * ELEM[dtype])
        d.plane[c].ptr, d.plane[c].len = bufs[c].ptr, need[c] - (1 if shrink == c else 0)
    assert total == sum(need[c] for c in range(4) if bufs[c] is not None)
    import torch
    torch.cuda.synchronize()
    return d, bufs, pitches


def expected_buffer(image, pitch, g):
    buf = np.full(g.size, 0xA5, np.uint8)
    e = image.dtype.itemsize
    typed = buf[g.start:g.start + (g.size - g.start) // e * e].view(image.dtype)
    view = np.lib.stride_tricks.as_strided(typed, shape=image.shape, strides=(pitch, e))
    view[...] = image
    return buf


def check_buffers(bufs, images, pitches, what):
    for c in range(4):
        if bufs[c] is None:
            continue
        got = bufs[c].host()
        exp = expected_buffer(images[c], pitches[c], bufs[c]) if images is not None else np.full(bufs[c].size, 0xA5, np.uint8)
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError(f"{what}, plane {c}: {bad.size} bytes differ, first at {bad[0] - bufs[c].start} from the plane's start "
                                 f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def to_planes(capi, L, data, fmt, d, to_8bit=0, threads=2, item=0, ext_dst=None):
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, ext_dst, 0, 0, 0, to_8bit)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_planes(fh, item or L.hm_file_primary_item(fh), C.byref(prm), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(fh)


def variants(bits):
    """(dtype, scale, bias, pitches: 0 tight / 1 padded by 21 elements / 2 padded by 64 bytes, ptr offset in elements, msb_aligned)"""
    integer = U16 if bits > 8 else U8
    sc, bi = affine(float((1 << bits) - 1))
    v = [(integer, ONE, ZERO, 0, 0, 0), (integer, ONE, ZERO, 1, 0, 0), (integer, ONE, ZERO, 2, 0, 0), (integer, ONE, ZERO, 0, 1, 0),
         (F32, sc, bi, 0, 0, 0), (F32, sc, bi, 1, 1, 0), (F16, sc, bi, 0, 0, 0), (F16, sc, bi, 2, 0, 0),
         # a scale small enough for float16 subnormals (below 2 ** -14): 8-bit samples times 2 ** -20, deeper ones times 2 ** -28
         (F16, [2.0 ** (-28 if bits > 8 else -20)] * 4, ZERO, 0, 0, 0)]
    if bits > 8:
        v += [(U16, ONE, ZERO, 0, 0, 1), (U16, ONE, ZERO, 1, 1, 1)]
    return v


# name -> (file, out_format, convert_hdr_to_8bit, expected (chroma, bits) of the result)
CASES = {
    "as_coded_420_8": ("420_8", 0, 0, (1, 8)),
    "as_coded_420_8_clap_odd": ("420_8_clap_odd", 0, 0, (1, 8)),
    "as_coded_422_10": ("422_10", 0, 0, (2, 10)),
    "as_coded_444_8": ("444_8", 0, 0, (3, 8)),
    "as_coded_400_8": ("400_8", 0, 0, (0, 8)),
    "as_coded_grid_cropped": ("grid_cropped", 0, 0, (1, 8)),
    "as_coded_420_8_alpha": ("420_8_alpha", 0, 0, (1, 8)),
    "444_alpha_to_420": ("444_8_alpha", YCBCR[1], 0, (1, 8)),
    "422_10_to_420": ("422_10", YCBCR[1], 0, (1, 10)),
    "422_10_to_420_8bit": ("422_10", YCBCR[1], 1, (1, 8)),
    "420_to_444": ("420_8", YCBCR[3], 0, (3, 8)),
    "420_to_420_converts_nothing": ("420_8", YCBCR[1], 0, (1, 8)),
    "grid_400_to_420": ("grid_400", YCBCR[1], 0, (1, 8)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_item_to_device_planes_equals_host_decode(capi, L, inputs, name):
    file, fmt, to_8bit, (chroma, bits) = CASES[name]
    data, threads = inputs[file]
    host = host_decode(capi, L, data, fmt, to_8bit, threads)
    assert (host["chroma"], host["bits"]) == (chroma, bits)
    if name == "as_coded_420_8_clap_odd":
        assert (host["w"], host["h"]) == (121, 77) and host["planes"][1].shape == (39, 61)
    if name == "as_coded_grid_cropped":
        assert (host["w"], host["h"]) == (117, 171)
    if name == "as_coded_400_8":
        assert len(host["planes"]) == 1
    if name == "grid_400_to_420":
        assert (host["planes"][1] == 128).all()  # (neutral chroma)
    if name == "420_to_420_converts_nothing":
        same = host_decode(capi, L, data, 0, 0, threads)
        assert all(np.array_equal(a, b) for a, b in zip(host["planes"], same["planes"]))
    has_alpha = host["alpha"] is not None
    assert has_alpha == ("alpha" in file)
    seen_subnormal = False
    for layout in (SEPARATE, SEMI):
        for dtype, scale, bias, pad, off, msb in variants(bits):
            what = f"{name} layout {layout} dtype {dtype} pad {pad} offset {off} msb {msb}"
            d, bufs, pitches = make_planes(capi, L, host, layout, dtype, scale, bias, pad, off, msb, want_alpha=has_alpha)
            rc, msg, out = to_planes(capi, L, data, fmt, d, to_8bit, threads)
            assert rc == 0, f"{what}: {msg}"
            meta = host["meta"]
            assert all(getattr(out, k) == v for k, v in meta.items() if k != "plane_size"), what
            assert [(out.plane_width[c], out.plane_height[c]) for c in range(3)] == meta["plane_size"], what
            assert out.used_ext_dst == 1 and [out.stride[c] for c in range(3)] == pitches[:3] and out.alpha_stride == pitches[3], what
            images = dest_images(host, layout, dtype, scale, bias, msb, has_alpha)
            check_buffers(bufs, images, pitches, what)
            if msb:
                assert np.array_equal(images[0], host["planes"][0] << 6)
            if dtype == F16 and scale[0] < 1e-5:
                seen_subnormal = seen_subnormal or any(bool(((im != 0) & (np.abs(im) < 2.0 ** -14)).any()) for im in images if im is not None)
    # float16 is subnormal below 2 ** -14: 8-bit samples 1 .. 63 at 2 ** -20, every non-zero deeper sample at 2 ** -28
    dark = any(bool(((p > 0) & (p < (64 if bits == 8 else 1 << 14))).any()) for p in host["planes"] + ([host["alpha"]] if has_alpha else []))
    assert seen_subnormal == dark, "the small-scale case and the float16 subnormals it must produce"
    if name in ("as_coded_420_8", "as_coded_422_10", "422_10_to_420", "420_to_444"):
        assert seen_subnormal, "the small-scale case produced no float16 subnormal"


@pytest.mark.parametrize("chroma,bits,w,h,src_pad", [(1, 8, 4032, 37, None), (2, 16, 1001, 9, None), (3, 8, 67, 3, None),
                                                     (1, 8, 200, 10, 2), (2, 16, 131, 5, 2)])
def test_planes_to_tensor_on_random_planes(capi, L, chroma, bits, w, h, src_pad):
    """hm_planes_to_tensor alone: every sample value, several workgroups per row, odd chroma widths.  src_pad None: source strides as
    the library's own (multiples of 64); 2: rows of width * sample bytes + 2, so no source row but the first is 16-byte aligned and
    every plane takes the element-wise path because of its SOURCE, whatever the destination's alignment."""
    import torch
    rng = np.random.default_rng(chroma * 1000 + w)
    dt = np.uint16 if bits > 8 else np.uint8
    cw, ch = (w if chroma == 3 else (w + 1) // 2), ((h + 1) // 2 if chroma == 1 else h)
    sizes = [(w, h), (cw, ch), (cw, ch), (w, h)]
    planes, keep = [], []
    srcs, strides = (C.c_void_p * 4)(), (C.c_int32 * 4)()
    for c, (pw, ph) in enumerate(sizes):
        stride = (pw * dt().itemsize + 63) // 64 * 64 + 64 if src_pad is None else pw * dt().itemsize + src_pad
        assert src_pad is None or stride % 16 != 0
        raw = rng.integers(0, 256, (ph, stride), dtype=np.uint8)
        planes.append(np.ascontiguousarray(raw[:, :pw * dt().itemsize]).view(dt).copy())
        keep.append(torch.from_numpy(raw).cuda())
        srcs[c], strides[c] = keep[-1].data_ptr(), stride
    if w * h >= 1 << 16:
        assert np.unique(planes[0]).size == 256  # (every sample value)
    host = dict(w=w, h=h, chroma=chroma, bits=bits, planes=planes[:3], alpha=planes[3], alpha_bits=bits)
    for layout in (SEPARATE, SEMI):
        for dtype, scale, bias, pad, off, msb in variants(bits):
            d, bufs, pitches = make_planes(capi, L, host, layout, dtype, scale, bias, pad, off, msb, want_alpha=True)
            rc = L.hm_planes_to_tensor(chroma, bits, w, h, bits, C.byref(srcs), C.byref(strides), C.byref(d), None)
            assert rc == 0, L.hm_last_error().decode()
            torch.cuda.synchronize()
            check_buffers(bufs, dest_images(host, layout, dtype, scale, bias, msb, True), pitches, f"layout {layout} dtype {dtype} pad {pad} offset {off} msb {msb}")


def test_alpha_plane(capi, L, inputs):
    import torch
    data, threads = inputs["420_8_alpha"]
    host = host_decode(capi, L, data, 0, 0, threads)
    assert host["alpha"] is not None and host["alpha"].shape == (64, 96)
    # plane[3].ptr NULL: the alpha plane is not written.  Y, room for an alpha plane and CbCr lie one behind the other in ONE allocation,
    # plane[3] carries the len and pitch that room would have, and the whole allocation is compared: the two planes exact, every other
    # byte - the alpha plane's room between them, the gaps, both ends - still 0xA5
    ysz, csz, gap = 96 * 64, 96 * 32, 256
    arena = Guarded(ysz + gap + ysz + gap + csz)
    d = capi.DevicePlanes()
    d.layout, d.dtype = SEMI, U8
    d.plane[0].ptr, d.plane[0].len = arena.ptr, ysz
    d.plane[1].ptr, d.plane[1].len = arena.ptr + 2 * (ysz + gap), csz
    d.plane[3].ptr, d.plane[3].len, d.plane[3].row_pitch = None, ysz, 96
    torch.cuda.synchronize()
    rc, msg, out = to_planes(capi, L, data, 0, d, 0, threads)
    assert rc == 0 and out.has_alpha == 1 and out.alpha_stride == 0 and [out.stride[c] for c in range(3)] == [96, 96, 0], msg
    images = dest_images(host, SEMI, U8, ONE, ZERO, 0, False)
    exp = np.full(arena.size, 0xA5, np.uint8)
    exp[arena.start:arena.start + ysz] = images[0].reshape(-1)
    exp[arena.start + 2 * (ysz + gap):arena.start + 2 * (ysz + gap) + csz] = images[1].reshape(-1)
    got = arena.host()
    assert np.array_equal(got, exp), f"alpha not asked for: {np.flatnonzero(got != exp).size} bytes differ, first at {np.flatnonzero(got != exp)[:1]}"
    # an image without alpha, plane[3] given: refused, nothing written
    plain, _ = inputs["420_8"]
    hp = host_decode(capi, L, plain, 0, 0, threads)
    d, bufs, pitches = make_planes(capi, L, hp, SEPARATE, U8, ONE, ZERO, 0, 0)
    extra = Guarded(200 * 136)
    d.plane[3].ptr, d.plane[3].len = extra.ptr, 200 * 136
    rc, msg, _ = to_planes(capi, L, plain, 0, d, 0, threads)
    assert rc == -1 and "no alpha" in msg, msg
    torch.cuda.synchronize()
    check_buffers(bufs + [extra], None, None, "plane[3] without alpha")
    # an 8-bit image whose alpha plane has 10 bits: an integer dtype cannot hold both (HM_ERR_UNSUPPORTED, nothing written); a float one
    # takes each plane at its own depth
    deep, _ = inputs["420_8_alpha10"]
    hd = host_decode(capi, L, deep, 0, 0, threads, alpha_bits=10)
    assert hd["bits"] == 8 and hd["alpha"].max() > 255 and hd["alpha"].max() < 1024
    d, bufs, pitches = make_planes(capi, L, hd, SEPARATE, U8, ONE, ZERO, 0, 0, want_alpha=True)
    rc, msg, _ = to_planes(capi, L, deep, 0, d, 0, threads)
    assert rc == -2 and "alpha plane of 10 bits" in msg, msg
    torch.cuda.synchronize()
    check_buffers(bufs, None, None, "alpha depth class")
    sc, bi = affine(255.0)
    for layout in (SEPARATE, SEMI):
        d, bufs, pitches = make_planes(capi, L, hd, layout, F32, sc, bi, 1, 0, want_alpha=True)
        rc, msg, _ = to_planes(capi, L, deep, 0, d, 0, threads)
        assert rc == 0, msg
        check_buffers(bufs, dest_images(hd, layout, F32, sc, bi, 0, True), pitches, "float planes of two depths")


def test_refusals_leave_every_plane_untouched(capi, L, inputs):
    import torch
    data, threads = inputs["420_8"]
    host = host_decode(capi, L, data, 0, 0, threads)
    hdr, _ = inputs["422_10"]
    host10 = host_decode(capi, L, hdr, 0, 0, threads)

    def refused(file, fmt, d, bufs, status, word, **kw):
        rc, msg, _ = to_planes(capi, L, file, fmt, d, threads=threads, **kw)
        assert rc == status and word in msg, (rc, msg)
        torch.cuda.synchronize()
        check_buffers(bufs, None, None, f"a refused call ({msg})")

    for layout in (SEPARATE, SEMI):
        # len short by one byte, plane by plane
        for c in (0, 1) + ((2,) if layout == SEPARATE else ()):
            d, bufs, _ = make_planes(capi, L, host, layout, U8, ONE, ZERO, 0, 0, shrink=c)
            refused(data, 0, d, bufs, -1, f"plane[{c}].len")
        # a host pointer: pageable and pinned
        d, bufs, _ = make_planes(capi, L, host, layout, U8, ONE, ZERO, 0, 0)
        pageable = np.full(200 * 136, 0x5A, np.uint8)
        keep = d.plane[1].ptr
        d.plane[1].ptr = pageable.ctypes.data
        refused(data, 0, d, bufs, -1, "plane[1].ptr")
        pinned = torch.full((200 * 136,), 0x5A, dtype=torch.uint8).pin_memory()
        d.plane[1].ptr = pinned.data_ptr()
        refused(data, 0, d, bufs, -1, "plane[1].ptr")
        assert (pageable == 0x5A).all() and bool((pinned == 0x5A).all())
        # overlapping planes: the chroma plane begins inside the last luma row
        d.plane[1].ptr = keep
        d.plane[0].ptr = keep - 200 * 136 + 1
        refused(data, 0, d, bufs, -1, "overlap")
        # U8 for a 10-bit result, U16 for an 8-bit one
        d, bufs, _ = make_planes(capi, L, host10, layout, U16, ONE, ZERO, 0, 0)
        d.dtype = U8
        refused(hdr, 0, d, bufs, -1, "dtype")
        d8, bufs8, _ = make_planes(capi, L, host, layout, F16, ONE, ZERO, 0, 0)
        d8.dtype = U16
        refused(data, 0, d8, bufs8, -1, "dtype")
    # an interleaved target, ext_dst, msb_aligned on bytes
    d, bufs, _ = make_planes(capi, L, host, SEPARATE, U8, ONE, ZERO, 0, 0)
    refused(data, 10, d, bufs, -1, "hm_decode_item_to_device")
    spare = np.full(64, 0x5A, np.uint8)
    refused(data, 0, d, bufs, -1, "ext_dst", ext_dst=spare.ctypes.data)
    d.msb_aligned = 1
    refused(data, 0, d, bufs, -1, "msb_aligned")
    # ... and the library still decodes after all of that
    d, bufs, pitches = make_planes(capi, L, host, SEMI, U8, ONE, ZERO, 0, 0)
    assert to_planes(capi, L, data, 0, d, 0, threads)[0] == 0
    check_buffers(bufs, dest_images(host, SEMI, U8, ONE, ZERO, 0, False), pitches, "after the refusals")


def _keep_the_default_stream_busy():
    """queues some 15 ms of work on the default stream (60 passes over 512 MB) and returns its tensor"""
    import torch
    x = torch.ones(128 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(60):
        x.mul_(1.0)
    return x


def test_destination_with_work_pending_on_the_default_stream(capi, L, inputs):
    """the caller still writes the planes on the default stream (params->stream NULL) when the decode is called: the decode's writes come
    behind that work"""
    import torch
    data, threads = inputs["grid_cropped"]
    host = host_decode(capi, L, data, 0, 0, threads)
    sc, bi = affine(255.0)
    d, bufs, pitches = make_planes(capi, L, host, SEMI, F32, sc, bi, 1, 0)
    busy = _keep_the_default_stream_busy()
    for g in bufs:
        if g is not None:
            g.t.fill_(0x11)
            g.t.fill_(0xA5)
    behind = torch.cuda.Event()
    behind.record()
    assert not behind.query(), "the pending work was over before the decode was called: the test shows nothing"
    rc, msg, _ = to_planes(capi, L, data, 0, d, 0, threads)
    assert rc == 0, msg
    check_buffers(bufs, dest_images(host, SEMI, F32, sc, bi, 0, False), pitches, "behind pending work")
    del busy


def _movie(n=5):
    frames = [synthutil.picture(49000 + i, width=200, height=136, qp=30) for i in range(n)]
    return frames, moovwriter.write_movie(frames, (200, 136))


@pytest.mark.parametrize("layout,dtype", [(SEMI, U8), (SEPARATE, F16)])
def test_frames_to_device_planes_equal_per_frame_host_decodes(capi, L, layout, dtype):
    import torch
    pics, buf = _movie(5)
    order = [3, 1, 5, 1]
    sc, bi = affine(255.0) if dtype == F16 else (ONE, ZERO)
    hosts = {k: host_decode(capi, L, buf, 0, 0, 4, item=k) for k in set(order)}
    n = len(order)
    dests = (capi.DevicePlanes * n)()
    held = []
    for k, fid in enumerate(order):
        d, bufs, pitches = make_planes(capi, L, hosts[fid], layout, dtype, sc, bi, k % 3, 0)
        dests[k] = d
        held.append((bufs, pitches))
    fh = C.c_void_p()
    assert L.hm_file_open(buf, len(buf), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(0, 4, 0, 0, None, None, 0, 0, 0, 0)
        out = (capi.Decoded * n)()
        failed = C.c_int32(-2)
        rc = L.hm_decode_frames_to_device_planes(fh, (C.c_uint32 * n)(*order), n, C.byref(prm), dests, out, C.byref(failed))
        assert rc == 0 and failed.value == -1, L.hm_last_error().decode()
        for k, fid in enumerate(order):
            assert (out[k].width, out[k].height, out[k].used_ext_dst, out[k].chroma, out[k].bit_depth) == (200, 136, 1, 1, 8) and not out[k].plane[0]
            check_buffers(held[k][0], dest_images(hosts[fid], layout, dtype, sc, bi, 0, False), held[k][1], f"frames[{k}] = {fid}")
        # a destination that is too short fails the call with its frame's index before anything is written
        fresh = []
        for k, fid in enumerate(order):
            d, bufs, pitches = make_planes(capi, L, hosts[fid], layout, dtype, sc, bi, 0, 0, shrink=1 if k == 2 else None)
            dests[k] = d
            fresh.append(bufs)
        rc = L.hm_decode_frames_to_device_planes(fh, (C.c_uint32 * n)(*order), n, C.byref(prm), dests, out, C.byref(failed))
        assert rc == -1 and failed.value == 2 and "plane[1].len" in L.hm_last_error().decode()
        torch.cuda.synchronize()
        for bufs in fresh:
            check_buffers(bufs, None, None, "a short destination")
    finally:
        L.hm_file_close(fh)
    # a broken frame (its sample runs past the end of the file) fails the call with its index; every destination stays as it was
    info = moovwriter.fork_movie_info(buf)
    broken = moovwriter.write_movie(pics, (200, 136), stsz_entries=info["sizes"][:4] + [info["sizes"][4] + 5000])
    assert L.hm_file_open(broken, len(broken), C.byref(fh)) == 0
    try:
        fresh = []
        for k, fid in enumerate(order):
            d, bufs, pitches = make_planes(capi, L, hosts[fid], layout, dtype, sc, bi, 0, 0)
            dests[k] = d
            fresh.append(bufs)
        rc = L.hm_decode_frames_to_device_planes(fh, (C.c_uint32 * n)(*order), n, C.byref(prm), dests, out, C.byref(failed))
        assert rc < 0 and failed.value == 2, L.hm_last_error().decode()
        torch.cuda.synchronize()
        for bufs in fresh:
            check_buffers(bufs, None, None, "a broken frame")
    finally:
        L.hm_file_close(fh)


def test_pipeline_to_device_planes_equals_host_decodes_in_submission_order(capi, L, inputs):
    """six files of two kinds (8-bit 4:2:0, 10-bit 4:2:2) to NV12 through HM_OUT_YCBCR_420 | HM_OUT_YCBCR_8BIT, two in flight"""
    files = [inputs["420_8"][0], inputs["422_10"][0]] * 3
    fmt = YCBCR[1]
    hosts = [host_decode(capi, L, data, fmt, 1, 2) for data in files[:2]] * 3
    assert all((hst["chroma"], hst["bits"]) == (1, 8) for hst in hosts)
    cfg = capi.PipelineConfig(4, 2, fmt | YCBCR_8BIT, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    dests, order, full_seen = [], [], 0
    try:
        def take():
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0
            assert r.status == 0, L.hm_last_error().decode()
            hst = hosts[r.tag]
            assert (r.image.width, r.image.height, r.image.used_ext_dst, r.image.chroma, r.image.bit_depth) == (hst["w"], hst["h"], 1, 1, 8) and not r.image.plane[0]
            d, bufs, pitches = dests[r.tag]
            check_buffers(bufs, dest_images(hst, SEMI, U8, ONE, ZERO, 0, False), pitches, f"file {r.tag}")  # (complete when handed out)
            order.append(r.tag)
            L.hm_pipeline_release(pipe, C.byref(r))
        for k, data in enumerate(files):
            dests.append(make_planes(capi, L, hosts[k], SEMI, U8, ONE, ZERO, k % 3, 0))
            while True:
                rc = L.hm_pipeline_submit_to_device_planes(pipe, data, len(data), 0, k, C.byref(dests[k][0]))
                assert rc >= 0, L.hm_last_error().decode()
                if rc == 0:
                    break
                full_seen += 1
                take()
        # a destination that is refused fails the submit: nothing queued, nothing written
        d, bufs, _ = make_planes(capi, L, hosts[0], SEMI, U8, ONE, ZERO, 0, 0, shrink=1)
        while L.hm_pipeline_pending(pipe) >= 2:
            take()
        assert L.hm_pipeline_submit_to_device_planes(pipe, files[0], len(files[0]), 0, 99, C.byref(d)) == -1
        check_buffers(bufs, None, None, "a refused submit")
        while L.hm_pipeline_pending(pipe):
            take()
    finally:
        L.hm_pipeline_destroy(pipe)
    assert order == list(range(len(files))) and full_seen > 0


def test_python_decode_to_planes(pkg, capi, L, inputs, tmp_path):
    import torch
    data, threads = inputs["420_8_clap_odd"]
    host = host_decode(capi, L, data, 0, 0, threads)
    Y, Cb, Cr = host["planes"]
    # defaults: as coded, planar, the file's own integer type
    y, cb, cr = pkg.decode_to_planes(data)
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in (y, cb, cr))
    assert tuple(y.shape) == (77, 121) and tuple(cb.shape) == tuple(cr.shape) == (39, 61)
    assert np.array_equal(y.cpu().numpy(), Y) and np.array_equal(cb.cpu().numpy(), Cb) and np.array_equal(cr.cpu().numpy(), Cr)
    # NV12 as float16 with scale / bias
    sc, bi = affine(255.0)
    y, cbcr = pkg.decode_to_planes(data, layout="semiplanar", dtype=torch.float16, scale=sc, bias=bi, host_threads=threads)
    assert tuple(cbcr.shape) == (39, 61, 2) and cbcr.dtype == torch.float16
    assert np.array_equal(y.cpu().numpy().view(np.uint16), convert(Y, 0, F16, sc, bi, 0).view(np.uint16))
    assert np.array_equal(cbcr.cpu().numpy()[:, :, 0].view(np.uint16), np.ascontiguousarray(convert(Cb, 1, F16, sc, bi, 0)).view(np.uint16))
    assert np.array_equal(cbcr.cpu().numpy()[:, :, 1].view(np.uint16), np.ascontiguousarray(convert(Cr, 2, F16, sc, bi, 0)).view(np.uint16))
    # a 10-bit file: uint16 by default; P010 with msb_aligned; a chroma target with to_8bit
    hdr, _ = inputs["422_10"]
    h10 = host_decode(capi, L, hdr, 0, 0, threads)
    y, cbcr = pkg.decode_to_planes(hdr, layout="semiplanar", msb_aligned=True)
    assert y.dtype == torch.uint16 and tuple(cbcr.shape) == (96, 80, 2)
    assert np.array_equal(y.cpu().numpy(), h10["planes"][0] << 6) and np.array_equal(cbcr.cpu().numpy()[:, :, 1], h10["planes"][2] << 6)
    h8 = host_decode(capi, L, hdr, YCBCR[1], 1, threads)
    y, cb, cr = pkg.decode_to_planes(hdr, chroma="420", to_8bit=True)
    assert y.dtype == torch.uint8 and tuple(cb.shape) == (48, 80) and np.array_equal(cr.cpu().numpy(), h8["planes"][2])
    # out= is honoured, its row strides too: the columns behind the planes stay as they were
    big_y = torch.full((77 + 2, 121 + 9), 7, dtype=torch.uint8, device="cuda")
    big_c = torch.full((39, 61 + 5, 2), 7, dtype=torch.uint8, device="cuda")
    outs = (big_y[1:78, :121], big_c[:, :61])
    res = pkg.decode_to_planes(data, layout="semiplanar", out=outs)
    assert res[0] is outs[0] and res[1] is outs[1]
    gy, gc = big_y.cpu().numpy(), big_c.cpu().numpy()
    assert np.array_equal(gy[1:78, :121], Y) and (gy[0] == 7).all() and (gy[78] == 7).all() and (gy[:, 121:] == 7).all()
    assert np.array_equal(gc[:, :61, 0], Cb) and np.array_equal(gc[:, :61, 1], Cr) and (gc[:, 61:] == 7).all()
    with pytest.raises(ValueError, match="shape"):
        pkg.decode_to_planes(data, out=(torch.empty((77, 122), dtype=torch.uint8, device="cuda"),) + tuple(torch.empty((39, 61), dtype=torch.uint8, device="cuda") for _ in range(2)))
    with pytest.raises(capi.HmError, match="dtype"):
        pkg.decode_to_planes(data, dtype=torch.uint16)
    # the alpha plane comes with the image that has one; a 4:0:0 picture is Y alone
    ha = host_decode(capi, L, inputs["420_8_alpha"][0], 0, 0, threads)
    planes = pkg.decode_to_planes(inputs["420_8_alpha"][0])
    assert len(planes) == 4 and np.array_equal(planes[3].cpu().numpy(), ha["alpha"])
    assert len(pkg.decode_to_planes(inputs["400_8"][0])) == 1
    # alpha=False leaves the alpha plane out: the way to an integer dtype for an 8-bit image with a 10-bit alpha plane
    deep = inputs["420_8_alpha10"][0]
    with pytest.raises(capi.HmError, match="alpha plane of 10 bits"):
        pkg.decode_to_planes(deep)
    hd = host_decode(capi, L, deep, 0, 0, threads, alpha_bits=10)
    planes = pkg.decode_to_planes(deep, alpha=False)
    assert len(planes) == 3 and planes[0].dtype == torch.uint8 and all(np.array_equal(t.cpu().numpy(), p) for t, p in zip(planes, hd["planes"]))
    planes = pkg.decode_batch_to_planes([deep, inputs["420_8_alpha"][0]], alpha=False, layout="semiplanar")
    assert len(planes) == 2 and np.array_equal(planes[0][0].cpu().numpy(), hd["planes"][0]) and np.array_equal(planes[0][1].cpu().numpy(), ha["planes"][0])
    # sequence: T x ... tensors
    pics, movie = _movie(3)
    hosts = [host_decode(capi, L, movie, 0, 0, 4, item=k) for k in (1, 2, 3)]
    y, cbcr = pkg.decode_sequence_to_planes(movie, frames=[3, 1], layout="semiplanar")
    assert tuple(y.shape) == (2, 136, 200) and tuple(cbcr.shape) == (2, 68, 100, 2) and y.dtype == torch.uint8
    assert np.array_equal(y[0].cpu().numpy(), hosts[2]["planes"][0]) and np.array_equal(cbcr[1].cpu().numpy()[:, :, 0], hosts[0]["planes"][1])
    # batch: N x ... tensors through the pipeline; a file of another size or format is refused by name
    files = [heifwriter.write_heic([synthutil.picture(49500 + i, width=96, height=64)], (96, 64)) for i in range(5)]
    hb = [host_decode(capi, L, fdata, 0, 0, 2) for fdata in files]
    y, cb, cr = pkg.decode_batch_to_planes(files, max_in_flight=2)
    assert tuple(y.shape) == (5, 64, 96) and tuple(cb.shape) == tuple(cr.shape) == (5, 32, 48)
    for k in range(5):
        assert np.array_equal(y[k].cpu().numpy(), hb[k]["planes"][0]) and np.array_equal(cr[k].cpu().numpy(), hb[k]["planes"][2]), f"file {k}"
    odd = tmp_path / "other_size.heic"
    odd.write_bytes(inputs["420_8"][0])
    with pytest.raises(ValueError, match="other_size.heic"):
        pkg.decode_batch_to_planes(files[:2] + [odd])
    with pytest.raises(ValueError, match=r"files\[1\]"):
        pkg.decode_batch_to_planes([files[0], inputs["444_8"][0]])
