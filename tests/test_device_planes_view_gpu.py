"""GPU: planar views - a view (hm_device_view) into planar YCbCr in caller-owned device memory (hm_decode_item_to_device_planes_view,
hm_decode_frames_to_device_planes_view, hm_pipeline_submit_to_device_planes_view, hm_resample_planes_to_tensor, hm_plan_planes_view
and the crop= / size= / filter= arguments of the Python decode_to_planes family).  Everything is bit-exact: the reference of every
case is the same item decoded by hm_decode_item to host memory, through the numpy restatement tests/planes_view_ref.py (every plane
an image of its own; float16 is numpy's astype).  Every plane sits in a buffer of its own between two guard regions, pre-filled with
0xA5, and the WHOLE buffer is compared with its expected image, as tests/test_device_planes_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import hevcutil
import moovwriter
import planes_view_ref as ref
import synthutil
import test_device_planes_gpu as base

pytestmark = pytest.mark.gpu
SEPARATE, SEMI = base.SEPARATE, base.SEMI
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
ELEM, ONE, ZERO, YCBCR = base.ELEM, base.ONE, base.ZERO, base.YCBCR
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = ref.TRIANGLE, ref.NEAREST, ref.CUBIC, ref.LANCZOS3
FILTERS = (TRIANGLE, NEAREST, CUBIC, LANCZOS3)
capi, L, inputs = base.capi, base.L, base.inputs  # (the fixtures of that file: the same small inputs)


def make_view(capi, crop, size, filt):
    v = capi.DeviceView()
    if crop:
        v.crop_x, v.crop_y, v.crop_w, v.crop_h = crop
    if size:
        v.out_w, v.out_h = size
    v.filter = filt
    return v


def make_planes(capi, L, chroma, bits, ow, oh, images, layout, dtype, scale, bias, pad=0, off=0, msb=0, shrink=None, odd=None):
    """(hm_device_planes, guarded buffers per plane (None: no plane), pitches in use) for the expected `images` of an ow x oh result.
    pad / off: as tests/test_device_planes_gpu.py (1: 21 elements more per row, 2: 64 bytes more; a pointer offset in elements), and
    pad 3: the next multiple of 16 bytes plus 32 - with off 0 the plane takes 16-byte stores whatever its width, ragged last group included;
    odd: that plane alone gets a pointer offset of 2 bytes (one element of the 16-bit types) and a pitch that is no multiple of 16."""
    d = capi.DevicePlanes()
    d.layout, d.dtype, d.msb_aligned = layout, dtype, msb
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    pitches, offs = [0] * 4, [0] * 4
    for c, im in enumerate(images):
        if im is None:
            continue
        tight = im.shape[1] * ELEM[dtype]
        pitches[c] = tight if not pad else (tight + 15) // 16 * 16 + 32 if pad == 3 else tight + (21 * ELEM[dtype] if pad == 1 else 64)
        offs[c] = off * ELEM[dtype]
        if odd == c:
            pitches[c] = (tight + 15) // 16 * 16 + 4 * ((ELEM[dtype] + 1) // 2)
            offs[c] = 2 if ELEM[dtype] <= 2 else 4
            assert pitches[c] % 16 != 0
        d.plane[c].row_pitch = pitches[c] if (pad or odd == c) else 0
    if images[3] is not None:
        d.plane[3].ptr = 1 << 20  # (hm_device_planes_bytes only asks whether it is given)
    need = (C.c_int64 * 4)()
    total = L.hm_device_planes_bytes(chroma, bits, ow, oh, C.byref(d), C.byref(need))
    assert total > 0, L.hm_last_error().decode()
    bufs = [None] * 4
    for c, im in enumerate(images):
        if im is None:
            continue
        assert need[c] == pitches[c] * (im.shape[0] - 1) + im.shape[1] * ELEM[dtype], (c, need[c], im.shape)
        bufs[c] = base.Guarded(need[c], offs[c])
        d.plane[c].ptr, d.plane[c].len = bufs[c].ptr, need[c] - (1 if shrink == c else 0)
    import torch
    torch.cuda.synchronize()
    return d, bufs, pitches


def item_view(capi, L, data, fmt, view, d, to_8bit=0, threads=2, item=0, strict=0, lib=None):
    lib = lib or L
    fh = C.c_void_p()
    assert lib.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, strict, to_8bit)
        out = capi.Decoded()
        rc = lib.hm_decode_item_to_device_planes_view(fh, item or lib.hm_file_primary_item(fh), C.byref(prm), C.byref(view), C.byref(d), C.byref(out))
        msg = lib.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        lib.hm_file_close(fh)


def int_dtype(bits):
    return U16 if bits > 8 else U8


def check_item(capi, L, data, fmt, to_8bit, host, crop, size, filt, combos, what, alpha=None):
    """one view of one item for every (layout, dtype, scale, bias, pad, off, msb, odd plane) of `combos`, the sums computed once"""
    want_alpha = host["alpha"] is not None if alpha is None else alpha
    r, moved = ref.sums(host, crop, size, filt, want_alpha)
    ow, oh = r[0].shape[1], r[0].shape[0]
    view = make_view(capi, crop, size, filt)
    for layout, dtype, scale, bias, pad, off, msb, odd in combos:
        tag = f"{what} crop {crop} size {size} filter {filt} layout {layout} dtype {dtype} pad {pad} offset {off} msb {msb} odd {odd}"
        images = ref.images_from(r, moved, host, layout, dtype, scale, bias, msb)
        d, bufs, pitches = make_planes(capi, L, host["chroma"], host["bits"], ow, oh, images, layout, dtype, scale, bias, pad, off, msb, odd=odd)
        rc, msg, out = item_view(capi, L, data, fmt, view, d, to_8bit)
        assert rc == 0, f"{tag}: {msg}"
        assert (out.width, out.height, out.used_ext_dst, out.chroma, out.bit_depth) == (ow, oh, 1, host["chroma"], host["bits"]), tag
        sizes = [(im.shape[1] // (2 if layout == SEMI and c == 1 else 1), im.shape[0]) for c, im in enumerate(images[:3]) if im is not None]
        if layout == SEMI and len(sizes) == 2:
            sizes.append(sizes[1])
        assert [(out.plane_width[c], out.plane_height[c]) for c in range(len(sizes))] == sizes, tag
        assert [out.stride[c] for c in range(3)] == pitches[:3] and out.alpha_stride == pitches[3], tag
        base.check_buffers(bufs, images, pitches, tag)


def test_every_filter_dtype_and_layout_on_420(capi, L, inputs):
    data, threads = inputs["420_8"]
    host = base.host_decode(capi, L, data, 0, 0, threads)
    assert (host["w"], host["h"], host["chroma"], host["bits"]) == (200, 136, 1, 8)
    sc, bi = base.affine(255.0)
    combos = [(layout, dtype, *((sc, bi) if dtype in (F16, F32) else (ONE, ZERO)), pad, off, 0, None)
              for layout in (SEPARATE, SEMI) for dtype, pad, off in ((U8, 0, 0), (U8, 3, 0), (U8, 1, 1), (F16, 3, 0), (F16, 2, 0), (F32, 3, 0), (F32, 1, 1))]
    # 77 x 51: luma crosses a wave's 64 columns, chroma is 39 wide, both ragged: every combination.  16 x 16: whole vectors only;
    # 30 x 30 -> 77 x 77: up-sampling; 1 x 1 from 200 x 136: a reduction by 200, 400 taps on the x axis - inside the triangle's limit
    # and NEAREST's alone.  Those three with one pitch (16-byte stores) per dtype and layout.
    fewer = [cb for cb in combos if (cb[4], cb[5]) == (3, 0)]
    assert len(combos) == 14 and len(fewer) == 6
    for filt in FILTERS:
        check_item(capi, L, data, 0, 0, host, None, (77, 51), filt, combos, "420_8")
        check_item(capi, L, data, 0, 0, host, None, (16, 16), filt, fewer, "420_8")
        check_item(capi, L, data, 0, 0, host, (10, 20, 30, 30), (77, 77), filt, fewer, "420_8")
    for filt in (TRIANGLE, NEAREST):
        check_item(capi, L, data, 0, 0, host, None, (1, 1), filt, fewer, "420_8")


def test_crop_alone_moves_the_samples(capi, L, inputs):
    sc, bi = base.affine(255.0)
    for name, crop in (("420_8", (10, 20, 77, 51)), ("420_8", (0, 0, 200, 136)), ("422_10", (2, 3, 33, 20)), ("444_8", (5, 7, 19, 11)), ("400_8", (1, 1, 17, 9))):
        data, threads = inputs[name]
        host = base.host_decode(capi, L, data, 0, 0, threads)
        integer = int_dtype(host["bits"])
        combos = [(layout, dtype, s, b, pad, 0, msb, None) for layout in (SEPARATE, SEMI)
                  for dtype, s, b, pad, msb in ((integer, ONE, ZERO, 0, 0), (integer, ONE, ZERO, 1, 1 if integer == U16 else 0), (F32, sc, bi, 2, 0))]
        check_item(capi, L, data, 0, 0, host, crop, None, TRIANGLE, combos, name)
        r, _ = ref.sums(host, crop, None, TRIANGLE, False)
        x, y, w, h = crop
        assert np.array_equal(r[0], host["planes"][0][y:y + h, x:x + w])


@pytest.mark.parametrize("name,fmt,to_8bit", [("422_10", 0, 0), ("444_8", 0, 0), ("400_8", 0, 0), ("grid_cropped", 0, 0), ("420_8_alpha", 0, 0),
                                              ("420_8_clap_odd", 0, 0), ("444_8_alpha", YCBCR[1], 0), ("422_10", YCBCR[1], 1), ("420_8", YCBCR[3], 0)])
def test_other_formats_and_targets(capi, L, inputs, name, fmt, to_8bit):
    data, threads = inputs[name]
    host = base.host_decode(capi, L, data, fmt, to_8bit, threads)
    bits, integer = host["bits"], int_dtype(host["bits"])
    sc, bi = base.affine(float((1 << bits) - 1))
    if name == "420_8_clap_odd":
        assert (host["w"], host["h"]) == (121, 77)
    combos = [(layout, dtype, s, b, pad, off, msb, None) for layout in (SEPARATE, SEMI)
              for dtype, s, b, pad, off, msb in ((integer, ONE, ZERO, 3, 0, 0), (integer, ONE, ZERO, 1, 1, 1 if bits > 8 else 0), (integer, ONE, ZERO, 3, 0, 1 if bits > 8 else 0),
                                                 (F32, sc, bi, 3, 0, 0), (F16, sc, bi, 2, 0, 0))]
    W, H = host["w"], host["h"]
    for crop, size in ((None, (77, 51)), ((2, 2, min(30, W - 2), min(30, H - 2)), (77, 77)), ((W // 4 * 2, H // 4 * 2, W - W // 4 * 2, H - H // 4 * 2), (16, 16))):
        for filt in (TRIANGLE, NEAREST, LANCZOS3) if crop is None else (CUBIC,):
            check_item(capi, L, data, fmt, to_8bit, host, crop, size, filt, combos, name)
    if bits > 8:  # msb_aligned: the rounded, clamped sum << 6
        r, moved = ref.sums(host, None, (77, 51), TRIANGLE, False)
        im = ref.images_from(r, moved, host, SEPARATE, U16, ONE, ZERO, 1)
        assert np.array_equal(im[0], ref.vf.to_integer(r[0], 1023).astype(np.uint16) << 6) and int(im[0].max()) > 1023


def test_an_unaligned_plane_takes_the_element_path_alone(capi, L, inputs):
    """pointer offset 2 and a pitch that is no multiple of 16 on ONE plane: it takes the element-wise path for that plane alone, its
    neighbours (pitches of a multiple of 16 bytes, pad 3) stay on the vector path with their ragged last groups"""
    data, threads = inputs["420_8_alpha"]
    host = base.host_decode(capi, L, data, 0, 0, threads)
    assert host["alpha"] is not None
    sc, bi = base.affine(255.0)
    for filt in (TRIANGLE, LANCZOS3, NEAREST):
        combos = [(layout, dtype, s, b, 3, 0, 0, odd) for layout in (SEPARATE, SEMI) for dtype, s, b in ((U8, ONE, ZERO), (F16, sc, bi), (F32, sc, bi))
                  for odd in ((0, 1, 2, 3) if layout == SEPARATE else (0, 1, 3))]
        check_item(capi, L, data, 0, 0, host, None, (77, 51), filt, combos, "420_8_alpha")


def test_alpha_of_the_other_depth_under_a_float_dtype(capi, L, inputs):
    data, threads = inputs["420_8_alpha10"]
    host = base.host_decode(capi, L, data, 0, 0, threads, alpha_bits=10)
    assert host["bits"] == 8 and host["alpha"].max() > 255
    sc, bi = base.affine(255.0)
    combos = [(layout, dtype, sc, bi, pad, 0, 0, None) for layout in (SEPARATE, SEMI) for dtype, pad in ((F32, 0), (F16, 1))]
    for crop, size, filt in ((None, (77, 51), TRIANGLE), ((2, 2, 30, 30), (77, 77), CUBIC), (None, (16, 16), NEAREST), ((4, 6, 31, 17), None, TRIANGLE)):
        check_item(capi, L, data, 0, 0, host, crop, size, filt, combos, "420_8_alpha10")
    # an integer dtype cannot hold both depths: refused, nothing written
    r, moved = ref.sums(host, None, (16, 16), TRIANGLE, True)
    images = ref.images_from(r, moved, host, SEPARATE, U8, ONE, ZERO, 0)
    d, bufs, _ = make_planes(capi, L, 1, 8, 16, 16, images, SEPARATE, U8, ONE, ZERO)
    rc, msg, _ = item_view(capi, L, data, 0, make_view(capi, None, (16, 16), TRIANGLE), d)
    assert rc == -2 and "alpha plane of 10 bits" in msg, msg
    import torch
    torch.cuda.synchronize()
    base.check_buffers(bufs, None, None, "alpha depth class")


def _edge_planes(bits, seed):
    """synthetic planes of hard 0 / peak edges: blocks of random extent 1 .. 5, so that the negative lobes of the cubic and Lanczos
    weights overshoot on both sides"""
    rng = np.random.default_rng(seed)
    peak = (1 << bits) - 1

    def plane(w, h):
        cols = np.repeat(rng.integers(0, 2, w), rng.integers(1, 6, w))[:w]
        rows = np.repeat(rng.integers(0, 2, h), rng.integers(1, 6, h))[:h]
        return ((cols[None, :] ^ rows[:, None]) * peak).astype(np.uint16 if bits > 8 else np.uint8)
    return [plane(120, 90), plane(60, 45), plane(60, 45), plane(120, 90)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("filt", [CUBIC, LANCZOS3], ids=["cubic", "lanczos3"])
def test_clamp_census_on_hard_edges(capi, L, filt, bits):
    """the step on its own (hm_resample_planes_to_tensor) on hard edges: the restatement alone first shows that at least one sample is
    clamped at 0 and at least one at the plane's own peak - for 10 bits at least one unclamped sum exceeds 1023 while staying below
    65535, where a kernel that clamps to the wrong peak turns red"""
    import torch
    peak = (1 << bits) - 1
    planes = _edge_planes(bits, 9000 + bits)
    host = dict(w=120, h=90, chroma=1, bits=bits, planes=planes[:3], alpha=planes[3], alpha_bits=bits)
    crop, size = (2, 2, 117, 87), (77, 51)
    r, moved = ref.sums(host, crop, size, filt, True)
    for c in range(4):
        raw = np.trunc(r[c] + np.float32(0.5))
        assert (raw < 0).any() and (raw > peak).any(), f"plane {c}: the pattern clamps nothing"
        if bits == 10:
            assert ((raw > 1023) & (raw < 65535)).any()
    keep, srcs, strides = [], (C.c_void_p * 4)(), (C.c_int32 * 4)()
    for c, p in enumerate(planes):
        stride = (p.shape[1] * p.itemsize + 63) // 64 * 64
        raw = np.zeros((p.shape[0], stride), np.uint8)
        raw[:, :p.shape[1] * p.itemsize] = p.view(np.uint8).reshape(p.shape[0], -1)
        keep.append(torch.from_numpy(raw).cuda())
        srcs[c], strides[c] = keep[-1].data_ptr(), stride
    view = make_view(capi, crop, size, filt)
    for layout in (SEPARATE, SEMI):
        for pad, msb in ((3, 0), (1, 1 if bits > 8 else 0)):
            images = ref.images_from(r, moved, host, layout, int_dtype(bits), ONE, ZERO, msb)
            assert all(int(im.max()) == peak << (6 if msb else 0) and int(im.min()) == 0 for im in images if im is not None)
            d, bufs, pitches = make_planes(capi, L, 1, bits, 77, 51, images, layout, int_dtype(bits), ONE, ZERO, pad, 0, msb)
            rc = L.hm_resample_planes_to_tensor(1, bits, 120, 90, bits, C.byref(srcs), C.byref(strides), C.byref(view), C.byref(d), None)
            assert rc == 0, L.hm_last_error().decode()
            torch.cuda.synchronize()
            base.check_buffers(bufs, images, pitches, f"hard edges, {bits} bits, filter {filt}, layout {layout}, msb {msb}")


def _movie(n=8):
    frames = [synthutil.picture(49600 + i, width=200, height=136, qp=30) for i in range(n)]
    return moovwriter.write_movie(frames, (200, 136))


@pytest.fixture()
def hooks(pkg, capi):
    """libheif_mi355x_test.so with the image entry points bound (a library of its own, with its own knobs, put back behind the test)"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(capi.TEST_LIB_PATH)
    T.hm_last_error.restype = C.c_char_p
    T.hm_debug_set.argtypes = [C.c_char_p, C.c_int]
    capi.bind_image(T)
    try:
        yield T
    finally:
        assert T.hm_debug_set(b"view_batch_bytes", 0) == 0


def test_frames_equal_item_calls_in_one_grouped_write(capi, L, hooks):
    import torch
    movie = _movie(8)
    order = [3, 1, 8, 1, 5, 2, 7, 6, 4]  # a repeated and a reordered frame ID
    n = len(order)
    crop, size, filt = (10, 20, 150, 100), (77, 51), CUBIC
    view = make_view(capi, crop, size, filt)
    sc, bi = base.affine(255.0)
    hosts = {k: base.host_decode(capi, L, movie, 0, 0, 4, item=k) for k in set(order)}
    for layout, dtype, scale, bias in ((SEMI, U8, ONE, ZERO), (SEPARATE, F16, sc, bi)):
        expected = {k: ref.dest_images(hosts[k], layout, dtype, scale, bias, 0, False, crop, size, filt) for k in hosts}
        # eight item calls: the bytes every form below must give
        singles = {}
        for fid in sorted(hosts):
            d, bufs, pitches = make_planes(capi, L, 1, 8, 77, 51, expected[fid], layout, dtype, scale, bias)
            rc, msg, _ = item_view(capi, L, movie, 0, view, d, item=fid, threads=4)
            assert rc == 0, msg
            base.check_buffers(bufs, expected[fid], pitches, f"item call of frame {fid}")
            singles[fid] = [None if b is None else b.host() for b in bufs]

        def frames_call(lib, shrink_at=None):
            dests, held = (capi.DevicePlanes * n)(), []
            for k, fid in enumerate(order):
                d, bufs, pitches = make_planes(capi, L, 1, 8, 77, 51, expected[fid], layout, dtype, scale, bias, shrink=1 if k == shrink_at else None)
                dests[k] = d
                held.append((bufs, pitches))
            fh = C.c_void_p()
            assert lib.hm_file_open(movie, len(movie), C.byref(fh)) == 0
            try:
                prm = capi.DecodeParams(0, 4, 0, 0, None, None, 0, 0, 0, 0)
                out = (capi.Decoded * n)()
                failed = C.c_int32(-2)
                rc = lib.hm_decode_frames_to_device_planes_view(fh, (C.c_uint32 * n)(*order), n, C.byref(prm), C.byref(view), dests, out, C.byref(failed))
                return rc, failed.value, lib.hm_last_error().decode(), held, [(out[k].width, out[k].height, out[k].plane_width[1], out[k].plane_height[1]) for k in range(n)]
            finally:
                lib.hm_file_close(fh)

        # one group, one chunk; then view_batch_bytes set so that a chunk holds 3 frames (the intermediate of a frame: Y 80 x 100, Cb and Cr 48 x 50 float32)
        per_frame = (80 * 100 + 2 * 48 * 50) * 4
        for lib, bound in ((L, None), (hooks, 3 * per_frame + 100), (hooks, 1)):
            if bound is not None:
                assert lib.hm_debug_set(b"view_batch_bytes", bound) == 0
            rc, failed, msg, held, sizes = frames_call(lib)
            assert rc == 0 and failed == -1, msg
            assert sizes == [(77, 51, 39, 26)] * n
            for k, fid in enumerate(order):
                base.check_buffers(held[k][0], expected[fid], held[k][1], f"frames[{k}] = {fid}, bound {bound}")
                assert all(np.array_equal(b.host(), s) for b, s in zip(held[k][0], singles[fid]) if b is not None)
        # a frame whose destination is short fails the call with its index, every buffer still 0xA5
        rc, failed, msg, held, _ = frames_call(L, shrink_at=4)
        assert rc == -1 and failed == 4 and "plane[1].len" in msg, (rc, failed, msg)
        torch.cuda.synchronize()
        for bufs, _ in held:
            base.check_buffers(bufs, None, None, "a short destination")


def test_pipeline_files_of_different_sizes_into_equal_nv12_surfaces(capi, L, inputs):
    names = ["420_8", "grid_cropped", "420_8_clap_odd", "420_8_alpha"]
    files = [inputs[nm][0] for nm in names]
    hosts = [base.host_decode(capi, L, data, 0, 0, 2) for data in files]
    assert len({(h["w"], h["h"]) for h in hosts}) == 4 and all((h["chroma"], h["bits"]) == (1, 8) for h in hosts)
    size, filt = (64, 48), TRIANGLE
    view = make_view(capi, None, size, filt)
    cfg = capi.PipelineConfig(4, 2, 0, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    dests, order = [], []
    try:
        def take():
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0
            assert r.status == 0, L.hm_last_error().decode()
            assert (r.image.width, r.image.height, r.image.used_ext_dst) == (64, 48, 1)
            d, bufs, pitches, images = dests[r.tag]
            base.check_buffers(bufs, images, pitches, f"file {r.tag}")  # (complete when handed out)
            order.append(r.tag)
            L.hm_pipeline_release(pipe, C.byref(r))
        for k, data in enumerate(files):
            images = ref.dest_images(hosts[k], SEMI, U8, ONE, ZERO, 0, False, None, size, filt)
            dests.append(make_planes(capi, L, 1, 8, 64, 48, images, SEMI, U8, ONE, ZERO, k % 3) + (images,))
            while True:
                rc = L.hm_pipeline_submit_to_device_planes_view(pipe, data, len(data), 0, k, C.byref(view), C.byref(dests[k][0]))
                assert rc >= 0, L.hm_last_error().decode()
                if rc == 0:
                    break
                take()
        # a view that is refused fails the submit: nothing queued, nothing written
        images = ref.dest_images(hosts[0], SEMI, U8, ONE, ZERO, 0, False, None, size, filt)
        d, bufs, _ = make_planes(capi, L, 1, 8, 64, 48, images, SEMI, U8, ONE, ZERO)
        while L.hm_pipeline_pending(pipe) >= 2:
            take()
        odd = make_view(capi, (1, 0, 64, 48), size, filt)
        assert L.hm_pipeline_submit_to_device_planes_view(pipe, files[0], len(files[0]), 0, 99, C.byref(odd), C.byref(d)) == -1
        base.check_buffers(bufs, None, None, "a refused submit")
        while L.hm_pipeline_pending(pipe):
            take()
    finally:
        L.hm_pipeline_destroy(pipe)
    assert order == list(range(len(files)))


def _cut_short(picture):
    nals = hevcutil.split_nals(picture)
    return hevcutil.join_nals(nals[:-1] + [nals[-1][:len(nals[-1]) // 2]])


def test_sub_grid(capi, L, inputs):
    """of the 3 x 2 grid of 64 x 64 tiles (canvas 117 x 171) only the tiles the crop touches are decoded where the picture is taken as
    coded; an HM_OUT_YCBCR_* chain decodes the whole grid"""
    import torch
    data, threads = inputs["grid_cropped"]
    host = base.host_decode(capi, L, data, 0, 0, threads)
    host444 = base.host_decode(capi, L, data, YCBCR[3], 0, threads)
    assert (host["w"], host["h"]) == (117, 171) and host444["chroma"] == 3
    cases = {"inside_one_tile": ((70, 70, 30, 40), (1, 1, 1, 1)), "across_four": ((50, 100, 40, 50), (1, 2, 0, 2))}

    def plan(fmt, crop, size, which):
        fh = C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
        try:
            prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
            t = (C.c_int32 * 4)()
            assert which(fh, L.hm_file_primary_item(fh), C.byref(prm), C.byref(make_view(capi, crop, size, TRIANGLE)), C.byref(t)) == 0
            return tuple(t)
        finally:
            L.hm_file_close(fh)
    sc, bi = base.affine(255.0)
    combos = [(SEMI, U8, ONE, ZERO, 3, 0, 0, None), (SEPARATE, F32, sc, bi, 1, 0, 0, None)]
    for name, (crop, tiles) in cases.items():
        assert plan(0, crop, (20, 30), L.hm_plan_planes_view) == tiles, name
        assert plan(0, crop, (20, 30), L.hm_plan_view) == (0, 3, 0, 2)  # (hm_plan_view's own answer for the planar formats stays)
        assert plan(YCBCR[3], crop, (20, 30), L.hm_plan_planes_view) == (0, 3, 0, 2)
        assert plan(0, None, (20, 30), L.hm_plan_planes_view) == (0, 3, 0, 2)
        for size, filt in (((20, 30), TRIANGLE), ((77, 51), LANCZOS3), (None, TRIANGLE), ((33, 17), NEAREST)):
            check_item(capi, L, data, 0, 0, host, crop, size, filt, combos, f"grid {name}")
        # the same crop of the chain's result: the whole grid is decoded
        check_item(capi, L, data, YCBCR[3], 0, host444, crop, (20, 30), CUBIC, combos, f"grid {name} to 4:4:4")
    # a damaged tile outside the crop neither fails the call nor sets HM_WARN_CONCEALED; inside it fails the call, nothing written
    crop, size = cases["inside_one_tile"][0], (20, 30)
    tiles = [synthutil.picture(48100 + t, width=64, height=64) for t in range(6)]
    view = make_view(capi, crop, size, TRIANGLE)
    images = ref.dest_images(host, SEMI, U8, ONE, ZERO, 0, False, crop, size, TRIANGLE)
    for k, ok in ((0, True), (3, False)):  # (tile 3 = row 1, column 1: the crop's)
        bad = heifwriter.write_heic(tiles[:k] + [_cut_short(tiles[k])] + tiles[k + 1:], (64, 64), grid=(3, 2, 117, 171))
        for strict in (1, 0) if ok else (1,):
            d, bufs, pitches = make_planes(capi, L, 1, 8, 20, 30, images, SEMI, U8, ONE, ZERO)
            rc, msg, out = item_view(capi, L, bad, 0, view, d, strict=strict)
            if ok:
                assert rc == 0 and out.warnings == 0, msg
                base.check_buffers(bufs, images, pitches, f"damage in tile {k}, strict {strict}")
            else:
                assert rc < 0 and "tile" in msg, msg
                torch.cuda.synchronize()
                base.check_buffers(bufs, None, None, "damage inside the crop")


def test_refusals_leave_every_plane_untouched(capi, L, inputs):
    import torch
    data, threads = inputs["420_8"]
    host = base.host_decode(capi, L, data, 0, 0, threads)
    hdr, _ = inputs["422_10"]
    host10 = base.host_decode(capi, L, hdr, 0, 0, threads)

    def refused(file, hst, fmt, crop, size, filt, status, word, shrink=None):
        ow, oh = size if size else (crop[2], crop[3])
        sx, sy = ref.sub(hst["chroma"])
        dt = np.uint16 if hst["bits"] > 8 else np.uint8
        images = [np.zeros((oh, ow), dt)] + [np.zeros(((oh + sy - 1) // sy, (ow + sx - 1) // sx), dt) for _ in range(2)] + [None]
        d, bufs, _ = make_planes(capi, L, hst["chroma"], hst["bits"], ow, oh, images, SEPARATE, int_dtype(hst["bits"]), ONE, ZERO, shrink=shrink)
        rc, msg, _ = item_view(capi, L, file, fmt, make_view(capi, crop, size, filt), d)
        assert rc == status and word in msg, (rc, msg)
        torch.cuda.synchronize()
        base.check_buffers(bufs, None, None, f"a refused call ({msg})")

    refused(data, host, 0, (11, 20, 64, 48), (32, 24), TRIANGLE, -1, "crop_x")          # an odd crop_x on 4:2:0
    refused(data, host, 0, (10, 21, 64, 48), (32, 24), TRIANGLE, -1, "crop_y")          # an odd crop_y on 4:2:0 ...
    refused(hdr, host10, 0, (11, 20, 64, 48), (32, 24), TRIANGLE, -1, "crop_x")         # (4:2:2: x still)
    refused(data, host, 0, (150, 100, 64, 48), (32, 24), TRIANGLE, -1, "not inside")    # a crop outside the image
    refused(data, host, 0, None, (1, 1), CUBIC, -1, "reduction")                        # 200 -> 1 beyond the cubic's 128
    refused(data, host, 0, None, (2, 2), LANCZOS3, -1, "reduction")                     # 200 -> 2 beyond Lanczos-3's 85
    refused(data, host, 0, None, (32, 24), 5, -1, "filter")
    for c in (0, 1, 2):
        refused(data, host, 0, (10, 20, 64, 48), (77, 51), TRIANGLE, -1, f"plane[{c}].len", shrink=c)   # one byte short for the out-sized plane
    refused(data, host, 10, (10, 20, 64, 48), (32, 24), TRIANGLE, -1, "hm_decode_item_to_device")        # an interleaved HM_OUT_RGB target
    # ... but an odd crop_y on 4:2:2 is fine
    check_item(capi, L, hdr, 0, 0, host10, (10, 21, 64, 48), (32, 24), TRIANGLE, [(SEMI, U16, ONE, ZERO, 0, 0, 1, None)], "422_10 odd crop_y")
    # ... and the library still decodes after all of that
    check_item(capi, L, data, 0, 0, host, (10, 20, 64, 48), (32, 24), TRIANGLE, [(SEMI, U8, ONE, ZERO, 0, 0, 0, None)], "after the refusals")


def test_python_crop_size_and_filter(pkg, capi, L, inputs):
    import torch
    data, threads = inputs["420_8"]
    host = base.host_decode(capi, L, data, 0, 0, threads)
    crop, size = (10, 20, 150, 100), (77, 51)
    # single image, I420 u8 and NV12 float16 with scale / bias
    exp = ref.dest_images(host, SEPARATE, U8, ONE, ZERO, 0, False, crop, size, CUBIC)
    y, cb, cr = pkg.decode_to_planes(data, crop=crop, size=size, filter="bicubic")
    assert tuple(y.shape) == (51, 77) and tuple(cb.shape) == tuple(cr.shape) == (26, 39) and y.dtype == torch.uint8
    assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip((y, cb, cr), exp))
    sc, bi = base.affine(255.0)
    exp = ref.dest_images(host, SEMI, F16, sc, bi, 0, False, None, size, TRIANGLE)
    y, cbcr = pkg.decode_to_planes(data, layout="semiplanar", dtype=torch.float16, scale=sc, bias=bi, size=size)
    assert tuple(cbcr.shape) == (26, 39, 2)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), exp[0].view(np.uint16))
    assert np.array_equal(cbcr.cpu().numpy().reshape(26, 78).view(np.uint16), np.ascontiguousarray(exp[1]).view(np.uint16))
    # the crop alone
    exp = ref.dest_images(host, SEPARATE, U8, ONE, ZERO, 0, False, crop, None, TRIANGLE)
    planes = pkg.decode_to_planes(data, crop=crop)
    assert tuple(planes[0].shape) == (100, 150) and all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(planes, exp))
    with pytest.raises(capi.HmError, match="crop_x"):
        pkg.decode_to_planes(data, crop=(11, 20, 64, 48), size=size)
    with pytest.raises(ValueError, match="filter"):
        pkg.decode_to_planes(data, size=size, filter="box")
    # the sequence form
    movie = _movie(3)
    hosts = [base.host_decode(capi, L, movie, 0, 0, 4, item=k) for k in (1, 2, 3)]
    y, cbcr = pkg.decode_sequence_to_planes(movie, frames=[3, 1, 3], layout="semiplanar", crop=crop, size=size, filter="lanczos3")
    assert tuple(y.shape) == (3, 51, 77) and tuple(cbcr.shape) == (3, 26, 39, 2)
    for k, fid in enumerate((3, 1, 3)):
        exp = ref.dest_images(hosts[fid - 1], SEMI, U8, ONE, ZERO, 0, False, crop, size, LANCZOS3)
        assert np.array_equal(y[k].cpu().numpy(), exp[0]) and np.array_equal(cbcr[k].cpu().numpy().reshape(26, 78), exp[1]), f"frames[{k}]"
    # the batch form: files of different sizes into equally sized slices, a crop for one of them
    names = ["420_8", "grid_cropped", "420_8_clap_odd"]
    files = [inputs[nm][0] for nm in names]
    crops = [None, (50, 100, 40, 50), None]
    y, cb, cr = pkg.decode_batch_to_planes(files, size=(64, 48), crops=crops, max_in_flight=2)
    assert tuple(y.shape) == (3, 48, 64) and tuple(cb.shape) == tuple(cr.shape) == (3, 24, 32)
    for k, fdata in enumerate(files):
        exp = ref.dest_images(base.host_decode(capi, L, fdata, 0, 0, 2), SEPARATE, U8, ONE, ZERO, 0, False, crops[k], (64, 48), TRIANGLE)
        assert all(np.array_equal(t[k].cpu().numpy(), e) for t, e in zip((y, cb, cr), exp)), names[k]
    with pytest.raises(ValueError, match="crops"):
        pkg.decode_batch_to_planes(files, crops=crops)


def test_no_instance_uses_scratch(hm_hooks):
    """through hook code 7: every instance of k_planes_resample_h / _v and k_planes_view_nearest reports zero scratch"""
    hm_hooks.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    n = 0
    while True:
        out = (C.c_int * 2)()
        if hm_hooks.hm_debug_kernel_regs(7, n, 0, 0, C.byref(out)) != 0:
            break
        assert out[0] > 0 and out[1] == 0, f"instance {n}: {out[0]} registers, {out[1]} bytes of scratch"
        n += 1
    assert n == 10  # 2 horizontal, 4 vertical, 4 nearest
