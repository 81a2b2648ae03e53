"""GPU: views (hm_decode_item_to_device_view, hm_pipeline_submit_to_device_view, hm_resample_to_tensor and the crop / size arguments
of decode_to_tensor / decode_batch_to_tensor).  Everything is bit-exact: the expected image of every case is tests/view_ref.py
applied to the rows hm_decode_item returns in host memory (which the rest of the suite holds to the reference decoder).  Every
destination sits in a guarded buffer pre-filled with 0xA5 and the WHOLE buffer is compared, as in test_device_out_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import hevcutil
import synthutil
import test_device_out_gpu as base
import view_ref

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBB_LE = 10, 11, 12, 14
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
TRIANGLE, NEAREST = view_ref.TRIANGLE, view_ref.NEAREST
GRID = (4, 3, 181, 243)
# the crops of the plan test (tests/test_device_view.py) and the sub-grids they decode
GRID_CROPS = {"inside_one_tile": ((70, 70, 30, 40), (1, 1, 1, 1)), "across_a_2x2_corner": ((50, 100, 40, 50), (1, 2, 0, 2)),
              "clipped_last_column_and_row": ((150, 200, 31, 43), (3, 1, 2, 1))}


def _grid_tiles():
    return [synthutil.picture(47100 + t, width=64, height=64) for t in range(12)]


def _cut_short(picture):
    nals = hevcutil.split_nals(picture)
    return hevcutil.join_nals(nals[:-1] + [nals[-1][:len(nals[-1]) // 2]])


@pytest.fixture(scope="module")
def images(hm):
    """name -> (file bytes, out_format, host threads, the host decode's pixels as h x w x c samples)"""
    full = synthutil.picture(47000, width=200, height=136, qp=30, vui=1, full_range=1, matrix=6)
    files = {"single": (heifwriter.write_heic([full], (200, 136)), RGB),
             "grid": (heifwriter.write_heic(_grid_tiles(), (64, 64), grid=GRID), RGB),
             "ten_bit": (heifwriter.write_heic([synthutil.picture(47300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)],
                                               (160, 96), bit_depth=10), RRGGBB_LE),
             "alpha_aux": (heifwriter.write_heic([synthutil.picture(47200, width=96, height=64, vui=1, full_range=1, matrix=6)], (96, 64),
                                                 aux=[(synthutil.picture(47201, width=48, height=32), (48, 32), base.ALPHA_URN)]), RGBA),
             "clap_irot": (heifwriter.write_heic([full], (200, 136), transforms=[base._clap(121, 77, 7, -5), ("irot", 1)]), RGB)}
    out = {}
    for name, (data, fmt) in files.items():
        rows, w, h = base.host_rows(hm, data, fmt, 2)
        c = 3 if base.OBPP[fmt] in (3, 6) else 4
        out[name] = (data, fmt, 2, rows.reshape(h, w, c) if base.OBPP[fmt] <= 4 else rows.view("<u2").reshape(h, w, c))
    return out


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def make_view(capi, crop, size, filt):
    x, y, w, h = crop if crop else (0, 0, 0, 0)
    ow, oh = size if size else (0, 0)
    return capi.DeviceView(x, y, w, h, ow, oh, filt)


def view_to_device(capi, L, data, fmt, view, d, threads, strict=0):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, strict, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_view(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(view), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def destination_values(ref, filt, crop_only, dtype, peak, scale, bias):
    """what the view's reference (view_ref.resample) becomes in a destination of `dtype`"""
    if dtype in (U8, U16):
        v = ref if (crop_only or filt == NEAREST) else view_ref.to_integer(ref, peak)
        return v.astype(np.uint8 if dtype == U8 else np.uint16)
    v = view_ref.to_float(ref, scale, bias)
    return v.astype(np.float16) if dtype == F16 else v


def place(vals, layout, dtype, row, plane, size, start):
    """the whole guarded buffer as it must look: `vals` (h x w x c, the destination's dtype) under the pitches, 0xA5 elsewhere"""
    buf = np.full(size, 0xA5, np.uint8)
    e = base.ELEM[dtype]
    h, w, c = vals.shape
    typed = buf[start:start + (size - start) // e * e].view(vals.dtype)
    if layout == CHW:
        np.lib.stride_tricks.as_strided(typed, shape=(c, h, w), strides=(plane, row, e))[...] = vals.transpose(2, 0, 1)
    else:
        np.lib.stride_tricks.as_strided(typed, shape=(h, w, c), strides=(row, c * e, e))[...] = vals
    return buf


def destinations(fmt):
    """(layout, dtype, scale, bias) x pitches (0 tight / 1 padded off 16-byte alignment / 2 padded by 64 bytes): both store paths"""
    wide = base.OBPP[fmt] >= 6
    integer = U16 if wide else U8
    sc, bi = base.imagenet(65535.0 if wide else 255.0)
    one, zero = [1.0] * 4, [0.0] * 4
    return [(lay, dt, s, b, pad) for lay, dt, s, b in ((CHW, F32, sc, bi), (CHW, F16, sc, bi), (HWC, integer, one, zero), (CHW, integer, one, zero))
            for pad in (0, 1, 2)]


def views_of(w, h):
    """(crop, size, filter) for a w x h image"""
    return [((7, 5, 33, 21), None, TRIANGLE),            # the crop alone, odd offsets and odd sizes
            ((w - 35, h - 23, 35, 23), None, NEAREST),   # ... up to the last column and row
            ((7, 5, 33, 21), (33, 21), TRIANGLE),        # m == n through the resampling kernels
            (None, (50, 37), TRIANGLE), (None, (7, 5), TRIANGLE), (None, (1, 1), TRIANGLE),
            ((7, 5, 33, 21), (64, 48), TRIANGLE),        # up-sampling
            ((0, 5, w, 21), (20, 48), TRIANGLE),         # down in x and up in y at once
            (None, (77, 201), NEAREST), ((7, 5, 33, 21), (64, 9), NEAREST)]


@pytest.mark.parametrize("name", ["single", "grid", "ten_bit", "alpha_aux", "clap_irot"])
def test_view_decode_equals_the_restatement(capi, L, images, name):
    data, fmt, threads, pixels = images[name]
    h, w, _ = pixels.shape
    if name == "grid":
        assert (w, h) == (181, 243)
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    for crop, size, filt in views_of(w, h):
        ref = view_ref.resample(pixels, crop, size, filt)
        oh, ow, _ = ref.shape
        view = make_view(capi, crop, size, filt)
        for layout, dtype, scale, bias, pad in destinations(fmt):
            what = f"{name} crop {crop} size {size} filter {filt} layout {layout} dtype {dtype} pad {pad}"
            d, g, row, plane = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, scale, bias, pad, 0)
            rc, msg, out = view_to_device(capi, L, data, fmt, view, d, threads)
            assert rc == 0, f"{what}: {msg}"
            assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, fmt), what
            exp = place(destination_values(ref, filt, size is None, dtype, peak, scale, bias), layout, dtype, row, plane, g.size, g.start)
            got = g.host()
            if not np.array_equal(got, exp):
                bad = np.flatnonzero(got != exp)
                raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - g.start} from the destination's start "
                                     f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def test_rounding_and_interpolation_are_exercised(images):
    """the cases are not all trivial: resampled values fall strictly between samples, and some land within 5e-3 of a rounding tie"""
    pixels = images["grid"][3]
    r = view_ref.resample(pixels, None, (50, 37))
    frac = r - np.floor(r)
    assert (frac > 0.01).any() and (np.abs(frac - 0.5) < 5e-3).any()


def test_big_endian_target_moves_bytes(hm, capi, L, images):
    """the crop alone and NEAREST to HWC with the target's own integer type move bytes: a _BE target is allowed there"""
    data = images["ten_bit"][0]
    rows, w, h = base.host_rows(hm, data, RRGGBB_BE, 2)
    words = rows.view(np.uint16).reshape(h, w, 3)  # (the big-endian words as they lie in memory)
    for crop, size, filt in (((7, 5, 33, 21), None, TRIANGLE), (None, (77, 201), NEAREST)):
        ref = view_ref.resample(words, crop, size, NEAREST)
        oh, ow, _ = ref.shape
        d, g, row, plane = base.make_dest(capi, L, RRGGBB_BE, HWC, U16, ow, oh, [1.0] * 4, [0.0] * 4, 1, 0)
        rc, msg, _ = view_to_device(capi, L, data, RRGGBB_BE, make_view(capi, crop, size, filt), d, 2)
        assert rc == 0, msg
        assert np.array_equal(g.host(), place(ref, HWC, U16, row, plane, g.size, g.start))


@pytest.mark.parametrize("fmt,w,h", [(RGB, 1001, 301), (RGBA, 130, 70)])
def test_resample_on_random_pixels(capi, L, fmt, w, h):
    """hm_resample_to_tensor alone: every sample value, several blocks per row and a ragged last group, a reduction by more than 16"""
    import torch
    rng = np.random.default_rng(fmt * 1000 + w)
    c = base.OBPP[fmt]
    src_stride = (w * c + 63) // 64 * 64 + 64
    src = rng.integers(0, 256, (h, src_stride), dtype=np.uint8)
    pixels = np.ascontiguousarray(src[:, :w * c]).reshape(h, w, c)
    dsrc = torch.from_numpy(src).cuda()
    for crop, size in ((None, (w // 17, 19)), ((3, 1, w - 4, h - 2), (259, 67))):
        ref = view_ref.resample(pixels, crop, size)
        oh, ow, _ = ref.shape
        for layout, dtype, scale, bias, pad in destinations(fmt):
            d, g, row, plane = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, scale, bias, pad, 0)
            rc = L.hm_resample_to_tensor(fmt, w, h, dsrc.data_ptr(), src_stride, C.byref(make_view(capi, crop, size, TRIANGLE)), C.byref(d), None)
            assert rc == 0, L.hm_last_error().decode()
            torch.cuda.synchronize()
            exp = place(destination_values(ref, TRIANGLE, False, dtype, 255, scale, bias), layout, dtype, row, plane, g.size, g.start)
            assert np.array_equal(g.host(), exp), f"fmt {fmt} crop {crop} size {size} layout {layout} dtype {dtype} pad {pad}"


def _full_decode_on_device(capi, L, data, w, h, threads):
    """the whole image as tight H x W x 3 bytes in device memory (hm_decode_item_to_device)"""
    d, g, _, _ = base.make_dest(capi, L, RGB, HWC, U8, w, h, [1.0] * 4, [0.0] * 4, 0, 0)
    rc, msg, _ = base.to_device(capi, L, data, RGB, d, threads)
    assert rc == 0, msg
    return g


@pytest.mark.parametrize("threads", [1, 2, 16])
def test_reduced_decode_equals_the_view_of_the_full_decode(capi, L, images, threads):
    """the sub-grid decode gives the bytes hm_resample_to_tensor makes of the full decode, whatever the number of parsing threads"""
    import torch
    data, fmt, _, pixels = images["grid"]
    h, w, _ = pixels.shape
    full = _full_decode_on_device(capi, L, data, w, h, threads)
    assert np.array_equal(full.host()[full.start:full.start + w * h * 3].reshape(h, w, 3), pixels)
    sc, bi = base.imagenet(255.0)
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        for name, (crop, tiles) in GRID_CROPS.items():
            for size, layout, dtype in (((50, 37), CHW, F32), (None, HWC, U8), ((64, 48), HWC, F16)):
                view = make_view(capi, crop, size, TRIANGLE)
                prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
                t = (C.c_int32 * 4)()
                assert L.hm_plan_view(fh, L.hm_file_primary_item(fh), C.byref(prm), C.byref(view), C.byref(t)) == 0 and tuple(t) == tiles
                ow, oh = size if size else crop[2:]
                d1, g1, _, _ = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, sc, bi, 1, 0)
                d2, g2, _, _ = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, sc, bi, 1, 0)
                rc, msg, _ = view_to_device(capi, L, data, fmt, view, d1, threads)
                assert rc == 0, msg
                assert L.hm_resample_to_tensor(fmt, w, h, full.ptr, w * 3, C.byref(view), C.byref(d2), None) == 0, L.hm_last_error().decode()
                torch.cuda.synchronize()
                assert np.array_equal(g1.host(), g2.host()), (name, size, layout, dtype)
                assert not (g1.host()[g1.start:g1.start + 64] == 0xA5).all()
    finally:
        L.hm_file_close(fh)


def test_a_damaged_tile_outside_the_crop_is_not_looked_at(hm, capi, L, images):
    import torch
    data, fmt, threads, pixels = images["grid"]
    crop, size = GRID_CROPS["inside_one_tile"][0], (20, 30)  # tile 4 (row 1, column 1) alone
    ref = view_ref.resample(pixels, crop, size)
    one, zero = [1.0] * 4, [0.0] * 4
    view = make_view(capi, crop, size, TRIANGLE)

    def damaged(k):
        tiles = _grid_tiles()
        tiles[k] = _cut_short(tiles[k])
        return heifwriter.write_heic(tiles, (64, 64), grid=GRID)
    outside, inside = damaged(11), damaged(4)
    # the full decode of either file fails under strict decoding ...
    messages = {}
    for k, bad in ((11, outside), (4, inside)):
        d, g, _, _ = base.make_dest(capi, L, fmt, HWC, U8, 181, 243, one, zero, 0, 0)
        h = C.c_void_p()
        assert L.hm_file_open(bad, len(bad), C.byref(h)) == 0
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 1, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(d), C.byref(out))
        messages[k] = L.hm_last_error().decode()
        L.hm_file_close(h)
        assert rc < 0 and f"tile {k} " in messages[k], messages[k]
    # ... the view decode of the file whose damage lies outside the crop succeeds, equal to the intact twin's view, without a warning
    for strict in (1, 0):
        d, g, row, plane = base.make_dest(capi, L, fmt, CHW, U8, size[0], size[1], one, zero, 1, 0)
        rc, msg, out = view_to_device(capi, L, outside, fmt, view, d, threads, strict=strict)
        assert rc == 0, msg
        assert out.warnings == 0
        assert np.array_equal(g.host(), place(view_ref.to_integer(ref, 255).astype(np.uint8), CHW, U8, row, plane, g.size, g.start))
    # ... and with the damaged tile inside the crop the call fails with that tile's message; the destination keeps 0xA5 everywhere
    d, g, _, _ = base.make_dest(capi, L, fmt, CHW, U8, size[0], size[1], one, zero, 1, 0)
    rc, msg, _ = view_to_device(capi, L, inside, fmt, view, d, threads, strict=1)
    assert rc < 0 and msg.split(": ", 1)[1] == messages[4].split(": ", 1)[1], (msg, messages[4])
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()


def test_python_batch_of_different_sizes_and_strided_out(pkg, images):
    import torch
    names = ["single", "grid", "clap_irot"]
    files = [images[n][0] for n in names]
    assert len({images[n][3].shape for n in names}) == 3
    crops = [None, (3, 5, 40, 30), None]
    t = pkg.decode_batch_to_tensor(files, size=(32, 32), crops=crops)
    assert tuple(t.shape) == (3, 3, 32, 32) and t.dtype == torch.float32
    got = t.cpu().numpy()
    for k, n in enumerate(names):
        ref = view_ref.resample(images[n][3], crops[k], (32, 32))
        assert np.array_equal(got[k], view_ref.to_float(ref, [1.0] * 4, [0.0] * 4).transpose(2, 0, 1)), n
    # without size the files must still be equally sized
    with pytest.raises(ValueError, match=r"files\[1\]"):
        pkg.decode_batch_to_tensor(files)
    # decode_to_tensor with a crop, a size and a strided out: what lies around the view stays as it was
    sc, bi = base.imagenet(255.0)
    big = torch.full((3, 40 + 2, 50 + 9), -7.0, dtype=torch.float32, device="cuda")
    out = big[:, 1:41, :50]
    assert pkg.decode_to_tensor(files[1], crop=(50, 100, 40, 50), size=(50, 40), out=out, scale=sc, bias=bi) is out
    ref = view_ref.to_float(view_ref.resample(images["grid"][3], (50, 100, 40, 50), (50, 40)), sc, bi)
    res = big.cpu().numpy()
    assert np.array_equal(res[:, 1:41, :50], ref.transpose(2, 0, 1))
    assert (res[:, :, 50:] == -7.0).all() and (res[:, 0] == -7.0).all() and (res[:, 41] == -7.0).all()
    u8 = pkg.decode_to_tensor(files[0], crop=(7, 5, 33, 21), layout="hwc", dtype=torch.uint8)
    assert np.array_equal(u8.cpu().numpy(), images["single"][3][5:26, 7:40])
    near = pkg.decode_to_tensor(files[0], size=(77, 201), filter="nearest", layout="hwc", dtype=torch.uint8)
    assert np.array_equal(near.cpu().numpy(), view_ref.resample(images["single"][3], None, (77, 201), NEAREST))
    with pytest.raises(ValueError, match="shape"):
        pkg.decode_to_tensor(files[0], size=(50, 40), out=torch.empty((3, 40, 51), device="cuda"))
    with pytest.raises(ValueError, match="filter"):
        pkg.decode_to_tensor(files[0], size=(50, 40), filter="lanczos")


def test_refusals_on_the_device_leave_the_destination_untouched(capi, L, images):
    import torch
    data, fmt, threads, pixels = images["single"]
    hdr = images["ten_bit"][0]
    one, zero = [1.0] * 4, [0.0] * 4

    def refused(file, f, view, d, g, word):
        rc, msg, _ = view_to_device(capi, L, file, f, view, d, threads)
        assert rc == -1 and word in msg, (rc, msg)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"
    # a short len for out_w x out_h, both kinds of write
    for layout, dtype in ((HWC, U8), (CHW, F32)):
        d, g, _, _ = base.make_dest(capi, L, RGB, layout, dtype, 50, 37, one, zero, 0, 0, shrink=1)
        refused(data, RGB, make_view(capi, None, (50, 37), TRIANGLE), d, g, "len")
        refused(data, RGB, make_view(capi, (0, 0, 50, 37), None, TRIANGLE), d, g, "len")
    # a crop that is inside the size the file declares and outside the image that is decoded
    tall = heifwriter.write_heic([synthutil.picture(47000, width=200, height=136, qp=30, vui=1, full_range=1, matrix=6)], (300, 200))
    d, g, _, _ = base.make_dest(capi, L, RGB, CHW, F32, 16, 16, one, zero, 0, 0)
    refused(tall, RGB, make_view(capi, (250, 150, 20, 20), (16, 16), TRIANGLE), d, g, "not inside")
    refused(tall, RGB, make_view(capi, (190, 100, 20, 20), (16, 16), NEAREST), d, g, "not inside")
    # _BE with TRIANGLE
    d, g, _, _ = base.make_dest(capi, L, RRGGBB_BE, HWC, U16, 50, 37, one, zero, 0, 0)
    refused(hdr, RRGGBB_BE, make_view(capi, None, (50, 37), TRIANGLE), d, g, "_LE")
    # ... and the library still decodes after all of that
    d, g, row, plane = base.make_dest(capi, L, RGB, HWC, U8, 50, 37, one, zero, 0, 0)
    assert view_to_device(capi, L, data, RGB, make_view(capi, None, (50, 37), TRIANGLE), d, threads)[0] == 0
    exp = view_ref.to_integer(view_ref.resample(pixels, None, (50, 37)), 255).astype(np.uint8)
    assert np.array_equal(g.host(), place(exp, HWC, U8, row, plane, g.size, g.start))


def test_resample_kernels_use_no_scratch(pkg):
    """every instance of the resampling kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 4): no scratch"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(4, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 64, (n, out[0], out[1])
        n += 1
    # 8 horizontal (sample width x channels x layout), 24 vertical (dtype x store width x row kind), 6 nearest
    assert n == 38
