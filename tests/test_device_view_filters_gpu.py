"""GPU: HM_VIEW_CUBIC and HM_VIEW_LANCZOS3 through hm_decode_item_to_device_view, hm_pipeline_submit_to_device_view, hm_resample_to_tensor
and decode_to_tensor(filter=).  Everything is bit-exact: the expected image of every case is tests/view_filters_ref.py applied to the
rows hm_decode_item returns in host memory (or to the pixels the test put on the device).  Every destination sits in a guarded
buffer pre-filled with 0xA5 and the WHOLE buffer is compared, as in test_device_view_gpu.py, whose helpers are used."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as tv
import view_filters_ref as vf

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBB_LE = 10, 11, 12, 14
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
CUBIC, LANCZOS3 = vf.CUBIC, vf.LANCZOS3
FILTERS = (CUBIC, LANCZOS3)
GRID = (4, 3, 181, 243)  # rows, cols, canvas: the last column is clipped to 53 of 64, the last row to 51 of 64
ONE, ZERO = [1.0] * 4, [0.0] * 4

# (crop, size) on the 181 x 243 grid
VIEWS = {"across_a_tile_corner": ((50, 100, 40, 50), (50, 40)),
         "whole_image": (None, (97, 50)),
         "up_sampling": ((7, 5, 30, 21), (77, 201)),
         "identity_size": ((7, 5, 33, 21), (33, 21)),
         "one_column": ((3, 5, 80, 60), (1, 9)),
         "ragged_second_wave": (None, (65, 30)),
         "lanczos_limit_on_x": ((5, 3, 170, 40), (2, 11))}
# the staged run's first byte at 0, 3, 9 and 21 bytes behind the row's: its head is unaligned in every way
HEADS = {f"head_at_x_{x}": ((x, 11, 120, 30), (31, 13)) for x in (0, 1, 3, 7)}


@pytest.fixture(scope="module")
def images(hm):
    """name -> (file bytes, out_format, the host decode's pixels as h x w x c samples)"""
    tiles = [synthutil.picture(46000 + t, width=64, height=64) for t in range(12)]
    files = {"grid": (heifwriter.write_heic(tiles, (64, 64), grid=GRID), RGB),
             "ten_bit": (heifwriter.write_heic([synthutil.picture(47300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)],
                                               (160, 96), bit_depth=10), RRGGBB_LE),
             "alpha_aux": (heifwriter.write_heic([synthutil.picture(47200, width=96, height=64, vui=1, full_range=1, matrix=6)], (96, 64),
                                                 aux=[(synthutil.picture(47201, width=48, height=32), (48, 32), base.ALPHA_URN)]), RGBA)}
    out = {}
    for name, (data, fmt) in files.items():
        rows, w, h = base.host_rows(hm, data, fmt, 2)
        c = 3 if base.OBPP[fmt] in (3, 6) else 4
        out[name] = (data, fmt, rows.reshape(h, w, c) if base.OBPP[fmt] <= 4 else rows.view("<u2").reshape(h, w, c))
    assert out["grid"][2].shape == (243, 181, 3)
    return out


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def refs(images):
    """the restatement of a view, computed once: (image name, crop, size, filter) -> float32 sums"""
    cache = {}

    def get(name, crop, size, filt):
        key = (name, crop, size, filt)
        if key not in cache:
            cache[key] = vf.resample(images[name][2], crop, size, filt)
            cache[key].setflags(write=False)
        return cache[key]
    return get


def block_image(w, h, c=3, bw=9, bh=7):
    """hard black and white blocks: every edge makes the cubic and the Lanczos sums overshoot"""
    img = np.zeros((h, w, c), np.uint8)
    for y0 in range(0, h, bh):
        for x0 in range(0, w, bw):
            if (y0 // bh + x0 // bw) % 2:
                img[y0:y0 + bh, x0:x0 + bw] = 255
    return img


CENSUS_VIEWS = ((None, (97, 150)), ((3, 2, 100, 90), (77, 201)), ((1, 0, 170, 60), (150, 33)))


def values(ref, dtype, peak, scale, bias):
    if dtype in (U8, U16):
        return vf.to_integer(ref, peak).astype(np.uint8 if dtype == U8 else np.uint16)
    v = vf.to_float(ref, scale, bias)
    return v.astype(np.float16) if dtype == F16 else v


def destinations(fmt, pads=(0, 1, 2)):
    """(layout, dtype, scale, bias, pad): pad 1 = pitches that are no multiple of 16 (the P = 1 store path), pad 2 = 64 bytes between the
    rows that must come back untouched"""
    wide = base.OBPP[fmt] >= 6
    sc, bi = base.imagenet(65535.0 if wide else 255.0)
    kinds = ((HWC, U16 if wide else U8, ONE, ZERO), (CHW, F32, sc, bi), (CHW, F16, sc, bi))
    return [k + (pad,) for k in kinds for pad in pads]


def check(capi, L, data, fmt, ref, crop, size, filt, layout, dtype, scale, bias, pad, what):
    oh, ow, _ = ref.shape
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    d, g, row, plane = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, scale, bias, pad, 0)
    rc, msg, out = tv.view_to_device(capi, L, data, fmt, tv.make_view(capi, crop, size, filt), d, 2)
    assert rc == 0, f"{what}: {msg}"
    assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, fmt), what
    exp = tv.place(values(ref, dtype, peak, scale, bias), layout, dtype, row, plane, g.size, g.start)
    got = g.host()
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - g.start} from the destination's start "
                             f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


@pytest.mark.parametrize("filt", FILTERS)
def test_view_decode_of_the_grid_equals_the_restatement(capi, L, images, refs, filt):
    data, fmt, _ = images["grid"]
    for name, (crop, size) in list(VIEWS.items()) + list(HEADS.items()):
        ref = refs("grid", crop, size, filt)
        for layout, dtype, scale, bias, pad in destinations(fmt, (1,) if name in HEADS else (0, 1, 2)):
            check(capi, L, data, fmt, ref, crop, size, filt, layout, dtype, scale, bias, pad, f"grid {name} filter {filt} layout {layout} dtype {dtype} pad {pad}")


@pytest.mark.parametrize("name", ["ten_bit", "alpha_aux"])
def test_view_decode_of_wide_samples_and_alpha_equals_the_restatement(capi, L, images, refs, name):
    """HWC u16 from rrggbb_le, and RGBA (alpha like any other channel): the 2-byte and the 4-channel instances"""
    data, fmt, pixels = images[name]
    h, w, _ = pixels.shape
    for crop, size in ((None, (50, 37)), ((1, 3, 77, 50), (65, 40)), ((7, 2, w - 7, 20), (3, 33))):
        for filt in FILTERS:
            ref = refs(name, crop, size, filt)
            for layout, dtype, scale, bias, pad in destinations(fmt):
                check(capi, L, data, fmt, ref, crop, size, filt, layout, dtype, scale, bias, pad, f"{name} crop {crop} size {size} filter {filt} layout {layout} dtype {dtype} pad {pad}")


def test_pipeline_views_equal_the_restatement(capi, L, images, refs):
    data, fmt, _ = images["grid"]
    sc, bi = base.imagenet(255.0)
    jobs = [(VIEWS[v], filt, layout, dtype, s, b, pad) for v, filt, (layout, dtype, s, b), pad in
            (("across_a_tile_corner", CUBIC, (CHW, F32, sc, bi), 0), ("across_a_tile_corner", LANCZOS3, (HWC, U8, ONE, ZERO), 1),
             ("whole_image", CUBIC, (HWC, U8, ONE, ZERO), 2), ("whole_image", LANCZOS3, (CHW, F16, sc, bi), 1),
             ("lanczos_limit_on_x", LANCZOS3, (CHW, F32, sc, bi), 1), ("ragged_second_wave", CUBIC, (CHW, F16, sc, bi), 0))]
    cfg = capi.PipelineConfig(4, 4, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    dests, seen = [], []
    try:
        def take():
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0
            assert r.status == 0, L.hm_last_error().decode()
            (crop, size), filt, layout, dtype, s, b, _ = jobs[r.tag]
            d, g, row, plane = dests[r.tag]
            exp = tv.place(values(refs("grid", crop, size, filt), dtype, 255, s, b), layout, dtype, row, plane, g.size, g.start)
            assert (r.image.width, r.image.height) == size
            assert np.array_equal(g.host(), exp), f"job {r.tag}"
            seen.append(r.tag)
            L.hm_pipeline_release(pipe, C.byref(r))
        for k, ((crop, size), filt, layout, dtype, s, b, pad) in enumerate(jobs):
            dests.append(base.make_dest(capi, L, fmt, layout, dtype, size[0], size[1], s, b, pad, 0))
            view = tv.make_view(capi, crop, size, filt)
            while True:
                rc = L.hm_pipeline_submit_to_device_view(pipe, data, len(data), 0, k, C.byref(view), C.byref(dests[k][0]))
                assert rc >= 0, L.hm_last_error().decode()
                if rc == 0:
                    break
                take()
        while L.hm_pipeline_pending(pipe):
            take()
    finally:
        L.hm_pipeline_destroy(pipe)
    assert seen == list(range(len(jobs)))


def on_device(pixels, pad_bytes=64):
    """h x w x c samples as rows in device memory, `pad_bytes` behind every row: (tensor, stride)"""
    import torch
    h, w, c = pixels.shape
    raw = np.ascontiguousarray(pixels).view(np.uint8).reshape(h, -1)
    stride = raw.shape[1] + pad_bytes
    rows = np.full((h, stride), 0x5A, np.uint8)
    rows[:, :raw.shape[1]] = raw
    return torch.from_numpy(rows).cuda(), stride


def resample_check(capi, lib, fmt, pixels, dsrc, stride, crop, size, filt, ref, layout, dtype, scale, bias, pad, what):
    import torch
    h, w, _ = pixels.shape
    oh, ow, _ = ref.shape
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    d, g, row, plane = base.make_dest(capi, lib, fmt, layout, dtype, ow, oh, scale, bias, pad, 0)
    rc = lib.hm_resample_to_tensor(fmt, w, h, dsrc.data_ptr(), stride, C.byref(tv.make_view(capi, crop, size, filt)), C.byref(d), None)
    assert rc == 0, f"{what}: {lib.hm_last_error().decode()}"
    torch.cuda.synchronize()
    got = g.host()
    assert np.array_equal(got, tv.place(values(ref, dtype, peak, scale, bias), layout, dtype, row, plane, g.size, g.start)), what
    return got


def test_overshoot_reaches_both_clamps(capi, L):
    """a single image of hard black and white blocks: the pre-clamp sums leave 0 .. 255 on both sides - shown from the restatement
    alone -, so the integer destination's two clamps act, the conversion of a negative r + 0.5f is towards zero, and a float
    destination receives the overshoot as it is"""
    pixels = block_image(181, 243)
    dsrc, stride = on_device(pixels)
    sc, bi = base.imagenet(255.0)
    for filt in FILTERS:
        for crop, size in CENSUS_VIEWS:
            ref = vf.resample(pixels, crop, size, filt)
            half = ref + np.float32(0.5)
            assert (half <= -1.0).any(), "no sum whose truncation is below 0: the clamp at 0 is not reached"
            assert ((half < 0) & (half > -1.0)).any(), "no negative r + 0.5f that the conversion alone takes to 0"
            assert (half >= 256.0).any(), "no sum above the peak: the clamp at 255 is not reached"
            u8 = vf.to_integer(ref, 255)
            assert (u8 == 0).any() and (u8 == 255).any() and ((u8 > 0) & (u8 < 255)).any()
            for layout, dtype, scale, bias, pad in ((HWC, U8, ONE, ZERO, 0), (CHW, U8, ONE, ZERO, 1), (CHW, F32, sc, bi, 2), (HWC, F16, ONE, ZERO, 1)):
                resample_check(capi, L, RGB, pixels, dsrc, stride, crop, size, filt, ref, layout, dtype, scale, bias, pad,
                               f"blocks crop {crop} size {size} filter {filt} layout {layout} dtype {dtype} pad {pad}")


@pytest.mark.parametrize("fmt,w,h", [(RGB, 2600, 9), (RGBA, 1100, 6), (RRGGBB_LE, 700, 5)])
def test_a_run_longer_than_the_staging_buffer(capi, L, fmt, w, h):
    """a wave's 64 columns read more bytes of a row than the LDS holds for it (3712 with the alignment head): the chunked loop runs
    two to three times without any hook; random samples of every value, source rows at odd offsets from one another"""
    rng = np.random.default_rng(fmt * 1000 + w)
    wide = base.OBPP[fmt] >= 6
    c = 3 if base.OBPP[fmt] in (3, 6) else 4
    pixels = rng.integers(0, 65536 if wide else 256, (h, w, c)).astype(np.uint16 if wide else np.uint8)
    dsrc, stride = on_device(pixels, pad_bytes=64 + (2 if wide else 5))
    assert (w - 1) * base.OBPP[fmt] > 3712
    sc, bi = base.imagenet(65535.0 if wide else 255.0)
    crop, size = (1, 0, w - 1, h), (40, 4)
    for filt in FILTERS:
        ref = vf.resample(pixels, crop, size, filt)
        for layout, dtype, scale, bias, pad in ((CHW, F32, sc, bi, 1), (HWC, U16 if wide else U8, ONE, ZERO, 0)):
            resample_check(capi, L, fmt, pixels, dsrc, stride, crop, size, filt, ref, layout, dtype, scale, bias, pad, f"fmt {fmt} filter {filt} layout {layout} dtype {dtype}")


@pytest.fixture()
def hooks(pkg, capi):
    """libheif_mi355x_test.so (the shipping library's objects + the test hooks) as a ctypes object of this module's own, with the image
    entry points bound; the view knobs are put back behind the test"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(capi.TEST_LIB_PATH)
    T.hm_last_error.restype = C.c_char_p
    T.hm_debug_set.argtypes = [C.c_char_p, C.c_int]
    capi.bind_image(T)
    try:
        yield T
    finally:
        assert T.hm_debug_set(b"view_h_staged", 1) == 0 and T.hm_debug_set(b"view_stage_px", 0) == 0


def test_per_lane_and_staged_kernels_agree(capi, hooks, images, refs):
    """cubic through the per-lane k_resample_h (hook view_h_staged = 0), through the staged kernel, and through the staged kernel with
    chunks of 40 and of 7 pixels (hook view_stage_px: the chunked loop runs several times also on the 170-pixel crop at the Lanczos-3
    limit): identical destinations, equal to the restatement"""
    _, fmt, pixels = images["grid"]
    dsrc, stride = on_device(pixels, pad_bytes=64 + 3)
    sc, bi = base.imagenet(255.0)
    for name, filt in (("whole_image", CUBIC), ("across_a_tile_corner", CUBIC), ("lanczos_limit_on_x", LANCZOS3), ("head_at_x_3", LANCZOS3)):
        crop, size = VIEWS[name] if name in VIEWS else HEADS[name]
        ref = refs("grid", crop, size, filt)
        for layout, dtype, scale, bias, pad in ((CHW, F32, sc, bi, 0), (HWC, U8, ONE, ZERO, 1)):
            got = []
            for staged, px in ((0, 0), (1, 0), (1, 40), (1, 7)):
                assert hooks.hm_debug_set(b"view_h_staged", staged) == 0 and hooks.hm_debug_set(b"view_stage_px", px) == 0
                got.append(resample_check(capi, hooks, fmt, pixels, dsrc, stride, crop, size, filt, ref, layout, dtype, scale, bias, pad,
                                          f"{name} filter {filt} staged {staged} chunk {px} layout {layout} dtype {dtype}"))
            assert all(np.array_equal(got[0], x) for x in got[1:])


def test_staged_kernels_use_no_scratch(pkg):
    """every instance of k_resample_h_staged as the loaded code object has it (test hook hm_debug_kernel_regs, code 5): no scratch"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(5, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 64, (n, out[0], out[1])
        n += 1
    assert n == 8  # sample width x channels x layout


def test_reduced_decode_and_python(pkg, capi, L, images, refs):
    import torch
    data, fmt, pixels = images["grid"]
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        for filt in FILTERS:  # a view inside one tile decodes that tile alone, whatever the filter
            prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
            t = (C.c_int32 * 4)()
            view = tv.make_view(capi, (70, 70, 30, 40), (20, 30), filt)
            assert L.hm_plan_view(fh, L.hm_file_primary_item(fh), C.byref(prm), C.byref(view), C.byref(t)) == 0 and tuple(t) == (1, 1, 1, 1)
            ref = refs("grid", (70, 70, 30, 40), (20, 30), filt)
            check(capi, L, data, fmt, ref, (70, 70, 30, 40), (20, 30), filt, CHW, F32, ONE, ZERO, 0, f"inside one tile, filter {filt}")
    finally:
        L.hm_file_close(fh)
    sc, bi = base.imagenet(255.0)
    for name, filt in (("bicubic", CUBIC), ("lanczos3", LANCZOS3)):
        crop, size = VIEWS["across_a_tile_corner"]
        t = pkg.decode_to_tensor(data, crop=crop, size=size, filter=name, scale=sc, bias=bi)
        assert tuple(t.shape) == (3, size[1], size[0]) and t.dtype == torch.float32
        assert np.array_equal(t.cpu().numpy(), vf.to_float(refs("grid", crop, size, filt), sc, bi).transpose(2, 0, 1)), name
    u8 = pkg.decode_to_tensor(data, size=(97, 50), filter="bicubic", layout="hwc", dtype=torch.uint8)
    assert np.array_equal(u8.cpu().numpy(), vf.to_integer(refs("grid", None, (97, 50), CUBIC), 255).astype(np.uint8))
    many = pkg.decode_batch_to_tensor([data, data], size=(65, 30), filter="lanczos3")
    exp = vf.to_float(refs("grid", None, (65, 30), LANCZOS3), ONE, ZERO).transpose(2, 0, 1)
    assert np.array_equal(many[0].cpu().numpy(), exp) and np.array_equal(many[1].cpu().numpy(), exp)


def test_refusals_on_the_device_leave_the_destination_untouched(capi, L, images):
    import torch
    data, fmt, _ = images["grid"]
    hdr = images["ten_bit"][0]
    for file, f, crop, size, filt, dtype, word in ((data, RGB, (5, 3, 172, 40), (2, 11), LANCZOS3, U8, "reduction"), (data, RGB, None, (1, 50), CUBIC, U8, "reduction"),
                                                   (data, RGB, None, (50, 1), CUBIC, U8, "reduction"), (hdr, RRGGBB_BE, None, (50, 37), CUBIC, U16, "_LE"),
                                                   (hdr, RRGGBB_BE, None, (50, 37), LANCZOS3, U16, "_LE"), (data, RGB, None, (50, 37), 2, U8, "filter")):
        d, g, _, _ = base.make_dest(capi, L, f, HWC, dtype, size[0], size[1], ONE, ZERO, 0, 0)
        rc, msg, _ = tv.view_to_device(capi, L, file, f, tv.make_view(capi, crop, size, filt), d, 2)
        assert rc == -1 and word in msg, (rc, msg)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"
