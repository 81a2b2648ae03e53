"""GPU: sequences under a view (hm_decode_frames_to_device_view, decode_sequence_to_tensor).  Everything is bit-exact, three ways:
every frame of the one call equals hm_decode_item_to_device_view on that frame, equals the numpy restatement (tests/view_ref.py,
tests/view_filters_ref.py) applied to the rows hm_decode_item returns in host memory, and the batched write (one launch per pass
for all frames) equals the per-frame write (test hook view_batch = 0) and itself cut into chunks.  The destinations of a call are
slices of ONE guarded allocation pre-filled with 0xA5, and the whole allocation is compared."""
import ctypes as C

import numpy as np
import pytest

import moovwriter
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv
import view_filters_ref as vf

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_LE = base.RGB, base.RGBA, base.RRGGBB_LE
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = vf.TRIANGLE, vf.NEAREST, vf.CUBIC, vf.LANCZOS3
ONE, ZERO = [1.0] * 4, [0.0] * 4
THREADS = 4
# (crop, size): a reduction from an odd origin; an enlargement of the whole frame; tight CHW float32 rows of 308 bytes, no multiple
# of 16 (the element-store instance); the crop alone
VIEWS = {"reduce_odd_origin": ((3, 5, 191, 127), (97, 50)), "enlarge_whole": (None, (224, 224)), "rows_off_16": ((10, 8, 30, 30), (77, 77)),
         "crop_only": ((10, 8, 30, 30), None)}
# name -> (movie, out_format, layout, dtype, float destination)
CLASSES = {"rgb_chw_f32": ("m8", RGB, CHW, F32, True), "rgb_hwc_u8": ("m8", RGB, HWC, U8, False), "rgba_chw_f16": ("m8", RGBA, CHW, F16, True),
           "rrggbb_le_chw_u16": ("m10", RRGGBB_LE, CHW, U16, False)}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def movies():
    """name -> (file bytes, frames)"""
    m8, _, _ = base._movie(5)
    s10 = [synthutil.picture(49000 + i, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1) for i in range(4)]
    return {"m8": (m8, 5), "m10": (moovwriter.write_movie(s10, (160, 96), bit_depth=10, params_in="sample"), 4)}


@pytest.fixture(scope="module")
def pixels(hm, movies):
    """(movie, out_format, frame ID) -> the host decode's samples, h x w x c; computed once"""
    cache = {}

    def get(name, fmt, frame, data=None):
        key = (name, fmt, frame)
        if key not in cache:
            rows, w, h = base.host_rows(hm, data if data is not None else movies[name][0], fmt, THREADS, item=frame)
            c = 3 if base.OBPP[fmt] in (3, 6) else 4
            cache[key] = rows.reshape(h, w, c) if base.OBPP[fmt] <= 4 else rows.view("<u2").reshape(h, w, c)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def refs(pixels):
    """(movie, out_format, frame ID, crop, size, filter) -> the restatement's float32 sums (or moved samples); computed once"""
    cache = {}

    def get(name, fmt, frame, crop, size, filt):
        key = (name, fmt, frame, crop, size, filt)
        if key not in cache:
            cache[key] = vf.resample(pixels(name, fmt, frame), crop, size, filt)
        return cache[key]
    return get


def values(ref, filt, crop_only, dtype, peak, scale, bias):
    """the restatement in a destination of `dtype` (the cubic and Lanczos sums can be negative: view_filters_ref's conversion)"""
    if dtype in (U8, U16) and not crop_only and filt in (CUBIC, LANCZOS3):
        return vf.to_integer(ref, peak).astype(np.uint8 if dtype == U8 else np.uint16)
    return dv.destination_values(ref, filt, crop_only, dtype, peak, scale, bias)


def scale_bias(fmt, is_float):
    return base.imagenet(65535.0 if base.OBPP[fmt] >= 6 else 255.0) if is_float else (ONE, ZERO)


def tight(fmt, layout, dtype, ow, oh):
    c = 3 if base.OBPP[fmt] in (3, 6) else 4
    row = ow * base.ELEM[dtype] * (1 if layout == CHW else c)
    return row, row * oh, row * oh * (c if layout == CHW else 1)


def slices(capi, fmt, layout, dtype, ow, oh, n, scale, bias):
    """n tight destinations behind one another in ONE guarded allocation: (dests, the allocation, bytes per slice)"""
    row, plane, per = tight(fmt, layout, dtype, ow, oh)
    g = base.Guarded(per * n)
    dests = (capi.DeviceDest * n)()
    for k in range(n):
        dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = g.ptr + k * per, per, layout, dtype
        for c in range(4):
            dests[k].scale[c], dests[k].bias[c] = scale[c], bias[c]
    return dests, g, per


def expected(g, per, images, layout, dtype, row, plane):
    """the whole allocation as it must look: images[k] (h x w x c, the destination's dtype) in slice k, 0xA5 elsewhere"""
    exp = np.full(g.size, 0xA5, np.uint8)
    for k, vals in enumerate(images):
        exp[g.start + k * per:g.start + (k + 1) * per] = dv.place(vals, layout, dtype, row, plane, per, 0)
    return exp


def same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at byte {bad[0]} of the allocation (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


class Opened:
    def __init__(self, lib, data):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.hm_file_open(data, len(data), C.byref(self.h)) == 0

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        self.lib.hm_file_close(self.h)


def frames_to_device(capi, lib, fh, frames, fmt, view, dests):
    """hm_decode_frames_to_device_view: (status, message, failed_frame, out[])"""
    n = len(frames)
    prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
    out = (capi.Decoded * n)()
    failed = C.c_int32(-2)
    rc = lib.hm_decode_frames_to_device_view(fh, (C.c_uint32 * n)(*frames), n, C.byref(prm), C.byref(view) if view is not None else None, dests, out,
                                             C.byref(failed))
    msg = lib.hm_last_error().decode()
    for k in range(n):
        assert not out[k].plane[0] and not out[k].plane[1] and not out[k].plane[2] and not out[k].alpha
    return rc, msg, failed.value, out


def frame_to_device(capi, lib, fh, frame, fmt, view, dest):
    prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
    out = capi.Decoded()
    rc = lib.hm_decode_item_to_device_view(fh, frame, C.byref(prm), C.byref(view), C.byref(dest), C.byref(out))
    assert rc == 0, lib.hm_last_error().decode()


@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("filt", [TRIANGLE, CUBIC, LANCZOS3, NEAREST], ids=["triangle", "bicubic", "lanczos3", "nearest"])
def test_one_call_equals_per_frame_calls_and_the_restatement(capi, L, movies, refs, filt, cls):
    name, fmt, layout, dtype, is_float = CLASSES[cls]
    data, n = movies[name]
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    scale, bias = scale_bias(fmt, is_float)
    frames = list(range(1, n + 1))
    with Opened(L, data) as fh:
        for vname, (crop, size) in VIEWS.items():
            if name == "m10" and crop is not None and crop[0] + crop[2] > 160:
                crop = (3, 5, 151, 87)  # (the 10-bit frames are 160 x 96: the same kind of view inside them)
            ow, oh = size if size else crop[2:]
            view = dv.make_view(capi, crop, size, filt)
            what = f"{cls} filter {filt} view {vname}"
            row, plane, _ = tight(fmt, layout, dtype, ow, oh)
            dests, g, per = slices(capi, fmt, layout, dtype, ow, oh, n, scale, bias)
            rc, msg, failed, out = frames_to_device(capi, L, fh, frames, fmt, view, dests)
            assert rc == 0 and failed == -1, f"{what}: {msg}"
            for k in range(n):
                assert (out[k].width, out[k].height, out[k].used_ext_dst, out[k].stride[0], out[k].out_format) == (ow, oh, 1, row, fmt), (what, k)
            got = g.host()
            # ... the restatement on the host decode of each frame, and 0xA5 everywhere else
            images = [values(refs(name, fmt, f, crop, size, filt), filt, size is None, dtype, peak, scale, bias) for f in frames]
            same(got, expected(g, per, images, layout, dtype, row, plane), what + ": against the restatement")
            # ... and hm_decode_item_to_device_view, frame by frame, into a second allocation
            dests2, g2, _ = slices(capi, fmt, layout, dtype, ow, oh, n, scale, bias)
            for k, f in enumerate(frames):
                frame_to_device(capi, L, fh, f, fmt, view, dests2[k])
            same(got, g2.host(), what + ": against the per-frame calls")


def test_frame_list_in_any_order_with_repeats(capi, L, movies, refs):
    data, _ = movies["m8"]
    frames = [5, 1, 3, 3]
    crop, size = VIEWS["reduce_odd_origin"]
    sc, bi = base.imagenet(255.0)
    with Opened(L, data) as fh:
        for filt in (TRIANGLE, CUBIC):
            dests, g, per = slices(capi, RGB, CHW, F32, 97, 50, len(frames), sc, bi)
            rc, msg, failed, _ = frames_to_device(capi, L, fh, frames, RGB, dv.make_view(capi, crop, size, filt), dests)
            assert rc == 0 and failed == -1, msg
            row, plane, _ = tight(RGB, CHW, F32, 97, 50)
            images = [values(refs("m8", RGB, f, crop, size, filt), filt, False, F32, 255, sc, bi) for f in frames]
            same(g.host(), expected(g, per, images, CHW, F32, row, plane), f"frames {frames} filter {filt}")
    assert not np.array_equal(images[0], images[1]) and np.array_equal(images[2], images[3])


@pytest.fixture()
def hooks(pkg, capi):
    """libheif_mi355x_test.so with the image entry points bound (a library of its own in this process, with its own knobs); the
    view knobs are put back behind the test"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(capi.TEST_LIB_PATH)
    T.hm_last_error.restype = C.c_char_p
    T.hm_debug_set.argtypes = [C.c_char_p, C.c_int]
    capi.bind_image(T)
    try:
        yield T
    finally:
        for knob, v in ((b"view_batch", 1), (b"view_batch_bytes", 0), (b"view_stage_px", 0)):
            assert T.hm_debug_set(knob, v) == 0


def run_with_knobs(capi, T, data, frames, fmt, view, layout, dtype, ow, oh, scale, bias, knobs):
    for knob, v in knobs.items():
        assert T.hm_debug_set(knob.encode(), v) == 0
    dests, g, per = slices(capi, fmt, layout, dtype, ow, oh, len(frames), scale, bias)
    with Opened(T, data) as fh:
        rc, msg, failed, _ = frames_to_device(capi, T, fh, frames, fmt, view, dests)
    assert rc == 0 and failed == -1, msg
    return g.host(), g, per


@pytest.mark.parametrize("filt", [TRIANGLE, CUBIC, LANCZOS3], ids=["triangle", "bicubic", "lanczos3"])
def test_chunks_and_the_per_frame_path_give_the_same_bytes(capi, hooks, movies, refs, filt):
    """the intermediate's bound set so that a chunk holds 2 of the 5 frames (out_w x crop_h x C x 4 bytes per frame: chunks of 2, 2
    and 1), the same with staged chunks of 40 pixels inside the batched launch, and view_batch = 0 (hm_view_write per frame): all
    equal to the unchunked batched call and to the restatement"""
    data, n = movies["m8"]
    frames = list(range(1, n + 1))
    sc, bi = base.imagenet(255.0)
    for vname, layout, dtype, scale, bias in (("reduce_odd_origin", CHW, F32, sc, bi), ("enlarge_whole", HWC, U8, ONE, ZERO)):
        crop, size = VIEWS[vname]
        ow, oh = size
        crop_h = crop[3] if crop else 136
        per_frame = ow * crop_h * 3 * 4
        view = dv.make_view(capi, crop, size, filt)
        args = (capi, hooks, data, frames, RGB, view, layout, dtype, ow, oh, scale, bias)
        whole, g, per = run_with_knobs(*args, {"view_batch": 1, "view_batch_bytes": 0, "view_stage_px": 0})
        row, plane, _ = tight(RGB, layout, dtype, ow, oh)
        images = [values(refs("m8", RGB, f, crop, size, filt), filt, False, dtype, 255, scale, bias) for f in frames]
        same(whole, expected(g, per, images, layout, dtype, row, plane), f"{vname} filter {filt}: against the restatement")
        for what, knobs in (("chunks of 2, 2, 1", {"view_batch_bytes": 2 * per_frame + per_frame // 2}),
                            ("a frame per chunk", {"view_batch_bytes": 1}),
                            ("chunks of 2, 2, 1 with staged chunks of 40 pixels", {"view_batch_bytes": 2 * per_frame, "view_stage_px": 40}),
                            ("view_batch = 0", {"view_batch": 0, "view_batch_bytes": 0, "view_stage_px": 0})):
            same(run_with_knobs(*args, knobs)[0], whole, f"{vname} filter {filt}: {what}")
        hooks.hm_debug_set(b"view_batch", 1)


def test_two_groups_in_one_call(capi, L, movies, refs):
    """frames 0-2 into destinations with a padded row pitch, frames 3-4 into tight ones: two launch groups; every frame is right
    and the padding keeps its fill"""
    data, n = movies["m8"]
    frames = list(range(1, n + 1))
    crop, size = VIEWS["reduce_odd_origin"]
    sc, bi = base.imagenet(255.0)
    with Opened(L, data) as fh:
        for filt, layout, dtype, scale, bias in ((TRIANGLE, CHW, F32, sc, bi), (CUBIC, HWC, U8, ONE, ZERO)):
            made = [base.make_dest(capi, L, RGB, layout, dtype, 97, 50, scale, bias, 2 if k < 3 else 0, 0) for k in range(n)]
            dests = (capi.DeviceDest * n)(*[m[0] for m in made])
            assert dests[0].row_pitch != dests[4].row_pitch
            rc, msg, failed, out = frames_to_device(capi, L, fh, frames, RGB, dv.make_view(capi, crop, size, filt), dests)
            assert rc == 0 and failed == -1, msg
            for k, (_, g, row, plane) in enumerate(made):
                assert out[k].stride[0] == row
                vals = values(refs("m8", RGB, frames[k], crop, size, filt), filt, False, dtype, 255, scale, bias)
                same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), f"filter {filt} frame {k}")


def test_frames_of_two_sizes(hm, capi, L, pixels):
    """a track whose samples carry pictures of two sizes: the whole-frame view resolves against each frame's own size (its own tap
    tables: two groups); a crop that fits the larger pictures alone fails the call on the first smaller one, nothing written"""
    import torch
    pics = [synthutil.picture(49100 + i, width=128, height=64) for i in range(2)] + [synthutil.picture(49200 + i, width=96, height=80, vui=0) for i in range(2)] + \
        [synthutil.picture(49300, width=128, height=64)]
    data = moovwriter.write_movie(pics, (128, 64), params_in="sample")
    n = 5
    frames = list(range(1, n + 1))
    sizes = [pixels("two_sizes", RGB, f, data).shape[:2] for f in frames]
    assert sizes == [(64, 128), (64, 128), (80, 96), (80, 96), (64, 128)]
    sc, bi = base.imagenet(255.0)
    row, plane, _ = tight(RGB, CHW, F32, 64, 48)
    with Opened(L, data) as fh:
        for filt in (TRIANGLE, LANCZOS3):
            dests, g, per = slices(capi, RGB, CHW, F32, 64, 48, n, sc, bi)
            rc, msg, failed, out = frames_to_device(capi, L, fh, frames, RGB, dv.make_view(capi, None, (64, 48), filt), dests)
            assert rc == 0 and failed == -1, msg
            images = [values(vf.resample(pixels("two_sizes", RGB, f), None, (64, 48), filt), filt, False, F32, 255, sc, bi) for f in frames]
            same(g.host(), expected(g, per, images, CHW, F32, row, plane), f"two sizes, filter {filt}")
        dests, g, per = slices(capi, RGB, CHW, F32, 64, 48, n, sc, bi)
        rc, msg, failed, out = frames_to_device(capi, L, fh, frames, RGB, dv.make_view(capi, (100, 0, 28, 64), (64, 48), TRIANGLE), dests)
        assert rc == -1 and failed == 2 and "not inside the 96 x 80 image" in msg, (rc, failed, msg)
        assert all(out[k].width == 0 for k in range(n))
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all()


def test_a_refused_call_leaves_the_memory_alone(capi, L, movies, refs):
    import torch
    data, n = movies["m8"]
    frames = list(range(1, n + 1))
    crop, size = VIEWS["reduce_odd_origin"]
    view = dv.make_view(capi, crop, size, TRIANGLE)
    with Opened(L, data) as fh:
        dests, g, per = slices(capi, RGB, HWC, U8, 97, 50, n, ONE, ZERO)
        dests[n - 1].len = per - 1
        rc, msg, failed, out = frames_to_device(capi, L, fh, frames, RGB, view, dests)
        assert rc == -1 and failed == n - 1 and "len" in msg, (rc, failed, msg)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), "a refused call wrote to a destination"
        # ... and the next call on the same file succeeds
        dests[n - 1].len = per
        rc, msg, failed, _ = frames_to_device(capi, L, fh, frames, RGB, view, dests)
        assert rc == 0 and failed == -1, msg
        row, plane, _ = tight(RGB, HWC, U8, 97, 50)
        images = [values(refs("m8", RGB, f, crop, size, TRIANGLE), TRIANGLE, False, U8, 255, ONE, ZERO) for f in frames]
        same(g.host(), expected(g, per, images, HWC, U8, row, plane), "the call behind a refused one")


def test_without_a_view_it_is_the_sequence_call(capi, L, movies):
    data, n = movies["m8"]
    sc, bi = base.imagenet(255.0)
    with Opened(L, data) as fh:
        a, ga, _ = slices(capi, RGB, CHW, F32, 200, 136, n, sc, bi)
        b, gb, _ = slices(capi, RGB, CHW, F32, 200, 136, n, sc, bi)
        rc, msg, failed, out = frames_to_device(capi, L, fh, list(range(1, n + 1)), RGB, None, a)
        assert rc == 0 and failed == -1, msg
        prm = capi.DecodeParams(RGB, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out2 = (capi.Decoded * n)()
        assert L.hm_decode_sequence_to_device(fh, 1, n, C.byref(prm), b, out2, None) == 0, L.hm_last_error().decode()
        for k in range(n):
            assert (out[k].width, out[k].height, out[k].stride[0], out[k].used_ext_dst) == (out2[k].width, out2[k].height, out2[k].stride[0], 1)
    got = ga.host()
    assert np.array_equal(got, gb.host()) and not (got[ga.start:ga.start + 4096] == 0xA5).all()


def test_python_decode_sequence_to_tensor(pkg, capi, L, movies, refs):
    import torch
    data, _ = movies["m8"]
    crop, size = (3, 5, 191, 127), (64, 48)
    frames = range(1, 6, 2)
    t = pkg.decode_sequence_to_tensor(data, frames=frames, crop=crop, size=size, dtype=torch.float16, scale=1 / 255)
    assert t.is_cuda and t.dtype == torch.float16 and tuple(t.shape) == (3, 3, 48, 64)
    # ... equal to the C call, bit for bit
    sc = [float(np.float32(1 / 255))] * 4
    dests, g, per = slices(capi, RGB, CHW, F16, 64, 48, 3, sc, ZERO)
    with Opened(L, data) as fh:
        rc, msg, failed, _ = frames_to_device(capi, L, fh, list(frames), RGB, dv.make_view(capi, crop, size, TRIANGLE), dests)
    assert rc == 0, msg
    low = g.host()[g.start:g.start + 3 * per].view(np.uint16).reshape(3, 3, 48, 64)
    assert np.array_equal(t.cpu().numpy().view(np.uint16), low)
    images = [values(refs("m8", RGB, f, crop, size, TRIANGLE), TRIANGLE, False, F16, 255, sc, ZERO) for f in frames]
    assert np.array_equal(low, np.stack([v.transpose(2, 0, 1) for v in images]).view(np.uint16))
    # all frames, as they are: T x H x W x C bytes
    u8 = pkg.decode_sequence_to_tensor(data, layout="hwc", dtype=torch.uint8)
    assert tuple(u8.shape) == (5, 136, 200, 3)
    assert np.array_equal(u8[4].cpu().numpy(), refs("m8", RGB, 5, None, None, NEAREST))
    # out= with a row-strided tensor: the gaps stay as they were
    big = torch.full((3, 3, 48 + 2, 64 + 9), -7.0, dtype=torch.float32, device="cuda")
    out = big[:, :, 1:49, :64]
    assert pkg.decode_sequence_to_tensor(data, frames=[5, 1, 3], crop=crop, size=size, filter="bicubic", out=out) is out
    res = big.cpu().numpy()
    for k, f in enumerate((5, 1, 3)):
        ref = vf.to_float(refs("m8", RGB, f, crop, size, CUBIC), ONE, ZERO)
        assert np.array_equal(res[k, :, 1:49, :64], ref.transpose(2, 0, 1)), f
    assert (res[:, :, :, 64:] == -7.0).all() and (res[:, :, 0] == -7.0).all() and (res[:, :, 49] == -7.0).all()


def test_python_refuses_frames_of_differing_sizes_without_a_size(pkg):
    pics = [synthutil.picture(49100, width=128, height=64), synthutil.picture(49200, width=96, height=80, vui=0)]
    data = moovwriter.write_movie(pics, (128, 64), params_in="sample")
    # the track declares one size for all its samples: the decode finds the second frame's own size, and the error names the frame
    with pytest.raises(ValueError, match=r"frames\[1\] \(frame 2\) is 96 x 80"):
        pkg.decode_sequence_to_tensor(data)


def test_batched_kernels_use_no_scratch(pkg):
    """every instance of the batched resampling kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 6)"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(6, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and out[0] > 0, (n, out[0], out[1])
        n += 1
    # 8 horizontal and 8 staged (sample width x channels x layout), 24 vertical (dtype x store width x row kind)
    assert n == 40
