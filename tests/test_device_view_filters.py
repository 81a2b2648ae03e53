"""HM_VIEW_CUBIC and HM_VIEW_LANCZOS3, the part that needs no GPU: the tap table hm_view_filter_taps hands out against the numpy
restatement (tests/view_filters_ref.py) bit for bit, the limits and the refusals decided on the host, the exports, and the cubic
restatement against torch's antialiased bicubic interpolation on the CPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import view_filters_ref as vf

HM_ERR_INVALID_ARG = -1
RGB, RRGGBB_BE, RRGGBBAA_BE = 10, 12, 13
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
CUBIC, LANCZOS3 = vf.CUBIC, vf.LANCZOS3
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused)
# identity, up-sampling, mild reduction, prime sizes; the pair exactly at each filter's limit is added per filter
PAIRS = [(64, 64), (30, 77), (1, 5), (181, 50), (243, 97), (127, 31), (31, 127), (509, 7), (13, 11)]
AT_LIMIT = {CUBIC: (1280, 10), LANCZOS3: (850, 10)}
MAX_TAPS = 2 * 256 + 2
# test_cubic_restatement_against_torch: the largest |restatement - torch| over the four cases of the test, measured on the CPU with
# torch 2.10.  Against torch on float32 input 1.167e-3 (hard edges, 243 x 181 -> 97 x 50): torch builds its weights in float32 there,
# and its own float32 result lies 1.159e-3 from its float64 result.  Against torch on float64 input 9.58e-5, which is 3 ulp of
# float32 at 255: the restatement's float32 sums.  Each bound is 4 times its measured value (another build's summation order).
TORCH_MEASURED_F32, TORCH_MEASURED_F64 = 1.167e-3, 9.58e-5
TORCH_BOUND_F32, TORCH_BOUND_F64 = 4 * TORCH_MEASURED_F32, 4 * TORCH_MEASURED_F64


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def lib_taps(L, n, m, j, filt, cap=600):
    first = C.c_int32(-1)
    w = (C.c_float * cap)()
    cnt = L.hm_view_filter_taps(n, m, filt, j, C.byref(first), w, cap)
    assert cnt > 0, L.hm_last_error().decode()
    return first.value, np.frombuffer(w, np.float32, cnt).copy()


@pytest.mark.parametrize("filt", [CUBIC, LANCZOS3])
def test_filter_taps_equal_the_restatement_bit_for_bit(L, filt):
    negative = 0
    for n, m in PAIRS + [AT_LIMIT[filt]]:
        most = 0
        for j in range(m):
            first, w = lib_taps(L, n, m, j, filt)
            rfirst, rw, total = vf.taps_total(n, m, j, filt)
            assert first == rfirst and w.size == rw.size, (filt, n, m, j)
            assert np.array_equal(w.view(np.uint32), rw.view(np.uint32)), (filt, n, m, j)
            assert 0 <= first and first + w.size <= n and w.size <= MAX_TAPS
            assert total > 0.5, (filt, n, m, j, total)
            most = max(most, w.size)
            negative += int((w < 0).sum())
            if m == n:  # the identity: weight 1 on source index j; the window's other taps sit on the kernel's zeros
                assert first <= j < first + w.size and w[j - first] == np.float32(1.0)
                assert np.abs(np.delete(w, j - first)).max(initial=0.0) < 1e-15
        if (n, m) == AT_LIMIT[filt]:
            assert most > 500, (filt, most)  # (the limit is where the table is nearly full)
    assert negative > 0  # (lobes below zero: what the triangle never had)


def test_refusals(capi, L):
    first = C.c_int32()
    w = (C.c_float * 8)()
    for n, m, filt, words in ((1281, 10, CUBIC, ("reduction", "CUBIC", "128")), (851, 10, LANCZOS3, ("reduction", "LANCZOS3", "85")),
                              (16, 4, 2, ("filter",)), (16, 4, 3, ("filter",)), (16, 4, 15, ("filter",)), (16, 4, 18, ("filter",))):
        assert L.hm_view_filter_taps(n, m, filt, 0, C.byref(first), w, 8) == HM_ERR_INVALID_ARG, (n, m, filt)
        msg = L.hm_last_error().decode()
        assert all(word in msg for word in words), (n, m, filt, msg)
    # the limits hold for a view as for the tap entry point, on either axis, and the unknown codes stay unknown there
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = FAKE, 1 << 28, HWC, U8
    V = capi.DeviceView
    for sw, sh, view, words in ((1281, 16, V(0, 0, 0, 0, 10, 8, CUBIC), ("reduction", "CUBIC", "width")), (16, 1281, V(0, 0, 0, 0, 8, 10, CUBIC), ("reduction", "CUBIC", "height")),
                                (851, 16, V(0, 0, 0, 0, 10, 8, LANCZOS3), ("reduction", "LANCZOS3", "width")), (16, 851, V(0, 0, 0, 0, 8, 10, LANCZOS3), ("reduction", "LANCZOS3", "height")),
                                (16, 16, V(0, 0, 0, 0, 8, 8, 2), ("filter",)), (16, 16, V(0, 0, 0, 0, 8, 8, 3), ("filter",)),
                                (16, 16, V(0, 0, 0, 0, 8, 8, 15), ("filter",)), (16, 16, V(0, 0, 0, 0, 8, 8, 18), ("filter",))):
        assert L.hm_resample_to_tensor(RGB, sw, sh, FAKE, sw * 3, C.byref(view), C.byref(d), None) == HM_ERR_INVALID_ARG
        msg = L.hm_last_error().decode()
        assert all(word in msg for word in words), msg
    # a big-endian target has no sample values to resample, whatever the filter
    for filt in (CUBIC, LANCZOS3):
        for fmt, ch in ((RRGGBB_BE, 3), (RRGGBBAA_BE, 4)):
            d.dtype = U16
            assert L.hm_resample_to_tensor(fmt, 16, 16, FAKE, 16 * ch * 2, C.byref(V(0, 0, 0, 0, 8, 8, filt)), C.byref(d), None) == HM_ERR_INVALID_ARG
            assert "_LE" in L.hm_last_error().decode(), (filt, fmt, L.hm_last_error().decode())


def test_python_side(pkg, capi):
    assert (capi.HM_VIEW_CUBIC, capi.HM_VIEW_LANCZOS3) == (16, 17)
    assert (capi.HM_VIEW_TRIANGLE, capi.HM_VIEW_NEAREST) == (0, 1)
    filters = pkg.decode.FILTERS
    assert filters["bicubic"] == 16 and filters["lanczos3"] == 17 and filters["triangle"] == 0 and filters["nearest"] == 1
    assert "lanczos" not in filters and "cubic" not in filters
    assert inspect.signature(pkg.decode_to_tensor).parameters["filter"].default == "triangle"
    assert inspect.signature(pkg.decode_batch_to_tensor).parameters["filter"].default == "triangle"
    assert [n for n, _ in capi.DeviceView._fields_] == "crop_x crop_y crop_w crop_h out_w out_h filter".split()


def test_to_integer_rounds_towards_zero_and_clamps():
    r = np.array([-3.0, -1.5, -0.75, -0.5, -0.25, 0.25, 0.5, 254.49, 254.5, 255.4, 255.5, 300.0], np.float32)
    assert vf.to_integer(r, 255).tolist() == [0, 0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 255]
    assert np.trunc(np.float32(-1.5) + np.float32(0.5)) == -1.0  # (what the clamp at 0 is for)


def _images():
    rng = np.random.default_rng(4801)
    out = {}
    for h, w in ((181, 243), (30, 30)):
        edges = np.zeros((h, w, 3), np.uint8)
        for y0 in range(0, h, 7):
            for x0 in range(0, w, 9):
                if (y0 // 7 + x0 // 9) % 2:
                    edges[y0:y0 + 7, x0:x0 + 9] = 255
        out[(h, w)] = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), edges)
    return out


def test_cubic_restatement_against_torch():
    """the cubic tap rule is torch's (and PIL's) antialiased bicubic: the float32 sums of the restatement, before any rounding,
    against torch.nn.functional.interpolate on the CPU, on float32 input (what a pipeline runs) and on float64 input (torch's
    weights in double, as the restatement's).  The two differ in rounding only."""
    import torch
    worst = {torch.float32: 0.0, torch.float64: 0.0}
    images = _images()
    for (h, w), (oh, ow) in (((181, 243), (50, 97)), ((30, 30), (77, 77))):
        for k, img in enumerate(images[(h, w)]):
            ours = vf.resample(img, None, (ow, oh), CUBIC).astype(np.float64)
            for dt in worst:
                t = torch.from_numpy(img).to(dt).permute(2, 0, 1)[None]
                theirs = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
                diff = float(np.abs(ours - theirs.astype(np.float64)).max())
                print(f"cubic restatement against torch {torch.__version__} on {dt}: {w} x {h} -> {ow} x {oh}, image {k}: largest difference {diff:.3e}")
                worst[dt] = max(worst[dt], diff)
                if k == 1:  # hard edges: both overshoot
                    assert ours.min() < -1.0 and ours.max() > 256.0 and theirs.min() < -1.0 and theirs.max() > 256.0
    print(f"largest of all: {worst[torch.float32]:.3e} (bound {TORCH_BOUND_F32:.3e}), {worst[torch.float64]:.3e} (bound {TORCH_BOUND_F64:.3e})")
    assert worst[torch.float32] < TORCH_BOUND_F32 and worst[torch.float64] < TORCH_BOUND_F64, worst
