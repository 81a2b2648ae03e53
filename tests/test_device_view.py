"""Views (hm_device_view), the part that needs no GPU: the tap table hm_view_filter_taps hands out against the numpy restatement
(tests/view_ref.py) bit for bit, the sub-grid hm_plan_view picks, every refusal that is decided on the host, and the exports."""
import ctypes as C
import inspect

import numpy as np
import pytest

import heifwriter
import synthutil
import view_ref

HM_ERR_INVALID_ARG, HM_ERR_NO_DEVICE = -1, -4
RGB, RRGGBB_BE, RRGGBB_LE = 10, 12, 14
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
TRIANGLE, NEAREST = 0, 1
PAIRS = [(1, 1), (7, 7), (181, 50), (243, 37), (200, 7), (33, 64), (4032, 224), (5, 1)]
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def lib_taps(L, n, m, j, filt=TRIANGLE, cap=600):
    first = C.c_int32(-1)
    w = (C.c_float * cap)()
    cnt = L.hm_view_filter_taps(n, m, filt, j, C.byref(first), w, cap)
    assert cnt > 0, L.hm_last_error().decode()
    return first.value, np.frombuffer(w, np.float32, cnt).copy()


@pytest.mark.parametrize("n,m", PAIRS)
def test_filter_taps_equal_the_restatement_bit_for_bit(L, n, m):
    for j in range(m):
        first, w = lib_taps(L, n, m, j)
        rfirst, rw = view_ref.taps(n, m, j)
        assert first == rfirst and w.size == rw.size, (n, m, j)
        assert np.array_equal(w.view(np.uint32), rw.view(np.uint32)), (n, m, j)
        assert 0 <= first and first + w.size <= n
        # every row sums to 1 within 2 ulp of float32 (checked, not relied on), summed the way the kernels sum
        total = np.float32(0)
        for x in w:
            total = np.float32(total + x)
        assert abs(float(total) - 1.0) <= 2 * float(np.spacing(np.float32(1.0))), (n, m, j, total)
        if m == n:  # the identity: weight 1 on source index j, and exact zeros where the window reaches a neighbour
            assert first <= j < first + w.size and w[j - first] == np.float32(1.0) and np.count_nonzero(w) == 1
        nfirst, nw = lib_taps(L, n, m, j, NEAREST)
        assert nfirst == j * n // m and nw.size == 1 and nw[0] == 1.0


def test_filter_taps_refusals(L):
    first = C.c_int32()
    w = (C.c_float * 8)()
    for n, m, filt, j, word in ((0, 4, TRIANGLE, 0, "extent"), (4, 0, TRIANGLE, 0, "1 .. 32768"), (4, 32769, TRIANGLE, 0, "1 .. 32768"),
                                (2571, 10, TRIANGLE, 0, "more than 256"), (16, 4, 2, 0, "filter"), (16, 4, TRIANGLE, 4, "index"), (16, 4, TRIANGLE, -1, "index")):
        assert L.hm_view_filter_taps(n, m, filt, j, C.byref(first), w, 8) == HM_ERR_INVALID_ARG
        assert word in L.hm_last_error().decode(), (n, m, filt, j, L.hm_last_error().decode())
    assert L.hm_view_filter_taps(16, 4, TRIANGLE, 0, None, w, 8) == HM_ERR_INVALID_ARG
    # 2560 -> 10 is a reduction by exactly 256: allowed, and the count may exceed the caller's cap
    cnt = L.hm_view_filter_taps(2560, 10, TRIANGLE, 5, C.byref(first), w, 8)
    assert 500 < cnt <= 514


GRID = (4, 3, 181, 243)  # rows, cols, canvas: the last column is clipped to 53 of 64, the last row to 51 of 64
CROPS = {"inside_one_tile": ((70, 70, 30, 40), (1, 1, 1, 1)), "across_a_2x2_corner": ((50, 100, 40, 50), (1, 2, 0, 2)),
         "clipped_last_column_and_row": ((150, 200, 31, 43), (3, 1, 2, 1)), "whole_image": ((0, 0, 0, 0), (0, 4, 0, 3)),
         "whole_image_spelled_out": ((0, 0, 181, 243), (0, 4, 0, 3))}


@pytest.fixture(scope="module")
def grid_files():
    tiles = [synthutil.picture(46000 + t, width=64, height=64) for t in range(12)]
    plain = heifwriter.write_heic(tiles, (64, 64), grid=GRID)
    turned = heifwriter.write_heic(tiles, (64, 64), grid=GRID, transforms=[("irot", 1)])
    single = heifwriter.write_heic([synthutil.picture(46100, width=96, height=64)], (96, 64))
    return plain, turned, single


class File:
    def __init__(self, L, data):
        self.L, self.h = L, C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(self.h)) == 0
        self.id = L.hm_file_primary_item(self.h)

    def plan(self, capi, crop, upsampling=0, ignore=0, size=(32, 32)):
        prm = capi.DecodeParams(RGB, 1, ignore, upsampling, None, None, 0, 0, 0, 0)
        v = capi.DeviceView(*crop, size[0], size[1], TRIANGLE)
        t = (C.c_int32 * 4)()
        assert self.L.hm_plan_view(self.h, self.id, C.byref(prm), C.byref(v), C.byref(t)) == 0, self.L.hm_last_error().decode()
        return tuple(t)

    def close(self):
        self.L.hm_file_close(self.h)


def test_plan_view(capi, L, grid_files):
    plain, turned, single = grid_files
    f, g, s = File(L, plain), File(L, turned), File(L, single)
    try:
        for name, (crop, want) in CROPS.items():
            assert f.plan(capi, crop) == want, name
            assert f.plan(capi, crop, size=(0, 0)) == want, name  # (the output size plays no part)
        small = CROPS["inside_one_tile"][0]
        assert g.plan(capi, small) == (0, 4, 0, 3)                 # irot on the item: no reduction
        assert g.plan(capi, small, ignore=1) == (1, 1, 1, 1)       # ... unless it is not applied
        assert f.plan(capi, small, upsampling=2) == (0, 4, 0, 3)   # forced bilinear chroma up-sampling: no reduction
        assert f.plan(capi, (170, 70, 30, 40)) == (0, 4, 0, 3)     # a crop that is refused anyway
        assert s.plan(capi, (3, 5, 40, 30)) == (0, 1, 0, 1)        # a single image
        prm = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0)
        v = capi.DeviceView()
        t = (C.c_int32 * 4)()
        assert L.hm_plan_view(None, f.id, C.byref(prm), C.byref(v), C.byref(t)) == HM_ERR_INVALID_ARG
        assert L.hm_plan_view(f.h, f.id, C.byref(prm), None, C.byref(t)) == HM_ERR_INVALID_ARG
        assert L.hm_plan_view(f.h, f.id, C.byref(prm), C.byref(v), None) == HM_ERR_INVALID_ARG
        assert L.hm_plan_view(f.h, 999, C.byref(prm), C.byref(v), C.byref(t)) == HM_ERR_INVALID_ARG
    finally:
        f.close(), g.close(), s.close()


def dest(capi, layout, dtype, length, ptr=FAKE):
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = ptr, length, layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    return d


def test_view_host_side_refusals(capi, L, grid_files):
    plain, _, single = grid_files
    f, s = File(L, plain), File(L, single)
    big = 1 << 28

    def call(file, fmt, view, d):
        prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_view(file.h, file.id, C.byref(prm), C.byref(view), C.byref(d), C.byref(out))
        assert not out.plane[0]
        return rc, L.hm_last_error().decode()
    try:
        V = capi.DeviceView
        for fmt, view, d, word in (
                (RGB, V(0, 0, -3, 10, 8, 8, TRIANGLE), dest(capi, HWC, U8, big), "not positive"),
                (RGB, V(0, 0, 10, 0, 8, 8, TRIANGLE), dest(capi, HWC, U8, big), "not positive"),
                (RGB, V(170, 0, 12, 10, 8, 8, TRIANGLE), dest(capi, HWC, U8, big), "not inside"),
                (RGB, V(0, 240, 12, 4, 8, 8, TRIANGLE), dest(capi, HWC, U8, big), "not inside"),
                (RGB, V(-1, 0, 12, 4, 8, 8, TRIANGLE), dest(capi, HWC, U8, big), "not inside"),
                (RGB, V(0, 0, 0, 0, 8, 0, TRIANGLE), dest(capi, HWC, U8, big), "1 .. 32768"),
                (RGB, V(0, 0, 0, 0, 0, 8, TRIANGLE), dest(capi, HWC, U8, big), "1 .. 32768"),
                (RGB, V(0, 0, 0, 0, 32769, 8, TRIANGLE), dest(capi, HWC, U8, big), "1 .. 32768"),
                (RGB, V(0, 0, 0, 0, 8, -2, TRIANGLE), dest(capi, HWC, U8, big), "1 .. 32768"),
                (RGB, V(0, 0, 0, 0, 8, 8, 2), dest(capi, HWC, U8, big), "filter"),
                (RGB, V(0, 0, 0, 0, 0, 0, -1), dest(capi, HWC, U8, big), "filter"),
                (RRGGBB_BE, V(0, 0, 0, 0, 8, 8, TRIANGLE), dest(capi, HWC, U16, big), "_LE"),
                (RRGGBB_BE, V(0, 0, 0, 0, 8, 8, NEAREST), dest(capi, CHW, U16, big), "_LE"),
                # what hm_decode_item_to_device refuses, judged against out_w x out_h
                (RGB, V(0, 0, 0, 0, 50, 37, TRIANGLE), dest(capi, HWC, U8, 50 * 37 * 3 - 1), "len"),
                (RGB, V(0, 0, 0, 0, 50, 37, TRIANGLE), dest(capi, CHW, F32, 50 * 37 * 12 - 1), "len"),
                (RGB, V(5, 5, 33, 21, 0, 0, TRIANGLE), dest(capi, HWC, U8, 33 * 21 * 3 - 1), "len"),
                (RGB, V(0, 0, 0, 0, 50, 37, TRIANGLE), dest(capi, CHW, U16, big), "dtype"),
                (RGB, V(0, 0, 0, 0, 50, 37, TRIANGLE), dest(capi, HWC, U8, big, ptr=None), "null ptr"),
                (0x101, V(0, 0, 0, 0, 50, 37, TRIANGLE), dest(capi, HWC, U8, big), "not supported with a device destination")):
            rc, msg = call(f, fmt, view, d)
            assert rc < 0 and word in msg, (fmt, tuple(getattr(view, n) for n, _ in view._fields_), rc, msg)
            assert rc == (HM_ERR_INVALID_ARG if fmt != 0x101 else -2)
        # a reduction by more than 256 on an axis (a single 96 x 64 image cannot show it: the grid's 243 rows to none either - use the tap entry point's bound,
        # and the resampling step on its own with a 300-row source)
        v = V(0, 0, 0, 0, 8, 1, TRIANGLE)
        assert L.hm_resample_to_tensor(RGB, 16, 300, FAKE, 64, C.byref(v), C.byref(dest(capi, HWC, U8, big)), None) == HM_ERR_INVALID_ARG
        assert "more than 256" in L.hm_last_error().decode()
        assert L.hm_resample_to_tensor(RGB, 16, 300, None, 64, C.byref(v), C.byref(dest(capi, HWC, U8, big)), None) == HM_ERR_INVALID_ARG
        assert L.hm_resample_to_tensor(RGB, 16, 300, FAKE, 47, C.byref(V(0, 0, 0, 0, 8, 8, TRIANGLE)), C.byref(dest(capi, HWC, U8, big)), None) == HM_ERR_INVALID_ARG
        assert "src_stride" in L.hm_last_error().decode()
        # NULL arguments
        prm = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        ok_view, ok_dest = V(0, 0, 0, 0, 8, 8, TRIANGLE), dest(capi, HWC, U8, big)
        assert L.hm_decode_item_to_device_view(s.h, s.id, C.byref(prm), None, C.byref(ok_dest), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device_view(s.h, s.id, C.byref(prm), C.byref(ok_view), None, C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_pipeline_submit_to_device_view(None, single, len(single), 0, 0, C.byref(ok_view), C.byref(ok_dest)) == HM_ERR_INVALID_ARG
        # a request that is in order: a box without a GPU says so; with one, the pointer is found not to be device memory
        rc, msg = call(s, RGB, ok_view, ok_dest)
        if L.hm_device_count() == 0:
            assert rc == HM_ERR_NO_DEVICE, msg
        else:
            assert rc == HM_ERR_INVALID_ARG and "ptr" in msg
    finally:
        f.close(), s.close()


def test_exports(pkg, capi, L):
    for name in ("hm_decode_item_to_device_view", "hm_pipeline_submit_to_device_view", "hm_resample_to_tensor", "hm_plan_view", "hm_view_filter_taps"):
        assert hasattr(L, name), name
    assert (capi.HM_VIEW_TRIANGLE, capi.HM_VIEW_NEAREST) == (0, 1)
    assert [n for n, _ in capi.DeviceView._fields_] == "crop_x crop_y crop_w crop_h out_w out_h filter".split()
    one = inspect.signature(pkg.decode_to_tensor).parameters
    assert one["crop"].default is None and one["size"].default is None and one["filter"].default == "triangle"
    many = inspect.signature(pkg.decode_batch_to_tensor).parameters
    assert many["size"].default is None and many["crops"].default is None
    with pytest.raises(ValueError, match="crops"):
        pkg.decode_batch_to_tensor([b"x"], crops=[None])
