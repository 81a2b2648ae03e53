"""Host side of many views of one picture (hm_decode_item_to_device_views, hm_resample_views_to_tensor, hm_plan_views,
decode_to_views): the sub-grid the bounding rectangle of all crops picks, every refusal that is decided before a device is looked
at, and the exports.  No GPU."""
import ctypes as C
import inspect
import os

import pytest

import heifwriter
import synthutil
import test_device_view as tv

RGB = tv.RGB
HWC, CHW, U8, F32 = tv.HWC, tv.CHW, tv.U8, tv.F32
TRIANGLE, NEAREST = tv.TRIANGLE, tv.NEAREST
HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_NO_DEVICE = tv.HM_ERR_INVALID_ARG, -2, tv.HM_ERR_NO_DEVICE
FAKE = tv.FAKE
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def files():
    """the 4 x 3 grid of 64 x 64 tiles on a 181 x 243 canvas of test_device_view.py's plan test, and a single image"""
    tiles = [synthutil.picture(46000 + t, width=64, height=64) for t in range(12)]
    return heifwriter.write_heic(tiles, (64, 64), grid=tv.GRID), heifwriter.write_heic([synthutil.picture(46100, width=96, height=64)], (96, 64))


def views_of(capi, specs):
    """specs: (crop, size) pairs -> hm_device_view[]"""
    v = (capi.DeviceView * len(specs))()
    for k, (crop, size) in enumerate(specs):
        v[k] = capi.DeviceView(*(crop or (0, 0, 0, 0)), *(size or (0, 0)), TRIANGLE)
    return v


def plan_views(capi, f, crops, upsampling=0):
    prm = capi.DecodeParams(RGB, 1, 0, upsampling, None, None, 0, 0, 0, 0)
    t = (C.c_int32 * 4)()
    v = views_of(capi, [(c, (16, 16)) for c in crops])
    assert f.L.hm_plan_views(f.h, f.id, C.byref(prm), v, len(crops), C.byref(t)) == 0, f.L.hm_last_error().decode()
    return tuple(t)


def test_plan_views(capi, L, files):
    f, s = tv.File(L, files[0]), tv.File(L, files[1])
    try:
        # two crops in opposite corners: the bounding rectangle is the image, the whole grid is decoded
        assert plan_views(capi, f, [(0, 0, 10, 10), (171, 233, 10, 10)]) == (0, 4, 0, 3)
        # two crops inside tile row 1 (rows 64 .. 127), at both ends of it: that row's sub-grid
        assert plan_views(capi, f, [(5, 70, 20, 20), (150, 100, 20, 20)]) == (1, 1, 0, 3)
        # ... and inside one tile: that tile; in any order
        assert plan_views(capi, f, [(70, 70, 10, 10), (90, 100, 20, 20), (80, 64, 5, 5)]) == (1, 1, 1, 1)
        assert plan_views(capi, f, [(130, 200, 20, 20), (70, 70, 10, 10)]) == (1, 3, 1, 2)
        # a bounding rectangle with an odd origin (65, 71): the sub-grid's origin is a tile's, even in both directions, and the answer is
        # hm_plan_view's for the bounding rectangle taken as one crop
        odd = plan_views(capi, f, [(65, 75, 10, 10), (91, 71, 5, 5)])
        assert odd == f.plan(capi, (65, 71, 31, 14)) == (1, 1, 1, 1) and (odd[0] * 64) % 2 == 0 and (odd[2] * 64) % 2 == 0
        # count = 1: hm_plan_view
        for name, (crop, want) in tv.CROPS.items():
            assert plan_views(capi, f, [crop]) == want == f.plan(capi, crop), name
        # a view without a crop among them takes the whole image; so does what stops hm_plan_view's reduction
        assert plan_views(capi, f, [(70, 70, 10, 10), (0, 0, 0, 0)]) == (0, 4, 0, 3)
        assert plan_views(capi, f, [(70, 70, 10, 10)], upsampling=2) == (0, 4, 0, 3)
        assert plan_views(capi, f, [(70, 70, 10, 10), (175, 70, 10, 10)]) == (0, 4, 0, 3)  # (a crop that is refused anyway)
        assert plan_views(capi, s, [(3, 5, 40, 30), (50, 5, 10, 10)]) == (0, 1, 0, 1)      # a single image
        prm = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0)
        v, t = views_of(capi, [((1, 1, 5, 5), None)]), (C.c_int32 * 4)()
        assert L.hm_plan_views(None, f.id, C.byref(prm), v, 1, C.byref(t)) == HM_ERR_INVALID_ARG
        assert L.hm_plan_views(f.h, f.id, C.byref(prm), None, 1, C.byref(t)) == HM_ERR_INVALID_ARG
        assert L.hm_plan_views(f.h, f.id, C.byref(prm), v, 1, None) == HM_ERR_INVALID_ARG
        assert L.hm_plan_views(f.h, f.id, C.byref(prm), v, 0, C.byref(t)) == HM_ERR_INVALID_ARG
        assert L.hm_plan_views(f.h, 999, C.byref(prm), v, 1, C.byref(t)) == HM_ERR_INVALID_ARG
    finally:
        f.close(), s.close()


def dests_of(capi, lens, layout=HWC, dtype=U8, step=1 << 20):
    """destinations `step` bytes apart from FAKE on (never dereferenced on the host)"""
    d = (capi.DeviceDest * len(lens))()
    for k, n in enumerate(lens):
        d[k] = tv.dest(capi, layout, dtype, n, ptr=FAKE + k * step)
    return d


def call(capi, L, f, views, dests, n, fmt=RGB, light=None, tone=None):
    prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
    out = (capi.Decoded * max(n, 1))()
    failed = C.c_int32(-7)
    rc = L.hm_decode_item_to_device_views(f.h, f.id, C.byref(prm), views, dests, n, light, tone, None, None, out, C.byref(failed))
    assert not out[0].plane[0]
    return rc, L.hm_last_error().decode(), failed.value


def test_refusals_without_a_device(capi, L, files):
    f, s = tv.File(L, files[0]), tv.File(L, files[1])
    big = 1 << 19
    try:
        specs = [((3, 5, 40, 30), (16, 16)), (None, (50, 37)), ((100, 100, 33, 21), None)]
        good = views_of(capi, specs)
        # count outside 1 .. HM_VIEWS_MOST, null arrays: no view's refusal
        many_v, many_d = (capi.DeviceView * 4097)(), (capi.DeviceDest * 4097)()
        for n in (0, -1, 4097):
            rc, msg, failed = call(capi, L, f, many_v, many_d, n)
            assert rc == HM_ERR_INVALID_ARG and "count" in msg and "4096" in msg and failed == -1, (n, rc, msg, failed)
        assert capi.HM_VIEWS_MOST == 4096
        for v, d in ((None, dests_of(capi, [big] * 3)), (good, None)):
            rc, msg, failed = call(capi, L, f, v, d, 3)
            assert rc == HM_ERR_INVALID_ARG and "null argument" in msg and failed == -1
        # what the single-view entry refuses for one view, with that view's index: in the last, the middle and the first
        for k, view, d_len, word in ((2, ((170, 100, 33, 21), None), big, "not inside"), (1, (None, (50, 37)), 50 * 37 * 3 - 1, "len"),
                                     (0, ((3, 5, 40, 30), (0, 16)), big, "1 .. 32768"), (2, ((100, 100, 0, 21), None), big, "not positive")):
            sp, lens = list(specs), [big] * 3
            sp[k], lens[k] = view, d_len
            rc, msg, failed = call(capi, L, f, views_of(capi, sp), dests_of(capi, lens), 3)
            assert rc == HM_ERR_INVALID_ARG and word in msg and msg.startswith(f"view {k}: ") and failed == k, (k, rc, msg, failed)
        bad = views_of(capi, specs)
        bad[1].filter = 2
        rc, msg, failed = call(capi, L, f, bad, dests_of(capi, [big] * 3), 3)
        assert rc == HM_ERR_INVALID_ARG and "filter" in msg and failed == 1
        d = dests_of(capi, [big] * 3)
        d[2].ptr = None
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert rc == HM_ERR_INVALID_ARG and "null ptr" in msg and failed == 2
        d = dests_of(capi, [big] * 3)
        d[1].dtype = tv.U16
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert rc == HM_ERR_INVALID_ARG and "dtype" in msg and failed == 1
        # two destinations whose byte ranges overlap: by one byte, and one inside another; both indices are named, no view is singled out
        need = [16 * 16 * 3, 50 * 37 * 3, 33 * 21 * 3]
        d = dests_of(capi, [big] * 3)
        d[2].ptr = FAKE + need[0] - 1
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert rc == HM_ERR_INVALID_ARG and "views 0 and 2 overlap" in msg and failed == -1, msg
        d[2].ptr = FAKE + need[0]  # (behind the bytes view 0 writes, whatever len says: the range is the size written)
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert "overlap" not in msg
        d = dests_of(capi, [big] * 3)
        d[0].ptr = FAKE + (1 << 20) + 100  # inside view 1's 5550 bytes
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert rc == HM_ERR_INVALID_ARG and "views 0 and 1 overlap" in msg and failed == -1, msg
        # ... with the row pitch as resolved: rows 1000 bytes apart reach further than the tight size
        d = dests_of(capi, [big] * 3)
        d[0].row_pitch = 1000
        d[2].ptr = FAKE + 15 * 1000 + 47
        rc, msg, failed = call(capi, L, f, good, d, 3)
        assert rc == HM_ERR_INVALID_ARG and "views 0 and 2 overlap" in msg, msg
        d[2].ptr = FAKE + 15 * 1000 + 48
        assert "overlap" not in call(capi, L, f, good, d, 3)[1]
        # the steps: a tone step needs a light step; a planar target has no device destination
        tone = capi.DeviceTone()
        rc, msg, failed = call(capi, L, f, good, dests_of(capi, [big] * 3), 3, tone=C.byref(tone))
        assert rc == HM_ERR_INVALID_ARG and "tone: null light step" in msg and failed == -1
        rc, msg, failed = call(capi, L, f, good, dests_of(capi, [big] * 3), 3, fmt=0x101)
        assert rc == HM_ERR_UNSUPPORTED and "not supported with a device destination" in msg and failed == 0
        # a request that is in order: a box without a GPU says so; with one, the first pointer is found not to be device memory
        rc, msg, failed = call(capi, L, s, views_of(capi, [((3, 5, 40, 30), (16, 16)), (None, (8, 8))]), dests_of(capi, [big] * 2), 2)
        if L.hm_device_count() == 0:
            assert rc == HM_ERR_NO_DEVICE and failed == -1, msg
        else:
            assert rc == HM_ERR_INVALID_ARG and "ptr" in msg and failed == 0, msg
    finally:
        f.close(), s.close()


def test_an_unci_item_is_refused(capi, L):
    data = open(os.path.join(HERE, "golden", "unci", "uncompressed_pix_RGB_tiled.heif"), "rb").read()
    f = tv.File(L, data)
    try:
        rc, msg, failed = call(capi, L, f, views_of(capi, [((0, 0, 2, 2), None)]), dests_of(capi, [1 << 19]), 1)
        assert rc == HM_ERR_UNSUPPORTED and "unci" in msg and "hm_decode_item_to_device_view" in msg and failed == -1, (rc, msg)
    finally:
        f.close()


def test_resample_views_refusals(capi, L):
    big = 1 << 19
    good = views_of(capi, [((3, 5, 40, 30), (16, 16)), (None, (50, 37))])

    def run(views, dests, n, w=200, h=136, src=FAKE + (1 << 24), stride=600):
        rc = L.hm_resample_views_to_tensor(RGB, w, h, src, stride, views, dests, n, None)
        return rc, L.hm_last_error().decode()
    for n in (0, 4097):
        rc, msg = run((capi.DeviceView * 4097)(), (capi.DeviceDest * 4097)(), n)
        assert rc == HM_ERR_INVALID_ARG and "count" in msg
    assert run(None, dests_of(capi, [big] * 2), 2)[0] == HM_ERR_INVALID_ARG and run(good, None, 2)[0] == HM_ERR_INVALID_ARG
    assert run(good, dests_of(capi, [big] * 2), 2, src=None)[0] == HM_ERR_INVALID_ARG
    rc, msg = run(views_of(capi, [((3, 5, 40, 30), (16, 16)), ((190, 5, 40, 30), (16, 16))]), dests_of(capi, [big] * 2), 2)
    assert rc == HM_ERR_INVALID_ARG and msg.startswith("view 1: ") and "not inside" in msg
    rc, msg = run(good, dests_of(capi, [big, 50 * 37 * 3 - 1]), 2)
    assert rc == HM_ERR_INVALID_ARG and msg.startswith("view 1: ") and "len" in msg
    d = dests_of(capi, [big] * 2)
    d[1].ptr = FAKE + 16 * 16 * 3 - 1
    rc, msg = run(good, d, 2)
    assert rc == HM_ERR_INVALID_ARG and "views 0 and 1 overlap" in msg
    rc, msg = run(good, dests_of(capi, [big] * 2), 2, stride=599)
    assert rc == HM_ERR_INVALID_ARG and "src_stride" in msg
    rc, msg = run(good, dests_of(capi, [big] * 2), 2)
    assert rc == (HM_ERR_NO_DEVICE if L.hm_device_count() == 0 else HM_ERR_INVALID_ARG), msg


def test_python_refusals_and_crops_of_regions(pkg, files):
    with pytest.raises(ValueError, match="decode_to_tensor"):
        pkg.decode_to_views(files[1], [((0, 0, 8, 8), None)], light=True, gain=dict(headroom=1.0))
    with pytest.raises(ValueError, match="decode_to_tensor"):
        pkg.decode_to_views(files[1], [((0, 0, 8, 8), None)], light=True, tone=dict(dst_peak=203.0, src_peak="measured"))
    with pytest.raises(ValueError, match="views"):
        pkg.decode_to_views(files[1], [])
    with pytest.raises(ValueError, match=r"views\[1\]"):
        pkg.decode_to_views(files[1], [((0, 0, 8, 8), None), ((0, 0, 8, 8),)])
    import numpy as np
    item = dict(item_id=7, reference_size=(64, 48), regions=[
        dict(type="rectangle", x=3, y=4, w=20, h=9, points=np.zeros((0, 2), np.int32), mask_item=0),
        dict(type="rectangle", x=-5, y=40, w=20, h=20, points=np.zeros((0, 2), np.int32), mask_item=0),     # clipped to the image
        dict(type="polygon", x=0, y=0, w=0, h=0, points=np.array([(5, 3), (60, 10), (20, 40)], np.int32), mask_item=0),
        dict(type="ellipse", x=30, y=20, w=12, h=7, points=np.zeros((0, 2), np.int32), mask_item=0),
        dict(type="point", x=63, y=47, w=0, h=0, points=np.zeros((0, 2), np.int32), mask_item=0),
        dict(type="rectangle", x=70, y=4, w=20, h=9, points=np.zeros((0, 2), np.int32), mask_item=0)])       # outside: left out
    assert pkg.crops_of_regions([item], (64, 48)) == [(3, 4, 20, 9), (0, 40, 15, 8), (5, 3, 56, 38), (18, 13, 25, 15), (63, 47, 1, 1)]
    assert pkg.crops_of_regions(item) == [(3, 4, 20, 9), (-5, 40, 20, 20), (5, 3, 56, 38), (18, 13, 25, 15), (63, 47, 1, 1), (70, 4, 20, 9)]
    # a reference space of half the image's size: the rectangles are scaled outwards
    assert pkg.crops_of_regions([item], (128, 96))[0] == (6, 8, 40, 18)


def test_exports(pkg, capi, L):
    for name in ("hm_decode_item_to_device_views", "hm_resample_views_to_tensor", "hm_plan_views"):
        assert hasattr(L, name), name
    sig = inspect.signature(pkg.decode_to_views).parameters
    assert list(sig)[:2] == ["data", "views"] and sig["filter"].default == "triangle" and sig["out"].default is None
    assert callable(pkg.crops_of_regions)
