"""Planar views (a view, hm_device_view, into hm_device_planes), the part that needs no GPU: the exported geometry
(hm_planes_view_geometry) against the numpy restatement (tests/planes_view_ref.py) over every chroma format, odd and even sizes and
crops at even origins; odd origins refused in exactly the sub-sampled directions; the reduction limits per plane and axis; and the
argument that the chroma crop lies inside the chroma plane, exhaustively for small images."""
import ctypes as C
import itertools

import pytest

import planes_view_ref as ref

HM_ERR_INVALID_ARG = -1
FILTERS = (ref.TRIANGLE, ref.NEAREST, ref.CUBIC, ref.LANCZOS3)


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def geometry(capi, L, chroma, W, H, crop, size, filt=ref.TRIANGLE):
    """(status, crops, outs, message) of hm_planes_view_geometry"""
    v = capi.DeviceView()
    if crop:
        v.crop_x, v.crop_y, v.crop_w, v.crop_h = crop
    if size:
        v.out_w, v.out_h = size
    v.filter = filt
    crops, outs = (C.c_int32 * 4 * 4)(), (C.c_int32 * 2 * 4)()
    rc = L.hm_planes_view_geometry(chroma, W, H, C.byref(v), C.byref(crops), C.byref(outs))
    return rc, [tuple(crops[c]) for c in range(4)], [tuple(outs[c]) for c in range(4)], L.hm_last_error().decode()


def test_geometry_equals_the_restatement(capi, L):
    seen = 0
    for chroma, (W, H) in itertools.product(range(4), [(200, 136), (117, 171), (121, 77), (64, 64), (1, 1), (2, 3)]):
        crops = [None, (0, 0, W, H), (0, 0, (W + 1) // 2, (H + 1) // 2), (W // 4 * 2, H // 4 * 2, W - W // 4 * 2, H - H // 4 * 2),
                 (W // 4 * 2, H // 4 * 2, max(1, W // 3), max(1, H // 3)), (0, 0, 1, 1)]
        for crop, size in itertools.product(crops, [None, (77, 51), (16, 16), (1, 1), (W, H), (2 * W + 1, 2 * H + 1)]):
            n_w, n_h = (crop[2], crop[3]) if crop else (W, H)
            if size and (n_w > 256 * size[0] or n_h > 256 * size[1]):
                continue
            rc, crops_c, outs_c, msg = geometry(capi, L, chroma, W, H, crop, size)
            assert rc == 0, (chroma, W, H, crop, size, msg)
            exp_crops, exp_outs = ref.geometry(chroma, W, H, crop, size)
            assert crops_c == exp_crops and outs_c == exp_outs, (chroma, W, H, crop, size)
            # the chroma output is the plane size of an ow x oh result, and every crop lies inside its plane
            ow, oh = outs_c[0]
            cw, ch = (ow if chroma == 3 else (ow + 1) // 2), ((oh + 1) // 2 if chroma == 1 else oh)
            assert outs_c[3] == outs_c[0] and (chroma == 0 or outs_c[1] == outs_c[2] == (cw, ch))
            pw, ph = (W if chroma == 3 else (W + 1) // 2), ((H + 1) // 2 if chroma == 1 else H)
            for c in (1, 2) if chroma else ():
                x, y, w, h = crops_c[c]
                assert w >= 1 and h >= 1 and x + w <= pw and y + h <= ph
            if chroma == 0:
                assert crops_c[1] == crops_c[2] == (0, 0, 0, 0) and outs_c[1] == outs_c[2] == (0, 0)
            seen += 1
    assert seen > 500


def test_odd_origins_are_refused_in_exactly_the_subsampled_directions(capi, L):
    for chroma in range(4):
        sx, sy = ref.sub(chroma)
        for x, y in itertools.product((0, 1, 2, 3), repeat=2):
            rc, _, _, msg = geometry(capi, L, chroma, 40, 30, (x, y, 20, 10), (10, 5))
            ok = x % sx == 0 and y % sy == 0
            assert (rc == 0) == ok, (chroma, x, y, msg)
            if not ok:
                assert rc == HM_ERR_INVALID_ARG and ("crop_x" if x % sx else "crop_y") in msg, msg
                with pytest.raises(ValueError):
                    ref.geometry(chroma, 40, 30, (x, y, 20, 10), (10, 5))
    # odd extents are fine
    assert geometry(capi, L, 1, 41, 31, (2, 2, 39, 29), (7, 3))[0] == 0


def test_refusals_of_the_view_itself(capi, L):
    for crop in [(0, 0, 41, 30), (2, 0, 39, 30), (0, 2, 40, 29), (-2, 0, 10, 10), (0, 0, 0, 5), (0, 0, 5, -1)]:
        rc, _, _, msg = geometry(capi, L, 1, 40, 30, crop, (8, 8))
        assert rc == HM_ERR_INVALID_ARG and "crop" in msg, (crop, msg)
    assert geometry(capi, L, 1, 40, 30, None, (8, 8), filt=5)[0] == HM_ERR_INVALID_ARG
    assert geometry(capi, L, 4, 40, 30, None, (8, 8))[0] == HM_ERR_INVALID_ARG
    assert geometry(capi, L, 1, 0, 30, None, (8, 8))[0] == HM_ERR_INVALID_ARG
    assert geometry(capi, L, 1, 40, 30, None, (0, 8))[0] == HM_ERR_INVALID_ARG
    assert geometry(capi, L, 1, 40, 30, None, (32769, 8))[0] == HM_ERR_INVALID_ARG
    assert L.hm_planes_view_geometry(1, 40, 30, None, None, None) == HM_ERR_INVALID_ARG


def test_reduction_limits_hold_per_plane_and_axis(capi, L):
    """accepted exactly where every plane's every axis is inside the filter's limit: around the limit on each axis, odd and even
    crops, so that the chroma axis (w + 1) / 2 -> (ow + 1) / 2 sits on both sides of its luma axis"""
    for filt, chroma in itertools.product(FILTERS, range(4)):
        most = ref.vf.MAX_REDUCTION.get(filt, 256)
        for ow, d in itertools.product((1, 2, 3, 4), (-2, -1, 0, 1, 2)):
            n = most * ow + d
            for crop, size in (((0, 0, n, 8), (ow, 4)), ((0, 0, 8, n), (4, ow))):
                W, H = max(crop[2], 8), max(crop[3], 8)
                rc, crops, outs, msg = geometry(capi, L, chroma, W, H, crop, size, filt)
                exp_crops, exp_outs = ref.geometry(chroma, W, H, crop, size)
                assert (rc == 0) == ref.within_limits(exp_crops, exp_outs, filt, chroma), (filt, chroma, crop, size, msg)
                if rc:
                    assert rc == HM_ERR_INVALID_ARG and "reduction" in msg, msg


def test_the_chroma_crop_lies_inside_the_chroma_plane():
    """(x + w + 1) / 2 <= (W + 1) / 2 for every even x and every w with x + w <= W: exhaustively for W <= 20 (the vertical axis is
    the same statement), and through the restatement for every origin and extent of either axis of images up to 20 x 20"""
    for W in range(1, 21):
        for x in range(0, W, 2):
            for w in range(1, W - x + 1):
                assert x // 2 + (w + 1) // 2 == (x + w + 1) // 2 <= (W + 1) // 2
    for chroma in (1, 2, 3):
        sx, sy = ref.sub(chroma)
        for N in range(1, 21):  # every origin and every extent on one axis, the other axis held at 2 rows / columns
            for o in range(N):
                for n in range(1, N - o + 1):
                    if o % sx == 0:
                        cx, _, cw, _ = ref.geometry(chroma, N, 2, (o, 0, n, 2), None)[0][1]
                        assert cw >= 1 and cx + cw <= (N + sx - 1) // sx
                    if o % sy == 0:
                        _, cy, _, ch = ref.geometry(chroma, 2, N, (0, o, 2, n), None)[0][1]
                        assert ch >= 1 and cy + ch <= (N + sy - 1) // sy
        for W, H in itertools.product(range(1, 21), repeat=2):  # ... and both axes together at the extremes
            pw, ph = (W + sx - 1) // sx, (H + sy - 1) // sy
            for x, y in itertools.product(range(0, W, sx), range(0, H, sy)):
                for w, h in ((1, 1), (W - x, H - y)):
                    cx, cy, cw, ch = ref.geometry(chroma, W, H, (x, y, w, h), None)[0][1]
                    assert cw >= 1 and ch >= 1 and cx + cw <= pw and cy + ch <= ph
