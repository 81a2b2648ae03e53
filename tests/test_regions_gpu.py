"""GPU: the region rasteriser (csrc/regions.hip) against the serial model tests/regions_ref.py, bit for bit.  Canvas 67 x 45 - the width
is no multiple of 4, so every row ends in a partial dword -; destinations sit between 0xA5 guards and the WHOLE buffer is compared (the
convention of tests/test_device_planes_gpu.py): tight and padded pitches, pointers aligned to 16 bytes and odd by one byte.
STACK and LABELS, U8 / F16 / F32, a crop with an odd origin, the crop resized (STACK against tests/planes_view_ref.py applied to the
model's planes, compared as the planar-view tests compare: equal), 200 random polygons and polylines in 8 launches, and a census of
which rule decided the model's pixels (CPU: computed from the model alone)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import planes_view_ref as pv
import regions_ref as ref

CANVAS = (67, 45)
U8, F16, F32 = 0, 2, 3
ELEM = {U8: 1, F16: 2, F32: 4}
NP = {U8: np.uint8, F16: np.float16, F32: np.float32}
STACK, LABELS = 0, 1
GUARD = 512
TYPES = {"point": 0, "rectangle": 1, "ellipse": 2, "polygon": 3, "referenced_mask": 4, "inline_mask": 5, "polyline": 6}
MANY = 300  # (edges reach the lanes by uniform-address loads: no staged chunk whose size a polygon could exceed)


def _bits(w, h, seed):
    rng = np.random.default_rng(seed)
    flat = rng.integers(0, 2, w * h)
    out = bytearray((w * h + 7) // 8)
    for i, v in enumerate(flat):
        if v:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


def _mask(w, h, seed):
    m = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)
    m[::3, ::2] = 127
    m[1::3, 1::2] = 128
    return m


def _many_points(n):
    """a closed curve of n vertices around the canvas' middle whose radius wobbles: concave, with runs of collinear and repeated points"""
    return [(33 + int(round((14 + 9 * math.sin(7 * t)) * math.cos(t) * 1.6)), 22 + int(round((14 + 9 * math.sin(7 * t)) * math.sin(t))))
            for t in (2 * math.pi * k / n for k in range(n))]


GEOMETRY = [
    ("polygon", [(5, 3), (60, 10), (20, 40)]),                                   # a triangle
    ("polygon", [(10, 5), (50, 5), (50, 35), (30, 15), (10, 35)]),               # concave; horizontal and vertical edges
    ("polygon", [(5, 5), (40, 35), (40, 5), (5, 35)]),                           # a self-intersecting bow-tie: even-odd
    ("polygon", [(8, 8), (30, 8), (30, 20), (19, 14), (8, 20)]),                 # vertices exactly on sampled rows: the half-open rule
    ("polygon", []), ("polygon", [(7, 7)]), ("polygon", [(3, 40), (60, 42)]),    # 0, 1 and 2 points
    ("polygon", _many_points(MANY)),
    ("polygon", [(100, 100), (150, 100), (120, 140)]),                           # wholly off the canvas
    ("polygon", [(-20, -10), (30, 20), (-15, 60)]),                              # partly off
    ("polygon", [(60, 30), (90, 38), (62, 70)]),                                 # over the right and bottom edge
    ("polyline", [(0, 44), (20, 0), (40, 44), (66, 0)]),
    ("polyline", [(9, 9)]), ("polyline", []), ("polyline", [(-8, 20), (80, 23)]),
    ("ellipse", 20, 20, 0, 10), ("ellipse", 40, 10, 15, 0), ("ellipse", 66, 44, 0, 0), ("ellipse", 33, 22, 20, 12), ("ellipse", 0, 0, 10, 30),
    ("rectangle", 5, 5, 0, 10), ("rectangle", 5, 5, 10, 0), ("rectangle", -5, -5, 20, 20), ("rectangle", 60, 40, 100, 100), ("rectangle", 13, 7, 9, 1),
    ("point", 66, 44), ("point", -1, 3), ("point", 67, 0), ("point", 0, 0),
    ("inline_mask", -5, 3, 13, 9, _bits(13, 9, 5)),                              # unaligned rows, the left edge clipped
    ("inline_mask", 61, 40, 11, 7, _bits(11, 7, 6)),
    ("referenced_mask", -4, -6, 80, 60, _mask(80, 60, 7)),                        # a negative offset, hanging over the right and bottom edge
    ("referenced_mask", 30, 11, 5, 3, _mask(5, 3, 8)),
]
# overlap order, and a referenced-mask value of 127 against 128
_step = np.zeros((20, 30), np.uint8)
_step[:, :10], _step[:, 10:20], _step[:, 20:] = 127, 128, 255
ORDER = [("rectangle", 0, 0, 67, 45), ("ellipse", 30, 20, 25, 15), ("referenced_mask", 20, 10, 30, 20, _step), ("polygon", [(45, 0), (66, 22), (45, 44)]),
         ("rectangle", 40, 18, 10, 10), ("point", 45, 22)]


def random_shapes(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pts = [(int(x), int(y)) for x, y in rng.integers(-20, 91, (int(rng.integers(3, 13)), 2))]
        out.append(("polygon" if rng.integers(0, 2) else "polyline", pts))
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    """(regions, planes R x 45 x 67 of the model, census) - computed once, shared, left unchanged"""
    regions = {"geometry": GEOMETRY, "order": ORDER}[name] if not name.startswith("random") else random_shapes(1000 + int(name[6:]), 25)
    census = {}
    planes = ref.stack(regions, CANVAS, None, census)
    planes.setflags(write=False)
    return regions, planes, census


def test_census_of_the_cases():
    """every rule decides at least one pixel each way over the cases of this file (the model alone: no GPU)"""
    total = {}
    for name in ("geometry", "order", "random0"):
        for k, v in model(name)[2].items():
            total[k] = total.get(k, 0) + v
    assert all(total.get(k, 0) > 0 for k in ref.CENSUS_KEYS), {k: total.get(k, 0) for k in ref.CENSUS_KEYS}
    regions, planes, _ = model("geometry")
    assert not planes[4].any() and planes[5].sum() == 255 and not planes[8].any() and not planes[13].any() and planes[12].sum() == 255
    assert planes[17].sum() == 255 and not planes[20].any() and not planes[21].any() and not planes[26].any() and not planes[27].any()
    vals = set(np.unique(model("order")[1][2]))
    assert {127, 128, 255, 0} <= vals


# ---- the device side ----

@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


class Guarded:
    """`need` bytes of device memory between two guards, everything pre-filled with 0xA5"""

    def __init__(self, need, offset=0):
        import torch
        self.size = GUARD + offset + need + GUARD
        self.t = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.start = GUARD + offset
        self.ptr = self.t.data_ptr() + self.start
        assert self.t.data_ptr() % 256 == 0
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def to_c(capi, regions):
    """(hm_region array, void* array, what keeps the data alive)"""
    n = len(regions)
    arr, data, keep = (capi.Region * max(n, 1))(), (C.c_void_p * max(n, 1))(), []
    for i, r in enumerate(regions):
        g = arr[i]
        g.type = TYPES[r[0]]
        if r[0] in ("polygon", "polyline"):
            p = np.ascontiguousarray(np.array(r[1], dtype=np.int32).reshape(-1, 2))
            g.n_points = p.shape[0]
            keep.append(p)
            data[i] = p.ctypes.data if p.size else None
        else:
            g.x, g.y = r[1], r[2]
            if r[0] != "point":
                g.w, g.h = r[3], r[4]
            if r[0] == "inline_mask":
                b = C.create_string_buffer(bytes(r[5]), len(r[5]))
                keep.append(b)
                data[i], g.mask_bytes = C.addressof(b), len(r[5])
            if r[0] == "referenced_mask":
                m = np.ascontiguousarray(r[5], dtype=np.uint8)
                keep.append(m)
                data[i], g.mask_bytes = m.ctypes.data, m.size
    return arr, data, keep


def elements(values, dtype, scale, bias):
    if dtype == U8:
        return values.astype(np.uint8)
    r = values.astype(np.float32) * np.float32(scale) + np.float32(bias)
    assert r.dtype == np.float32
    return r.astype(NP[dtype])


def run(capi, L, regions, mode, images, dtype=U8, view=None, pad=0, offset=0, scale=1.0, bias=0.0, expect=0):
    """rasterise into a guarded buffer and compare the whole buffer with `images` (P x h x w elements; expect != 0: the status, and
    the buffer untouched)"""
    planes, h, w = images.shape
    es = ELEM[dtype]
    row = w * es + pad * es
    plane = row * h + (3 * row if pad else 0)
    need = plane * (planes - 1) + row * (h - 1) + w * es if planes else 0
    buf = Guarded(max(need, 1), offset)
    d = capi.RegionsDest(buf.ptr, need, dtype, 0, row if pad else 0, plane if pad else 0, scale, bias)
    n = len(regions)
    if expect == 0:
        assert L.hm_regions_dest_bytes(mode, n, w, h, C.byref(d)) == need, L.hm_last_error().decode()
    arr, data, keep = to_c(capi, regions)
    rc = L.hm_rasterise_regions(arr, data, n, CANVAS[0], CANVAS[1], C.byref(view) if view is not None else None, mode, C.byref(d), None)
    msg = L.hm_last_error().decode()
    got = buf.host()
    exp = np.full(buf.size, 0xA5, np.uint8)
    if expect == 0:
        assert rc == 0, msg
        for p in range(planes):
            for y in range(h):
                at = buf.start + p * plane + y * row
                exp[at:at + w * es] = np.ascontiguousarray(images[p, y]).view(np.uint8)
    else:
        assert rc == expect and msg, (rc, msg)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        at = int(bad[0]) - buf.start
        raise AssertionError(f"{bad.size} bytes differ, first at {at} from the start (plane {at // max(plane, 1)}, row {at % max(plane, 1) // row}, "
                             f"byte {at % max(plane, 1) % row}): got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x}")
    return msg


def make_view(capi, crop, size, filt):
    v = capi.DeviceView()
    if crop:
        v.crop_x, v.crop_y, v.crop_w, v.crop_h = crop
    if size:
        v.out_w, v.out_h = size
    v.filter = filt
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("pad,offset", [(0, 0), (0, 1), (13, 0), (13, 1), (29, 16)])
def test_stack_u8_every_geometry(capi, L, pad, offset):
    regions, planes, _ = model("geometry")
    run(capi, L, regions, STACK, planes, U8, None, pad, offset)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["geometry", "order"])
@pytest.mark.parametrize("pad,offset", [(0, 0), (5, 1)])
def test_labels(capi, L, name, pad, offset):
    regions, planes, _ = model(name)
    lab = ref.labels(planes)
    if name == "order":  # 127 does not label, 128 does; the last region wins
        assert lab[15, 25] == 2 and lab[15, 35] == 3 and lab[15, 45] == 4 and lab[12, 22] == 2 and lab[22, 45] == 6 and lab[20, 42] == 5 and lab[0, 0] == 1
    run(capi, L, regions, LABELS, lab[None], U8, None, pad, offset)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,pad,offset", [(F16, 0, 0), (F16, 3, 2), (F32, 0, 0), (F32, 5, 4), (F32, 0, 16)])
def test_stack_float_dtypes(capi, L, dtype, pad, offset):
    regions, planes, _ = model("order")
    scale, bias = 1.0 / 255.0, -0.4375
    run(capi, L, regions, STACK, elements(planes, dtype, scale, bias), dtype, None, pad, offset, scale, bias)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [STACK, LABELS])
def test_crop_with_an_odd_origin(capi, L, mode):
    regions, planes, _ = model("geometry")
    x, y, w, h = 3, 5, 41, 29
    cut = planes[:, y:y + h, x:x + w]
    view = make_view(capi, (x, y, w, h), None, pv.TRIANGLE)
    run(capi, L, regions, mode, cut if mode == STACK else ref.labels(cut)[None], U8, view, 7, 1)
    # the same crop with its own size stated is the crop
    view = make_view(capi, (x, y, w, h), (w, h), pv.NEAREST)
    run(capi, L, regions, mode, cut if mode == STACK else ref.labels(cut)[None], U8, view)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [pv.TRIANGLE, pv.NEAREST])
@pytest.mark.parametrize("dtype", [U8, F32])
def test_stack_crop_resized(capi, L, filt, dtype):
    """the model's planes through tests/planes_view_ref.py as monochrome 8-bit planes, compared as the planar-view tests compare: equal"""
    regions, planes, _ = model("order")
    crop, size = (3, 5, 41, 29), (23, 37)
    scale, bias = (1.0 / 255.0, 0.125) if dtype != U8 else (1.0, 0.0)
    exp = []
    for p in planes:
        r = pv.plane_view(np.asarray(p), crop, size, filt, False)
        exp.append(pv.store(r, 0, dtype, [scale] * 4, [bias] * 4, 8, 0, filt == pv.NEAREST))
    run(capi, L, regions, STACK, np.stack(exp), dtype, make_view(capi, crop, size, filt), 3, 0, scale, bias)


@pytest.mark.gpu
def test_labels_resized(capi, L):
    """HM_VIEW_NEAREST moves labels under the view's index rule; any other filter is refused with the destination unwritten"""
    regions, planes, _ = model("order")
    crop, size = (3, 5, 41, 29), (23, 37)
    lab = ref.labels(planes)
    exp = pv.store(pv.plane_view(lab, crop, size, pv.NEAREST, False), 0, U8, [1.0] * 4, [0.0] * 4, 8, 0, True)
    run(capi, L, regions, LABELS, exp[None], U8, make_view(capi, crop, size, pv.NEAREST), 2, 1)
    msg = run(capi, L, regions, LABELS, exp[None], U8, make_view(capi, crop, size, pv.TRIANGLE), expect=-1)
    assert "HM_VIEW_NEAREST" in msg


@pytest.mark.gpu
def test_refusals_leave_the_destination_unwritten(capi, L):
    regions, planes, _ = model("order")
    run(capi, L, regions, STACK, planes, U8, make_view(capi, (60, 40, 10, 10), None, 0), expect=-1)      # a crop outside the canvas
    run(capi, L, [("ellipse", 0, 0, 32768, 1)] + list(regions), STACK, np.zeros((7, 45, 67), np.uint8), U8, None, expect=-2)
    run(capi, L, [("rectangle", 0, 0, 1, 1)] * 256, LABELS, np.zeros((1, 45, 67), np.uint8), U8, None, expect=-1)
    # a destination in host memory
    host = np.zeros(6 * 67 * 45, np.uint8)
    d = capi.RegionsDest(host.ctypes.data, host.size, U8, 0, 0, 0, 1.0, 0.0)
    arr, data, keep = to_c(capi, regions)
    assert L.hm_rasterise_regions(arr, data, len(regions), 67, 45, None, STACK, C.byref(d), None) == -1 and not host.any()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", range(8))
def test_random_polygons_and_polylines(capi, L, batch):
    """200 seeded shapes of 3 .. 12 points with coordinates in [-20, 90], 25 regions per launch, bit-exact against the model"""
    regions, planes, _ = model(f"random{batch}")
    assert len(regions) == 25
    run(capi, L, regions, STACK, planes, U8, None, 0, batch & 1)


@pytest.mark.gpu
def test_python_on_one_file(pkg):
    """read_regions and decode_regions_to_tensor: a file whose regions' reference space is the image's, and one where it differs"""
    import torch
    import synthutil
    from regionwriter import Writer
    pic = synthutil.picture(97002, width=64, height=48)
    mask = _mask(20, 10, 11)
    shapes = [("rectangle", 3, 4, 20, 9), ("polygon", [(5, 3), (60, 10), (20, 40)]), ("ellipse", 30, 20, 12, 7), ("inline_mask", -5, 3, 13, 9, _bits(13, 9, 5))]

    def file(reference):
        w = Writer()
        img = w.hvc1(pic, (64, 48))
        m = w.mski(mask.tobytes(), (20, 10))
        r1 = w.rgan(shapes + [("referenced_mask", 40, 30, 0, 0, m)], reference, annotates=[img])
        r2 = w.rgan([("point", 7, 7)], reference, annotates=[img], wide=True)
        return w.finish(primary=img), r1, r2
    data, r1, r2 = file((64, 48))
    items = pkg.read_regions(data)
    assert [it["item_id"] for it in items] == [r1, r2] and [g["type"] for g in items[0]["regions"]] == ["rectangle", "polygon", "ellipse", "inline_mask", "referenced_mask"]
    model_regions = shapes + [("referenced_mask", 40, 30, 20, 10, mask), ("point", 7, 7)]
    exp = ref.stack(model_regions, (64, 48))
    t = pkg.decode_regions_to_tensor(data)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (6, 48, 64) and np.array_equal(t.cpu().numpy(), exp)
    lab = pkg.decode_regions_to_tensor(data, mode="labels", region_items=[r1])
    assert tuple(lab.shape) == (48, 64) and np.array_equal(lab.cpu().numpy(), ref.labels(exp[:5]))
    out = torch.full((6, 20, 40), 7.0, dtype=torch.float32, device="cuda")[:, :, :31]
    got = pkg.decode_regions_to_tensor(data, crop=(1, 3, 31, 20), out=out, scale=1 / 255, bias=0.5)
    assert got is out and np.array_equal(out.cpu().numpy(), elements(exp[:, 3:23, 1:32], F32, 1 / 255, 0.5))
    rgb = pkg.decode_to_tensor(data, dtype=torch.uint8)
    assert tuple(rgb.shape)[1:] == tuple(t.shape)[1:]  # the planes line up with the image
    # a reference space of twice the image's size: the default size is the image's
    data2, _, _ = file((128, 96))
    t2 = pkg.decode_regions_to_tensor(data2, dtype=torch.float32)
    assert tuple(t2.shape) == (6, 48, 64)
    big = ref.stack(model_regions, (128, 96))
    e2 = np.stack([pv.store(pv.plane_view(p, (0, 0, 128, 96), (64, 48), pv.TRIANGLE, False), 0, F32, [1.0] * 4, [0.0] * 4, 8, 0, False) for p in big])
    assert np.array_equal(t2.cpu().numpy(), e2)
    with pytest.raises(ValueError, match="reference space"):
        pkg.decode_regions_to_tensor(data2, crop=(0, 0, 10, 10))
    with pytest.raises(pkg.HmError):
        pkg.decode_regions_to_tensor(data2, mode="labels")  # (the default size resamples: labels take filter="nearest" only)
    lab2 = pkg.decode_regions_to_tensor(data2, mode="labels", filter="nearest")
    assert tuple(lab2.shape) == (48, 64)
