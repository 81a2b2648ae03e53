"""GPU: many views of one picture (hm_decode_item_to_device_views, hm_resample_views_to_tensor, decode_to_views).  Everything is
bit-exact, three ways: every view of the one call equals the single-view call on that view (hm_resample_to_tensor,
hm_decode_item_to_device_view), equals the numpy restatement (tests/view_filters_ref.py) of the source pixels, and the multi launch
(one launch per pass for all views of a group) equals itself cut into chunks and the per-view path (test hook view_multi = 0).  Every
destination sits in a guarded buffer pre-filled with 0xA5 and the WHOLE buffer is compared."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import test_device_out_gpu as base
import test_device_view_gpu as dv
import test_sequence_view_gpu as sv
import view_filters_ref as vf

pytestmark = pytest.mark.gpu
images = dv.images  # (the module fixture of test_device_view_gpu: single, grid, ten_bit, alpha_aux, clap_irot with their host decodes)
RGB, RGBA, RRGGBB_LE = base.RGB, base.RGBA, base.RRGGBB_LE
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = vf.TRIANGLE, vf.NEAREST, vf.CUBIC, vf.LANCZOS3
ONE, ZERO = [1.0] * 4, [0.0] * 4
W, H = 190, 130
# (crop, size, nearest?) on a 190 x 130 source: a reduction from an odd origin; an enlargement of the whole image (wider than 128
# columns); tight CHW float32 rows of 308 bytes, no multiple of 16 (the element-store instance); a 1 x 1 output; a crop one row high (both
# narrower than 64 columns); the crop alone; a nearest view.  Views of different widths share a launch: workgroups beyond their own
# view's width return early.
VIEWS = [((3, 5, 181, 121), (97, 50), False), (None, (224, 224), False), ((10, 8, 30, 30), (77, 77), False), ((20, 20, 40, 30), (1, 1), False),
         ((5, 60, 100, 1), (50, 3), False), ((10, 8, 30, 30), None, False), (None, (77, 101), True)]
RESAMPLED = [k for k, (_, size, near) in enumerate(VIEWS) if size and not near]
# name -> (out_format, layout, dtype, float destination): the destination classes of test_sequence_view_gpu
CLASSES = {name: c[1:] for name, c in sv.CLASSES.items()}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture()
def hooks(pkg, capi):
    """libheif_mi355x_test.so with the image entry points bound; the view knobs are put back behind the test"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(capi.TEST_LIB_PATH)
    T.hm_last_error.restype = C.c_char_p
    T.hm_debug_set.argtypes = [C.c_char_p, C.c_int]
    capi.bind_image(T)
    try:
        yield T
    finally:
        for knob, v in ((b"view_multi", 1), (b"view_batch_bytes", 0), (b"view_stage_px", 0)):
            assert T.hm_debug_set(knob, v) == 0


@pytest.fixture(scope="module")
def sources():
    """out_format -> (the samples h x w x c, the device tensor they lie in, bytes between its rows): random pixels, 8-bit RGB and RGBA,
    10 bits in 16 for RRGGBB_LE"""
    import torch
    out = {}
    for fmt in (RGB, RGBA, RRGGBB_LE):
        rng = np.random.default_rng(7700 + fmt)
        c = 4 if fmt == RGBA else 3
        if fmt == RRGGBB_LE:
            pixels = rng.integers(0, 1024, (H, W, c), dtype=np.uint16)
        else:
            pixels = rng.integers(0, 256, (H, W, c), dtype=np.uint8)
        stride = (W * c * pixels.itemsize + 63) // 64 * 64 + 64
        rows = np.zeros((H, stride), np.uint8)
        rows[:, :W * c * pixels.itemsize] = pixels.view(np.uint8).reshape(H, -1)
        out[fmt] = (pixels, torch.from_numpy(rows).cuda(), stride)
    return out


@pytest.fixture(scope="module")
def refs(sources):
    """(out_format, view index, filter) -> the restatement's float32 sums (or moved samples); computed once"""
    cache = {}

    def get(fmt, k, filt):
        crop, size, near = VIEWS[k]
        key = (fmt, k, NEAREST if near or size is None else filt)
        if key not in cache:
            cache[key] = vf.resample(sources[fmt][0], crop, size, key[2])
        return cache[key]
    return get


def view_array(capi, filt, specs=VIEWS):
    v = (capi.DeviceView * len(specs))()
    for k, (crop, size, near) in enumerate(specs):
        v[k] = dv.make_view(capi, crop, size, NEAREST if near else filt)
    return v


def dest_set(capi, lib, specs, classes):
    """a tight destination per view, each in a guarded buffer of its own: (hm_device_dest[], [(guard, row, plane)])"""
    made = []
    for (crop, size, _), (fmt, layout, dtype, is_float) in zip(specs, classes):
        ow, oh = size if size else crop[2:]
        scale, bias = sv.scale_bias(fmt, is_float)
        made.append(base.make_dest(capi, lib, fmt, layout, dtype, ow, oh, scale, bias, 0, 0))
    return (capi.DeviceDest * len(made))(*[m[0] for m in made]), [m[1:] for m in made]


def multi(lib, fmt, src, views, dests, n):
    import torch
    rc = lib.hm_resample_views_to_tensor(fmt, W, H, src[1].data_ptr(), src[2], views, dests, n, None)
    assert rc == 0, lib.hm_last_error().decode()
    torch.cuda.synchronize()


def single(lib, fmt, src, views, dests, n):
    import torch
    for k in range(n):
        rc = lib.hm_resample_to_tensor(fmt, W, H, src[1].data_ptr(), src[2], C.byref(views[k]), C.byref(dests[k]), None)
        assert rc == 0, lib.hm_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("filt", [TRIANGLE, CUBIC, LANCZOS3], ids=["triangle", "bicubic", "lanczos3"])
def test_one_call_equals_per_view_calls_and_the_restatement(capi, hooks, sources, refs, filt, cls):
    fmt, layout, dtype, is_float = CLASSES[cls]
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    scale, bias = sv.scale_bias(fmt, is_float)
    if filt != TRIANGLE:  # the staged horizontal pass, several staged chunks on these short rows
        assert hooks.hm_debug_set(b"view_stage_px", 40) == 0
    views = view_array(capi, filt)
    n = len(VIEWS)
    d1, m1 = dest_set(capi, hooks, VIEWS, [CLASSES[cls]] * n)
    d2, m2 = dest_set(capi, hooks, VIEWS, [CLASSES[cls]] * n)
    if (layout, dtype) == (CHW, F32):
        assert m1[2][1] == 308  # (tight rows that are no multiple of 16 bytes: the group of view 2 takes the element-store instance)
    multi(hooks, fmt, sources[fmt], views, d1, n)
    single(hooks, fmt, sources[fmt], views, d2, n)
    for k, (crop, size, near) in enumerate(VIEWS):
        what = f"{cls} filter {filt} view {k}"
        g, row, plane = m1[k]
        got = g.host()
        sv.same(got, m2[k][0].host(), what + ": against hm_resample_to_tensor")
        f = NEAREST if near else filt
        vals = sv.values(refs(fmt, k, filt), f, size is None, dtype, peak, scale, bias)
        sv.same(got, dv.place(vals, layout, dtype, row, plane, g.size, g.start), what + ": against the restatement")


@pytest.mark.parametrize("filt", [TRIANGLE, CUBIC], ids=["triangle", "bicubic"])
def test_chunks_and_the_per_view_path_give_the_same_bytes(capi, hooks, sources, filt):
    """the intermediate's bound (out_w x crop_h x C x 4 bytes per view: 140 844, 349 440, 27 720, 360, 600 for the five resampled views) at
    170 000: chunks of view 0, of view 1 alone - beyond the bound by itself - and of views 2 to 4; a view per chunk; and view_multi = 0"""
    cls = [CLASSES["rgb_chw_f32"]] * len(VIEWS)
    views = view_array(capi, filt)
    runs = {}
    for what, knobs in (("one chunk", {}), ("chunks of 1, 1, 3", {"view_batch_bytes": 170000}), ("a view per chunk", {"view_batch_bytes": 1}),
                        ("chunks of 1, 1, 3 with staged chunks of 40 pixels", {"view_batch_bytes": 170000, "view_stage_px": 40}), ("view_multi = 0", {"view_multi": 0})):
        for knob, v in {"view_multi": 1, "view_batch_bytes": 0, "view_stage_px": 0, **knobs}.items():
            assert hooks.hm_debug_set(knob.encode(), v) == 0
        d, m = dest_set(capi, hooks, VIEWS, cls)
        multi(hooks, RGB, sources[RGB], views, d, len(VIEWS))
        runs[what] = [g.host() for g, _, _ in m]
    for what, got in runs.items():
        for k in range(len(VIEWS)):
            sv.same(got[k], runs["view_multi = 0"][k], f"filter {filt} view {k}: {what}")
    assert not (runs["one chunk"][1][base.GUARD:base.GUARD + 4096] == 0xA5).all()


def test_two_groups_in_one_call(capi, L, sources):
    """the views alternate between float32 CHW and uint8 HWC destinations: two launch groups whose members interleave in the list;
    every view lands in its own destination"""
    specs = [VIEWS[k] for k in RESAMPLED] + [VIEWS[0], VIEWS[2], VIEWS[4]]
    classes = [CLASSES["rgb_chw_f32"] if k % 2 == 0 else CLASSES["rgb_hwc_u8"] for k in range(len(specs))]
    for filt in (TRIANGLE, LANCZOS3):
        views = view_array(capi, filt, specs)
        d1, m1 = dest_set(capi, L, specs, classes)
        d2, m2 = dest_set(capi, L, specs, classes)
        multi(L, RGB, sources[RGB], views, d1, len(specs))
        single(L, RGB, sources[RGB], views, d2, len(specs))
        for k in range(len(specs)):
            sv.same(m1[k][0].host(), m2[k][0].host(), f"filter {filt} view {k}")
            assert not (m1[k][0].host() == 0xA5).all()


# ---- the decode entry ----

def image_views(w, h):
    """(crop, size, nearest?) for a w x h image: reductions, an enlargement, the crop alone, a nearest view, the whole image"""
    return [((3, 5, w - 9, h - 11), (50, 37), False), ((w // 2, h // 2, 33, 21), (64, 48), False), ((7, 5, 33, 21), None, False), (None, (40, 30), False),
            ((w - 35, h - 23, 35, 23), (20, 31), True), ((1, 1, 30, 1), (17, 2), False)]


def decode_views(capi, lib, data, fmt, views, dests, n, threads=2, strict=0):
    h = C.c_void_p()
    assert lib.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, strict, 0)
        out = (capi.Decoded * n)()
        failed = C.c_int32(-7)
        rc = lib.hm_decode_item_to_device_views(h, lib.hm_file_primary_item(h), C.byref(prm), views, dests, n, None, None, None, None, out, C.byref(failed))
        msg = lib.hm_last_error().decode()
        for k in range(n):
            assert not out[k].plane[0] and not out[k].plane[1] and not out[k].plane[2] and not out[k].alpha
        return rc, msg, failed.value, out
    finally:
        lib.hm_file_close(h)


@pytest.mark.parametrize("name", ["single", "grid", "ten_bit", "alpha_aux", "clap_irot"])
def test_views_decode_equals_single_view_decodes_and_the_restatement(capi, L, images, name):
    data, fmt, threads, pixels = images[name]
    h, w, _ = pixels.shape
    peak = 65535 if base.OBPP[fmt] >= 6 else 255
    specs = image_views(w, h)
    n = len(specs)
    for filt, (layout, dtype, is_float) in ((TRIANGLE, (CHW, F32, True)), (CUBIC, (HWC, U16 if peak > 255 else U8, False))):
        cls = [(fmt, layout, dtype, is_float)] * n
        scale, bias = sv.scale_bias(fmt, is_float)
        views = view_array(capi, filt, specs)
        d1, m1 = dest_set(capi, L, specs, cls)
        d2, m2 = dest_set(capi, L, specs, cls)
        rc, msg, failed, out = decode_views(capi, L, data, fmt, views, d1, n, threads)
        assert rc == 0 and failed == -1, f"{name}: {msg}"
        for k, (crop, size, near) in enumerate(specs):
            what = f"{name} filter {filt} view {k}"
            ow, oh = size if size else crop[2:]
            g, row, plane = m1[k]
            rc1, msg1, out1 = dv.view_to_device(capi, L, data, fmt, views[k], d2[k], threads)
            assert rc1 == 0, msg1
            assert (out[k].width, out[k].height, out[k].used_ext_dst, out[k].stride[0], out[k].out_format) == (ow, oh, 1, row, fmt), what
            assert (out[k].bit_depth, out[k].has_alpha, out[k].has_nclx, out[k].transfer, out[k].warnings) == \
                (out1.bit_depth, out1.has_alpha, out1.has_nclx, out1.transfer, out1.warnings), what
            got = g.host()
            sv.same(got, m2[k][0].host(), what + ": against hm_decode_item_to_device_view")
            f = NEAREST if near else filt
            vals = sv.values(vf.resample(pixels, crop, size, NEAREST if size is None else f), f, size is None, dtype, peak, scale, bias)
            sv.same(got, dv.place(vals, layout, dtype, row, plane, g.size, g.start), what + ": against the restatement of the host decode")


def test_a_crop_set_inside_a_sub_grid_and_a_damaged_tile_outside_it(capi, L, images):
    """crops confined to tile rows 1 .. 2 and columns 0 .. 1 of the 4 x 3 grid: that sub-grid alone is decoded, and the bytes are the
    views of the full decode; a damaged tile outside it is not looked at, one inside it fails the call with nothing written"""
    import torch
    data, fmt, threads, pixels = images["grid"]
    specs = [((50, 100, 40, 50), (20, 30), False), ((70, 70, 30, 40), (33, 21), False), ((5, 130, 100, 60), None, False), ((66, 66, 60, 120), (16, 40), True)]
    n = len(specs)
    views = view_array(capi, TRIANGLE, specs)
    cls = [(fmt, CHW, U8, False)] * n
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
    t = (C.c_int32 * 4)()
    assert L.hm_plan_views(fh, L.hm_file_primary_item(fh), C.byref(prm), views, n, C.byref(t)) == 0 and tuple(t) == (1, 2, 0, 2)
    L.hm_file_close(fh)

    def expected(m):
        exp = []
        for (crop, size, near), (g, row, plane) in zip(specs, m):
            f = NEAREST if near or size is None else TRIANGLE
            vals = sv.values(vf.resample(pixels, crop, size, f), f, size is None, U8, 255, ONE, ZERO)
            exp.append(dv.place(vals, CHW, U8, row, plane, g.size, g.start))
        return exp
    tiles = dv._grid_tiles()

    def damaged(k):
        t = list(tiles)
        t[k] = dv._cut_short(t[k])
        return heifwriter.write_heic(t, (64, 64), grid=dv.GRID)
    for what, file, strict in (("the intact file", data, 1), ("tile 11 damaged", damaged(11), 1), ("tile 2 damaged", damaged(2), 0)):
        d, m = dest_set(capi, L, specs, cls)
        rc, msg, failed, out = decode_views(capi, L, file, fmt, views, d, n, threads, strict=strict)
        assert rc == 0 and failed == -1 and out[0].warnings == 0, f"{what}: {msg}"
        for k, exp in enumerate(expected(m)):
            sv.same(m[k][0].host(), exp, f"{what}: view {k}")
    d, m = dest_set(capi, L, specs, cls)
    rc, msg, failed, out = decode_views(capi, L, damaged(4), fmt, views, d, n, threads, strict=1)
    assert rc < 0 and "tile" in msg and all(out[k].width == 0 for k in range(n)), (rc, msg)
    torch.cuda.synchronize()
    for g, _, _ in m:
        assert (g.host() == 0xA5).all()


def test_a_refused_call_leaves_every_destination_as_it_was(capi, L, images):
    import torch
    data, fmt, threads, pixels = images["single"]
    h, w, _ = pixels.shape
    specs = image_views(w, h)
    n = len(specs)
    cls = [(fmt, CHW, F32, True)] * n

    def refused(views, d, m, word, want_failed):
        rc, msg, failed, out = decode_views(capi, L, data, fmt, views, d, n, threads)
        assert rc == -1 and word in msg and failed == want_failed, (rc, msg, failed)
        torch.cuda.synchronize()
        for g, _, _ in m:
            assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to a destination"
    # a bad crop in the last view
    bad = list(specs)
    bad[n - 1] = ((w - 10, 1, 30, 1), (17, 2), False)
    d, m = dest_set(capi, L, specs, cls)
    refused(view_array(capi, TRIANGLE, bad), d, m, "not inside", n - 1)
    # two destinations that overlap: view 3 is to be written into the middle of view 0's
    d, m = dest_set(capi, L, specs, cls)
    d[3].ptr, d[3].len = d[0].ptr + 64, d[0].len - 64
    refused(view_array(capi, TRIANGLE, specs), d, m, "views 0 and 3 overlap", -1)
    # a destination one byte short
    d, m = dest_set(capi, L, specs, cls)
    d[1].len -= 1
    refused(view_array(capi, TRIANGLE, specs), d, m, "len", 1)
    # ... and the library still decodes after all of that
    d, m = dest_set(capi, L, specs, cls)
    rc, msg, failed, _ = decode_views(capi, L, data, fmt, view_array(capi, TRIANGLE, specs), d, n, threads)
    assert rc == 0 and failed == -1, msg
    assert not (m[0][0].host() == 0xA5).all()


def test_the_per_view_path_under_a_light_step_and_an_alpha_matte(pkg, images):
    """with a step every view is written on its own from the one decoded image: equal to the single-view calls with that step"""
    import torch
    data = images["single"][0]
    specs = [((3, 5, 181, 121), (50, 37)), (None, (64, 48)), ((7, 5, 33, 21), None), ((100, 60, 35, 23), (20, 31), "nearest")]
    for kw in (dict(light=True), dict(light=dict(to_transfer="srgb", to_primaries="bt709"), dtype=torch.float16), dict(filter="bicubic", light=True)):
        got = pkg.decode_to_views(data, specs, **kw)
        for k, spec in enumerate(specs):
            one = pkg.decode_to_tensor(data, crop=spec[0], size=spec[1], **{**kw, **({"filter": spec[2]} if len(spec) == 3 else {})})
            assert got[k].dtype == one.dtype and torch.equal(got[k].view(torch.uint8), one.view(torch.uint8)), (kw, k)
    cut = images["alpha_aux"][0]  # 96 x 64 with an alpha image
    specs = [((3, 5, 81, 51), (30, 17)), (None, (48, 32)), ((7, 5, 33, 21), None)]
    for kw in (dict(alpha=dict(mode="matte", background=(10, 200, 30))), dict(alpha="premultiplied", layout="hwc"), dict(alpha=dict(mode="matte", background=(0, 0, 255)), light=True)):
        got = pkg.decode_to_views(cut, specs, out_format="rgba", **kw)
        for k, (crop, size) in enumerate(specs):
            one = pkg.decode_to_tensor(cut, out_format="rgba", crop=crop, size=size, **kw)
            assert tuple(got[k].shape) == tuple(one.shape) and torch.equal(got[k], one), (kw, k)


def test_python_decode_to_views(pkg, images):
    import torch
    data, _, _, pixels = images["grid"]
    specs = [((50, 100, 40, 50), (50, 40)), ((70, 70, 30, 40), (33, 21), "lanczos3"), (None, (96, 96)), ((7, 5, 33, 21), None), (None, None), ((5, 5, 60, 60), (20, 20), "nearest")]
    sc, bi = base.imagenet(255.0)
    got = pkg.decode_to_views(data, specs, scale=sc, bias=bi)
    assert isinstance(got, list) and len(got) == len(specs)
    for k, spec in enumerate(specs):
        one = pkg.decode_to_tensor(data, crop=spec[0], size=spec[1], filter=spec[2] if len(spec) == 3 else "triangle", scale=sc, bias=bi)
        assert got[k].is_cuda and got[k].dtype == torch.float32 and tuple(got[k].shape) == tuple(one.shape) and torch.equal(got[k], one), k
    u8 = pkg.decode_to_views(data, [((7, 5, 33, 21), None), ((70, 70, 30, 40), (15, 20))], layout="hwc", dtype=torch.uint8)
    assert np.array_equal(u8[0].cpu().numpy(), pixels[5:26, 7:40])
    # out= as ONE K x 3 x 96 x 96 tensor, a strided slice of a larger one: the multi-crop case; what lies around the views stays as it was
    crops = [(0, 0, 100, 120), (60, 100, 96, 96), (20, 30, 150, 200), (100, 10, 40, 50)]
    big = torch.full((4, 3, 96 + 2, 96 + 9), -7.0, dtype=torch.float32, device="cuda")
    out = big[:, :, 1:97, :96]
    res = pkg.decode_to_views(data, [(c, (96, 96)) for c in crops], out=out)
    assert len(res) == 4 and all(r.data_ptr() == out[k].data_ptr() for k, r in enumerate(res))
    for k, c in enumerate(crops):
        assert torch.equal(out[k], pkg.decode_to_tensor(data, crop=c, size=(96, 96))), k
    host = big.cpu().numpy()
    assert (host[:, :, :, 96:] == -7.0).all() and (host[:, :, 0] == -7.0).all() and (host[:, :, 97] == -7.0).all()
    with pytest.raises(ValueError, match=r"out\[1\]"):
        pkg.decode_to_views(data, [(crops[0], (96, 96)), (crops[1], (64, 64))], out=out[:2])
    with pytest.raises(pkg.HmError, match="overlap"):
        pkg.decode_to_views(data, [(crops[0], (96, 96)), (crops[1], (96, 96))], out=[out[0], out[0]])


def test_crops_of_regions_to_fixed_size_crops(pkg):
    """faces -> fixed-size crops in two lines: a file whose region item holds two rectangles"""
    import synthutil
    import torch
    from regionwriter import Writer
    w = Writer()
    img = w.hvc1(synthutil.picture(97002, width=64, height=48), (64, 48))
    w.rgan([("rectangle", 3, 4, 20, 9), ("rectangle", 30, 20, 25, 27)], (64, 48), annotates=[img])
    data = w.finish(primary=img)
    crops = pkg.crops_of_regions(pkg.read_regions(data), (64, 48))
    assert crops == [(3, 4, 20, 9), (30, 20, 25, 27)]
    faces = pkg.decode_to_views(data, [(c, (16, 16)) for c in crops])
    for k, c in enumerate(crops):
        assert tuple(faces[k].shape) == (3, 16, 16) and torch.equal(faces[k], pkg.decode_to_tensor(data, crop=c, size=(16, 16))), k


def test_views_of_derived_items(pkg):
    """an 'iovl' overlay and an 'iden' over it go the plain path - decoded and composed once, whole - and the views are taken of the result"""
    import synthutil
    import torch
    from overlaywriter import Writer
    def file(through_iden):
        w = Writer()
        a = w.hvc1(synthutil.picture(97101, width=64, height=48), (64, 48))
        b = w.hvc1(synthutil.picture(97102, width=64, height=48), (64, 48))
        over = w.iovl([(a, 3, 5), (b, 40, 30)], (96, 80), (0x20FF, 0x8000, 0xE0AB, 0xFFFF))
        return w.finish(primary=w.iden([over], (96, 80), transforms=[("irot", 1)]) if through_iden else over)
    specs = [((1, 2, 70, 70), (33, 21)), ((40, 40, 30, 30), None), (None, (48, 40), "bicubic"), ((0, 0, 20, 20), (40, 40), "nearest")]
    for primary in (False, True):
        data = file(primary)
        got = pkg.decode_to_views(data, specs, dtype=torch.float32, scale=1 / 255)
        for k, spec in enumerate(specs):
            one = pkg.decode_to_tensor(data, crop=spec[0], size=spec[1], filter=spec[2] if len(spec) == 3 else "triangle", scale=1 / 255)
            assert tuple(got[k].shape) == tuple(one.shape) and torch.equal(got[k], one), (primary, k)


def test_multi_kernels_use_no_scratch(pkg):
    """every instance of the multi resampling kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 14)"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(14, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and out[0] > 0, (n, out[0], out[1])
        n += 1
    # 8 horizontal and 8 staged (sample width x channels x layout), 24 vertical (dtype x store width x row kind)
    assert n == 40
