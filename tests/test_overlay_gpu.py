"""GPU: derived image items - 'iovl' overlays composed by k_overlay, and 'iden'.

Every overlay is compared byte for byte with tests/overlay_ref.py: the planes of each child are what hm_decode_item hands out for
that child's own item (out_format 0 - the rest of the suite holds those to the reference decoder), converted with
planar_ref.op_ycbcr_to_rgb under the profile Op_YCbCr_to_RGB<uint8_t> sees (a grid canvas carries none), and composed - through the
literal transcription of HeifPixelImage::overlay where the placement lies inside DESIGN Q20's domain, through the clipping composer
elsewhere.  An hvc1 child the reference has no chain for (Q19) takes its planes from the 1 x 1 grid over the same picture.
'iden' results are compared with the child decoded under the concatenated transformation list."""
import ctypes as C

import numpy as np
import pytest

import overlay_ref
import pipeline
import synthutil
import view_ref
from overlaywriter import Writer

pytestmark = pytest.mark.gpu
RGB, RGBA = 10, 11
BKG = (0x20FF, 0x8000, 0xE0AB, 0x1234)
CANVASES = [(96, 80), (70, 53), (300, 5)]


def pic(seed, w, h, **kw):
    return synthutil.picture(seed, width=w, height=h, **kw)


@pytest.fixture(scope="module")
def P():
    """coded pictures, synthesised once"""
    d = dict(a444=pic(92001, 48, 40, chroma_format=3), b420=pic(92002, 64, 64), c444=pic(92003, 24, 24, chroma_format=3),
             tiles=[pic(92010 + i, 24, 24) for i in range(4)], mono=pic(92020, 24, 24, chroma_format=0),
             alpha48=pic(92030, 48, 40, chroma_format=0, level_span=1000, density=100, qp=40), alpha24=pic(92031, 24, 24, chroma_format=0, level_span=1000, density=100, qp=40),
             alpha64=pic(92032, 64, 64, chroma_format=0, level_span=1000, density=100, qp=40))
    return d


def rows_of(planes, meta, bpp):
    w, h = meta["width"], meta["height"]
    return planes[0][:h, :w * bpp].reshape(h, w, bpp)


class Scene:
    """one file: items are added through .w (overlaywriter.Writer); a spec tree says how the reference composes them:
       ("item", id, planes_from_id)            a coded child; planes_from_id: the 1 x 1 grid standing in for a Q19 child (else None)
       ("iovl", canvas, [(spec, dx, dy)], transforms)"""

    def __init__(self):
        self.w = Writer()
        self.cache = {}

    def open(self, hm, primary):
        self.data = self.w.finish(primary=primary)
        self.f = pipeline.HeifFile(hm, self.data)
        return self

    def child(self, spec):
        """([R, G, B], alpha or None) of a coded child - computed once per file and shared, never modified"""
        if spec not in self.cache:
            self.cache[spec] = self._child(spec)
        return self.cache[spec]

    def _child(self, spec):
        _, iid, planes_from = spec
        planes, meta = self.f.decode(planes_from or iid, 0, threads=2)
        assert meta["bit_depth"] == 8
        cut = [p[:meta["plane_size"][c][1], :meta["plane_size"][c][0]] for c, p in enumerate(planes)]
        rgb = overlay_ref.layer_rgb(cut, meta["chroma"], (meta["has_nclx"], meta["matrix"], meta["primaries"], meta["full_range"]))
        alpha = None
        if planes_from:
            _, ameta = self.f.decode(iid, 0, threads=2)
        else:
            ameta = meta
        if ameta["has_alpha"]:
            alpha = ameta["alpha"][:meta["height"], :meta["width"]]
        return rgb, alpha

    def reference(self, spec):
        """-> ([R, G, B], alpha or None, every placement inside the Q20 domain)"""
        if spec[0] == "item":
            rgb, alpha = self.child(spec)
            return rgb, alpha, True
        _, canvas, layers, transforms = spec
        done, inside = [], True
        for sub, dx, dy in layers:
            rgb, alpha, ok = self.reference(sub)
            inside = inside and ok
            done.append((rgb, alpha, dx, dy))
        r, g, b, ok = overlay_ref.compose(canvas, BKG, done)
        out = [r, g, b]
        for kind, v in transforms or []:
            if kind == "irot":
                out = [np.rot90(p, v) for p in out]  # counter-clockwise quarter turns
            elif kind == "clap":  # (integer apertures only: left = (W - w) / 2 + hoff, context.cc:1986-2003)
                wn, wd, hn, hd, hon, hod, von, vod = v
                assert wd == hd == hod == vod == 1
                H, W = out[0].shape
                assert (W - wn) % 2 == 0 and (H - hn) % 2 == 0
                left, top = (W - wn) // 2 + hon, (H - hn) // 2 + von
                out = [p[top:top + hn, left:left + wn] for p in out]
            else:
                raise ValueError(kind)
        return out, None, inside and ok

    def expect(self, spec, fmt):
        rgb, _, inside = self.reference(spec)
        return overlay_ref.interleave(*rgb, fmt == RGBA), inside

    def decoded(self, iid, fmt):
        planes, meta = self.f.decode(iid, fmt, threads=3)
        return rows_of(planes, meta, 4 if fmt == RGBA else 3), meta

    def close(self):
        self.f.close()


def check(scene, iid, spec, fmts=(RGB, RGBA)):
    inside = None
    for fmt in fmts:
        exp, inside = scene.expect(spec, fmt)
        got, meta = scene.decoded(iid, fmt)
        assert got.shape == exp.shape, (got.shape, exp.shape)
        assert np.array_equal(got, exp), f"fmt {fmt}: {np.argwhere(got != exp)[:5].tolist()}"
        assert (meta["chroma"], meta["bit_depth"], meta["has_alpha"], meta["has_nclx"]) == (3, 8, 0, 1)
        assert (meta["primaries"], meta["transfer"], meta["matrix"], meta["full_range"]) == (1, 13, 6, 1)  # the sRGB defaults
    return inside


def add_opaque(s, P):
    return ("item", s.w.hvc1(P["a444"], (48, 40), chroma_format=3), None)


def add_alpha_layer(s, P, size_of_alpha=24):
    c = s.w.hvc1(P["c444"], (24, 24), chroma_format=3)
    s.w.alpha(P["alpha24"] if size_of_alpha == 24 else P["alpha48"], (size_of_alpha, size_of_alpha if size_of_alpha == 24 else 40), c)
    return ("item", c, None)


def add_grid(s, P, **kw):
    tiles = [s.w.hvc1(t, (24, 24)) for t in P["tiles"]]
    return ("item", s.w.grid(tiles, 2, 2, 48, 40, **kw), None)


@pytest.mark.parametrize("canvas", CANVASES)
def test_placements_of_one_opaque_layer(hm, pkg, P, canvas):
    """no layer; inside; overhanging each border; dx < 0 and dy < 0 with and without reaching the far edge; wholly outside on each
    side (not decoded); a left edge inside a lane's group of four pixels and in the middle of a span"""
    cw, ch = canvas
    W, H = 48, 40
    places = [(0, 0), (5, 7), (cw - W + 9, 3), (3, ch - H + 6), (-9, 2), (-(W - 3), 0), (2, -11), (0, -(H - 2)), (-5, -6), (cw - 1, ch - 1),
              (-W, 0), (cw, 0), (0, -H), (0, ch), (-(1 << 31), 5), ((1 << 31) - 1, (1 << 31) - 1),
              (1, 0), (2, 1), (3, 2), (cw // 2 + 1, 0)] + ([(130, -2), (255, 0), (257, 1), (253, -30)] if cw > 256 else [])
    s = Scene()
    child = add_opaque(s, P)
    ids = [s.w.iovl([], canvas, BKG, wide=True)] + [s.w.iovl([(child[1], dx, dy)], canvas, BKG, wide=True) for dx, dy in places]
    s.open(hm, ids[0])
    try:
        assert check(s, ids[0], ("iovl", canvas, [], None)) is True
        prm = pkg.capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
        f2 = C.c_void_p()
        L = pkg.capi.image_lib()
        assert L.hm_file_open(s.data, len(s.data), C.byref(f2)) == 0
        n_inside = n_outside = 0
        for iid, (dx, dy) in zip(ids[1:], places):
            inside = check(s, iid, ("iovl", canvas, [(child, dx, dy)], None))
            touches = dx < cw and dy < ch and dx + W > 0 and dy + H > 0
            assert pkg.capi.plan_overlay(f2, iid, prm) == [touches], (dx, dy)
            assert inside == overlay_ref.reference_defined(cw, ch, W, H, dx, dy, False)
            n_inside += inside
            n_outside += not inside
        L.hm_file_close(f2)
        assert n_inside >= 8 and n_outside >= 3  # both sides of Q20 were exercised
    finally:
        s.close()


@pytest.mark.parametrize("canvas", CANVASES)
def test_alpha_layers_over_background_and_over_layers(hm, P, canvas):
    cw, ch = canvas
    s = Scene()
    base, grid = add_opaque(s, P), add_grid(s, P)
    a24, a_scaled = add_alpha_layer(s, P), add_alpha_layer(s, P, 48)  # (an alpha image of another size: scaled nearest neighbour)
    big = ("item", s.w.hvc1(P["b420"], (64, 64)), None)
    big_grid = s.w.grid([big[1]], 1, 1, 64, 64)
    s.w.alpha(P["alpha64"], (64, 64), big[1])
    big = ("item", big[1], big_grid)
    over_bkg = s.w.iovl([(a24[1], 3, 1)], canvas, BKG)
    layers = [(base, 1, -3), (a24, 7, 2), (grid, cw - 30, 0), (a_scaled, cw - 40, ch - 5), (big, 10, -20), (a24, -5, 1), (a24, 30, -8)]
    stack = s.w.iovl([(c[1], dx, dy) for c, dx, dy in layers], canvas, BKG)
    s.open(hm, stack)
    try:
        for name, spec in (("a24", a24), ("a64", big)):  # the blend is exercised at both ends and in the middle of the alpha range
            alpha = s.child(spec)[1]
            assert alpha is not None and {0, 255} <= set(np.unique(alpha).tolist()), name
        present = set(np.unique(np.concatenate([s.child(a24)[1].ravel(), s.child(big)[1].ravel(), s.child(a_scaled)[1].ravel()])).tolist())
        assert {0, 1, 127, 128, 254, 255} <= present, sorted({0, 1, 127, 128, 254, 255} - present)
        assert check(s, over_bkg, ("iovl", canvas, [(a24, 3, 1)], None)) is True
        assert check(s, stack, ("iovl", canvas, layers, None)) is False  # (an alpha layer at dx < 0 is outside the Q20 domain)
    finally:
        s.close()


@pytest.mark.parametrize("chroma", [1, 2, 3, 0])
@pytest.mark.parametrize("as_grid", [False, True])
def test_children_of_every_chroma_range_and_matrix(hm, P, chroma, as_grid):
    """4:2:0 / 4:2:2 / 4:4:4 / 4:0:0 children, full and limited range, matrices 0, 1, 6, 8 and 9, as hvc1 items and as 2 x 2 grids: ten
    layers on one canvas per (chroma format, kind).  An hvc1 child that is not 4:4:4 is a Q19 child: it equals its 1 x 1 grid."""
    s = Scene()
    layers = []
    k = 0
    for matrix in (0, 1, 6, 8, 9):
        for full in (1, 0):
            seed = 93000 + 100 * chroma + 10 * matrix + full
            kw = dict(chroma_format=chroma, vui=1, matrix=matrix, full_range=full, primaries=1 if matrix != 9 else 9)
            if as_grid:
                tiles = [s.w.hvc1(pic(seed * 10 + t, 16, 16, **kw), (16, 16), chroma_format=chroma) for t in range(4)]
                spec = ("item", s.w.grid(tiles, 2, 2, 24, 24), None)
            else:
                h = s.w.hvc1(pic(seed, 24, 24, **kw), (24, 24), chroma_format=chroma)
                spec = ("item", h, s.w.grid([h], 1, 1, 24, 24) if chroma != 3 else None)
            layers.append((spec, 2 + 23 * (k % 4), 1 + 25 * (k // 4)))
            k += 1
    canvas = (96, 80)
    o = s.w.iovl([(c[1], dx, dy) for c, dx, dy in layers], canvas, BKG)
    s.open(hm, o)
    try:
        assert check(s, o, ("iovl", canvas, layers, None)) is True
    finally:
        s.close()


def test_transformed_children_transformed_and_nested_overlays(hm, P):
    s = Scene()
    turned = ("item", s.w.hvc1(P["a444"], (48, 40), chroma_format=3, transforms=[("irot", 1), ("clap", (30, 1, 40, 1, 2, 1, -3, 1))]), None)
    mirrored = ("item", s.w.hvc1(P["c444"], (24, 24), chroma_format=3, transforms=[("imir", 1), ("irot", 2)]), None)
    grid = add_grid(s, P, transforms=[("clap", (40, 1, 30, 1, 0, 1, 0, 1)), ("irot", 3)])
    a24 = add_alpha_layer(s, P)
    inner_layers = [(turned, 1, 2), (a24, 20, 10), (mirrored, 40, 30)]
    inner = s.w.iovl([(c[1], dx, dy) for c, dx, dy in inner_layers], (70, 53), BKG)
    inner_spec = ("iovl", (70, 53), inner_layers, None)
    outer_layers = [(grid, 0, 0), (inner_spec, 20, 25), (a24, 60, 60)]
    outer = s.w.iovl([(inner if c is inner_spec else c[1], dx, dy) for c, dx, dy in outer_layers], (96, 80), BKG)
    t = [("irot", 1), ("clap", (40, 1, 56, 1, 4, 1, -2, 1))]
    outer_t = s.w.iovl([(inner if c is inner_spec else c[1], dx, dy) for c, dx, dy in outer_layers], (96, 80), BKG, transforms=t, ispe=(96, 80))
    via_iden = s.w.iden([outer], (40, 56), transforms=t)
    s.open(hm, outer)
    try:
        assert check(s, inner, inner_spec) is True
        assert check(s, outer, ("iovl", (96, 80), outer_layers, None)) is True
        assert check(s, outer_t, ("iovl", (96, 80), outer_layers, t)) is True
        for fmt in (RGB, RGBA):  # an 'iden' over the overlay with the same list is the transformed overlay
            a, ma = s.decoded(outer_t, fmt)
            b, mb = s.decoded(via_iden, fmt)
            assert a.shape == (56, 40, 4 if fmt == RGBA else 3) and np.array_equal(a, b)
        # ignore_transformations: the children's and the overlay's own
        planes, meta = s.f.decode(outer_t, RGB, threads=2, ignore_transformations=1)
        assert (meta["width"], meta["height"]) == (96, 80)
    finally:
        s.close()


@pytest.mark.parametrize("canvas", [(96, 80), (300, 5)])
def test_start_layer_equals_walking_every_layer(hm, hm_hooks, P, canvas):
    """an opaque top layer covering the canvas (and one covering part of it) over alpha layers: the composition that starts at the
    span's start layer equals the one forced to start at layer 0 (test hook overlay_start = 0), and both equal the reference"""
    cw, ch = canvas
    s = Scene()
    base, a24 = add_opaque(s, P), add_alpha_layer(s, P)
    tiles = [s.w.hvc1(P["b420"], (64, 64)) for _ in range(10 if cw > 256 else 4)]
    cover = ("item", s.w.grid(tiles, 2, len(tiles) // 2, 64 * (len(tiles) // 2), 128), None)
    layers = [(a24, 3, 1), (base, 10, -5), (cover, -2, -40), (a24, 50, 2), (base, cw - 20, 1)]
    o = s.w.iovl([(c[1], dx, dy) for c, dx, dy in layers], canvas, BKG)
    s.open(hm, o)
    try:
        check(s, o, ("iovl", canvas, layers, None))
        got, _ = s.decoded(o, RGBA)
        f2 = pipeline.HeifFile(hm_hooks, s.data)
        try:
            assert hm_hooks.hm_debug_set(b"overlay_start", 0) == 0
            planes, meta = f2.decode(o, RGBA, threads=2)
            assert np.array_equal(rows_of(planes, meta, 4), got)
        finally:
            hm_hooks.hm_debug_set(b"overlay_start", 1)
            f2.close()
    finally:
        s.close()


def test_kernel_resources(hm_hooks):
    """no instance of k_overlay spills (scratch 0), as the loaded code object has it"""
    hm_hooks.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    for inst in range(3):
        out = (C.c_int * 2)()
        assert hm_hooks.hm_debug_kernel_regs(8, inst, 0, 0, C.byref(out)) == 0
        assert out[1] == 0 and 0 < out[0] <= 64, (inst, out[0], out[1])
    assert hm_hooks.hm_debug_kernel_regs(8, 3, 0, 0, C.byref((C.c_int * 2)())) == -1


@pytest.fixture(scope="module")
def stack_scene(hm, P):
    """one overlay on the ragged 70 x 53 canvas for the destination tests, with its reference"""
    s = Scene()
    base, grid, a24 = add_opaque(s, P), add_grid(s, P), add_alpha_layer(s, P)
    layers = [(grid, 30, 20), (base, -3, -4), (a24, 40, 3), (a24, 10, 35)]
    o = s.w.iovl([(c[1], dx, dy) for c, dx, dy in layers], (70, 53), BKG)
    s.open(hm, o)
    s.primary = o
    s.ref = {fmt: s.expect(("iovl", (70, 53), layers, None), fmt)[0] for fmt in (RGB, RGBA)}
    yield s
    s.close()


@pytest.mark.parametrize("fmt", [RGB, RGBA])
def test_destinations(hm, pkg, stack_scene, fmt):
    """ext_dst, HWC u8 and CHW f32 device tensors with their padding untouched, and a cropped, resized view"""
    import torch
    s, capi, L = stack_scene, pkg.capi, pkg.capi.image_lib()
    ref = s.ref[fmt]
    h, w, c = ref.shape
    f = C.c_void_p()
    assert L.hm_file_open(s.data, len(s.data), C.byref(f)) == 0
    try:
        # ext_dst (host memory of the caller, its own stride)
        stride = w * c + 11
        buf = np.full(h * stride + 5, 0xA5, np.uint8)
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, buf.ctypes.data, buf.size, stride, 0, 0)
        d = capi.Decoded()
        capi.check_image(L.hm_decode_item(f, s.primary, C.byref(prm), C.byref(d)))
        assert d.used_ext_dst == 1 and (d.width, d.height, d.stride[0]) == (w, h, stride)
        L.hm_decoded_free(C.byref(d))
        exp = np.full(h * stride + 5, 0xA5, np.uint8)
        for y in range(h):
            exp[y * stride:y * stride + w * c] = ref[y].ravel()
        assert np.array_equal(buf, exp)
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
        one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
        # HWC u8 with a row pitch of its own
        pitch = w * c + 13
        t = torch.full((h * pitch + 7,), 0xA5, dtype=torch.uint8, device="cuda")
        dest = capi.DeviceDest(t.data_ptr(), t.numel(), capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U8, pitch, 0, one, zero)
        capi.check_image(L.hm_decode_item_to_device(f, s.primary, C.byref(prm), C.byref(dest), C.byref(d)))
        exp = np.full(h * pitch + 7, 0xA5, np.uint8)
        for y in range(h):
            exp[y * pitch:y * pitch + w * c] = ref[y].ravel()
        assert np.array_equal(t.cpu().numpy(), exp)
        # CHW f32, padded rows and planes
        rp, pp = (w + 5), (w + 5) * (h + 2)
        t = torch.full((c * pp + 3,), -7.0, dtype=torch.float32, device="cuda")
        dest = capi.DeviceDest(t.data_ptr(), t.numel() * 4, capi.HM_DEV_LAYOUT_CHW, capi.HM_DEV_F32, rp * 4, pp * 4, one, zero)
        capi.check_image(L.hm_decode_item_to_device(f, s.primary, C.byref(prm), C.byref(dest), C.byref(d)))
        exp = np.full(c * pp + 3, -7.0, np.float32)
        for k in range(c):
            for y in range(h):
                exp[k * pp + y * rp:k * pp + y * rp + w] = ref[y, :, k]
        assert np.array_equal(t.cpu().numpy(), exp)
        # a cropped, resized view against view_ref on the composed reference
        crop, size = (9, 6, 50, 41), (33, 20)
        view = capi.DeviceView(*crop, *size, capi.HM_VIEW_TRIANGLE)
        pitch = size[0] * c + 5
        t = torch.full((size[1] * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
        dest = capi.DeviceDest(t.data_ptr(), t.numel(), capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U8, pitch, 0, one, zero)
        capi.check_image(L.hm_decode_item_to_device_view(f, s.primary, C.byref(prm), C.byref(view), C.byref(dest), C.byref(d)))
        assert (d.width, d.height) == size
        want = view_ref.to_integer(view_ref.resample(ref, crop, size), 255).astype(np.uint8)
        exp = np.full(size[1] * pitch, 0xA5, np.uint8)
        for y in range(size[1]):
            exp[y * pitch:y * pitch + size[0] * c] = want[y].ravel()
        assert np.array_equal(t.cpu().numpy(), exp)
        # a crop that leaves a layer out: that layer is not decoded, the view is the same rectangle of the reference
        crop = (0, 40, 30, 13)  # (only the last layer and the background)
        view = capi.DeviceView(*crop, 0, 0, capi.HM_VIEW_TRIANGLE)
        assert capi.plan_overlay(f, s.primary, prm, view) == [False, False, False, True]
        t = torch.full((crop[3] * crop[2] * c,), 0xA5, dtype=torch.uint8, device="cuda")
        dest = capi.DeviceDest(t.data_ptr(), t.numel(), capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U8, crop[2] * c, 0, one, zero)
        capi.check_image(L.hm_decode_item_to_device_view(f, s.primary, C.byref(prm), C.byref(view), C.byref(dest), C.byref(d)))
        assert np.array_equal(t.cpu().numpy().reshape(crop[3], crop[2], c), ref[40:53, 0:30])
    finally:
        L.hm_file_close(f)


def test_python_and_pipeline(hm, pkg, stack_scene):
    import torch
    s = stack_scene
    t = pkg.decode_to_tensor(s.data, layout="hwc", dtype=torch.uint8)
    assert np.array_equal(t.cpu().numpy(), s.ref[RGB])
    t = pkg.decode_to_tensor(s.data, out_format="rgba", crop=(9, 6, 50, 41), size=(33, 20), filter="nearest", layout="hwc", dtype=torch.uint8)
    assert np.array_equal(t.cpu().numpy(), view_ref.resample(s.ref[RGBA], (9, 6, 50, 41), (33, 20), view_ref.NEAREST))
    # the pipeline and batch calls take coded images and grids: a derived item is refused, naming the file
    with pytest.raises(pkg.capi.HmError, match=r"files\[0\].*derived image item") as e:
        pkg.decode_batch_to_tensor([s.data, s.data])
    assert e.value.status == -2


def test_iden_equals_the_child_with_the_concatenated_list(hm, P):
    """'iden' over hvc1 4:4:4, over hvc1 4:2:0 (Q19: its 1 x 1 grid) and over a grid, clap + irot on both items, with alpha, to RGB24 and
    RGBA32 - the grid child also to out_format 0: each equals the child carrying child ++ iden itself"""
    t1 = [("clap", (40, 1, 32, 1, 2, 1, -1, 1)), ("irot", 1)]       # on the child: 40 x 32, turned to 32 x 40
    t2 = [("irot", 2), ("clap", (20, 1, 30, 1, -3, 1, 2, 1))]       # on the 'iden' item
    s = Scene()
    cases = []
    # hvc1 4:4:4 with alpha
    a = s.w.hvc1(P["a444"], (48, 40), chroma_format=3, transforms=t1)
    s.w.alpha(P["alpha48"], (48, 40), a, transforms=t1)
    b = s.w.hvc1(P["a444"], (48, 40), chroma_format=3, transforms=t1 + t2)
    s.w.alpha(P["alpha48"], (48, 40), b, transforms=t1 + t2)
    cases.append((s.w.iden([a], (20, 30), transforms=t2), b, (RGB, RGBA)))
    # hvc1 4:2:0: the 1 x 1 grid of itself
    sq1 = [("clap", (48, 1, 40, 1, 0, 1, 0, 1)), ("irot", 1)]
    c = s.w.hvc1(P["b420"], (64, 64), transforms=sq1)
    plain = s.w.hvc1(P["b420"], (64, 64))
    g1 = s.w.grid([plain], 1, 1, 64, 64, transforms=sq1 + t2)
    cases.append((s.w.iden([c], (20, 30), transforms=t2), g1, (RGB, RGBA, 0)))
    # a 2 x 2 grid with alpha on the grid item
    tiles = [s.w.hvc1(t, (24, 24)) for t in P["tiles"]]
    t1g = [("clap", (40, 1, 32, 1, 0, 1, 0, 1)), ("irot", 1)]
    g = s.w.grid(tiles, 2, 2, 48, 40, transforms=t1g)
    s.w.alpha(P["alpha48"], (48, 40), g, transforms=t1g)
    g2 = s.w.grid(tiles, 2, 2, 48, 40, transforms=t1g + t2)
    s.w.alpha(P["alpha48"], (48, 40), g2, transforms=t1g + t2)
    cases.append((s.w.iden([g], (20, 30), transforms=t2), g2, (RGB, RGBA, 0)))
    # 'iden' over 'iden'
    cases.append((s.w.iden([s.w.iden([a], (32, 40))], (20, 30), transforms=t2), b, (RGBA,)))
    s.open(hm, cases[0][0])
    try:
        for ident, direct, fmts in cases:
            for fmt in fmts:
                pa, ma = s.f.decode(ident, fmt, threads=2)
                pb, mb = s.f.decode(direct, fmt, threads=2)
                assert (ma["width"], ma["height"]) == (20, 30) and len(pa) == len(pb)
                for k in ("width", "height", "chroma", "bit_depth", "has_alpha", "has_nclx", "matrix", "full_range", "plane_size"):
                    assert ma[k] == mb[k], (ident, fmt, k)
                for x, y, (pw, ph) in zip(pa, pb, ma["plane_size"]):
                    bpp = {RGB: 3, RGBA: 4, 0: 1}[fmt]
                    assert np.array_equal(x[:ph, :pw * bpp], y[:ph, :pw * bpp]), (ident, fmt)
                if fmt == 0 and ma["has_alpha"]:
                    assert np.array_equal(ma["alpha"][:30, :20], mb["alpha"][:30, :20])
    finally:
        s.close()


def test_facade(hm, pkg, stack_scene):
    """heif_decode_image on a derived primary item, and the fork's error code for a bad overlay payload"""
    import os
    s = stack_scene
    api = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libheif_mi355x_api.so"))

    class Err(C.Structure):
        _fields_ = [("code", C.c_int), ("subcode", C.c_int), ("message", C.c_char_p)]
    api.heif_context_alloc.restype = C.c_void_p
    api.heif_context_free.argtypes = [C.c_void_p]
    api.heif_context_read_from_memory.restype = Err
    api.heif_context_read_from_memory.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
    api.heif_context_get_primary_image_handle.restype = Err
    api.heif_context_get_primary_image_handle.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    api.heif_image_handle_release.argtypes = [C.c_void_p]
    api.heif_image_handle_get_width.argtypes = [C.c_void_p]
    api.heif_image_handle_get_height.argtypes = [C.c_void_p]
    api.heif_image_handle_has_alpha_channel.argtypes = [C.c_void_p]
    api.heif_decode_image.restype = Err
    api.heif_decode_image.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    api.heif_image_get_plane_readonly.restype = C.POINTER(C.c_uint8)
    api.heif_image_get_plane_readonly.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    api.heif_image_release.argtypes = [C.c_void_p]

    def run(data, chroma):
        ctx = api.heif_context_alloc()
        try:
            e = api.heif_context_read_from_memory(ctx, data, len(data), None)
            assert e.code == 0, e.message
            h = C.c_void_p()
            e = api.heif_context_get_primary_image_handle(ctx, C.byref(h))
            if e.code:
                return e.code, e.subcode, None
            size = (api.heif_image_handle_get_width(h), api.heif_image_handle_get_height(h), api.heif_image_handle_has_alpha_channel(h))
            img = C.c_void_p()
            e = api.heif_decode_image(h, C.byref(img), 1, chroma, None)  # heif_colorspace_RGB
            out = None
            if e.code == 0:
                stride = C.c_int()
                p = api.heif_image_get_plane_readonly(img, 10, C.byref(stride))  # heif_channel_interleaved
                bpp = 4 if chroma == RGBA else 3
                out = np.ctypeslib.as_array(p, shape=(size[1], stride.value))[:, :size[0] * bpp].reshape(size[1], size[0], bpp).copy()
                api.heif_image_release(img)
            api.heif_image_handle_release(h)
            return e.code, e.subcode, (size, out)
        finally:
            api.heif_context_free(ctx)

    for fmt in (RGB, RGBA):
        code, sub, (size, out) = run(s.data, fmt)
        assert code == 0 and size == (70, 53, 0)
        assert np.array_equal(out, s.ref[fmt])
    w = Writer()
    kid = w.hvc1(pic(92001, 48, 40, chroma_format=3), (48, 40), chroma_format=3)
    bad = w.iovl([], (70, 53), payload=bytes([0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 70]), refs=[kid])
    code, sub, _ = run(w.finish(primary=bad), RGB)
    assert (code, sub) == (2, 121)    # heif_error_Invalid_input, heif_suberror_Invalid_overlay_data
    w = Writer()
    kid = w.hvc1(pic(92001, 48, 40, chroma_format=3), (48, 40), chroma_format=3)
    bad = w.iovl([], (70, 53), payload=bytes([1, 0]) + bytes(20), refs=[kid])
    code, sub, _ = run(w.finish(primary=bad), RGB)
    assert (code, sub) == (4, 3002)   # heif_error_Unsupported_feature, heif_suberror_Unsupported_data_version
