"""Transformative item properties irot / imir / clap on the device planes: hm_decode_item vs the
CPU flow (oracle restatement of pixelimage.cc:539-888 and box.cc's clap arithmetic).  No reference vectors exist for
these (libheif cannot be built here): the oracle side is a restatement only."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import hevcutil
import orc
import pipeline
import synthutil


def _clap(w, h, cw, ch, dx2=0, dy2=0):
    """aperture cw x ch, centre offset (dx2/2, dy2/2) from the image centre"""
    return ("clap", (cw, 1, ch, 1, dx2, 2, dy2, 2))


def test_clap_rectangle_arithmetic(oracle):
    """Box_clap rounding (box.cc:3771-3804): left rounds down, top / right / bottom round to nearest."""
    rect = (C.c_int * 4)()
    def r(clap, w, h):
        assert oracle.orc_clap_rect((C.c_int64 * 8)(*clap), w, h, rect) == 0
        return list(rect)
    assert r((100, 1, 50, 1, 0, 1, 0, 1), 200, 100) == [50, 149, 25, 74]      # centred, even sizes: exact
    assert r((101, 1, 51, 1, 0, 1, 0, 1), 200, 100) == [49, 149, 25, 75]      # left 49.5 -> 49 (round down), top 24.5 -> 25 (round)
    assert r((100, 1, 50, 1, -200, 2, 0, 1), 200, 100) == [0, 49, 25, 74]     # clamped at the left border (left -50.5 -> -50 -> 0)
    assert r((64, 1, 64, 1, 0, 1, 0, 1), 64, 64) == [0, 63, 0, 63]
    assert oracle.orc_clap_rect((C.c_int64 * 8)(10, 1, 10, 1, 4000, 1, 0, 1), 64, 64, rect) == -1  # outside the image
    assert oracle.orc_clap_rect((C.c_int64 * 8)(10, 0, 10, 1, 0, 1, 0, 1), 64, 64, rect) == -2     # zero denominator


def test_plane_transforms_oracle(oracle):
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)  # w = 4, h = 3
    out = np.zeros((4, 3), np.uint8)
    oracle.orc_rotate_ccw_plane(orc.ptr(a), 4, 4, 3, 1, 90, orc.ptr(out), 3)
    assert out.tolist() == np.rot90(a, 1).tolist()
    oracle.orc_rotate_ccw_plane(orc.ptr(a), 4, 4, 3, 1, 270, orc.ptr(out), 3)
    assert out.tolist() == np.rot90(a, 3).tolist()
    o2 = np.zeros((3, 4), np.uint8)
    oracle.orc_rotate_ccw_plane(orc.ptr(a), 4, 4, 3, 1, 180, orc.ptr(o2), 4)
    assert o2.tolist() == np.rot90(a, 2).tolist()
    b = a.copy()
    oracle.orc_mirror_plane(orc.ptr(b), 4, 4, 3, 1)
    assert b.tolist() == a[:, ::-1].tolist()
    b = a.copy()
    oracle.orc_mirror_plane(orc.ptr(b), 4, 4, 3, 0)
    assert b.tolist() == a[::-1].tolist()


def test_handle_size_follows_transforms(hm):
    pic = synthutil.picture(8101, width=96, height=64)
    f = pipeline.HeifFile(hm, heifwriter.write_heic([pic], (96, 64), transforms=[_clap(96, 64, 80, 40), ("irot", 1)]))
    info = f.info(f.primary())
    f.close()
    assert (info.coded_width, info.coded_height, info.has_transforms) == (96, 64, 1)
    assert (info.width, info.height) == (40, 80)


CASES = {
    "rot90": [("irot", 1)], "rot180": [("irot", 2)], "rot270": [("irot", 3)], "rot0": [("irot", 0)],
    "mirror_h": [("imir", 1)], "mirror_v": [("imir", 0)],
    "clap_centre": [_clap(200, 136, 120, 80)], "clap_odd": [_clap(200, 136, 121, 77, 7, -5)], "clap_clamped": [_clap(200, 136, 180, 120, 60, 40)],
    "iphone_like": [("irot", 3), _clap(136, 200, 130, 190)],
    "clap_rot_mirror": [_clap(200, 136, 150, 100, -10, 6), ("irot", 1), ("imir", 1)],
    "mirror_rot_clap": [("imir", 0), ("irot", 2), _clap(200, 136, 64, 64)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("fmt", [10, 0])
def test_single_image_transforms(hm, name, fmt):
    tr = CASES[name]
    pic = synthutil.picture(8200, width=200, height=136, log2_ctb=5, qp=30, vui=1, full_range=1, matrix=6)
    f = pipeline.HeifFile(hm, heifwriter.write_heic([pic], (200, 136), transforms=tr))
    planes, meta = f.decode(f.primary(), fmt)
    f.close()
    exp, stride, canv = pipeline.cpu_decode(hm, [pic], 200, 136, 200, 136, 1, False, fmt or 10, transforms=tr)
    if fmt:
        w, h = meta["width"], meta["height"]
        assert meta["stride"][0] == stride
        np.testing.assert_array_equal(planes[0][:h, :w * 3], exp[:h, :w * 3])
    else:  # native planar output: the transformed planes themselves
        for c in range(3):
            assert planes[c].shape[1] == canv[c][1]
            pw, ph = meta["plane_size"][c]
            np.testing.assert_array_equal(planes[c][:ph, :pw], canv[c][0][:ph, :pw])


@pytest.mark.gpu
def test_grid_with_rotation_and_clap(hm):
    """the usual phone layout: a grid whose output is cropped and rotated by item properties of the grid item"""
    from corpus import TILE
    tiles = [synthutil.picture(8300 + i, **{**TILE, "width": 128, "height": 128}, vui=0) for i in range(6)]
    tr = [_clap(360, 250, 350, 240), ("irot", 3)]
    data = heifwriter.write_heic(tiles, (128, 128), grid=(2, 3, 360, 250), transforms=tr)
    f = pipeline.HeifFile(hm, data)
    info = f.info(f.primary())
    assert (info.width, info.height, info.coded_width, info.coded_height) == (240, 350, 360, 250)
    planes, meta = f.decode(f.primary(), 11, threads=2)
    f.close()
    assert (meta["width"], meta["height"]) == (240, 350)
    exp, stride, _ = pipeline.cpu_decode(hm, tiles, 128, 128, 360, 250, 3, True, 11, transforms=tr)
    np.testing.assert_array_equal(planes[0][:350, :240 * 4], exp[:350, :240 * 4])


@pytest.mark.gpu
def test_transform_limits_are_loud(hm):
    hi = synthutil.picture(8400, width=64, height=64, bit_depth=10, chroma_format=2, log2_ctb=5)
    # 10-bit planes cannot be mirrored (pixelimage.cc:748-752); 4:2:2 + quarter turn is undefined in the reference
    for tr, text in (([("imir", 1)], "mirror"), ([("irot", 1)], "4:2:2")):
        f = pipeline.HeifFile(hm, heifwriter.write_heic([hi], (64, 64), chroma_format=2, bit_depth=10, transforms=tr))
        with pytest.raises(RuntimeError, match=text):
            f.decode(f.primary(), 14)
        f.close()
    # 180 degrees on 10-bit 4:2:2 is fine
    f = pipeline.HeifFile(hm, heifwriter.write_heic([hi], (64, 64), chroma_format=2, bit_depth=10, transforms=[("irot", 2)]))
    planes, meta = f.decode(f.primary(), 14)
    f.close()
    exp, stride, _ = pipeline.cpu_decode(hm, [hi], 64, 64, 64, 64, 1, False, 14, transforms=[("irot", 2)])
    np.testing.assert_array_equal(planes[0][:64, :64 * 6], exp[:64, :64 * 6])
    # an aperture outside the image
    pic = synthutil.picture(8401, width=64, height=64)
    f = pipeline.HeifFile(hm, heifwriter.write_heic([pic], (64, 64), transforms=[("clap", (10, 1, 10, 1, 4000, 1, 0, 1))]))
    with pytest.raises(RuntimeError, match="clean aperture"):
        f.decode(f.primary(), 10)
    # ... is skipped with ignore_transformations
    f.close()


def _write_with_alpha(main, main_size, alpha, alpha_size, transforms=None):
    """single image + an auxiliary alpha image (auxC urn:mpeg:mpegB:cicp:systems:auxiliary:alpha, 'auxl' reference)"""
    return heifwriter.write_heic([main], main_size, transforms=transforms, aux=[(alpha, alpha_size, "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha")])


@pytest.mark.gpu
@pytest.mark.parametrize("alpha_size", [(96, 64), (48, 32), (40, 56)], ids=["same_size", "half_size", "odd_ratio"])
def test_alpha_auxiliary_image(hm, alpha_size):
    """the alpha auxiliary image is decoded, scaled nearest-neighbour when its size differs
    (context.cc:2029-2078) and lands in byte 3 of RGBA / as a fourth plane of the native output."""
    main = synthutil.picture(8500, width=96, height=64, vui=1, full_range=1, matrix=6)
    alpha = synthutil.picture(8501, width=alpha_size[0], height=alpha_size[1])
    f = pipeline.HeifFile(hm, _write_with_alpha(main, (96, 64), alpha, alpha_size))
    iid = f.primary()
    assert f.info(iid).has_alpha == 1 and f.alpha_item(iid) != 0
    rgba, meta = f.decode(iid, 11)
    rgb, _ = f.decode(iid, 10)
    native, nmeta = f.decode(iid, 0)
    f.close()
    exp, stride, _ = pipeline.cpu_decode(hm, [main], 96, 64, 96, 64, 1, False, 11)
    a, a_stride = pipeline.attach_alpha(hm, exp, stride, 96, 64, alpha, *alpha_size)
    assert meta["has_alpha"] == 1
    np.testing.assert_array_equal(rgba[0][:64, :96 * 4], exp[:64, :96 * 4])
    assert len(set(exp[:64, 3:96 * 4:4].ravel().tolist())) > 4  # a real alpha plane, not a constant
    exp3, s3, _ = pipeline.cpu_decode(hm, [main], 96, 64, 96, 64, 1, False, 10)
    np.testing.assert_array_equal(rgb[0][:64, :96 * 3], exp3[:64, :96 * 3])  # RGB24: the alpha plane is dropped
    np.testing.assert_array_equal(nmeta["alpha"][:64, :96], a[:64, :96])


@pytest.mark.gpu
@pytest.mark.parametrize("main_bd,alpha_bd", [(10, 10), (10, 8), (8, 8), (12, 10)])
@pytest.mark.parametrize("cf", [1, 2])
def test_alpha_through_depth_changing_chains(hm, main_bd, alpha_bd, cf):
    """The alpha plane in the chains that change the sample depth (the chains of oracle/
    pipeline_search.py): a deeper image to RGBA32 (Op_to_sdr_planes shifts a deeper alpha plane down, copies an 8-bit
    one), any image to RRGGBBAA (an 8-bit image's alpha plane goes through Op_to_hdr_planes: (a << 2) | (a >> 6), a
    deeper image's is copied as 16-bit words; planes of the other depth class are refused as the reference's ops
    misread them)."""
    W, H = 96, 64
    kw = dict(width=W, height=H, vui=1, full_range=0, matrix=1, primaries=1, chroma_format=cf)
    main = synthutil.picture(8700 + main_bd + cf, bit_depth=main_bd, **kw)
    alpha = synthutil.picture(8750 + alpha_bd, width=W, height=H, chroma_format=0, bit_depth=alpha_bd)
    data = heifwriter.write_heic([main], (W, H), chroma_format=cf, bit_depth=main_bd,
                                 aux=[(alpha, (W, H), "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha", 0, alpha_bd)])
    a = orc.oracle_decode(hevcutil.parse(hm, alpha), 3)[0][0][:H, :W].astype(np.int64)
    f = pipeline.HeifFile(hm, data)
    iid = f.primary()
    # RGBA32
    if main_bd == 8 and alpha_bd != 8:
        with pytest.raises(RuntimeError):
            f.decode(iid, 11)
    else:
        got, meta = f.decode(iid, 11)
        exp, stride, _ = pipeline.cpu_decode(hm, [main], W, H, W, H, 1, False, 11, has_alpha=True)
        exp[:H, 3:W * 4:4] = (a >> (alpha_bd - 8) if (alpha_bd > 8) else a).astype(np.uint8)
        assert meta["stride"][0] == stride and meta["bit_depth"] == 8
        np.testing.assert_array_equal(got[0][:H, :W * 4], exp[:H, :W * 4])
    # RRGGBBAA
    for fmt in (13, 15):
        if (main_bd > 8) != (alpha_bd > 8):
            with pytest.raises(RuntimeError):
                f.decode(iid, fmt)
            continue
        got, meta = f.decode(iid, fmt)
        exp, stride, _ = pipeline.cpu_decode(hm, [main], W, H, W, H, 1, False, fmt, has_alpha=True)
        aw = ((a << 2) | (a >> 6)) if alpha_bd == 8 else a
        hi, lo = (6, 7) if fmt == 13 else (7, 6)
        exp[:H, hi:W * 8:8] = (aw >> 8).astype(np.uint8)
        exp[:H, lo:W * 8:8] = (aw & 0xFF).astype(np.uint8)
        assert meta["stride"][0] == stride and meta["bit_depth"] == (main_bd if main_bd > 8 else 10)
        np.testing.assert_array_equal(got[0][:H, :W * 8], exp[:H, :W * 8])
    # RRGGBB (no alpha in the target): the plane is dropped
    got, _ = f.decode(iid, 14)
    exp, _, _ = pipeline.cpu_decode(hm, [main], W, H, W, H, 1, False, 14, has_alpha=True)
    np.testing.assert_array_equal(got[0][:H, :W * 6], exp[:H, :W * 6])
    f.close()


@pytest.mark.gpu
def test_monochrome_alpha_and_monochrome_image(hm):
    """4:0:0 pictures (the usual coding of alpha planes): as the alpha auxiliary image of a colour
    image, and as a main image (Op_mono_to_RGB24_32, monochrome.cc:160-273: v, v, v[, 0xFF])."""
    main = synthutil.picture(8600, width=96, height=64, vui=1, full_range=1, matrix=6)
    alpha = synthutil.picture(8601, width=96, height=64, chroma_format=0)
    data = heifwriter.write_heic([main], (96, 64), aux=[(alpha, (96, 64), "urn:mpeg:hevc:2015:auxid:1", 0)])
    f = pipeline.HeifFile(hm, data)
    rgba, meta = f.decode(f.primary(), 11)
    f.close()
    exp, stride, _ = pipeline.cpu_decode(hm, [main], 96, 64, 96, 64, 1, False, 11)
    a_planes, _ = orc.oracle_decode(hevcutil.parse(hm, alpha), 3)
    assert len(a_planes) == 1
    exp[:64, 3:96 * 4:4] = a_planes[0][:64, :96].astype(np.uint8)
    np.testing.assert_array_equal(rgba[0][:64, :96 * 4], exp[:64, :96 * 4])

    mono = synthutil.picture(8602, width=200, height=136, chroma_format=0, log2_ctb=5)
    y = orc.oracle_decode(hevcutil.parse(hm, mono), 3)[0][0].astype(np.uint8)
    f = pipeline.HeifFile(hm, heifwriter.write_heic([mono], (200, 136), chroma_format=0, transforms=[("irot", 1)]))
    info = f.info(f.primary())
    assert (info.chroma, info.width, info.height) == (0, 136, 200)
    rgb, m3 = f.decode(f.primary(), 10)
    rgba, m4 = f.decode(f.primary(), 11)
    native, nm = f.decode(f.primary(), 0)
    f.close()
    yr = np.rot90(y, 1)
    np.testing.assert_array_equal(native[0][:200, :136], yr)
    for k in range(3):
        np.testing.assert_array_equal(rgb[0][:200, k:136 * 3:3], yr)
        np.testing.assert_array_equal(rgba[0][:200, k:136 * 4:4], yr)
    assert (rgba[0][:200, 3:136 * 4:4] == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nclx", [dict(full_range=1, matrix=6), dict(full_range=0, matrix=1), dict(full_range=1, matrix=0)],
                         ids=["bt601_full", "bt709_limited", "gbr"])
def test_444_images(hm, nclx):
    """4:4:4 pictures end to end: single image with a transformation -> RGB24 / RGBA / native planes
    (Op_YCbCr_to_RGB incl. the GBR branch of matrix_coefficients 0), and a 2x2 grid with the paste geometry of
    context.cc:2466-2480 (chroma origin = luma origin)."""
    pic = synthutil.picture(8700, width=200, height=136, chroma_format=3, log2_ctb=5, qp=29, vui=1, **nclx)
    tr = [("irot", 1), _clap(136, 200, 120, 180, 3, -4)]
    f = pipeline.HeifFile(hm, heifwriter.write_heic([pic], (200, 136), chroma_format=3, transforms=tr))
    info = f.info(f.primary())
    assert info.chroma == 3
    rgb, m3 = f.decode(f.primary(), 10)
    rgba, m4 = f.decode(f.primary(), 11)
    native, nm = f.decode(f.primary(), 0)
    f.close()
    exp, stride, canv = pipeline.cpu_decode(hm, [pic], 200, 136, 200, 136, 1, False, 10, transforms=tr)
    exp4, stride4, _ = pipeline.cpu_decode(hm, [pic], 200, 136, 200, 136, 1, False, 11, transforms=tr)
    w, h = m3["width"], m3["height"]
    assert (w, h) == (120, 180) and m3["stride"][0] == stride
    np.testing.assert_array_equal(rgb[0][:h, :w * 3], exp[:h, :w * 3])
    np.testing.assert_array_equal(rgba[0][:h, :w * 4], exp4[:h, :w * 4])
    for c in range(3):
        pw, ph = nm["plane_size"][c]
        assert (pw, ph) == (w, h)
        np.testing.assert_array_equal(native[c][:ph, :pw], canv[c][0][:ph, :pw])

    tiles = [synthutil.picture(8710 + i, width=128, height=64, chroma_format=3, bit_depth=10, log2_ctb=[4, 5, 6, 5][i], qp=30, vui=1, **nclx) for i in range(4)]
    data = heifwriter.write_heic(tiles, (128, 64), grid=(2, 2, 250, 120), chroma_format=3, bit_depth=10)
    f = pipeline.HeifFile(hm, data)
    out, meta = f.decode(f.primary(), 14, threads=2)
    f.close()
    exp, stride, _ = pipeline.cpu_decode(hm, tiles, 128, 64, 250, 120, 2, True, 14)
    assert (meta["width"], meta["height"], meta["bit_depth"]) == (250, 120, 10) and meta["stride"][0] == stride
    np.testing.assert_array_equal(out[0][:120, :250 * 6], exp[:120, :250 * 6])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["8bit_full", "8bit_limited_paste_rescale", "10bit"])
def test_grid_tiles_with_their_own_transforms(hm, variant):
    """VERDICT r01 item 9 / SURVEY 8a row A3: a grid whose TILE items carry irot / imir (decode_image_planar applies them to
    the tile image before decode_and_paste_tile_image pastes it, context.cc:1957-2020, 2407-2539): such tiles are decoded
    to planes of their own, transformed and pasted (k_paste_bytes, incl. the byte-wise range rescale), the others go
    straight into the canvas.  2x2 grid of 64x64 tiles, canvas 120x100 (right / bottom tiles cropped)."""
    kw = dict(width=64, height=64)
    bd = 8
    if variant == "8bit_full":
        kw.update(vui=1, full_range=1, matrix=6)
    elif variant == "8bit_limited_paste_rescale":
        kw.update(vui=0)
    else:
        kw.update(vui=1, full_range=1, matrix=1, bit_depth=10)
        bd = 10
    tiles = [synthutil.picture(9300 + i, **kw) for i in range(4)]
    tt = {0: [("irot", 1)], 1: [("irot", 2)], 3: [("irot", 3)]} if bd == 10 else {0: [("irot", 1)], 1: [("imir", 1)], 3: [("irot", 2), ("imir", 0)]}
    data = heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 120, 100), bit_depth=bd, tile_transforms=tt)
    f = pipeline.HeifFile(hm, data)
    for fmt in ((10, 0) if bd == 8 else (14, 0)):
        got, meta = f.decode(f.primary(), fmt)
        exp, stride, canv = pipeline.cpu_decode(hm, tiles, 64, 64, 120, 100, 2, True, fmt if fmt else 10, tile_transforms=tt)
        if fmt:
            bpp = orc.OUT_BYTES[fmt]
            np.testing.assert_array_equal(got[0][:100, :120 * bpp], exp[:100, :120 * bpp])
        else:
            bps = 2 if bd > 8 else 1
            for c, (w, h) in enumerate(((120, 100), (60, 50), (60, 50))):
                np.testing.assert_array_equal(got[c][:h, :w * bps], canv[c][0][:h, :w * bps])
    # ignore_transformations: the tiles are pasted as coded
    got, _ = f.decode(f.primary(), 0, ignore_transformations=1)
    _, _, canv = pipeline.cpu_decode(hm, tiles, 64, 64, 120, 100, 2, True, 10 if bd == 8 else 14)
    np.testing.assert_array_equal(got[0][:100, :120 * (2 if bd > 8 else 1)], canv[0][0][:100, :120 * (2 if bd > 8 else 1)])
    f.close()


@pytest.mark.gpu
def test_own_transform_tiles_at_odd_origins(hm):
    """The reference's rounding of a chroma origin, (x0 + 1) / 2 (context.cc:2466-2483; csrc/hm_plane_geom.h: hm_place_tile), where it
    shows: a 4:2:0 grid of 64x64 pictures whose items declare 63x63, so column 1 starts at x = 63 and row 1 at y = 63, chroma at 32 -
    one sample further than the luma origin halved.  Tile 1 (odd x) and tile 3 (odd x and y) carry an irot of their own and are pasted
    from planes of their own, tile 2 (odd y) goes straight into the canvas.  Tiles 0, 1 and 3 also carry a clap to 63x63, the size
    they declare: no two tiles then overlap but tiles 2 and 3 in one column, where the paste of tile 3 comes behind the batch that
    pastes tile 2 - the order of the reference's sequential paste (tiles that overlap inside one batch have no defined order).
    Expected: the fingerprints of tests/golden/grid_odd_origin.json, recorded from the commit named there - and the CPU flow of the
    reference, which agrees with them."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_odd_origin.json")))
    tiles = [synthutil.picture(9500 + i, width=64, height=64, vui=1, full_range=1, matrix=6) for i in range(4)]
    c63 = ("clap", (63, 1, 63, 1, 0, 1, 0, 1))
    tt = {0: [c63], 1: [("irot", 2), c63], 3: [("irot", 1), c63]}
    data = heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 120, 100), sizes=[(63, 63)] * 4, tile_transforms=tt)
    f = pipeline.HeifFile(hm, data)
    rgb, meta = f.decode(f.primary(), 10)
    planes, _ = f.decode(f.primary(), 0)
    f.close()
    assert (meta["width"], meta["height"]) == (120, 100)
    got = {"rgb": pipeline.survey_fnv(rgb[0], meta["stride"][0], 120 * 3, 100)}
    for c, (w, h) in enumerate(((120, 100), (60, 50), (60, 50))):
        got["y cb cr".split()[c]] = pipeline.survey_fnv(planes[c], planes[c].shape[1], w, h)
    exp, _, canv = pipeline.cpu_decode(hm, tiles, 64, 64, 120, 100, 2, True, 10, tile_transforms=tt, step=(63, 63))
    np.testing.assert_array_equal(rgb[0][:100, :360], exp[:100, :360])
    for c, (w, h) in enumerate(((120, 100), (60, 50), (60, 50))):
        np.testing.assert_array_equal(planes[c][:h, :w], canv[c][0][:h, :w])
    assert got == gold["fingerprints"]


@pytest.mark.gpu
def test_own_transform_tile_outside_the_canvas_is_refused_before_anything_runs(hm):
    """A crafted grid: tiles with their own irot, a canvas narrower than one tile column, so that the second column's origin
    lies at / beyond the canvas edge (the reference: context.cc:2466-2483 returns an error for it).  The image must be
    refused - by the per-tile check that runs before any device work is queued - and the next decode of a good file on
    the same thread must be unaffected (the own-tile planes of the refused job are released behind its stream)."""
    tiles = [synthutil.picture(9400 + i, width=64, height=64) for i in range(4)]
    tt = {0: [("irot", 1)], 1: [("irot", 1)], 2: [("irot", 2)], 3: [("irot", 3)]}
    bad = heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 64, 100), tile_transforms=tt)  # canvas 64 wide: column 1 starts at x = 64
    f = pipeline.HeifFile(hm, bad)
    for _ in range(3):
        with pytest.raises(RuntimeError):
            f.decode(f.primary(), 10)
    f.close()
    good = heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 120, 100), tile_transforms=tt)
    g = pipeline.HeifFile(hm, good)
    got, _ = g.decode(g.primary(), 10)
    exp, _, _ = pipeline.cpu_decode(hm, tiles, 64, 64, 120, 100, 2, True, 10, tile_transforms=tt)
    np.testing.assert_array_equal(got[0][:100, :120 * 3], exp[:100, :120 * 3])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vui", [1, 0])
def test_alpha_images_of_grid_tiles(hm, vui):
    """VERDICT r02 missing 5: alpha auxiliary images that belong to TILE items of a grid.  decode_image_planar attaches a
    tile's alpha image to the tile image (context.cc:2029-2078: Y plane, scaled nearest-neighbour to the tile's size);
    decode_and_paste_tile_image gives the canvas an alpha plane filled with the maximum value as soon as a tile has one
    (:2437-2455) and pastes the tile's alpha like its luma plane - with the byte-wise range rescale when the tile's VUI
    says limited range (:2504-2528: the loop runs over every channel of the tile image).  2x2 grid of 64x64 tiles on a
    120x100 canvas; tile 0 has a same-size alpha image, tile 3 a half-size one (scaled), tiles 1 and 2 none (opaque)."""
    kw = dict(width=64, height=64)
    kw.update(dict(vui=1, full_range=1, matrix=6) if vui else dict(vui=0))
    tiles = [synthutil.picture(9500 + i, **kw) for i in range(4)]
    a0 = synthutil.picture(9510, width=64, height=64, chroma_format=0)
    a3 = synthutil.picture(9511, width=32, height=32)
    urn = "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"
    data = heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 120, 100),
                                 aux=[(a0, (64, 64), urn, 0, 8, 1), (a3, (32, 32), urn, 1, 8, 4)])
    f = pipeline.HeifFile(hm, data)
    iid = f.primary()
    assert f.info(iid).has_alpha == 1
    rgba, meta = f.decode(iid, 11)
    native, nmeta = f.decode(iid, 0)
    rgb, _ = f.decode(iid, 10)
    f.close()
    assert meta["has_alpha"] == 1
    # expected alpha plane: opaque canvas, the tiles' alpha Y planes pasted at the tile origins (cropped at the canvas edge)
    o = orc.load()
    exp_a = np.full((100, 120), 255, np.uint8)
    ya0 = orc.oracle_decode(hevcutil.parse(hm, a0), 3)[0][0][:64, :64].astype(np.uint8)
    ya3 = orc.oracle_decode(hevcutil.parse(hm, a3), 3)[0][0][:32, :32].astype(np.uint8)
    src, s_stride = orc.alloc_plane(32, 32, 1)
    src[:32, :32] = ya3
    scaled, sc_stride = orc.alloc_plane(64, 64, 1)
    o.orc_scale_nn_plane(orc.ptr(src), s_stride, 32, 32, 1, orc.ptr(scaled), sc_stride, 64, 64)
    for (x0, y0, plane) in ((0, 0, ya0), (64, 64, scaled[:64, :64])):
        p = plane.astype(np.float32)
        if not vui:  # tile nclx (from the VUI defaults) says limited range: the paste rescales, luma constants
            p = np.clip(np.trunc((p - np.float32(16)) * np.float32(1.1689) + np.float32(0.5)), 0, 255)
        h, w = min(64, 100 - y0), min(64, 120 - x0)
        exp_a[y0:y0 + h, x0:x0 + w] = p[:h, :w].astype(np.uint8)
    np.testing.assert_array_equal(nmeta["alpha"][:100, :120], exp_a)
    np.testing.assert_array_equal(rgba[0][:100, 3:120 * 4:4], exp_a)
    # the colour channels are those of the same grid without alpha images
    exp, _, _ = pipeline.cpu_decode(hm, tiles, 64, 64, 120, 100, 2, True, 10)
    np.testing.assert_array_equal(rgb[0][:100, :120 * 3], exp[:100, :120 * 3])
    for c in range(3):
        np.testing.assert_array_equal(rgba[0][:100, c:120 * 4:4], exp[:100, c:120 * 3:3])
