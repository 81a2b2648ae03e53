"""CPU: ISO/IEC 23001-17 'unci' items at the file level - the cmpd / uncC properties, hm_unci_info, the closed-form layout
(hm_unci_sample_bit, the payload length) held against the serial model of tests/unci_ref.py on the reference's 79 fixtures and on
synthetic files, every refusal with its status, and the tiles a view needs.  Nothing here needs a device."""
import ctypes as C
import glob
import os
import struct

import numpy as np
import pytest

import unci_ref as U
import unciwriter as W

OK, INVALID_ARG, UNSUPPORTED, BITSTREAM = 0, -1, -2, -3
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "unci", "uncompressed_*.heif")))
# the families of the fixtures by what they decode to: name fragment -> members
FAMILIES = {"rgb8": 20, "rgb7": 12, "abgr": 9, "rgb16": 7, "mono": 7, "yuv420": 6, "yuv422": 6, "rgb565": 4, "yuv444": 4, "yuv420_16": 2, "yuv422_16": 2}


def family_of(name):
    n = os.path.basename(name)
    if "Y16U16V16_420" in n: return "yuv420_16"
    if "Y16U16V16_422" in n: return "yuv422_16"
    if "_420" in n: return "yuv420"
    if "_422" in n: return "yuv422"
    if "YUV_tiled" in n: return "yuv444"
    if "R5G6B5" in n: return "rgb565"
    if "R7" in n: return "rgb7"
    if "B16R16G16" in n: return "rgb16"
    if "ABGR" in n or "R8G8B8A8" in n: return "abgr"
    if "_M" in n: return "mono"
    return "rgb8"


class File:
    def __init__(self, pkg, data):
        self.capi, self.L = pkg.capi, pkg.capi.image_lib()
        self.h = C.c_void_p()
        rc = self.L.hm_file_open(data, len(data), C.byref(self.h))
        assert rc == 0, self.L.hm_last_error()
        self.id = self.L.hm_file_primary_item(self.h)

    def unci(self):
        info = self.capi.UnciInfo()
        return self.L.hm_file_unci_info(self.h, self.id, C.byref(info)), info

    def image_info(self):
        i = self.capi.ImageInfo()
        return self.L.hm_file_image_info(self.h, self.id, C.byref(i)), i

    def error(self):
        return self.L.hm_last_error().decode()

    def close(self):
        self.L.hm_file_close(self.h)


@pytest.fixture(scope="module")
def models():
    """name -> (desc, payload, planes, positions, consumed) of every fixture and synthetic case: the serial model, run once"""
    out = {}
    for p in FIXTURES:
        data = open(p, "rb").read()
        desc, payload = U.describe(data)
        out[os.path.basename(p)] = (data, desc, payload) + U.decode(desc, payload)
    for name, desc in W.cases().items():
        data, _, payload = W.synthetic(desc, seed=len(name))
        out[name] = (data, desc, payload) + U.decode(desc, payload)
    return out


def test_the_fixtures_are_all_there():
    assert len(FIXTURES) == 79
    counts = {}
    for p in FIXTURES:
        counts[family_of(p)] = counts.get(family_of(p), 0) + 1
    assert counts == FAMILIES


def test_model_consumes_every_payload_and_families_agree(models):
    first = {}
    for name, (data, desc, payload, planes, where, used) in models.items():
        assert used == len(payload), name
        if not name.endswith(".heif"):
            continue
        out = U.output_planes(desc, planes)
        ref = first.setdefault(family_of(name), out)
        for a, b in zip(ref, out):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), name


def test_the_writer_is_the_models_inverse(models):
    for name, desc in W.cases().items():
        planes = W.random_planes(desc, len(name))
        got = models[name][3]
        assert all(np.array_equal(a, b) for a, b in zip(planes, got)), name
        # the padding bits in front of an aligned value are ones in these payloads: the model did not take them for sample bits
        assert W.pack(desc, planes, pad_bits=0) != models[name][2] or not any(a for _, _, a in desc["components"])


def test_info_of_every_file(pkg, models):
    capi = pkg.capi
    for name, (data, desc, payload, planes, where, used) in models.items():
        f = File(pkg, data)
        assert f.L.hm_file_item_kind(f.h, f.id) == capi.HM_ITEM_UNCI
        ids = (C.c_uint32 * 4)()
        assert f.L.hm_file_top_level_images(f.h, ids, 4) == 1 and ids[0] == f.id
        rc, u = f.unci()
        assert rc == OK, (name, f.error())
        assert (u.width, u.height) == (desc["width"], desc["height"])
        assert u.n_components == len(desc["components"])
        assert [(u.comp[c].type, u.comp[c].depth, u.comp[c].align_size) for c in range(u.n_components)] == [tuple(c) for c in desc["components"]], name
        assert (u.sampling, u.interleave, u.pixel_size, u.row_align, u.tile_align) == tuple(desc[k] for k in ("sampling", "interleave", "pixel_size", "row_align", "tile_align"))
        assert (u.tile_cols, u.tile_rows) == (desc["tile_cols"], desc["tile_rows"])
        assert (u.tile_width, u.tile_height) == (desc["width"] // desc["tile_cols"], desc["height"] // desc["tile_rows"])
        assert u.colour_space == U.colour_space(desc)
        # the layout's length is the payload's, to the byte
        assert u.payload_bytes == len(payload) == used, name
        n = C.c_uint64()
        assert f.L.hm_unci_payload_bytes(C.byref(u), C.byref(n)) == OK and n.value == len(payload)
        rc, i = f.image_info()
        assert rc == OK, (name, f.error())
        types = {t: d for t, d, _ in desc["components"]}
        depth = types[U.Y] if U.Y in types else max(d for t, d in types.items() if t in (U.MONO, U.R, U.G, U.B))
        cs = U.colour_space(desc)
        chroma = 0 if cs == 0 else 3 if cs == 2 else {0: 3, 1: 2, 2: 1}[desc["sampling"]]
        assert (i.width, i.height, i.bit_depth, i.chroma, i.has_alpha, i.is_grid, i.has_nclx) == (desc["width"], desc["height"], depth, chroma, int(U.ALPHA in types), 0, 0), name
        f.close()


def test_closed_form_equals_the_models_read_position_for_every_sample(pkg, models):
    L = pkg.capi.image_lib()
    bit = C.c_uint64()
    for name, (data, desc, payload, planes, where, used) in models.items():
        f = File(pkg, data)
        rc, u = f.unci()
        assert rc == OK
        for c, pos in enumerate(where):
            h, w = pos.shape
            got = np.zeros((h, w), np.uint64)
            for y in range(h):
                for x in range(w):
                    assert L.hm_unci_sample_bit(C.byref(u), c, x, y, C.byref(bit)) == OK
                    got[y, x] = bit.value
            assert np.array_equal(got, pos), (name, c, np.argwhere(got != pos)[:4])
            assert L.hm_unci_sample_bit(C.byref(u), c, w, 0, C.byref(bit)) == INVALID_ARG
            assert L.hm_unci_sample_bit(C.byref(u), c, 0, h, C.byref(bit)) == INVALID_ARG
        assert L.hm_unci_sample_bit(C.byref(u), len(where), 0, 0, C.byref(bit)) == INVALID_ARG
        f.close()


def test_uncc_version_1_profiles(pkg):
    for profile, types in ((b"rgb3", [U.R, U.G, U.B]), (b"rgba", [U.R, U.G, U.B, U.ALPHA]), (b"abgr", [U.ALPHA, U.B, U.G, U.R])):
        desc = W.make_desc(6, 4, [(t, 8, 0) for t in types], U.PIXEL)
        payload = W.pack(desc, W.random_planes(desc, 5))
        f = File(pkg, W.heif_file(desc, payload, uncc=W.uncc_box(desc, version=1, profile=profile), cmpd=False))
        rc, u = f.unci()
        assert rc == OK, f.error()
        assert [u.comp[c].type for c in range(u.n_components)] == types and all(u.comp[c].depth == 8 for c in range(u.n_components))
        assert (u.interleave, u.tile_cols, u.tile_rows, u.payload_bytes) == (U.PIXEL, 1, 1, len(payload))
        f.close()
    desc = W.make_desc(6, 4, [(U.R, 8, 0), (U.G, 8, 0), (U.B, 8, 0)], U.PIXEL)
    f = File(pkg, W.heif_file(desc, b"", uncc=W.uncc_box(desc, version=1, profile=b"yuv2"), cmpd=False))
    assert f.unci()[0] == UNSUPPORTED and "yuv2" in f.error()
    f.close()


RGB8 = [(U.R, 8, 0), (U.G, 8, 0), (U.B, 8, 0)]
YUV8 = [(U.Y, 8, 0), (U.CB, 8, 0), (U.CR, 8, 0)]


def refusals():
    d = lambda **kw: W.make_desc(8, 8, kw.pop("comps", RGB8), **kw)
    plain = d()
    return {
        # what the reference refuses
        "block_size": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, block_size=4))),
        "components_little_endian": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, flags=0x80))),
        "block_pad_lsb": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, flags=0x40))),
        "block_little_endian": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, flags=0x20))),
        "block_reversed": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, flags=0x10))),
        "format_float": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, formats=[1, 0, 0]))),
        "format_complex": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, formats=[0, 2, 0]))),
        "format_signed": (UNSUPPORTED, plain, dict(uncc=W.uncc_box(plain, formats=[0, 0, 3]))),
        "multi_y": (UNSUPPORTED, d(comps=YUV8, interleave=5, sampling=U.S_422), {}),
        "sampling_411": (UNSUPPORTED, d(comps=YUV8, sampling=3), {}),
        "component_type_depth": (UNSUPPORTED, d(comps=[(8, 8, 0)]), {}),
        "component_type_filter_array": (UNSUPPORTED, d(comps=RGB8 + [(11, 8, 0)]), {}),
        "mixed_without_subsampling": (UNSUPPORTED, d(comps=YUV8, interleave=U.MIXED), {}),
        # the rest of the list
        "cmpC": (UNSUPPORTED, plain, dict(extra_props=[W._full(b"cmpC", 0, 0, b"defl" + b"\0")])),
        "icbr": (UNSUPPORTED, plain, dict(extra_props=[W._full(b"icbr", 0, 0, struct.pack(">I", 0))])),
        "width_not_divisible": (UNSUPPORTED, d(tile_cols=3), {}),
        "height_not_divisible": (UNSUPPORTED, d(tile_rows=5), {}),
        "pixel_size_in_component_mode": (UNSUPPORTED, d(pixel_size=4), {}),
        "pixel_size_in_row_mode": (UNSUPPORTED, d(pixel_size=4, interleave=U.ROW), {}),
        "pixel_size_too_small": (UNSUPPORTED, d(pixel_size=2, interleave=U.PIXEL), {}),
        "align_smaller_than_depth": (UNSUPPORTED, d(comps=[(U.R, 9, 1), (U.G, 8, 0), (U.B, 8, 0)]), {}),
        "subsampling_in_pixel_mode": (UNSUPPORTED, d(comps=YUV8, sampling=U.S_420, interleave=U.PIXEL), {}),
        "subsampling_of_rgb": (UNSUPPORTED, d(sampling=U.S_422), {}),
        "subsampling_odd_tile": (UNSUPPORTED, W.make_desc(6, 6, YUV8, sampling=U.S_420, tile_cols=2, tile_rows=2), {}),
        "r_g_only": (UNSUPPORTED, d(comps=RGB8[:2]), {}),
        "red_twice": (UNSUPPORTED, d(comps=RGB8 + [(U.R, 8, 0)]), {}),
        "nine_components": (UNSUPPORTED, d(comps=RGB8 + [(U.PADDED, 8, 0)] * 6), {}),
        "uncC_version_2": (UNSUPPORTED, plain, dict(uncc=W._full(b"uncC", 2, 0, b"\0" * 4))),
        # broken files
        "no_cmpd": (BITSTREAM, plain, dict(cmpd=False)),
        "no_ispe": (BITSTREAM, plain, dict(ispe=False)),
        "index_outside_cmpd": (BITSTREAM, dict(plain, indices=[0, 1, 7]), {}),
    }


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusals_with_their_status(pkg, name):
    status, desc, args = refusals()[name]
    f = File(pkg, W.heif_file(desc, b"\0" * 256, **args))
    rc, _ = f.unci()
    assert rc == status, (name, rc, f.error())
    assert f.error()
    rc, _ = f.image_info()
    assert rc == status, (name, rc, f.error())
    f.close()


def test_no_uncc_and_not_an_unci_item(pkg):
    desc = W.make_desc(8, 8, RGB8)
    f = File(pkg, W.heif_file(desc, b"\0" * 192, uncc=W._box(b"free", b"")))
    assert f.unci()[0] == BITSTREAM
    f.close()
    f = File(pkg, W.heif_file(desc, b"\0" * 192, item_type=b"mski"))
    assert f.L.hm_file_item_kind(f.h, f.id) == pkg.capi.HM_ITEM_OTHER
    assert f.unci()[0] == INVALID_ARG
    assert f.image_info()[0] == UNSUPPORTED
    f.close()


def test_truncated_uncc_box_fails_the_open(pkg):
    desc = W.make_desc(8, 8, RGB8)
    box = W.uncc_box(desc)
    short = struct.pack(">I", len(box) - 6) + box[4:-6]
    data = W.heif_file(desc, b"\0" * 192, uncc=short)
    L = pkg.capi.image_lib()
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == BITSTREAM


def test_sizes_that_overflow_are_refused(pkg):
    L = pkg.capi.image_lib()
    u = pkg.capi.UnciInfo()
    u.width, u.height, u.colour_space, u.n_components = 1 << 30, 1 << 30, 2, 3
    for c, t in enumerate((U.R, U.G, U.B)):
        u.comp[c].type, u.comp[c].depth, u.comp[c].align_size = t, 16, 255
    u.interleave, u.tile_cols, u.tile_rows, u.tile_width, u.tile_height = U.PIXEL, 1, 1, 1 << 30, 1 << 30
    u.row_align = u.tile_align = 0xFFFFFFFF
    n = C.c_uint64()
    assert L.hm_unci_payload_bytes(C.byref(u), C.byref(n)) == BITSTREAM  # 2^30 rows of 765 * 2^30 bytes: more than 64 bits hold
    assert "overflow" in L.hm_last_error().decode()
    u.tile_height = u.height = 1 << 10
    assert L.hm_unci_payload_bytes(C.byref(u), C.byref(n)) == OK and n.value == (1 << 10) * (-(-(765 << 30) // 0xFFFFFFFF) * 0xFFFFFFFF)
    u.tile_cols = u.tile_rows = 1 << 16
    u.tile_width = u.tile_height = 1 << 16
    assert L.hm_unci_payload_bytes(C.byref(u), C.byref(n)) == BITSTREAM  # the image size overflows 31 bits
    u.tile_cols = u.tile_rows = 0
    assert L.hm_unci_payload_bytes(C.byref(u), C.byref(n)) == BITSTREAM


# ---- the image level, as far as it goes without a device: everything here is refused before any work is queued -------------------

RGB, RGBA, RRGGBB_LE, YCBCR_444 = 10, 11, 14, 0x103
ALPHA_URN = b"urn:mpeg:mpegB:cicp:systems:auxiliary:alpha\0"


def decode_status(f, iid, fmt=0):
    prm = f.capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
    d = f.capi.Decoded()
    rc = f.L.hm_decode_item(f.h, iid, C.byref(prm), C.byref(d))
    return rc, f.error()


def test_a_payload_one_byte_short_is_a_bitstream_error(pkg, models):
    for name in ("uncompressed_pix_RGB_tiled.heif", "uncompressed_tile_M_tiled.heif", "row_align_30_tile_align_37"):
        data, desc, payload = models[name][:3]
        f = File(pkg, W.heif_file(desc, payload[:-1]))
        rc, u = f.unci()
        assert rc == OK and u.payload_bytes == len(payload)
        rc, msg = decode_status(f, f.id)
        assert rc == BITSTREAM and str(len(payload)) in msg, (name, rc, msg)
        # the step alone: refused before the pointer is looked at
        planes = pkg.capi.Planes()
        assert f.L.hm_unci_unpack(C.byref(u), 0x1000, len(payload) - 1, None, C.byref(planes), 0, None, None) == BITSTREAM
        f.close()


def test_unci_items_in_other_roles_are_refused(pkg):
    desc = W.make_desc(8, 8, RGB8)
    grid_descriptor = bytes([0, 0, 0, 0, 0, 8, 0, 8])  # version, flags, rows - 1, columns - 1, 8 x 8: what a 'grid' item 2 reads of the shared payload
    payload = grid_descriptor + bytes(192 - 8)
    # a grid whose tile is the unci item
    f = File(pkg, W.heif_file(desc, payload, extra_items=[(2, b"grid")], extra_refs=[(b"dimg", 2, [1])]))
    rc, msg = decode_status(f, 2, RGB)
    assert rc == UNSUPPORTED and "unci" in msg, (rc, msg)
    f.close()
    # the child of a derived item
    f = File(pkg, W.heif_file(desc, payload, extra_items=[(2, b"iden")], extra_refs=[(b"dimg", 2, [1])]))
    rc, msg = decode_status(f, 2, RGB)
    assert rc == UNSUPPORTED and "unci" in msg, (rc, msg)
    f.close()
    # an auxiliary alpha image - here an 'unci' item itself - attached to an 'unci' item
    f = File(pkg, W.heif_file(desc, payload, extra_props=[W._full(b"auxC", 0, 0, ALPHA_URN)], extra_items=[(2, b"unci")], extra_refs=[(b"auxl", 2, [1])]))
    assert f.L.hm_file_alpha_item(f.h, 1) == 2
    ids = (C.c_uint32 * 4)()
    assert f.L.hm_file_top_level_images(f.h, ids, 4) == 1 and ids[0] == 1
    rc, msg = decode_status(f, 1, RGB)
    assert rc == UNSUPPORTED and "alpha" in msg, (rc, msg)
    f.close()
    # the gain map of a gain step
    f = File(pkg, W.heif_file(desc, payload, extra_items=[(2, b"unci")]))
    prm = pkg.capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
    gain = pkg.capi.DeviceGain()
    gain.map_item, gain.headroom = 2, 1.0
    gain.params.alternate_headroom = 1.0
    for c in range(3):
        gain.params.map_max[c], gain.params.gamma[c] = 1.0, 1.0
    light = pkg.capi.DeviceLight(0, 0, 8, 0, 1.0)
    dest = pkg.capi.DeviceDest(0x1000, 1 << 30, 1, 3, 0, 0)
    d = pkg.capi.Decoded()
    rc = f.L.hm_decode_item_to_device_gain(f.h, 1, C.byref(prm), None, C.byref(light), None, C.byref(gain), C.byref(dest), C.byref(d))
    assert rc == UNSUPPORTED, (rc, f.error())
    f.close()


def test_targets_that_have_no_chain_are_refused_with_the_detail(pkg, models):
    L = pkg.capi.image_lib()
    no_chain = pkg.capi.HM_DETAIL_NO_COLOUR_CHAIN
    for name, fmts in (("uncompressed_pix_R5G6B5_tiled.heif", (RGB, RGBA, RRGGBB_LE)), ("uncompressed_comp_R7G7B7_tiled.heif", (RGB, RRGGBB_LE)),
                       ("uncompressed_comp_B16R16G16.heif", (RGB, RGBA, 12, 13)), ("uncompressed_comp_RGB.heif", (RRGGBB_LE, 15, 12)),
                       ("depths_12_15_16_row", (RGB, RRGGBB_LE))):
        f = File(pkg, models[name][0])
        for fmt in fmts:
            rc, msg = decode_status(f, f.id, fmt)
            assert rc == UNSUPPORTED and L.hm_last_error_detail() == no_chain, (name, fmt, rc, msg)
        rc, msg = decode_status(f, f.id, YCBCR_444)  # an R G B item has no chroma format to ask for
        assert rc == UNSUPPORTED and L.hm_last_error_detail() != no_chain, (name, msg)
        f.close()
    for name in ("uncompressed_mix_Y16U16V16_420.heif", "uncompressed_comp_Y16U16V16_422.heif", "mono_1bit"):
        f = File(pkg, models[name][0])
        for fmt in (RGB, RRGGBB_LE, YCBCR_444):
            rc, msg = decode_status(f, f.id, fmt)
            assert rc == UNSUPPORTED and "as coded only" in msg, (name, fmt, rc, msg)
        f.close()


def test_plan_view_names_the_internal_tiles_a_crop_touches(pkg, models):
    capi = pkg.capi
    for name in ("uncompressed_pix_RGB_tiled.heif", "uncompressed_tile_ABGR_tiled.heif", "uncompressed_comp_YUV_tiled.heif"):
        data, desc = models[name][:2]
        f = File(pkg, data)
        cols, rows = desc["tile_cols"], desc["tile_rows"]
        tw, th = desc["width"] // cols, desc["height"] // rows
        assert cols * rows > 1
        tiles = (C.c_int32 * 4)()

        def plan(crop, fmt=RGB, ignore=0, planes=False):
            prm = capi.DecodeParams(fmt, 2, ignore, 0, None, None, 0, 0, 0, 0)
            view = capi.DeviceView(crop[0], crop[1], crop[2], crop[3], 0, 0, 0)
            fn = f.L.hm_plan_planes_view if planes else f.L.hm_plan_view
            assert fn(f.h, f.id, C.byref(prm), C.byref(view), C.byref(tiles)) == OK
            return list(tiles)

        whole = [0, rows, 0, cols]
        assert plan((0, 0, 0, 0)) == whole
        assert plan((tw + 1, 1, 2, 2)) == [0, 1, 1, 1]
        assert plan((tw - 1, th - 1, 2, 2)) == [0, 2, 0, 2]
        assert plan((desc["width"] - 1, desc["height"] - 1, 1, 1)) == [rows - 1, 1, cols - 1, 1]
        assert plan((tw + 1, 1, 2, 2), fmt=0) == whole                    # the planes as coded go through hm_plan_planes_view
        assert plan((tw + 1, 1, 2, 2), fmt=0, planes=True) == [0, 1, 1, 1]
        assert plan((tw + 1, 1, 2, 2), planes=True) == whole
        assert plan((tw + 1, 1, 2, desc["height"] + 1)) == whole          # a crop outside the image: the decode's to refuse
        f.close()
    # a transformation on the item: everything is unpacked
    desc = W.make_desc(12, 8, RGB8, U.PIXEL, tile_cols=3, tile_rows=2)
    f = File(pkg, W.heif_file(desc, bytes(288), extra_props=[W._box(b"irot", bytes([1]))]))
    prm = capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
    view = capi.DeviceView(0, 0, 2, 2, 0, 0, 0)
    tiles = (C.c_int32 * 4)()
    assert f.L.hm_plan_view(f.h, f.id, C.byref(prm), C.byref(view), C.byref(tiles)) == OK and list(tiles) == [0, 2, 0, 3]
    prm.ignore_transformations = 1
    assert f.L.hm_plan_view(f.h, f.id, C.byref(prm), C.byref(view), C.byref(tiles)) == OK and list(tiles) == [0, 1, 0, 1]
    f.close()
