"""CPU: region items ('rgan') and mask items ('mski') at the file level, on files written by tests/regionwriter.py - every geometry type
read back field by field in both field sizes, the 'cdsc' and 'mask' references, the top-level list, hm_file_item_kind, and every
refusal with its status and a message.  All of it comes before a device is needed (this file runs without one)."""
import ctypes as C
import struct

import numpy as np
import pytest

import synthutil
from regionwriter import Writer, pack_bits, region_payload

OK, INVALID_ARG, UNSUPPORTED, BITSTREAM = 0, -1, -2, -3
NEW_SYMBOLS = ("hm_file_region_items", "hm_file_region_item_info", "hm_file_region", "hm_file_region_points", "hm_file_region_inline_mask",
               "hm_regions_dest_bytes", "hm_rasterise_regions", "hm_regions_to_device")


@pytest.fixture(scope="module")
def pic():
    return synthutil.picture(97001, width=64, height=64)


class File:
    def __init__(self, pkg, data):
        self.capi = pkg.capi
        self.L = pkg.capi.image_lib()
        self.h = C.c_void_p()
        rc = self.L.hm_file_open(data, len(data), C.byref(self.h))
        assert rc == 0, self.L.hm_last_error()

    def msg(self):
        return self.L.hm_last_error().decode()

    def items_of(self, image):
        ids = (C.c_uint32 * 16)()
        n = self.L.hm_file_region_items(self.h, image, ids, 16)
        return [ids[k] for k in range(n)]

    def info(self, rid):
        i = self.capi.RegionItemInfo()
        rc = self.L.hm_file_region_item_info(self.h, rid, C.byref(i))
        return rc, i

    def region(self, rid, k):
        g = self.capi.Region()
        rc = self.L.hm_file_region(self.h, rid, k, C.byref(g))
        return rc, g

    def points(self, rid, k, cap=64):
        xy = (C.c_int32 * (2 * cap))()
        n = self.L.hm_file_region_points(self.h, rid, k, xy, cap)
        return n, [(xy[2 * i], xy[2 * i + 1]) for i in range(max(0, min(n, cap)))]

    def bits(self, rid, k):
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        rc = self.L.hm_file_region_inline_mask(self.h, rid, k, C.byref(p), C.byref(n))
        return rc, (C.string_at(p, n.value) if rc == 0 else b"")

    def top(self):
        ids = (C.c_uint32 * 64)()
        n = self.L.hm_file_top_level_images(self.h, ids, 64)
        return [ids[k] for k in range(n)]

    def kind(self, iid):
        return self.L.hm_file_item_kind(self.h, iid)

    def image_info(self, iid):
        i = self.capi.ImageInfo()
        return self.L.hm_file_image_info(self.h, iid, C.byref(i)), i

    def decode_status(self, iid, out_format=0):
        prm = self.capi.DecodeParams(out_format, 2, 0, 0, None, None, 0, 0, 0, 0)
        d = self.capi.Decoded()
        rc = self.L.hm_decode_item(self.h, iid, C.byref(prm), C.byref(d))
        return rc, self.msg()

    def close(self):
        self.L.hm_file_close(self.h)


def test_the_new_symbols_exist(hm):
    for name in NEW_SYMBOLS:
        assert hasattr(hm, name), name


POLY = [(-3, 5), (40, -7), (12, 30)]
BITS = pack_bits([[(x + y) % 3 == 0 for x in range(13)] for y in range(5)])


def all_types(mask_a, mask_b):
    return [("point", -4, 9), ("rectangle", -10, 3, 20, 7), ("ellipse", 30, -2, 11, 0), ("polygon", POLY),
            ("referenced_mask", -2, 1, 0, 0, mask_a), ("inline_mask", -5, 2, 13, 5, BITS), ("referenced_mask", 50, 30, 37, 21, mask_b),
            ("polyline", POLY[:2]), ("polygon", [])]


@pytest.mark.parametrize("wide", [False, True])
def test_every_geometry_type_read_back(pkg, pic, wide):
    capi = pkg.capi
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    img2 = w.hvc1(pic, (64, 64))
    ma = w.mski(bytes(37 * 21), (37, 21))
    mb = w.mski(bytes(37 * 21), (37, 21))
    regions = all_types(ma, mb)
    if wide:  # coordinates that need the 32-bit fields
        regions[0] = ("point", -70000, 123456)
        regions[1] = ("rectangle", -(1 << 28), (1 << 28) - 1, (1 << 28) - 1, 70000)
    r1 = w.rgan(regions, (200, 100), annotates=[img, img2], wide=wide)
    r2 = w.rgan([("point", 1, 2)], (64, 64), annotates=[img])
    f = File(pkg, w.finish(primary=img))
    try:
        assert f.items_of(img) == [r1, r2] and f.items_of(img2) == [r1] and f.items_of(ma) == [] and f.items_of(99) == []
        rc, info = f.info(r1)
        assert rc == OK and (info.reference_width, info.reference_height, info.n_regions, info.field_bits) == (200, 100, len(regions), 32 if wide else 16)
        rc, info = f.info(r2)
        assert rc == OK and (info.reference_width, info.reference_height, info.n_regions) == (64, 64, 1)
        got = []
        for k in range(len(regions)):
            rc, g = f.region(r1, k)
            assert rc == OK, f.msg()
            got.append((g.type, g.x, g.y, g.w, g.h, g.n_points, g.mask_item, g.mask_bytes))
        assert got[0] == (capi.HM_REGION_POINT,) + tuple(regions[0][1:3]) + (0, 0, 0, 0, 0)
        assert got[1] == (capi.HM_REGION_RECTANGLE,) + tuple(regions[1][1:5]) + (0, 0, 0)
        assert got[2] == (capi.HM_REGION_ELLIPSE, 30, -2, 11, 0, 0, 0, 0)
        assert got[3] == (capi.HM_REGION_POLYGON, 0, 0, 0, 0, 3, 0, 0)
        # the k-th referenced-mask region takes the k-th entry of the 'mask' reference, an inline mask between them takes none;
        # width / height 0: the mask item's ispe
        assert got[4] == (capi.HM_REGION_REFERENCED_MASK, -2, 1, 37, 21, 0, ma, 37 * 21)
        assert got[5] == (capi.HM_REGION_INLINE_MASK, -5, 2, 13, 5, 0, 0, (13 * 5 + 7) // 8)
        assert got[6] == (capi.HM_REGION_REFERENCED_MASK, 50, 30, 37, 21, 0, mb, 37 * 21)
        assert got[7] == (capi.HM_REGION_POLYLINE, 0, 0, 0, 0, 2, 0, 0)
        assert got[8] == (capi.HM_REGION_POLYGON, 0, 0, 0, 0, 0, 0, 0)
        assert f.points(r1, 3) == (3, POLY) and f.points(r1, 7) == (2, POLY[:2]) and f.points(r1, 8) == (0, []) and f.points(r1, 0) == (0, [])
        assert f.points(r1, 3, cap=2) == (3, POLY[:2])
        assert f.L.hm_file_region_points(f.h, r1, 3, None, 0) == 3
        assert f.bits(r1, 5) == (OK, BITS)
        rc, _ = f.bits(r1, 1)
        assert rc == INVALID_ARG and "not an inline mask" in f.msg()
        rc, _ = f.region(r1, len(regions))
        assert rc == INVALID_ARG and f.msg()
        rc, _ = f.region(r1, -1)
        assert rc == INVALID_ARG
        rc, _ = f.info(img)
        assert rc == INVALID_ARG and "not a region item" in f.msg()
        assert f.kind(r1) == capi.HM_ITEM_OTHER
    finally:
        f.close()


def test_read_regions_python(pkg, pic):
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    ma = w.mski(bytes(37 * 21), (37, 21))
    mb = w.mski(bytes(37 * 21), (37, 21))
    regions = all_types(ma, mb)
    r1 = w.rgan(regions, (200, 100), annotates=[img])
    out = pkg.read_regions(w.finish(primary=img))
    assert len(out) == 1 and out[0]["item_id"] == r1 and out[0]["reference_size"] == (200, 100)
    got = out[0]["regions"]
    assert [g["type"] for g in got] == [r[0] for r in regions]
    assert (got[1]["x"], got[1]["y"], got[1]["w"], got[1]["h"]) == (-10, 3, 20, 7)
    assert got[3]["points"].dtype == np.int32 and got[3]["points"].tolist() == [list(p) for p in POLY] and got[8]["points"].shape == (0, 2)
    assert got[4]["mask_item"] == ma and got[6]["mask_item"] == mb and got[5]["bits"] == BITS and got[0]["mask_item"] == 0


def test_top_level_list_and_item_kind(pkg, pic):
    capi = pkg.capi
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    shown = w.mski(bytes(6), (3, 2), hidden=False)            # an image of its own
    hidden = w.mski(bytes(6), (3, 2), hidden=True)
    masked = w.mski(bytes(6), (3, 2), hidden=False)           # the target of a 'mask' reference
    bare = w.mski(bytes(6), (3, 2), hidden=False, mskc=False)  # no mskC: no image ("Missing required box for mask codec")
    deep = w.mski(bytes(12), (3, 2), bits=16, hidden=False)
    w.rgan([("referenced_mask", 0, 0, 3, 2, masked)], (64, 64), annotates=[img])
    f = File(pkg, w.finish(primary=img))
    try:
        assert f.top() == [img, shown, deep]
        assert [f.kind(i) for i in (shown, hidden, masked, bare, deep)] == [capi.HM_ITEM_MSKI] * 3 + [capi.HM_ITEM_OTHER, capi.HM_ITEM_MSKI] and capi.HM_ITEM_MSKI == 7
        rc, info = f.image_info(shown)
        assert rc == OK and (info.width, info.height, info.bit_depth, info.chroma, info.has_alpha) == (3, 2, 8, 0, 0)
        rc, _ = f.image_info(bare)
        assert rc == UNSUPPORTED and f.msg()
        rc, _ = f.image_info(deep)
        assert rc == UNSUPPORTED and "bits_per_pixel 16" in f.msg()
        rc, msg = f.decode_status(deep)
        assert rc == UNSUPPORTED and "bits_per_pixel 16" in msg
        rc, msg = f.decode_status(bare)
        assert rc == UNSUPPORTED and msg
    finally:
        f.close()


def region_status(pkg, data, rid, k=0):
    f = File(pkg, data)
    try:
        rc, _ = f.info(rid)
        msg = f.msg()
        rc2, _ = f.region(rid, k)
        assert rc2 == rc
        n = f.L.hm_file_region_points(f.h, rid, k, None, 0)
        assert n == rc
        return rc, msg
    finally:
        f.close()


REFUSALS = {
    "unknown_type": (dict(regions=[("point", 1, 1), ("raw", 7, b"\0" * 8)]), UNSUPPORTED, "geometry type 7"),
    "deflate": (dict(regions=[("inline_mask", 0, 0, 4, 2, b"\xff", 1)]), UNSUPPORTED, "Deflate"),
    "short_header": (dict(payload=b"\0\0\0\x40\0\x40"), BITSTREAM, "8 bytes"),
    "truncated_rectangle": (dict(payload=region_payload([("rectangle", 1, 2, 3, 4)], (64, 64))[:-1]), BITSTREAM, ""),
    "truncated_count": (dict(payload=region_payload([("point", 1, 2)], (64, 64), count=2)), BITSTREAM, ""),
    "truncated_points": (dict(payload=region_payload([("polygon", [(1, 2), (3, 4)])], (64, 64))[:-2]), BITSTREAM, "points"),
    "truncated_inline_bits": (dict(regions=[("inline_mask", 0, 0, 13, 5, BITS[:-1])]), BITSTREAM, "inline mask"),
    "few_mask_references": (dict(regions=lambda ids: [("referenced_mask", 0, 0, 0, 0, ids["m"]), ("referenced_mask", 5, 5, 0, 0, ids["m"])], masks=lambda ids: [ids["m"]]),
                            BITSTREAM, "'mask' reference"),
    "mask_is_no_mski": (dict(regions=lambda ids: [("referenced_mask", 0, 0, 0, 0, ids["img2"])]), UNSUPPORTED, "not a mask image"),
    "mask_without_mskc": (dict(regions=lambda ids: [("referenced_mask", 0, 0, 0, 0, ids["bare"])]), UNSUPPORTED, "not a mask image"),
    "mask_size_differs": (dict(regions=lambda ids: [("referenced_mask", 0, 0, 36, 21, ids["m"])]), UNSUPPORTED, "not scaled"),
    "coordinate_limit": (dict(regions=[("point", 1 << 28, 0)], wide=True), UNSUPPORTED, "2^28"),
    "negative_coordinate_limit": (dict(regions=[("polygon", [(0, 0), (5, -(1 << 28) - 1)])], wide=True), UNSUPPORTED, "2^28"),
    "size_limit": (dict(regions=[("rectangle", 0, 0, 1 << 28, 4)], wide=True), UNSUPPORTED, "2^28"),
    "radius_limit": (dict(regions=[("ellipse", 0, 0, 32768, 4)], wide=True), UNSUPPORTED, "32767"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_of_a_region_item(pkg, pic, name):
    """each with its status and a message; the file itself opens and the annotated image's info still reads"""
    spec, status, text = REFUSALS[name]
    spec = dict(spec)

    def extra(w):
        return dict(m=w.mski(bytes(37 * 21), (37, 21)), bare=w.mski(bytes(6), (3, 2), mskc=False), img2=w.hvc1(pic, (64, 64), hidden=True))
    ids_box = {}

    def extra_keep(w):
        ids_box.update(extra(w))
        return ids_box
    masks = spec.pop("masks", None)
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    ids = extra_keep(w)
    regions = spec.get("regions")
    regions = regions(ids) if callable(regions) else regions
    rid = w.rgan(regions or [], (64, 64), annotates=[img], payload=spec.get("payload"), masks=masks(ids) if masks else None, wide=spec.get("wide", False))
    data = w.finish(primary=img)
    rc, msg = region_status(pkg, data, rid, 0)
    assert rc == status and msg and text in msg, (rc, msg)
    f = File(pkg, data)  # a damaged region item leaves hm_file_open and the image working
    try:
        assert f.items_of(img) == [rid] and f.top() == [img]
        rc, info = f.image_info(img)
        assert rc == OK and (info.width, info.height) == (64, 64)
        # ... and hm_regions_to_device answers with the item's refusal before it needs a device
        dest = pkg.capi.RegionsDest(0x1000, 1 << 30, 0, 0, 0, 0, 1.0, 0.0)
        arr = (C.c_uint32 * 1)(rid)
        assert f.L.hm_regions_to_device(f.h, arr, 1, None, 0, C.byref(dest), None) == status
    finally:
        f.close()


def test_limits_are_inclusive_where_stated(pkg, pic):
    """-2^28 and 2^28 - 1 are coordinates, 2^28 - 1 a size, 32767 a radius"""
    lim = 1 << 28
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    rid = w.rgan([("rectangle", -lim, lim - 1, lim - 1, lim - 1), ("ellipse", lim - 1, -lim, 32767, 32767), ("polyline", [(-lim, lim - 1)])], (64, 64), annotates=[img], wide=True)
    data = w.finish(primary=img)
    f = File(pkg, data)
    try:
        rc, info = f.info(rid)
        assert rc == OK and info.n_regions == 3, f.msg()
    finally:
        f.close()


def test_mski_refused_uses(pkg, pic):
    """as a grid tile, a derived item's child, an auxiliary image, a gain map: HM_ERR_UNSUPPORTED, as for 'unci'; a short payload and
    another depth by name; all before a device is needed"""
    capi = pkg.capi
    w = Writer()
    img = w.hvc1(pic, (64, 64))
    m = w.mski(bytes(64 * 64), (64, 64), hidden=False)
    short = w.mski(bytes(37 * 21 - 1), (37, 21), hidden=False)
    g = w.grid([m, m], 1, 2, 128, 64)
    iden = w.iden([m], (64, 64))
    iovl = w.iovl([(img, 0, 0), (m, 3, 3)], (64, 64))
    aux = w.mski(bytes(64 * 64), (64, 64))
    w.assoc[aux].append(0x8000 | w._prop(struct.pack(">I4s", 12 + 27, b"auxC") + b"\0\0\0\0" + b"urn:mpeg:hevc:2015:auxid:1\0"))
    w.refs.append((b"auxl", aux, [img]))
    f = File(pkg, w.finish(primary=img))
    try:
        for iid, text in ((g, "mski"), (iden, "mski"), (iovl, "mski"), (img, "mski")):
            rc, msg = f.decode_status(iid, 10)
            assert rc == UNSUPPORTED and text in msg, (iid, rc, msg)
        rc, msg = f.decode_status(short)
        assert rc == BITSTREAM and "776" in msg, (rc, msg)
        # a gain map
        p = capi.GainParams()
        p.alternate_headroom = 2.0
        for c in range(3):
            p.map_max[c], p.gamma[c], p.base_offset[c], p.alternate_offset[c] = 2.0, 1.0, 1 / 64, 1 / 64
        gain = capi.DeviceGain(m, 1.0, p, (C.c_int32 * 4)(0, 0, 0, 0))
        lt = capi.DeviceLight(13, 1, 8, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
        dest = capi.DeviceDest(0x1000, 1 << 30, 0, capi.HM_DEV_F32, 0, 0)
        for k in range(4):
            dest.scale[k] = 1.0
        prm = capi.DecodeParams(10, 2, 0, 0, None, None, 0, 0, 0, 0)
        d = capi.Decoded()
        rc = f.L.hm_decode_item_to_device_gain(f.h, img, C.byref(prm), None, C.byref(lt), None, C.byref(gain), C.byref(dest), C.byref(d))
        assert rc == UNSUPPORTED and f.msg(), (rc, f.msg())
    finally:
        f.close()


def test_regions_dest_bytes_and_static_refusals(pkg):
    capi = pkg.capi
    L = capi.image_lib()

    def dest(dtype=0, row=0, plane=0, reserved=0):
        return capi.RegionsDest(0x1000, 1 << 30, dtype, reserved, row, plane, 1.0, 0.0)
    assert L.hm_regions_dest_bytes(capi.HM_REGIONS_STACK, 3, 67, 45, C.byref(dest())) == 3 * 67 * 45
    assert L.hm_regions_dest_bytes(capi.HM_REGIONS_STACK, 3, 67, 45, C.byref(dest(capi.HM_DEV_F32, 300, 20000))) == 2 * 20000 + 44 * 300 + 67 * 4
    assert L.hm_regions_dest_bytes(capi.HM_REGIONS_LABELS, 255, 67, 45, C.byref(dest(0, 80))) == 44 * 80 + 67
    assert L.hm_regions_dest_bytes(capi.HM_REGIONS_STACK, 0, 67, 45, C.byref(dest())) == 0
    for args, d in (((capi.HM_REGIONS_LABELS, 256, 67, 45), dest()), ((capi.HM_REGIONS_LABELS, 3, 67, 45), dest(capi.HM_DEV_F32)),
                    ((capi.HM_REGIONS_STACK, 3, 67, 45), dest(capi.HM_DEV_U16)), ((capi.HM_REGIONS_STACK, 3, 67, 45), dest(0, 66)),
                    ((capi.HM_REGIONS_STACK, 3, 67, 45), dest(capi.HM_DEV_F16, 135)), ((capi.HM_REGIONS_STACK, 3, 67, 45), dest(0, 0, 67 * 45 - 1)),
                    ((2, 3, 67, 45), dest()), ((capi.HM_REGIONS_STACK, 3, 0, 45), dest()), ((capi.HM_REGIONS_STACK, 3, 67, 45), dest(reserved=1))):
        assert L.hm_regions_dest_bytes(*args, C.byref(d)) == INVALID_ARG and L.hm_last_error(), args
    # the rasteriser's own refusals come before a device is needed
    g = capi.Region(capi.HM_REGION_RECTANGLE, 0, 0, 4, 4, 0, 0, 0)
    data = (C.c_void_p * 1)(None)
    view = capi.DeviceView(0, 0, 10, 10, 5, 5, capi.HM_VIEW_TRIANGLE)
    assert L.hm_rasterise_regions(C.byref(g), data, 1, 67, 45, C.byref(view), capi.HM_REGIONS_LABELS, C.byref(dest()), None) == INVALID_ARG
    assert "HM_VIEW_NEAREST" in L.hm_last_error().decode()
    view = capi.DeviceView(60, 0, 10, 10, 0, 0, 0)
    assert L.hm_rasterise_regions(C.byref(g), data, 1, 67, 45, C.byref(view), capi.HM_REGIONS_STACK, C.byref(dest()), None) == INVALID_ARG
    big = capi.Region(capi.HM_REGION_ELLIPSE, 0, 0, 40000, 4, 0, 0, 0)
    assert L.hm_rasterise_regions(C.byref(big), data, 1, 67, 45, None, capi.HM_REGIONS_STACK, C.byref(dest()), None) == UNSUPPORTED
    poly = capi.Region(capi.HM_REGION_POLYGON, 0, 0, 0, 0, 3, 0, 0)
    assert L.hm_rasterise_regions(C.byref(poly), data, 1, 67, 45, None, capi.HM_REGIONS_STACK, C.byref(dest()), None) == INVALID_ARG
    short = capi.Region(capi.HM_REGION_INLINE_MASK, 0, 0, 13, 5, 0, 0, 8)
    buf = C.create_string_buffer(16)
    data = (C.c_void_p * 1)(C.addressof(buf))
    assert L.hm_rasterise_regions(C.byref(short), data, 1, 67, 45, None, capi.HM_REGIONS_STACK, C.byref(dest()), None) == BITSTREAM
    small = capi.RegionsDest(0x1000, 67 * 45 - 1, 0, 0, 0, 0, 1.0, 0.0)
    assert L.hm_rasterise_regions(C.byref(g), data, 1, 67, 45, None, capi.HM_REGIONS_STACK, C.byref(small), None) == INVALID_ARG and "len" in L.hm_last_error().decode()


def test_default_size_rule(pkg):
    """decode_regions_to_tensor's argument handling: with neither crop nor size and a reference size that differs from the image's, size
    defaults to the image's; a crop in that case wants a size"""
    decode = pkg.decode
    view, w, h = decode._regions_view((200, 100), (64, 64), None, None, "triangle")
    assert (w, h) == (64, 64) and (view.crop_w, view.crop_h, view.out_w, view.out_h, view.filter) == (0, 0, 64, 64, pkg.capi.HM_VIEW_TRIANGLE)
    view, w, h = decode._regions_view((64, 64), (64, 64), None, None, "triangle")
    assert view is None and (w, h) == (64, 64)
    view, w, h = decode._regions_view((64, 64), (64, 64), (3, 5, 20, 10), None, "nearest")
    assert (w, h) == (20, 10) and (view.crop_x, view.crop_y, view.out_w) == (3, 5, 0)
    with pytest.raises(ValueError, match="reference space"):
        decode._regions_view((200, 100), (64, 64), (0, 0, 20, 10), None, "triangle")
    view, w, h = decode._regions_view((200, 100), (64, 64), (0, 0, 20, 10), (40, 20), "triangle")
    assert (w, h) == (40, 20) and (view.crop_w, view.out_w, view.out_h) == (20, 40, 20)
    view, w, h = decode._regions_view((200, 100), (64, 64), None, (50, 25), "nearest")
    assert (w, h) == (50, 25) and view.filter == pkg.capi.HM_VIEW_NEAREST
