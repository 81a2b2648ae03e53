"""CPU: derived image items at the file level - hm_file_item_kind / hm_file_overlay_info / hm_file_derived_child / hm_file_image_info
/ hm_file_top_level_images / hm_plan_overlay on files written by tests/overlaywriter.py, and every refusal of a derived item with its
status, all of which come before a device is needed (this file runs without one)."""
import ctypes as C
import struct

import pytest

import overlay_ref
import synthutil
from overlaywriter import Writer, iovl_payload

OK, INVALID_ARG, UNSUPPORTED, BITSTREAM = 0, -1, -2, -3
RGB, RGBA, RRGGBB_BE = 10, 11, 12


@pytest.fixture(scope="module")
def pics():
    return dict(p420=synthutil.picture(91001, width=64, height=64), p444=synthutil.picture(91002, width=48, height=40, chroma_format=3),
                p422=synthutil.picture(91003, width=24, height=24, chroma_format=2), mono=synthutil.picture(91004, width=24, height=24, chroma_format=0),
                p10=synthutil.picture(91005, width=24, height=24, bit_depth=10), mono10=synthutil.picture(91006, width=24, height=24, chroma_format=0, bit_depth=10))


class File:
    def __init__(self, pkg, data):
        self.capi = pkg.capi
        self.L = pkg.capi.image_lib()
        self.h = C.c_void_p()
        self.rc = self.L.hm_file_open(data, len(data), C.byref(self.h))
        assert self.rc == 0, self.L.hm_last_error()

    def kind(self, iid):
        return self.L.hm_file_item_kind(self.h, iid)

    def info(self, iid):
        i = self.capi.ImageInfo()
        rc = self.L.hm_file_image_info(self.h, iid, C.byref(i))
        return rc, i

    def top(self):
        ids = (C.c_uint32 * 64)()
        n = self.L.hm_file_top_level_images(self.h, ids, 64)
        return [ids[k] for k in range(n)]

    def decode_status(self, iid, out_format, entry="host"):
        """status and message of a decode that must be refused before any device work"""
        prm = self.capi.DecodeParams(out_format, 2, 0, 0, None, None, 0, 0, 0, 0)
        d = self.capi.Decoded()
        if entry == "host":
            rc = self.L.hm_decode_item(self.h, iid, C.byref(prm), C.byref(d))
        elif entry == "device":
            dest = self.capi.DeviceDest(0x1000, 1 << 30, 0, 0, 0, 0)
            rc = self.L.hm_decode_item_to_device(self.h, iid, C.byref(prm), C.byref(dest), C.byref(d))
        elif entry == "view":
            dest = self.capi.DeviceDest(0x1000, 1 << 30, 0, 0, 0, 0)
            view = self.capi.DeviceView(0, 0, 8, 8, 0, 0, 0)
            rc = self.L.hm_decode_item_to_device_view(self.h, iid, C.byref(prm), C.byref(view), C.byref(dest), C.byref(d))
        else:
            planes = self.capi.DevicePlanes()
            for c in range(3):
                planes.plane[c].ptr, planes.plane[c].len, planes.plane[c].row_pitch = 0x1000 * (c + 1), 1 << 20, 0
            if entry == "planes":
                rc = self.L.hm_decode_item_to_device_planes(self.h, iid, C.byref(prm), C.byref(planes), C.byref(d))
            else:
                view = self.capi.DeviceView(0, 0, 8, 8, 0, 0, 0)
                rc = self.L.hm_decode_item_to_device_planes_view(self.h, iid, C.byref(prm), C.byref(view), C.byref(planes), C.byref(d))
        return rc, self.L.hm_last_error().decode()

    def close(self):
        self.L.hm_file_close(self.h)


def test_kinds_info_and_top_level(pkg, pics):
    capi = pkg.capi
    w = Writer()
    tiles = [w.hvc1(pics["p420"], (64, 64)) for _ in range(4)]
    g = w.grid(tiles, 2, 2, 128, 100)
    a = w.hvc1(pics["p444"], (48, 40), chroma_format=3)
    aa = w.alpha(pics["mono"], (24, 24), a)
    m = w.hvc1(pics["mono"], (24, 24), chroma_format=0, hidden=True)
    inner = w.iovl([(a, 3, -2), (m, -40, 7)], (70, 53), background=(0xFFFF, 0x8000, 0x0102, 0x7777), wide=True)
    outer = w.iovl([(inner, 0, 0), (g, -2147483648, 2147483647)], (96, 80), wide=True, transforms=[("irot", 1)])
    ident = w.iden([g], (128, 100), transforms=[("clap", (100, 1, 60, 1, 0, 1, 0, 1)), ("irot", 1)])
    over_ident = w.iden([outer], (80, 96))
    lone = w.hvc1(pics["p422"], (24, 24), chroma_format=2)
    f = File(pkg, w.finish(primary=over_ident))
    try:
        assert [f.kind(i) for i in (tiles[0], g, ident, inner, aa)] == [capi.HM_ITEM_HVC1, capi.HM_ITEM_GRID, capi.HM_ITEM_IDEN, capi.HM_ITEM_IOVL, capi.HM_ITEM_HVC1]
        assert f.kind(999) == INVALID_ARG
        assert f.L.hm_file_primary_item(f.h) == over_ident
        # top level: derived items count as images; hidden items, auxiliary images and whatever a 'dimg' reference points at do not
        assert f.top() == [ident, over_ident, lone]
        o = capi.overlay_info(f.h, inner)
        assert o == dict(canvas=(70, 53), background=[0xFFFF, 0x8000, 0x0102, 0x7777], layers=[(a, 3, -2), (m, -40, 7)])
        o = capi.overlay_info(f.h, outer)
        assert o["canvas"] == (96, 80) and o["layers"] == [(inner, 0, 0), (g, -2147483648, 2147483647)]
        assert capi.derived_child(f.h, ident) == g and capi.derived_child(f.h, over_ident) == outer
        with pytest.raises(capi.HmError) as e:
            capi.derived_child(f.h, g)
        assert e.value.status == INVALID_ARG
        with pytest.raises(capi.HmError) as e:
            capi.overlay_info(f.h, ident)
        assert e.value.status == INVALID_ARG
        # handles: size from 'ispe' (then clap / irot, context.cc:810-838), depth and chroma of the first non-virtual child
        rc, i = f.info(inner)
        assert rc == 0 and (i.width, i.height, i.coded_width, i.coded_height) == (70, 53, 70, 53)
        assert (i.bit_depth, i.chroma, i.is_grid, i.has_alpha, i.has_transforms) == (8, 3, 0, 0, 0)  # (its first child has an alpha image: not the overlay)
        rc, i = f.info(outer)
        assert rc == 0 and (i.width, i.height, i.coded_width, i.coded_height, i.chroma, i.has_transforms) == (80, 96, 96, 80, 3, 1)
        rc, i = f.info(ident)
        assert rc == 0 and (i.width, i.height, i.coded_width, i.coded_height, i.bit_depth, i.chroma, i.is_grid) == (60, 100, 128, 100, 8, 1, 0)
        rc, i = f.info(over_ident)  # iden -> iovl -> iovl -> hvc1 4:4:4
        assert rc == 0 and (i.width, i.height, i.chroma) == (80, 96, 3)
        # the plan: the grid at INT32_MIN / INT32_MAX touches nothing and is not decoded; under a crop, neither is what lies outside it
        prm = capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
        assert capi.plan_overlay(f.h, outer, prm) == [True, False]
        assert capi.plan_overlay(f.h, inner, prm) == [True, False]  # (24 wide at x = -40)
        assert capi.plan_overlay(f.h, inner, prm, capi.DeviceView(0, 0, 3, 53, 0, 0, 0)) == [False, False]
        assert capi.plan_overlay(f.h, inner, prm, capi.DeviceView(50, 37, 2, 2, 0, 0, 0)) == [True, False]
        assert capi.plan_overlay(f.h, inner, prm, capi.DeviceView(51, 38, 19, 15, 0, 0, 0)) == [False, False]
        # (a transformed overlay: the crop is one of the transformed image, every layer on the canvas is decoded)
        assert capi.plan_overlay(f.h, outer, prm, capi.DeviceView(90, 70, 2, 2, 0, 0, 0)) == [True, False]
    finally:
        f.close()


@pytest.mark.parametrize("wide", [False, True])
def test_payload_through_the_library(pkg, pics, wide):
    """hm_file_overlay_info against the hand-written byte strings of test_overlay_ref.py's parser test: both field widths, truncation at
    every length, version 1, zero sizes, a count mismatch"""
    capi = pkg.capi
    offs = [(-(1 << 31), (1 << 31) - 1), (7, -70000)] if wide else [(-32768, 32767), (7, -300)]
    good = iovl_payload(offs, (70000 if wide else 96, 80), (1, 2, 3, 4), wide)

    def status(payload, n_refs=2):
        w = Writer()
        kids = [w.hvc1(pics["p444"], (48, 40), chroma_format=3) for _ in range(n_refs)]
        o = w.iovl([], (96, 80), payload=payload, refs=kids)
        f = File(pkg, w.finish(primary=o))
        try:
            info = capi.OverlayInfo()
            rc = f.L.hm_file_overlay_info(f.h, o, C.byref(info), None, None, 0)
            rc2, _ = f.info(o)
            rc3, _ = f.decode_status(o, RGB)
            return rc, rc3, f.L.hm_last_error().decode(), (capi.overlay_info(f.h, o) if rc == 0 else None), rc2
        finally:
            f.close()

    rc, _, _, o, rc2 = status(good)
    assert rc == 0 and rc2 == 0 and o["canvas"] == (70000 if wide else 96, 80) and o["background"] == [1, 2, 3, 4] and [(x, y) for _, x, y in o["layers"]] == offs
    assert overlay_ref.parse_overlay(2, good)["offsets"] == offs
    for n in range(len(good)):
        rc, rc3, msg, _, _ = status(good[:n])
        assert rc == BITSTREAM and rc3 == BITSTREAM and "incomplete" in msg, n
    assert status(good, n_refs=3)[:2] == (BITSTREAM, BITSTREAM)       # more references than offsets
    assert status(good, n_refs=1)[0] == 0                             # fewer: the tail is ignored (context.cc:343-345)
    rc, rc3, msg, _, _ = status(bytes([1]) + good[1:])
    assert rc == UNSUPPORTED and rc3 == UNSUPPORTED and "version 1" in msg
    for canvas in ((0, 80), (96, 0)):
        rc, rc3, msg, _, _ = status(iovl_payload(offs, canvas, (1, 2, 3, 4), wide))
        assert rc == BITSTREAM and rc3 == BITSTREAM and "zero width or height" in msg


def test_refusals_come_with_their_status_before_a_device_is_needed(pkg, pics):
    def one(build, out_format=RGB, entry="host"):
        w = Writer()
        primary = build(w)
        f = File(pkg, w.finish(primary=primary))
        try:
            return f.decode_status(primary, out_format, entry)
        finally:
            f.close()

    h444 = lambda w: w.hvc1(pics["p444"], (48, 40), chroma_format=3)  # noqa: E731
    h420 = lambda w: w.hvc1(pics["p420"], (64, 64))  # noqa: E731
    ovl = lambda w: w.iovl([(h444(w), 0, 0)], (96, 80))  # noqa: E731
    # ---- HM_ERR_UNSUPPORTED, each message naming its case ----
    rc, msg = one(lambda w: w.iovl([(w.hvc1(pics["p10"], (24, 24), bit_depth=10), 0, 0)], (96, 80)))
    assert rc == UNSUPPORTED and "deeper than 8 bits" in msg
    def deep_alpha(w):
        a = h444(w)
        w.alpha(pics["mono10"], (24, 24), a, bit_depth=10)
        return w.iden([a], (48, 40))
    rc, msg = one(deep_alpha)
    assert rc == UNSUPPORTED and "deeper than 8 bits" in msg
    def alpha_on_derived(w):
        o = ovl(w)
        w.alpha(pics["mono"], (24, 24), o)
        return o
    rc, msg = one(alpha_on_derived)
    assert rc == UNSUPPORTED and "alpha auxiliary image attached to the derived item" in msg
    for of, what in ((0, "out_format 0"), (0x101, "planar"), (0x103, "planar"), (RRGGBB_BE, "RRGGBB"), (13, "RRGGBB"), (14, "RRGGBB"), (15, "RRGGBB")):
        rc, msg = one(ovl, of)
        assert rc == UNSUPPORTED and "iovl" in msg and what in msg, (of, msg)
    for entry in ("planes", "planes_view"):
        rc, msg = one(ovl, 0, entry)
        assert rc == UNSUPPORTED and "device planes" in msg, (entry, msg)
    for entry in ("device", "view"):  # (an overlay to a device destination is refused for its format, not for the missing device)
        rc, msg = one(ovl, RRGGBB_BE, entry)
        assert rc == UNSUPPORTED and "iovl" in msg, (entry, msg)
    for of in (0, 0x101, 0x102, 0x103):
        rc, msg = one(lambda w: w.iden([h444(w)], (48, 40)), of)
        assert rc == UNSUPPORTED and "'iden' item over a 4:4:4" in msg, (of, msg)
    rc, msg = one(lambda w: w.iden([h444(w)], (48, 40)), 0, "planes")
    assert rc == UNSUPPORTED and "'iden' item over a 4:4:4" in msg
    rc, msg = one(lambda w: w.iden([w.iden([ovl(w)], (96, 80))], (96, 80)), 0)  # an overlay behind identity derivations stays an overlay
    assert rc == UNSUPPORTED and "iovl" in msg
    # ---- HM_ERR_BITSTREAM ----
    rc, msg = one(lambda w: w.iden([h420(w), h444(w)], (64, 64)))
    assert rc == BITSTREAM and "more than one reference" in msg
    rc, msg = one(lambda w: w.iden([], (64, 64)))
    assert rc == BITSTREAM
    def self_ref(w):
        d = w.iden([1], (64, 64))
        assert d == 1
        return d
    rc, msg = one(self_ref)
    assert rc == BITSTREAM and "referring to itself" in msg
    rc, msg = one(lambda w: w.iden([77], (64, 64)))
    assert rc == BITSTREAM and "missing item 77" in msg
    rc, msg = one(lambda w: w.iovl([(h444(w), 0, 0), (99, 1, 1)], (96, 80)))
    assert rc == BITSTREAM and "missing item 99" in msg
    def cycle(w):
        a = w.iden([2], (64, 64))      # item 1 -> 2
        b = w.iovl([(a, 0, 0)], (64, 64))  # item 2 -> 1
        assert (a, b) == (1, 2)
        return b
    rc, msg = one(cycle)
    assert rc == BITSTREAM and "cycle" in msg
    def nested(depth):
        def build(w):
            cur = h444(w)
            for _ in range(depth):
                cur = w.iovl([(cur, 0, 0)], (48, 40))
            return cur
        return build
    rc, msg = one(nested(9))
    assert rc == BITSTREAM and "nested deeper than 8" in msg
    rc, msg = one(nested(8))  # (8 levels plan; what comes back then is the missing device or a decode, not a refusal of the nesting)
    assert rc == 0 or "nested" not in msg  # (a decode that succeeds leaves the message of the refusal before it: hm_last_error is only written on failure)


def test_image_info_refusals(pkg, pics):
    w = Writer()
    d = w.iden([], (64, 64))
    cyc_a = w.iden([3], (64, 64))
    cyc_b = w.iden([2], (64, 64))
    f = File(pkg, w.finish(primary=d))
    try:
        rc, _ = f.info(d)
        assert rc == BITSTREAM and "does not reference any other image items" in f.L.hm_last_error().decode()
        assert (cyc_a, cyc_b) == (2, 3)
        rc, _ = f.info(cyc_a)
        assert rc == BITSTREAM and "nested deeper" in f.L.hm_last_error().decode()
    finally:
        f.close()
    assert struct.calcsize("i") == 4
