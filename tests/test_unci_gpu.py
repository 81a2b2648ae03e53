"""GPU: ISO/IEC 23001-17 'unci' items on the device.  hm_unci_unpack against the serial model of tests/unci_ref.py, bit for bit, on
the reference's 79 fixtures and on the synthetic cases of tests/unciwriter.py - planes, interleaved pixels, sub-grids of tiles - and
the image level on top of it: hm_decode_item / hm_decode_item_to_device[_planes][_view] and the Python calls.  Every destination is
pre-filled with 0xA5 and compared whole: the samples, and 0xA5 wherever nothing may be written."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import unci_ref as U
import unciwriter as W

pytestmark = pytest.mark.gpu
OK, INVALID_ARG, UNSUPPORTED, BITSTREAM = 0, -1, -2, -3
RGB, RGBA, RRGGBB_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 14, 15
NO_COLOUR_CHAIN = 2
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "unci", "uncompressed_*.heif")))
# one fixture per family (the families: tests/test_unci.py)
ONE_PER_FAMILY = ["pix_RGB_tiled", "tile_R7G7+1B7_tiled", "row_ABGR_tiled", "comp_B16R16G16_tiled", "tile_M_tiled", "mix_YVU_420", "comp_VUY_422",
                  "pix_R5G6B5_tiled", "row_YUV_tiled", "mix_Y16U16V16_420", "comp_Y16U16V16_422"]


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def models():
    """name -> (file, desc, payload, planes, positions, consumed): the serial model, run once for every test here"""
    out = {}
    for p in FIXTURES:
        data = open(p, "rb").read()
        desc, payload = U.describe(data)
        out[os.path.basename(p)[len("uncompressed_"):-len(".heif")]] = (data, desc, payload) + U.decode(desc, payload)
    for name, desc in W.cases().items():
        data, _, payload = W.synthetic(desc, seed=len(name))
        out[name] = (data, desc, payload) + U.decode(desc, payload)
    return out


class File:
    def __init__(self, capi, L, data):
        self.capi, self.L, self.h = capi, L, C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(self.h)) == 0, L.hm_last_error()
        self.id = L.hm_file_primary_item(self.h)

    def unci(self):
        u = self.capi.UnciInfo()
        assert self.L.hm_file_unci_info(self.h, self.id, C.byref(u)) == OK, self.L.hm_last_error()
        return u

    def close(self):
        self.L.hm_file_close(self.h)


def device_bytes(b):
    """exactly len(b) bytes of device memory holding b"""
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def unpack_planes(capi, L, u, payload, shapes, tiles=None, d_payload=None):
    """hm_unci_unpack into planes of 0xA5-filled rows with 8 spare bytes each -> [array or None] * 4; shapes[p] = (h, w, depth) or None"""
    import torch
    src = d_payload if d_payload is not None else device_bytes(payload)
    planes, bufs = capi.Planes(), [None] * 4
    for p, s in enumerate(shapes):
        if s is None:
            continue
        h, w, depth = s
        stride = ((w * (2 if depth > 8 else 1) + 3) & ~3) + 8
        bufs[p] = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
        planes.plane[p], planes.stride[p] = bufs[p].data_ptr(), stride
    t = (C.c_int32 * 4)(*tiles) if tiles else None
    rc = L.hm_unci_unpack(C.byref(u), src.data_ptr(), len(payload), C.byref(t) if tiles else None, C.byref(planes), 0, None, None)
    assert rc == OK, L.hm_last_error()
    torch.cuda.synchronize()
    out = [None] * 4
    for p, s in enumerate(shapes):
        if s is None:
            continue
        h, w, depth = s
        raw = bufs[p].cpu().numpy()
        row = w * (2 if depth > 8 else 1)
        assert (raw[:, (row + 3) & ~3:] == 0xA5).all(), "bytes behind the row's last dword were written"
        assert (raw[:, row:(row + 3) & ~3] == 0).all(), "the padding of the row's last dword is not zero"
        out[p] = raw[:, :row].copy().view(np.uint16 if depth > 8 else np.uint8)
    return out


def shapes_of(desc, ref):
    depth = {}
    base = {0: U.MONO, 1: U.Y, 2: U.R}[U.colour_space(desc)]
    for t, d, _ in desc["components"]:
        if t == U.ALPHA:
            depth[3] = d
        elif t != U.PADDED:
            depth[t - base] = d
    return [None if r is None else r.shape + (depth[p],) for p, r in enumerate(ref)]


def test_unpack_planes_are_the_models_on_every_fixture_and_case(capi, L, models):
    for name, (data, desc, payload, planes, where, used) in models.items():
        f = File(capi, L, data)
        u = f.unci()
        ref = U.output_planes(desc, planes)
        got = unpack_planes(capi, L, u, payload, shapes_of(desc, ref))
        for p in range(4):
            assert (ref[p] is None) == (got[p] is None), name
            if ref[p] is not None:
                assert np.array_equal(got[p].astype(np.uint16), ref[p]), (name, p, np.argwhere(got[p] != ref[p])[:4])
        f.close()


def test_payload_that_ends_with_its_allocation_and_one_that_is_short(capi, L, models):
    import torch
    for name in ("pixel_5_16_4", "depths_1_3_9_pixel", "wide_1030x3", "tall_3x1030"):
        data, desc, payload, planes, where, used = models[name]
        f = File(capi, L, data)
        u = f.unci()
        ref = U.output_planes(desc, planes)
        # the tensor holds the payload and nothing else; where the length allows an aligned start the payload also ENDS the storage
        n = len(payload)
        if n % 4 == 0:
            store = torch.full((((n + 511) // 512) * 512,), 0xA5, dtype=torch.uint8, device="cuda")
            d = store[store.numel() - n:]
            d.copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        else:
            d = device_bytes(payload)
        got = unpack_planes(capi, L, u, payload, shapes_of(desc, ref), d_payload=d)
        assert all(r is None or np.array_equal(g.astype(np.uint16), r) for g, r in zip(got, ref)), name
        # one byte short: refused before a launch, nothing written
        planes_arg, buf = capi.Planes(), torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
        for p in range(3):
            planes_arg.plane[p], planes_arg.stride[p] = buf.data_ptr(), 4096
        assert L.hm_unci_unpack(C.byref(u), d.data_ptr(), n - 1, None, C.byref(planes_arg), 0, None, None) == BITSTREAM
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all())
        f.close()
    assert sum(len(models[n][2]) % 4 != 0 for n in ("pixel_5_16_4", "depths_1_3_9_pixel", "wide_1030x3", "tall_3x1030")) >= 1  # (the tail path is taken)


def interleaved_dest(capi, w, h, channels, wide, pad=12):
    import torch
    pitch = w * channels * (2 if wide else 1) + pad
    buf = torch.full((h * pitch + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, pitch, capi.DeviceDest(buf.data_ptr(), h * pitch, capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U16 if wide else capi.HM_DEV_U8, pitch, 0)


def expected_interleaved(ref, pitch, total):
    """the whole buffer: rows of `ref` (h x w x c) at `pitch`, 0xA5 everywhere else"""
    exp = np.full(total, 0xA5, np.uint8)
    h = ref.shape[0]
    rows = np.ascontiguousarray(ref).view(np.uint8).reshape(h, -1)
    for y in range(h):
        exp[y * pitch:y * pitch + rows.shape[1]] = rows[y]
    return exp


def test_interleaved_output_equals_planes_and_interleave(capi, L, models):
    import torch
    tried = 0
    for name, (data, desc, payload, planes, where, used) in models.items():
        if U.colour_space(desc) != 2:
            continue
        depths = {d for t, d, _ in desc["components"] if t in (U.R, U.G, U.B)}
        alpha = [d for t, d, _ in desc["components"] if t == U.ALPHA]
        f = File(capi, L, data)
        u = f.unci()
        src = device_bytes(payload)
        for fmt, channels, wide in ((RGB, 3, False), (RGBA, 4, False), (RRGGBB_LE, 3, True), (RRGGBBAA_LE, 4, True)):
            bits = 16 if wide else 8
            buf, pitch, dest = interleaved_dest(capi, desc["width"], desc["height"], channels, wide, pad=13 if tried % 2 and not wide else 12)
            rc = L.hm_unci_unpack(C.byref(u), src.data_ptr(), len(payload), None, None, fmt, C.byref(dest), None)
            torch.cuda.synchronize()
            ok = depths == {bits} and (channels == 3 or not alpha or alpha == [bits])
            if ok:
                assert rc == OK, (name, fmt, L.hm_last_error())
                exp = expected_interleaved(U.interleaved(desc, planes, channels, bits), pitch, buf.numel())
                assert np.array_equal(buf.cpu().numpy(), exp), (name, fmt)
                tried += 1
            else:
                assert rc == UNSUPPORTED and L.hm_last_error_detail() == NO_COLOUR_CHAIN, (name, fmt)
                assert bool((buf == 0xA5).all())
        # a destination that is too small, a big-endian target and a float destination are refused
        buf, pitch, dest = interleaved_dest(capi, desc["width"], desc["height"], 3, False)
        need = pitch * (desc["height"] - 1) + desc["width"] * 3  # (the last-row form of hm_device_dest_bytes)
        dest.len = need - 1
        if depths == {8}:
            assert L.hm_unci_unpack(C.byref(u), src.data_ptr(), len(payload), None, None, RGB, C.byref(dest), None) == INVALID_ARG
            dest.len = need
            dest.dtype = capi.HM_DEV_F32
            assert L.hm_unci_unpack(C.byref(u), src.data_ptr(), len(payload), None, None, RGB, C.byref(dest), None) == UNSUPPORTED
        assert L.hm_unci_unpack(C.byref(u), src.data_ptr(), len(payload), None, None, RRGGBB_BE, C.byref(dest), None) == UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all())
        f.close()
    assert tried >= 40


def decode_host(capi, L, data, fmt=0, ignore_transformations=0):
    """hm_decode_item -> (status, dict(meta, planes [c] as uint8 rows cut to the plane's bytes, alpha))"""
    f = File(capi, L, data)
    prm = capi.DecodeParams(fmt, 2, ignore_transformations, 0, None, None, 0, 0, 0, 0)
    d = capi.Decoded()
    rc = L.hm_decode_item(f.h, f.id, C.byref(prm), C.byref(d))
    res = None
    if rc == OK:
        res = dict(width=d.width, height=d.height, bit_depth=d.bit_depth, chroma=d.chroma, has_alpha=d.has_alpha, has_nclx=d.has_nclx, planes=[], alpha=None)
        for c in range(3):
            if d.plane[c]:
                res["planes"].append(np.ctypeslib.as_array(d.plane[c], shape=(d.plane_height[c], d.stride[c])).copy())
        if d.alpha:
            res["alpha"] = np.ctypeslib.as_array(d.alpha, shape=(d.height, d.alpha_stride)).copy()
        L.hm_decoded_free(C.byref(d))
    f.close()
    return rc, res


def samples(rows, w, depth):
    return rows[:, :w * (2 if depth > 8 else 1)].copy().view(np.uint16 if depth > 8 else np.uint8).astype(np.uint16)


def test_decode_item_native_planes_and_interleaved_targets_per_family(capi, L, models):
    import torch
    for name in ONE_PER_FAMILY:
        data, desc, payload, planes, where, used = models[name]
        ref = U.output_planes(desc, planes)
        shapes = shapes_of(desc, ref)
        rc, got = decode_host(capi, L, data)
        assert rc == OK, (name, L.hm_last_error())
        assert (got["width"], got["height"]) == (desc["width"], desc["height"]) and got["has_nclx"] == 0
        assert got["bit_depth"] == max(s[2] for s in shapes[:3] if s) and got["has_alpha"] == int(ref[3] is not None)
        colour = [r for r in ref[:3] if r is not None]
        assert len(got["planes"]) == len(colour)
        for p, r in enumerate(colour):
            assert np.array_equal(samples(got["planes"][p], r.shape[1], shapes[p][2]), r), (name, p)
        if ref[3] is not None:
            assert np.array_equal(samples(got["alpha"], ref[3].shape[1], shapes[3][2]), ref[3]), name
        if U.colour_space(desc) != 2:
            continue
        depths = {s[2] for s in shapes[:3]}
        for fmt, channels, bits in ((RGB, 3, 8), (RGBA, 4, 8), (RRGGBB_LE, 3, 16), (RRGGBBAA_LE, 4, 16)):
            rc, got = decode_host(capi, L, data, fmt)
            buf, pitch, dest = interleaved_dest(capi, desc["width"], desc["height"], channels, bits == 16)
            f = File(capi, L, data)
            prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
            d = capi.Decoded()
            drc = L.hm_decode_item_to_device(f.h, f.id, C.byref(prm), C.byref(dest), C.byref(d))
            torch.cuda.synchronize()
            f.close()
            if depths == {bits} and (channels == 3 or ref[3] is None or shapes[3][2] == bits):
                exp = U.interleaved(desc, planes, channels, bits)
                assert rc == OK and drc == OK, (name, fmt, L.hm_last_error())
                rows = np.ascontiguousarray(exp).view(np.uint8).reshape(exp.shape[0], -1)
                assert np.array_equal(got["planes"][0][:, :rows.shape[1]], rows), (name, fmt)
                assert np.array_equal(buf.cpu().numpy(), expected_interleaved(exp, pitch, buf.numel())), (name, fmt)
            else:
                assert rc == UNSUPPORTED and drc == UNSUPPORTED and L.hm_last_error_detail() == NO_COLOUR_CHAIN, (name, fmt)
                assert bool((buf == 0xA5).all())


def test_ycbcr_unci_converts_like_the_same_planes_through_hm_colour_convert(capi, L, hm, models):
    """an 8-bit YCbCr 'unci' item to RGB: the bytes hm_colour_convert makes of the same planes (an image without nclx), which
    tests/test_colour_gpu.py holds to the reference for the planes of hvc1 pictures"""
    import torch
    for name, chroma in (("mix_YVU_420", 1), ("comp_VUY_422", 2), ("row_YUV_tiled", 3), ("yuv420_2x2_mixed", 1)):
        data, desc, payload, planes, where, used = models[name]
        ref = U.output_planes(desc, planes)
        w, h = desc["width"], desc["height"]
        rc, got = decode_host(capi, L, data, RGB)
        assert rc == OK, L.hm_last_error()
        dev = []
        for r in ref[:3]:
            stride = hm.hm_plane_stride(r.shape[1], 1)
            t = torch.zeros((max(r.shape[0], 64), stride), dtype=torch.uint8, device="cuda")
            t[:r.shape[0], :r.shape[1]] = torch.from_numpy(r.astype(np.uint8)).cuda()
            dev.append((t, stride))
        ostride = hm.hm_plane_stride(w, 3)
        out = torch.zeros((max(h, 64), ostride), dtype=torch.uint8, device="cuda")
        cd = capi.ColourDesc(w, h, 8, chroma, 0, 2, 2, 1, RGB, dev[0][1], dev[1][1], dev[2][1], ostride, 0, 0)
        assert hm.hm_colour_convert(C.byref(cd), dev[0][0].data_ptr(), dev[1][0].data_ptr(), dev[2][0].data_ptr(), out.data_ptr(), None) == OK
        torch.cuda.synchronize()
        assert np.array_equal(got["planes"][0][:h, :w * 3], out.cpu().numpy()[:h, :w * 3]), name


def test_deep_ycbcr_is_handed_out_as_coded_only(capi, L, models):
    for name in ("mix_Y16U16V16_420", "comp_Y16U16V16_422"):
        for fmt in (RGB, RRGGBB_LE, 0x103):
            rc, _ = decode_host(capi, L, models[name][0], fmt)
            assert rc == UNSUPPORTED, (name, fmt)
    rc, _ = decode_host(capi, L, models["comp_RGB"][0], 0x103)  # an R G B item has no chroma format to ask for
    assert rc == UNSUPPORTED


def test_view_takes_the_touched_tiles_and_gives_the_full_decodes_rectangle(capi, L, models):
    import torch
    # 30 x 20 fixtures of 2 x 4 internal tiles (15 x 5), in pixel, component and tile-component mode (one byte range per component)
    for name, fmt, channels in (("pix_RGB_tiled", RGB, 3), ("comp_RGB_tiled", RGB, 3), ("tile_RGB_tiled", RGBA, 4), ("tile_ABGR_tiled", RGBA, 4), ("row_YUV_tiled", RGB, 3)):
        data, desc, payload, planes, where, used = models[name]
        assert desc["tile_cols"] > 1 and desc["tile_rows"] > 1
        rc, full = decode_host(capi, L, data, fmt)
        assert rc == OK
        full = full["planes"][0][:desc["height"], :desc["width"] * channels].reshape(desc["height"], desc["width"], channels)
        f = File(capi, L, data)
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
        tw, th = desc["width"] // desc["tile_cols"], desc["height"] // desc["tile_rows"]
        for crop in ((tw + 1, th + 2, tw - 3, th - 4), (tw - 2, 1, 4, th + 3), (0, 0, desc["width"], desc["height"])):
            view = capi.DeviceView(crop[0], crop[1], crop[2], crop[3], 0, 0, 0)
            tiles = (C.c_int32 * 4)()
            assert L.hm_plan_view(f.h, f.id, C.byref(prm), C.byref(view), C.byref(tiles)) == OK
            c0, c1, r0, r1 = crop[0] // tw, (crop[0] + crop[2] - 1) // tw, crop[1] // th, (crop[1] + crop[3] - 1) // th
            assert list(tiles) == [r0, r1 - r0 + 1, c0, c1 - c0 + 1], (name, crop, list(tiles))
            buf, pitch, dest = interleaved_dest(capi, crop[2], crop[3], channels, False)
            d = capi.Decoded()
            rc = L.hm_decode_item_to_device_view(f.h, f.id, C.byref(prm), C.byref(view), C.byref(dest), C.byref(d))
            assert rc == OK, (name, crop, L.hm_last_error())
            torch.cuda.synchronize()
            exp = full[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
            assert np.array_equal(buf.cpu().numpy(), expected_interleaved(exp, pitch, buf.numel())), (name, crop)
        # the first crop lies inside one tile: fewer tiles than the item has
        view = capi.DeviceView(tw + 1, th + 2, tw - 3, th - 4, 0, 0, 0)
        tiles = (C.c_int32 * 4)()
        L.hm_plan_view(f.h, f.id, C.byref(prm), C.byref(view), C.byref(tiles))
        assert tiles[1] * tiles[3] == 1 < desc["tile_cols"] * desc["tile_rows"]
        f.close()


def test_unpack_of_a_sub_grid_takes_the_tiles_byte_ranges(capi, L, models):
    """the step alone with `tiles`: the tiles' byte ranges, cut out of the payload by the model's own read positions"""
    for name in ("pix_RGB_tiled", "tile_RGB_tiled", "depths_12_15_16_tile_component", "yuv420_2x2_mixed", "pixel_7_7p1_7"):
        data, desc, payload, planes, where, used = models[name]
        f = File(capi, L, data)
        u = f.unci()
        ref = U.output_planes(desc, planes)
        rows, cols = desc["tile_rows"], desc["tile_cols"]
        r0, nr, c0, nc = rows - 1, 1, cols - 2 if cols > 2 else 0, 2 if cols >= 2 else 1
        # a tile's bytes: from its first sample's byte to the next tile's first sample (the last tile: to the end of its unit)
        per_component = desc["interleave"] == U.TILE_COMPONENT
        starts = []  # (byte offset of the tile's data, component or -1)
        for c in (range(len(where)) if per_component else [0]):
            h, w = where[c].shape
            th, tw = h // rows, w // cols
            for ty in range(rows):
                for tx in range(cols):
                    at = min(int(where[k][ty * (where[k].shape[0] // rows), tx * (where[k].shape[1] // cols)]) for k in ([c] if per_component else range(len(where)))) // 8
                    starts.append((at, c if per_component else -1, ty, tx))
        order = sorted(starts)
        ends = {s[0]: (order[i + 1][0] if i + 1 < len(order) else len(payload)) for i, s in enumerate(order)}
        sub = b"".join(payload[at:ends[at]] for at, c, ty, tx in starts if r0 <= ty < r0 + nr and c0 <= tx < c0 + nc)
        shapes = []
        for p, r in enumerate(ref):
            if r is None:
                shapes.append(None)
                continue
            th, tw = r.shape[0] // rows, r.shape[1] // cols
            shapes.append((th * nr, tw * nc, shapes_of(desc, ref)[p][2]))
        got = unpack_planes(capi, L, u, sub, shapes, tiles=(r0, nr, c0, nc))
        for p, r in enumerate(ref):
            if r is None:
                continue
            th, tw = r.shape[0] // rows, r.shape[1] // cols
            assert np.array_equal(got[p].astype(np.uint16), r[r0 * th:(r0 + nr) * th, c0 * tw:(c0 + nc) * tw]), (name, p)
        f.close()


def transformed_file(desc, planes, props):
    import struct
    boxes = []
    for kind, v in props:
        if kind == "irot":
            boxes.append(W._box(b"irot", bytes([v])))
        elif kind == "imir":
            boxes.append(W._box(b"imir", bytes([v])))
        else:
            boxes.append(W._box(b"clap", struct.pack(">IIIIiIiI", *v)))
    return W.heif_file(desc, W.pack(desc, planes), extra_props=boxes)


def test_transformations_apply_to_unci_items(capi, L):
    """irot / imir / clap on the planes, as for any other item: RGB pixels through the planes and an interleave, YCbCr planes as coded"""
    desc = W.make_desc(12, 8, [(U.R, 8, 0), (U.G, 8, 0), (U.B, 8, 0), (U.ALPHA, 8, 0)], U.PIXEL, tile_cols=2)
    planes = W.random_planes(desc, 77)
    px = U.interleaved(desc, planes, 4, 8)
    for props, exp in (([("irot", 1)], np.rot90(px, 1)), ([("irot", 2)], np.rot90(px, 2)), ([("imir", 1)], px[:, ::-1]), ([("imir", 0)], px[::-1]),
                       ([("clap", (6, 1, 4, 1, 1, 1, 0, 1))], px[2:6, 4:10])):
        data = transformed_file(desc, planes, props)
        rc, got = decode_host(capi, L, data, RGBA)
        assert rc == OK, (props, L.hm_last_error())
        h, w = exp.shape[:2]
        assert (got["width"], got["height"]) == (w, h), props
        assert np.array_equal(got["planes"][0][:h, :w * 4].reshape(h, w, 4), exp), props
        rc, raw = decode_host(capi, L, data, RGBA, ignore_transformations=1)
        assert rc == OK and np.array_equal(raw["planes"][0][:8, :48].reshape(8, 12, 4), px)
    desc = W.make_desc(12, 8, [(U.Y, 8, 0), (U.CB, 8, 0), (U.CR, 8, 0)], U.COMPONENT, U.S_420)
    planes = W.random_planes(desc, 78)
    rc, got = decode_host(capi, L, transformed_file(desc, planes, [("irot", 1)]))
    assert rc == OK, L.hm_last_error()
    for p in range(3):
        exp = np.rot90(planes[p], 1)
        assert np.array_equal(got["planes"][p][:exp.shape[0], :exp.shape[1]], exp), p


def test_pipeline_refuses_unci_items_at_the_submit(capi, L, models):
    data = models["pix_RGB_tiled"][0]
    cfg = capi.PipelineConfig(2, 2, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    assert L.hm_pipeline_submit(pipe, data, len(data), 0, 7) == UNSUPPORTED
    assert b"unci" in L.hm_last_error()
    assert L.hm_pipeline_pending(pipe) == 0
    L.hm_pipeline_destroy(pipe)


def test_python_calls_take_unci_files(pkg, models):
    import torch
    data, desc, payload, planes, where, used = models["pix_RGB_tiled"]
    px = U.interleaved(desc, planes, 3, 8)
    t = pkg.decode.decode_to_tensor(data, out_format="rgb", layout="hwc", dtype=torch.uint8)
    assert np.array_equal(t.cpu().numpy(), px)
    t = pkg.decode.decode_to_tensor(data, out_format="rgb", layout="chw", crop=(3, 2, 20, 11))
    assert np.array_equal(t.cpu().numpy(), px[2:13, 3:23].transpose(2, 0, 1).astype(np.float32))
    r, g, b = pkg.decode.decode_to_planes(data)
    assert all(np.array_equal(x.cpu().numpy(), px[..., k]) for k, x in enumerate((r, g, b)))
    data, desc, payload, planes, where, used = models["row_ABGR_tiled"]
    out = pkg.decode.decode_to_planes(data)
    ref = U.output_planes(desc, planes)
    assert len(out) == 4 and all(np.array_equal(x.cpu().numpy(), ref[k]) for k, x in enumerate(out))
    for name in ("mix_YVU_420", "mix_Y16U16V16_420", "yuv420_10bit_2x2_mixed"):  # (16 bits: as coded is all a deep YCbCr item offers)
        data, desc, payload, planes, where, used = models[name]
        out = pkg.decode.decode_to_planes(data)
        ref = [r for r in U.output_planes(desc, planes) if r is not None]
        assert len(out) == len(ref) and all(np.array_equal(x.cpu().numpy().astype(np.uint16), ref[k]) for k, x in enumerate(out)), name
    with pytest.raises(pkg.HmError):
        pkg.decode.decode_to_planes(models["mix_Y16U16V16_420"][0], chroma="444")
    with pytest.raises(pkg.HmError):
        pkg.decode.decode_to_tensor(models["pix_R5G6B5_tiled"][0], out_format="rgb")
