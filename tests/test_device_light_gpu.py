"""GPU: the light step (hm_decode_item_to_device_light, hm_decode_frames_to_device_light, hm_pipeline_submit_to_device_light,
hm_light_to_tensor and light= of the Python calls).  Everything is bit-exact: the expected image of every case is the model of
tests/light_ref.py, fed with hm_light_table's entries, hm_light_matrix's matrix and hm_view_filter_taps' weights, applied to the
rows hm_decode_item returns in host memory.  Every destination sits in a guarded buffer pre-filled with 0xA5 and the WHOLE buffer
is compared, as in test_device_view_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import light_ref
import moovwriter
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBB_LE = 10, 11, 12, 14
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
GRID = (4, 3, 181, 243)
ONE, ZERO = [1.0] * 4, [0.0] * 4
# a scale and a bias per channel, chosen so that linear light (0 .. 1, or 0 .. gain) lands on values of every magnitude
SCALE, BIAS = [2.0, 0.75, 16.0, 1.0 / 255.0], [-1.0, 0.125, 0.5, -0.25]
THREADS = 2


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def images(hm):
    """name -> (file bytes, out_format, bits of the target's samples, the host decode's pixels as h x w x c samples)"""
    tiles = [synthutil.picture(48200 + t, width=64, height=64) for t in range(12)]
    hdr = synthutil.picture(48300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)
    files = {"grid": (heifwriter.write_heic(tiles, (64, 64), grid=GRID), RGB, 8),
             "alpha_aux": (heifwriter.write_heic([synthutil.picture(48400, width=96, height=64, vui=1, full_range=1, matrix=6)], (96, 64),
                                                 aux=[(synthutil.picture(48401, width=48, height=32), (48, 32), base.ALPHA_URN)]), RGBA, 8),
             "pq2020": (heifwriter.write_heic([hdr], (160, 96), bit_depth=10, colr=(9, 16, 1, 0)), RRGGBB_LE, 10)}
    out = {}
    for name, (data, fmt, bits) in files.items():
        rows, w, h = base.host_rows(hm, data, fmt, THREADS)
        c = 3 if base.OBPP[fmt] in (3, 6) else 4
        out[name] = (data, fmt, bits, rows.reshape(h, w, c) if base.OBPP[fmt] <= 4 else rows.view("<u2").reshape(h, w, c))
    assert out["grid"][3].shape == (243, 181, 3) and out["pq2020"][3].max() <= 1023
    return out


@pytest.fixture(scope="module")
def lib(L):
    """what the model is fed with, each computed once: tables (transfer, bits, gain, encode), matrices (from, to), taps (n, m, j, filter)"""
    tables, matrices, taps = {}, {}, {}

    class Lib:
        @staticmethod
        def table(transfer, bits, gain, encode):
            key = (transfer, bits, gain, bool(encode))
            if key not in tables:
                out = (C.c_float * (1 << bits))()
                assert L.hm_light_table(transfer, bits, gain, 1 if encode else 0, out) == 1 << bits, L.hm_last_error().decode()
                tables[key] = np.frombuffer(out, np.float32).copy()
            return tables[key]

        @staticmethod
        def matrix(a, b):
            if (a, b) not in matrices:
                m = (C.c_float * 9)()
                assert L.hm_light_matrix(a, b, C.byref(m)) == 0, L.hm_last_error().decode()
                matrices[(a, b)] = np.frombuffer(m, np.float32).copy()
            return matrices[(a, b)]

        @staticmethod
        def taps(n, m, j, filt):
            key = (n, m, j, filt)
            if key not in taps:
                first = C.c_int32(-1)
                w = (C.c_float * 600)()
                cnt = L.hm_view_filter_taps(n, m, filt, j, C.byref(first), w, 600)
                assert 0 < cnt <= 600, L.hm_last_error().decode()
                taps[key] = (first.value, np.frombuffer(w, np.float32, cnt).copy())
            return taps[key]
    return Lib


def light_of(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=0, gain=1.0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def light_to_device(capi, L, data, fmt, view, lt, d, threads=THREADS):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_light(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(view) if view is not None else None, C.byref(lt), C.byref(d),
                                              C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def same(got, exp, start, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - start} from the destination's start (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def check_item(capi, L, data, fmt, view, lt, vals, layout, dtype, scale, bias, pad, what):
    """decode under (view, lt) into a guarded destination and compare the whole buffer with `vals` (oh x ow x c of the destination's dtype)"""
    oh, ow, _ = vals.shape
    d, g, row, plane = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, scale, bias, pad, 0)
    v = dv.make_view(capi, *view) if view is not None else None
    rc, msg, out = light_to_device(capi, L, data, fmt, v, lt, d)
    assert rc == 0, f"{what}: {msg}"
    assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, fmt), what
    same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
    return out


@pytest.mark.parametrize("name", ["grid", "pq2020"])
def test_round_trip_gives_the_host_decodes_bytes(capi, L, images, name):
    """to_transfer == from_transfer, no view, no matrix, the target's own integer dtype: code = |{c : enc[c] <= lin[v]}| = v.
    Code 8 is HM_LIGHT_LINEAR, which takes no integer dtype (refused: test_refusals_leave_every_byte_unwritten): its round trip is
    the float one - the sample as the fraction v / peak of the peak, rounded once from double."""
    data, fmt, bits, pixels = images[name]
    integer = U16 if bits > 8 else U8
    for code in light_ref.TRANSFERS:
        for layout, pad in ((HWC, 0), (CHW, 0), (HWC, 1), (CHW, 2)):
            if code == light_ref.LINEAR:
                fraction = (pixels.astype(np.float64) / float((1 << bits) - 1)).astype(np.float32)
                check_item(capi, L, data, fmt, None, light_of(capi, from_transfer=8, to_transfer=8), fraction, layout, F32, ONE, ZERO, pad,
                           f"{name} transfer 8 layout {layout} pad {pad}")
                continue
            check_item(capi, L, data, fmt, None, light_of(capi, from_transfer=code, to_transfer=code), pixels, layout, integer, ONE, ZERO, pad,
                       f"{name} transfer {code} layout {layout} pad {pad}")


@pytest.mark.parametrize("name", ["grid", "alpha_aux", "pq2020"])
def test_linear_light_equals_the_model(capi, L, lib, images, name):
    """f32 and f16, CHW and HWC, scale and bias per channel; the 181-wide grid takes the scalar instance (no tight row of it is a
    multiple of 16 bytes), the 96- and 160-wide images the 16-byte stores - and with padded pitches (pad 1) the scalar one as well"""
    data, fmt, bits, pixels = images[name]
    transfer = 16 if name == "pq2020" else 13
    gain = 10000.0 / 203.0 if name == "pq2020" else 1.0
    lin = lib.table(transfer, bits, gain, False)
    r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, None, lib.taps)
    out = None
    for layout in (CHW, HWC):
        for dtype in (F32, F16):
            for pad in (0, 1, 2):
                vals = light_ref.finish(r, alpha, resampled, None, None, NP[dtype], SCALE, BIAS)
                out = check_item(capi, L, data, fmt, None, light_of(capi, gain=gain), vals, layout, dtype, SCALE, BIAS, pad,
                                 f"{name} linear layout {layout} dtype {dtype} pad {pad}")
    assert (out.transfer, out.primaries) == ((16, 9) if name == "pq2020" else (13, 1))  # (what from_* == 0 resolved to)
    if name == "alpha_aux":  # the alpha plane is today's: hm_decode_item_to_device's, bit for bit
        d1, g1, _, plane = base.make_dest(capi, L, fmt, CHW, F32, 96, 64, SCALE, BIAS, 0, 0)
        d2, g2, _, _ = base.make_dest(capi, L, fmt, CHW, F32, 96, 64, SCALE, BIAS, 0, 0)
        assert light_to_device(capi, L, data, fmt, None, light_of(capi), d1)[0] == 0
        assert base.to_device(capi, L, data, fmt, d2, THREADS)[0] == 0
        a1, a2 = g1.host()[g1.start + 3 * plane:], g2.host()[g2.start + 3 * plane:]
        assert np.array_equal(a1, a2) and not np.array_equal(g1.host()[g1.start:g1.start + plane], g2.host()[g2.start:g2.start + plane])


def test_re_encoded_without_a_view_equals_the_model(capi, L, lib, images):
    """another transfer function on the way out: integers of the target's own type, and floats of the code"""
    for name, to_transfer, gain in (("grid", 1, 1.0), ("grid", 16, 203.0 / 10000.0), ("alpha_aux", 18, 1.0), ("pq2020", 13, 10000.0 / 203.0)):
        data, fmt, bits, pixels = images[name]
        integer = U16 if bits > 8 else U8
        own = 16 if name == "pq2020" else 13
        lin, enc = lib.table(own, bits, gain, False), lib.table(to_transfer, bits, gain, True)
        r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, None, lib.taps)
        codes = light_ref.finish(r, alpha, resampled, enc, None, NP[integer], ONE, ZERO)
        assert not np.array_equal(codes, pixels) and len(np.unique(codes[..., :3])) > 50, name
        for layout, dtype, sc, bi, pad in ((HWC, integer, ONE, ZERO, 0), (CHW, integer, ONE, ZERO, 1), (CHW, F16, SCALE, BIAS, 0), (HWC, F32, SCALE, BIAS, 2)):
            vals = light_ref.finish(r, alpha, resampled, enc, None, NP[dtype], sc, bi)
            check_item(capi, L, data, fmt, None, light_of(capi, to_transfer=to_transfer, gain=gain), vals, layout, dtype, sc, bi, pad,
                       f"{name} to {to_transfer} layout {layout} dtype {dtype} pad {pad}")


def test_gamut_matrix_equals_the_model(capi, L, lib, images):
    """BT.2020 -> BT.709 with the profile taken from the image, and P3 -> BT.709 through explicit from_* on the 8-bit grid"""
    for name, lt, (ft, fp, tp) in (("pq2020", light_of(capi, to_primaries=1), (16, 9, 1)),
                                   ("grid", light_of(capi, from_transfer=13, from_primaries=12, to_primaries=1), (13, 12, 1))):
        data, fmt, bits, pixels = images[name]
        lin, m = lib.table(ft, bits, 1.0, False), lib.matrix(fp, tp)
        r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, None, lib.taps)
        vals = light_ref.finish(r, alpha, resampled, None, m, np.float32, ONE, ZERO)
        assert (vals < 0).any()  # (colours outside the smaller gamut: the matrix is not a formality)
        for layout, pad in ((CHW, 0), (HWC, 0), (CHW, 1)):
            check_item(capi, L, data, fmt, None, lt, vals, layout, F32, ONE, ZERO, pad, f"{name} matrix layout {layout} pad {pad}")
    # ... and re-encoded behind the matrix: negative light clamps to code 0 by itself
    data, fmt, bits, pixels = images["pq2020"]
    lin, enc, m = lib.table(16, 10, 1.0, False), lib.table(16, 10, 1.0, True), lib.matrix(9, 1)
    vals = light_ref.render(pixels, 10, lin, enc, m, None, lib.taps, np.uint16, ONE, ZERO)
    assert (vals == 0).any() and not np.array_equal(vals, pixels)
    check_item(capi, L, data, fmt, None, light_of(capi, to_transfer=16, to_primaries=1), vals, CHW, U16, ONE, ZERO, 0, "pq2020 matrix re-encoded")


# (crop, size) of the grid: one down-sampling, one up-sampling and the one-column view of test_device_view_filters_gpu.VIEWS
GRID_VIEWS = {"whole_image": (None, (97, 50)), "up_sampling": ((7, 5, 30, 21), (77, 201)), "one_column": ((3, 5, 80, 60), (1, 9))}


@pytest.mark.parametrize("filt", [TRIANGLE, CUBIC, LANCZOS3])
def test_views_resample_light(capi, L, lib, images, filt):
    """the sums run over lin[v], then the finish: linear f32, re-encoded u8, re-encoded f16 (the grid); re-encoded u16 and the matrix on
    the sums (10 bits); the alpha channel resampled as it always was (RGBA)"""
    data, fmt, bits, pixels = images["grid"]
    lin, enc = lib.table(13, 8, 1.0, False), lib.table(13, 8, 1.0, True)
    for vname, (crop, size) in GRID_VIEWS.items():
        view = (crop, size, filt)
        r, alpha, resampled = light_ref.light_sums(pixels, 8, lin, view, lib.taps)
        assert resampled
        for e, layout, dtype, sc, bi, pad in ((None, CHW, F32, SCALE, BIAS, 0), (None, HWC, F32, SCALE, BIAS, 1), (enc, HWC, U8, ONE, ZERO, 0),
                                              (enc, CHW, U8, ONE, ZERO, 1), (enc, CHW, F16, SCALE, BIAS, 2)):
            vals = light_ref.finish(r, alpha, resampled, e, None, NP[dtype], sc, bi)
            check_item(capi, L, data, fmt, view, light_of(capi, to_transfer=8 if e is None else 13), vals, layout, dtype, sc, bi, pad,
                       f"grid {vname} filter {filt} layout {layout} dtype {dtype} pad {pad}")
    data, fmt, bits, pixels = images["pq2020"]
    lin, enc, m = lib.table(16, 10, 1.0, False), lib.table(16, 10, 1.0, True), lib.matrix(9, 1)
    for crop, size in ((None, (50, 37)), ((3, 5, 80, 60), (1, 9))):
        view = (crop, size, filt)
        r, alpha, resampled = light_ref.light_sums(pixels, 10, lin, view, lib.taps)
        for e, mm, layout, dtype in ((enc, None, HWC, U16), (enc, None, CHW, U16), (None, m, CHW, F32), (enc, m, HWC, F16)):
            vals = light_ref.finish(r, alpha, resampled, e, mm, NP[dtype], ONE, ZERO)
            lt = light_of(capi, to_transfer=8 if e is None else 16, to_primaries=0 if mm is None else 1)
            check_item(capi, L, data, fmt, view, lt, vals, layout, dtype, ONE, ZERO, 0, f"pq2020 {crop} {size} filter {filt} layout {layout} dtype {dtype}")
    data, fmt, bits, pixels = images["alpha_aux"]
    lin, enc = lib.table(13, 8, 1.0, False), lib.table(13, 8, 1.0, True)
    view = ((5, 3, 80, 50), (33, 47), filt)
    r, alpha, resampled = light_ref.light_sums(pixels, 8, lin, view, lib.taps)
    for e, layout, dtype, sc, bi in ((enc, HWC, U8, ONE, ZERO), (enc, CHW, U8, ONE, ZERO), (None, CHW, F32, SCALE, BIAS), (None, HWC, F16, SCALE, BIAS)):
        vals = light_ref.finish(r, alpha, resampled, e, None, NP[dtype], sc, bi)
        check_item(capi, L, data, fmt, view, light_of(capi, to_transfer=8 if e is None else 13), vals, layout, dtype, sc, bi, 0,
                   f"alpha_aux filter {filt} layout {layout} dtype {dtype}")


def test_nearest_and_the_crop_alone_move_light(capi, L, lib, images):
    for name in ("grid", "alpha_aux", "pq2020"):
        data, fmt, bits, pixels = images[name]
        h, w, _ = pixels.shape
        own = 16 if name == "pq2020" else 13
        integer = U16 if bits > 8 else U8
        lin, enc = lib.table(own, bits, 1.0, False), lib.table(1, bits, 1.0, True)
        for view in (((7, 5, 33, 21), None, TRIANGLE), ((w - 35, h - 23, 35, 23), None, NEAREST), (None, (77, 201), NEAREST), ((7, 5, 33, 21), (64, 9), NEAREST)):
            r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, view, lib.taps)
            assert not resampled
            for e, layout, dtype, sc, bi, pad in ((None, CHW, F32, SCALE, BIAS, 0), (None, HWC, F16, SCALE, BIAS, 1), (enc, HWC, integer, ONE, ZERO, 0),
                                                  (enc, CHW, integer, ONE, ZERO, 2)):
                vals = light_ref.finish(r, alpha, resampled, e, None, NP[dtype], sc, bi)
                check_item(capi, L, data, fmt, view, light_of(capi, to_transfer=8 if e is None else 1), vals, layout, dtype, sc, bi, pad,
                           f"{name} view {view} layout {layout} dtype {dtype} pad {pad}")


def test_a_halved_checkerboard_is_188_not_128(capi, L, lib):
    """The semantic anchor, through hm_light_to_tensor: a 64 x 64 one-pixel checkerboard of 0 / 255, halved with HM_VIEW_TRIANGLE,
    sRGB -> sRGB.  The tap sums of light are exactly 0.5 and enc[188] < 0.5 < enc[189], so the output is 188 where hm_resample_to_tensor,
    which averages code values, gives 128.  The four corner pixels are the one exception, in both: a view's windows never leave the
    crop, so the first and the last output of an axis have the three taps 3/7, 3/7, 1/7, and a corner sees 24/49 or 25/49 of white -
    186 / 189 in light, 125 / 130 in code values; along the edges the other axis still averages 3/7 and 4/7 to one half."""
    import torch
    yy, xx = np.mgrid[0:64, 0:64]
    pixels = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    src = torch.from_numpy(pixels.reshape(64, 192).copy()).cuda()
    lin, enc = lib.table(13, 8, 1.0, False), lib.table(13, 8, 1.0, True)
    assert enc[188] < 0.5 < enc[189]
    for j in range(1, 31):
        w = lib.taps(64, 32, j, TRIANGLE)[1]
        assert np.float32(w[0] + w[2]) == 0.5 and np.float32(w[1] + w[3]) == 0.5
    view = dv.make_view(capi, None, (32, 32), TRIANGLE)
    lt = light_of(capi, from_transfer=13, from_primaries=1, to_transfer=13)
    inner = np.ones((32, 32), bool)
    inner[0, 0] = inner[0, 31] = inner[31, 0] = inner[31, 31] = False
    for layout in (HWC, CHW):
        d, g, row, plane = base.make_dest(capi, L, RGB, layout, U8, 32, 32, ONE, ZERO, 0, 0)
        assert L.hm_light_to_tensor(RGB, 8, 64, 64, src.data_ptr(), 192, C.byref(view), C.byref(lt), C.byref(d), None) == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        vals = light_ref.render(pixels, 8, lin, enc, None, (None, (32, 32), TRIANGLE), lib.taps, np.uint8, ONE, ZERO)
        assert (vals[inner] == 188).all() and sorted(vals[~inner][:, 0].tolist()) == [186, 186, 189, 189]
        same(g.host(), dv.place(vals, layout, U8, row, plane, g.size, g.start), g.start, f"checkerboard in light, layout {layout}")
        d, g, row, plane = base.make_dest(capi, L, RGB, layout, U8, 32, 32, ONE, ZERO, 0, 0)
        assert L.hm_resample_to_tensor(RGB, 64, 64, src.data_ptr(), 192, C.byref(view), C.byref(d), None) == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        got = g.host()[g.start:g.start + 32 * 32 * 3]
        got = got.reshape(32, 32, 3) if layout == HWC else got.reshape(3, 32, 32).transpose(1, 2, 0)
        assert (got[inner] == 128).all() and sorted(got[~inner][:, 0].tolist()) == [125, 125, 130, 130]


@pytest.mark.parametrize("fmt,bits,w,h", [(RRGGBB_LE, 12, 131, 37), (15, 12, 64, 21), (RGBA, 8, 1001, 9)])
def test_light_to_tensor_on_random_pixels(capi, L, lib, fmt, bits, w, h):
    """hm_light_to_tensor alone: the 12-bit tables (16 KB each: the most LDS a kernel takes), every sample value - also words above the
    peak, which are read as the peak -, several blocks per row and a ragged last group, RGBA of both widths"""
    import torch
    rng = np.random.default_rng(fmt * 1000 + w)
    c = 3 if base.OBPP[fmt] in (3, 6) else 4
    wide = base.OBPP[fmt] >= 6
    pixels = rng.integers(0, 1 << bits, (h, w, c), dtype=np.uint16 if wide else np.uint8)
    if wide:
        pixels[rng.integers(0, h, 40), rng.integers(0, w, 40), rng.integers(0, c, 40)] = rng.integers(1 << bits, 65536, 40, dtype=np.uint16)
    src_stride = (w * base.OBPP[fmt] + 63) // 64 * 64 + 64
    src = np.zeros((h, src_stride), np.uint8)
    src[:, :w * base.OBPP[fmt]] = pixels.reshape(h, -1).view(np.uint8)
    dsrc = torch.from_numpy(src).cuda()
    integer = U16 if wide else U8
    gain = 4.0
    lin, enc, m = lib.table(16, bits, gain, False), lib.table(18, bits, gain, True), lib.matrix(9, 12)
    for view in (None, ((3, 1, w - 4, h - 2), (41, 11), TRIANGLE), (None, (29, 50), NEAREST)):
        r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, view, lib.taps)
        for e, mm, layout, dtype, sc, bi, pad in ((enc, None, HWC, integer, ONE, ZERO, 0), (enc, m, CHW, integer, ONE, ZERO, 1), (None, m, CHW, F32, SCALE, BIAS, 0),
                                                  (None, None, HWC, F16, SCALE, BIAS, 2), (enc, None, CHW, F32, SCALE, BIAS, 2)):
            vals = light_ref.finish(r, alpha, resampled, e, mm, NP[dtype], sc, bi)
            oh, ow, _ = vals.shape
            d, g, row, plane = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, sc, bi, pad, 0)
            lt = light_of(capi, from_transfer=16, from_primaries=9, to_transfer=8 if e is None else 18, to_primaries=0 if mm is None else 12, gain=gain)
            v = dv.make_view(capi, *view) if view is not None else None
            rc = L.hm_light_to_tensor(fmt, bits, w, h, dsrc.data_ptr(), src_stride, C.byref(v) if v is not None else None, C.byref(lt), C.byref(d), None)
            assert rc == 0, L.hm_last_error().decode()
            torch.cuda.synchronize()
            same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, f"fmt {fmt} view {view} layout {layout} dtype {dtype} pad {pad}")


def _clip():
    frames = [synthutil.picture(48500 + i, width=200, height=136, qp=30) for i in range(3)]
    return moovwriter.write_movie(frames, (200, 136))


def test_every_route_gives_the_item_calls_bytes(hm, pkg, capi, L, lib, images):
    """the pipeline form, the frames form and the three Python calls against hm_decode_item_to_device_light; and a grid view under a
    light step still entropy-decodes only the tiles the crop touches"""
    import torch
    data, fmt, bits, pixels = images["grid"]
    crop, size = (50, 100, 40, 50), (50, 40)
    view = dv.make_view(capi, crop, size, CUBIC)
    lt = light_of(capi, to_transfer=1, to_primaries=9, gain=2.0)

    def item(file, v, layout, dtype, ow, oh):
        d, g, row, plane = base.make_dest(capi, L, RGB, layout, dtype, ow, oh, SCALE, BIAS, 0, 0)
        rc, msg, _ = light_to_device(capi, L, file, RGB, v, lt, d)
        assert rc == 0, msg
        return g.host()[g.start:g.size - base.GUARD]
    # the plan: unchanged by the light step, and honoured - a damaged tile outside the crop is not looked at
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    prm = capi.DecodeParams(RGB, THREADS, 0, 0, None, None, 0, 0, 1, 0)
    t = (C.c_int32 * 4)()
    assert L.hm_plan_view(fh, L.hm_file_primary_item(fh), C.byref(prm), C.byref(view), C.byref(t)) == 0 and tuple(t) == (1, 2, 0, 2)
    L.hm_file_close(fh)
    tiles = [synthutil.picture(48200 + k, width=64, height=64) for k in range(12)]
    tiles[11] = dv._cut_short(tiles[11])
    damaged = heifwriter.write_heic(tiles, (64, 64), grid=GRID)
    want = item(data, view, CHW, F32, *size)
    assert np.array_equal(item(damaged, view, CHW, F32, *size), want)
    lin, enc, m = lib.table(13, 8, 2.0, False), lib.table(1, 8, 2.0, True), lib.matrix(1, 9)
    vals = light_ref.render(pixels, 8, lin, enc, m, (crop, size, CUBIC), lib.taps, np.float32, SCALE, BIAS)
    assert np.array_equal(want.view(np.float32).reshape(3, size[1], size[0]), vals.transpose(2, 0, 1))
    # the pipeline form: with the view, and without one
    cfg = capi.PipelineConfig(4, 4, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        jobs = [(view, CHW, F32, size[0], size[1]), (None, HWC, F16, 181, 243)]
        dests = [base.make_dest(capi, L, RGB, lay, dt, ow, oh, SCALE, BIAS, 0, 0) for _, lay, dt, ow, oh in jobs]
        for k, (v, _, _, _, _) in enumerate(jobs):
            assert L.hm_pipeline_submit_to_device_light(pipe, data, len(data), 0, k, C.byref(v) if v is not None else None, C.byref(lt), C.byref(dests[k][0])) == 0
        for k, (v, lay, dt, ow, oh) in enumerate(jobs):
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0 and r.status == 0 and r.tag == k, L.hm_last_error().decode()
            g = dests[k][1]
            assert np.array_equal(g.host()[g.start:g.size - base.GUARD], item(data, v, lay, dt, ow, oh)), k
            assert (g.host()[:g.start] == 0xA5).all() and (g.host()[-base.GUARD:] == 0xA5).all()
            L.hm_pipeline_release(pipe, C.byref(r))
    finally:
        L.hm_pipeline_destroy(pipe)
    # the frames form: three frames, one of them twice, against the item call on a single-image file of the same picture
    clip = _clip()
    ids = (C.c_uint32 * 4)(3, 1, 2, 1)
    fview = dv.make_view(capi, (10, 6, 150, 100), (40, 30), TRIANGLE)
    for v, ow, oh in ((fview, 40, 30), (None, 200, 136)):
        d0 = capi.DeviceDest()
        d0.layout, d0.dtype = CHW, F32
        per = L.hm_device_dest_bytes(RGB, ow, oh, C.byref(d0))
        g = base.Guarded(per * 4)
        dests = (capi.DeviceDest * 4)()
        for k in range(4):
            dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = g.ptr + k * per, per, CHW, F32
            for c in range(4):
                dests[k].scale[c], dests[k].bias[c] = SCALE[c], BIAS[c]
        fh = C.c_void_p()
        assert L.hm_file_open(clip, len(clip), C.byref(fh)) == 0
        try:
            prm = capi.DecodeParams(RGB, 4, 0, 0, None, None, 0, 0, 0, 0)
            out = (capi.Decoded * 4)()
            failed = C.c_int32(-2)
            rc = L.hm_decode_frames_to_device_light(fh, ids, 4, C.byref(prm), C.byref(v) if v is not None else None, C.byref(lt), dests, out, C.byref(failed))
            assert rc == 0 and failed.value == -1, L.hm_last_error().decode()
            assert all((out[k].width, out[k].height, out[k].used_ext_dst) == (ow, oh, 1) for k in range(4))
        finally:
            L.hm_file_close(fh)
        got = g.host()
        assert (got[:g.start] == 0xA5).all() and (got[g.start + 4 * per:] == 0xA5).all()
        for k, frame in enumerate((3, 1, 2, 1)):
            single = heifwriter.write_heic([synthutil.picture(48500 + frame - 1, width=200, height=136, qp=30)], (200, 136))
            assert np.array_equal(got[g.start + k * per:g.start + (k + 1) * per], item(single, v, CHW, F32, ow, oh)), (k, frame)
    # the Python calls
    spec = dict(to_transfer="bt709", to_primaries="bt2020", gain=2.0)
    t1 = pkg.decode_to_tensor(data, crop=crop, size=size, filter="bicubic", scale=SCALE, bias=BIAS, light=spec)
    assert np.array_equal(t1.cpu().numpy().tobytes(), want.tobytes())
    t2 = pkg.decode_batch_to_tensor([data, data], size=size, crops=[crop, crop], filter="bicubic", scale=SCALE, bias=BIAS, light=spec)
    assert tuple(t2.shape) == (2, 3, size[1], size[0]) and all(t2[k].cpu().numpy().tobytes() == want.tobytes() for k in range(2))
    t3 = pkg.decode_sequence_to_tensor(clip, frames=[3, 1, 2, 1], crop=(10, 6, 150, 100), size=(40, 30), scale=SCALE, bias=BIAS, light=spec)
    assert tuple(t3.shape) == (4, 3, 30, 40)
    single = heifwriter.write_heic([synthutil.picture(48500, width=200, height=136, qp=30)], (200, 136))
    assert t3[1].cpu().numpy().tobytes() == item(single, fview, CHW, F32, 40, 30).tobytes() and torch.equal(t3[1], t3[3])
    lin8 = pkg.decode_to_tensor(data, light=True)
    assert np.array_equal(lin8.cpu().numpy(), lib.table(13, 8, 1.0, False)[pixels].transpose(2, 0, 1))
    with pytest.raises(pkg.HmError, match="float dtype"):
        pkg.decode_to_tensor(data, light=True, dtype=torch.uint8, layout="hwc")


def test_refusals_leave_every_byte_unwritten(capi, L, images):
    import torch
    data, fmt, bits, pixels = images["grid"]
    hdr = images["pq2020"][0]
    # an image whose own transfer characteristics (11: IEC 61966-2-4) and primaries (8: generic film) the step does not support
    odd_transfer = heifwriter.write_heic([synthutil.picture(48600, width=96, height=64)], (96, 64), colr=(1, 11, 6, 1))
    odd_primaries = heifwriter.write_heic([synthutil.picture(48600, width=96, height=64)], (96, 64), colr=(8, 13, 6, 1))

    def refused(file, f, view, lt, d, g, status, word):
        rc, msg, _ = light_to_device(capi, L, file, f, view, lt, d)
        assert rc == status and word in msg, (rc, msg, word)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"

    def fresh(f, layout, dtype, w, h, shrink=0):
        d, g, _, _ = base.make_dest(capi, L, f, layout, dtype, w, h, ONE, ZERO, 0, 0, shrink=shrink)
        return d, g
    bad = C.c_int32 * 3
    for lt, word, status in ((light_of(capi, to_transfer=0), "transfer", -2), (light_of(capi, to_transfer=11), "transfer", -2), (light_of(capi, from_transfer=7), "transfer", -2),
                             (light_of(capi, to_primaries=3), "primaries", -2), (light_of(capi, from_primaries=22), "primaries", -2),
                             (light_of(capi, gain=0.0), "gain", -1), (light_of(capi, gain=float("nan")), "gain", -1), (light_of(capi, gain=float("-inf")), "gain", -1),
                             (capi.DeviceLight(0, 0, 8, 0, 1.0, bad(0, 1, 0)), "reserved", -1)):
        d, g = fresh(RGB, CHW, F32, 181, 243)
        refused(data, RGB, None, lt, d, g, status, word)
    for layout, dtype in ((HWC, U8), (CHW, U8)):  # linear light into integers
        d, g = fresh(RGB, layout, dtype, 181, 243)
        refused(data, RGB, None, light_of(capi), d, g, -1, "float dtype")
    d, g = fresh(RRGGBB_BE, HWC, U16, 160, 96)  # _BE, even where the bytes would only be moved
    refused(hdr, RRGGBB_BE, None, light_of(capi, to_transfer=16), d, g, -1, "_LE")
    refused(hdr, RRGGBB_BE, dv.make_view(capi, (7, 5, 33, 21), None, TRIANGLE), light_of(capi, to_transfer=16), d, g, -1, "_LE")
    # what the view and the destination checks refuse today
    d, g = fresh(RGB, CHW, F32, 50, 37, shrink=1)
    refused(data, RGB, dv.make_view(capi, None, (50, 37), TRIANGLE), light_of(capi), d, g, -1, "len")
    d, g = fresh(RGB, CHW, F32, 16, 16)
    refused(data, RGB, dv.make_view(capi, (170, 70, 30, 40), (16, 16), TRIANGLE), light_of(capi), d, g, -1, "not inside")
    d, g = fresh(RGB, CHW, F32, 181, 243, shrink=1)
    refused(data, RGB, None, light_of(capi), d, g, -1, "len")
    # the image's own profile, known only once it is decoded: from_* == 0 is refused, an explicit from_* decodes
    for file, word, explicit in ((odd_transfer, "transfer", light_of(capi, from_transfer=13)), (odd_primaries, "primaries", light_of(capi, from_primaries=1))):
        for view in (None, dv.make_view(capi, None, (40, 30), TRIANGLE)):
            ow, oh = (96, 64) if view is None else (40, 30)
            d, g = fresh(RGB, CHW, F32, ow, oh)
            refused(file, RGB, view, light_of(capi, to_primaries=1), d, g, -2, word)
            rc, msg, _ = light_to_device(capi, L, file, RGB, view, explicit, d)
            assert rc == 0, msg
            assert not (g.host()[g.start:g.start + 64] == 0xA5).all()
    # the frames form: nothing of any frame is written when the request is refused
    clip = _clip()
    d, g = fresh(RGB, CHW, F32, 200, 136)
    fh = C.c_void_p()
    assert L.hm_file_open(clip, len(clip), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        ids = (C.c_uint32 * 1)(2)
        lt = light_of(capi, to_transfer=12)
        assert L.hm_decode_frames_to_device_light(fh, ids, 1, C.byref(prm), None, C.byref(lt), C.byref(d), C.byref(out), None) == -2
    finally:
        L.hm_file_close(fh)
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()
    # ... and the library still decodes after all of that
    d, g, row, plane = base.make_dest(capi, L, RGB, HWC, U8, 181, 243, ONE, ZERO, 0, 0)
    assert light_to_device(capi, L, data, RGB, None, light_of(capi, from_transfer=4, to_transfer=4), d)[0] == 0
    same(g.host(), dv.place(pixels, HWC, U8, row, plane, g.size, g.start), g.start, "a decode after the refusals")


def test_light_kernels_use_no_scratch(pkg):
    """every instance of the light kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 9): no scratch"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(9, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 128, (n, out[0], out[1])
        n += 1
    # 48 pointwise (sample width x dtype x channels x layout x store width), 12 nearest, 8 horizontal, 16 vertical
    assert n == 84
