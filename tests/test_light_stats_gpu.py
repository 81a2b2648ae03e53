"""GPU: the light statistics (hm_light_stats_of_tensor, hm_decode_item_light_stats, hm_decode_item_to_device_measured and the Python
calls).  Equality is exact everywhere - the histogram, the pixel count, max_norm by its bit pattern, max_code, max_nits, average_nits:
the expected statistic of every case is the model of tests/light_stats_ref.py fed with the library's host tables (hm_light_table,
hm_tone_table's thr, hm_light_matrix, hm_icc_table - each held to its own model elsewhere) and ootf_ref's tables.  The measured entry
is held to the _tone / _ootf entry called with the measured peak given explicitly, byte for byte over a guarded destination."""
import ctypes as C

import numpy as np
import pytest

import hdrwriter
import heifwriter
import light_ref
import light_stats_ref as ref
import ootf_ref
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv
from test_device_light_gpu import lib as light_lib  # noqa: F401  (a fixture: hm_light_table, hm_light_matrix, each result once)
from test_device_tone_gpu import images, lib as tone_lib  # noqa: F401  (fixtures: the 160 x 96 PQ files; hm_tone_table)

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
TRIANGLE = 0
ONE, ZERO = [1.0] * 4, [0.0] * 4
THREADS = 2
F = np.float32


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def lib(tone_lib):
    """tone_lib (tables, matrices, tone tables of the library, each once) with thr(gain, unit_nits): the tone step's thresholds"""
    class Lib(tone_lib):
        @staticmethod
        def thr(gain, unit_nits):
            return tone_lib.tone(gain, 1000.0, 1000.0, unit_nits, 1000.0)[0]
    return Lib


def light_of(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=0, gain=1.0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def tone_of(capi, dst_peak, src_peak=0.0, unit_nits=0.0, out_unit_nits=0.0, out_bits=0):
    return capi.DeviceTone(1, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(0, 0))


def ootf_of(capi, peak, gamma=0.0):
    return capi.DeviceOotf(1, peak, gamma, (C.c_int32 * 5)(0, 0, 0, 0, 0))


def ref_of(x):
    return C.byref(x) if x is not None else None


def on_device(pixels, aligned):
    """the interleaved pixels (h x w x c, uint8 or uint16) in device memory with the row pitch rounded up to 16 bytes (the vector
    instance runs) or one sample wider than that (the scalar instance) -> (tensor, pointer, stride)"""
    import torch
    h, w, c = pixels.shape
    sb = pixels.dtype.itemsize
    stride = (w * c * sb + 15) // 16 * 16 + (0 if aligned else sb)
    host = np.full((h, stride), 0x5A, np.uint8)
    host[:, :w * c * sb] = pixels.reshape(h, -1).view(np.uint8)
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr(), stride


def of_tensor(capi, L, pixels, bits, lt, oo=None, unit=0.0, crop=None, aligned=True):
    fmt = {(1, 3): RGB, (1, 4): RGBA, (2, 3): RRGGBB_LE, (2, 4): RRGGBBAA_LE}[(pixels.dtype.itemsize, pixels.shape[2])]
    keep, ptr, stride = on_device(pixels, aligned)
    view = capi.DeviceView(crop[0], crop[1], crop[2], crop[3], 0, 0, TRIANGLE) if crop else None
    s = capi.LightStatsC()
    rc = L.hm_light_stats_of_tensor(fmt, bits, pixels.shape[1], pixels.shape[0], ptr, stride, ref_of(view), C.byref(lt), ref_of(oo), unit, C.byref(s), None)
    assert rc == 0, L.hm_last_error().decode()
    return s


def random_pixels(seed, bits, w, h, c):
    rng = np.random.default_rng(seed)
    dtype = np.uint8 if bits == 8 else np.uint16
    return rng.integers(0, 1 << bits, (h, w, c), dtype=dtype)  # (alpha random too: it is ignored)


# (bits, channels, from_transfer, from_primaries, to_primaries, ootf peak or None, unit_nits as given, U, gain)
STEPS = {
    "rgb from sRGB": (8, 3, 13, 1, 0, None, 203.0, 203.0, 1.0),
    "10-bit PQ": (10, 3, 16, 9, 0, None, 0.0, 10000.0, 1.0),
    "12-bit PQ, 2020 to 709": (12, 3, 16, 9, 1, None, 0.0, 10000.0, 1.0),
    "rgba from sRGB, 709 to 2020, gain 0.5": (8, 4, 13, 1, 9, None, 100.0, 100.0, 0.5),
    "rrggbbaa PQ, 2020 to 709": (10, 4, 16, 9, 1, None, 10000.0, 10000.0, 1.0),
    "10-bit HLG through the OOTF, 2020 to 709": (10, 3, 18, 9, 1, 1000.0, 0.0, 1000.0, 1.0),
    "12-bit HLG through the OOTF": (12, 4, 18, 9, 0, 600.0, 600.0, 600.0, 2.0),
}
# (w, h, crop): 1 x 1; a ragged last group and rows that are no multiple of 4; more than one wave per row; a crop at odd x, y and odd extent
SHAPES = ((1, 1, None), (67, 5, None), (1043, 5, None), (257, 131, (33, 17, 191, 101)))


def expected(lib, pixels, step, crop):
    bits, c, ft, fp, tp, peak, unit, U, gain = step
    lin = lib.table(ft, bits, gain, False)
    m = lib.matrix(fp, tp) if tp else None
    oo = ((ootf_ref.luma(fp),) + ootf_ref.tables(gain, peak)) if peak else None
    return ref.stats(pixels, bits, lin, m, oo, lib.thr(gain, U), crop, U, gain)


@pytest.mark.parametrize("name", list(STEPS))
def test_the_step_alone_on_random_codes(capi, L, lib, name):
    """every format and step at the smallest shapes where the kernel can go wrong, each with the row pitch rounded up to 16 bytes (the
    vector instance) and one sample wider (the scalar instance); the matrix 2020 -> 709 produces negative channels, which the norm passes over"""
    step = STEPS[name]
    bits, c, ft, fp, tp, peak, unit, U, gain = step
    lt = light_of(capi, ft, fp, 8, tp, gain)
    oo = ootf_of(capi, peak) if peak else None
    for w, h, crop in SHAPES:
        pixels = random_pixels(bits * 100000 + w, bits, w, h, c)
        want = expected(lib, pixels, step, crop)
        assert want["pixels"] == (crop[2] * crop[3] if crop else w * h)
        for aligned in (True, False):
            got = ref.of_struct(of_tensor(capi, L, pixels, bits, lt, oo, unit, crop, aligned))
            ref.same(got, want, f"{name} {w} x {h} crop {crop} aligned {aligned}")
    if tp == 1 and ft == 16:  # saturated 2020 colours leave the 709 gamut: channels go negative behind the matrix, and the norm is the largest
        big = random_pixels(5, bits, 257, 131, c)
        r = light_ref.gamut(lib.matrix(fp, tp), lib.table(ft, bits, gain, False)[big[..., :3].astype(np.int64)])
        assert (r < 0).any() and (r.max(axis=2) >= 0).all()


@pytest.mark.parametrize("bits,c", [(8, 3), (10, 3), (10, 4)])
def test_more_rows_than_workgroups(capi, L, lib, bits, c):
    """1024 x 1024: more tasks than the launch has waves, so the grid-stride loop and a flush from every workgroup run"""
    step = (bits, c, 16 if bits > 8 else 13, 9 if bits > 8 else 1, 1 if bits > 8 else 0, None, 10000.0, 10000.0, 1.0)
    pixels = random_pixels(1024 + bits + c, bits, 1024, 1024, c)
    want = expected(lib, pixels, step, None)
    lt = light_of(capi, step[2], step[3], 8, step[4], 1.0)
    for aligned in (True, False):
        ref.same(ref.of_struct(of_tensor(capi, L, pixels, bits, lt, None, 10000.0, None, aligned)), want, f"1024 x 1024 {bits} bits aligned {aligned}")


def test_few_workgroups_loop_over_a_small_picture(pkg, hm_hooks, lib):
    """the test library with knob stats_groups = 3: twelve waves take the 393 tasks of a 1043 x 131 ten-bit picture in turn (every wave
    loops, the last round is ragged), with 1 four waves take them all - and with 1000 workgroups most waves find no task at all; the
    numbers are the model's"""
    import torch
    T = hm_hooks
    capi = pkg.capi
    T.hm_light_stats_of_tensor.argtypes = capi.image_lib().hm_light_stats_of_tensor.argtypes
    step = STEPS["10-bit PQ"]
    pixels = random_pixels(131, 10, 1043, 131, 3)
    want = expected(lib, pixels, step, None)
    keep, ptr, stride = on_device(pixels, True)
    lt = light_of(capi, 16, 9)
    try:
        for groups in (3, 1, 1000):
            assert T.hm_debug_set(b"stats_groups", groups) == 0
            s = capi.LightStatsC()
            assert T.hm_light_stats_of_tensor(RRGGBB_LE, 10, 1043, 131, ptr, stride, None, C.byref(lt), None, 0.0, C.byref(s), None) == 0, T.hm_last_error().decode()
            ref.same(ref.of_struct(s), want, f"{groups} workgroups")
    finally:
        T.hm_debug_set(b"stats_groups", 0)
    torch.cuda.synchronize()


def test_contents_that_aim_at_the_counting(capi, L, lib):
    lt = light_of(capi, 16, 9)
    thr = lib.thr(1.0, 10000.0)
    lin = lib.table(16, 10, 1.0, False)
    # a flat picture: one bin holds every pixel (all 64 lanes of every wave on one counter)
    flat = np.full((256, 256, 3), 517, np.uint16)
    s = of_tensor(capi, L, flat, 10, lt)
    got = ref.of_struct(s)
    ref.same(got, ref.stats(flat, 10, lin, None, None, thr, None), "flat")
    assert got["hist"].max() == 65536 and np.count_nonzero(got["hist"]) == 1
    # a ramp of 12-bit codes on all three channels: every one of the 2048 bins at least once (two 12-bit codes per 11-bit bin)
    lin12 = lib.table(16, 12, 1.0, False)
    codes = np.arange(4096, dtype=np.uint16)
    ramp = np.repeat(codes.reshape(64, 64, 1), 3, axis=2)
    got = ref.of_struct(of_tensor(capi, L, ramp, 12, lt))
    ref.same(got, ref.stats(ramp, 12, lin12, None, None, thr, None), "ramp")
    assert (got["hist"] > 0).all(), np.flatnonzero(got["hist"] == 0)[:8]
    # samples above the peak of `bits`: clamped by light_in - the statistic of the clamped picture
    rng = np.random.default_rng(9)
    wild = rng.integers(0, 65536, (37, 131, 3), dtype=np.uint16)
    got = ref.of_struct(of_tensor(capi, L, wild, 10, lt))
    ref.same(got, ref.stats(np.minimum(wild, 1023), 10, lin, None, None, thr, None), "samples above the peak")
    assert got["max_code"] == 2047 and got["max_nits"] == 10000.0
    # an all-zero picture
    zero = np.zeros((5, 67, 4), np.uint16)
    got = ref.of_struct(of_tensor(capi, L, zero, 10, lt))
    assert got["max_norm"] == 0.0 and got["max_code"] == 0 and got["hist"][0] == 5 * 67 and got["max_nits"] == 0.0 and got["average_nits"] == 0.0
    ref.same(got, ref.stats(zero, 10, lin, None, None, thr, None), "zero")


def test_the_same_call_twice_gives_identical_structs(capi, L):
    pixels = random_pixels(4, 10, 1043, 37, 3)
    lt = light_of(capi, 16, 9, 8, 1)
    a, b = of_tensor(capi, L, pixels, 10, lt), of_tensor(capi, L, pixels, 10, lt)
    assert bytes(a) == bytes(b) and a.reserved[0] == 0 and a.reserved[1] == 0


def decode_stats(capi, L, data, fmt, lt, oo=None, unit=0.0, view=None):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out, s = capi.Decoded(), capi.LightStatsC()
        rc = L.hm_decode_item_light_stats(h, L.hm_file_primary_item(h), C.byref(prm), ref_of(view), C.byref(lt), ref_of(oo), unit, C.byref(s), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, s, out
    finally:
        L.hm_file_close(h)


def test_items_with_and_without_light_level_properties(capi, L, lib, images):
    """the 160 x 96 PQ files with clli, with mdcv only, with neither: the model on the host decode's pixels, the same for all three"""
    files, pixels = images
    want = ref.stats(pixels, 10, lib.table(16, 10, 1.0, False), lib.matrix(9, 1), None, lib.thr(1.0, 10000.0), None)
    structs = []
    for name in ("clli", "mdcv", "neither"):
        rc, msg, s, out = decode_stats(capi, L, files[name], RRGGBB_LE, light_of(capi, to_primaries=1))
        assert rc == 0, msg
        assert (out.width, out.height, out.transfer, out.primaries, out.bit_depth) == (160, 96, 16, 9, 10)
        ref.same(ref.of_struct(s), want, name)
        structs.append(bytes(s))
    assert structs[0] == structs[1] == structs[2]
    assert want["max_code"] > 1000 and np.count_nonzero(want["hist"]) > 100  # (the picture spreads over the codes)


@pytest.fixture(scope="module")
def grid(hm):
    """a 2 x 2 grid of 64 x 64 ten-bit PQ tiles (128 x 128), its host decode"""
    tiles = [synthutil.picture(48500 + t, width=64, height=64, bit_depth=10, full_range=0, matrix=1, primaries=1, qp=40) for t in range(4)]
    data = hdrwriter.write_hdr_heic(tiles, (64, 64), grid=(2, 2, 128, 128))
    rows, w, h = base.host_rows(hm, data, RRGGBB_LE, THREADS)
    assert (w, h) == (128, 128)
    return data, rows.view("<u2").reshape(h, w, 3)


def test_a_grid_under_a_crop(capi, L, lib, grid):
    data, pixels = grid
    crop = (71, 3, 51, 47)  # inside the upper right tile
    view = capi.DeviceView(crop[0], crop[1], crop[2], crop[3], 25, 23, TRIANGLE)  # (an output size: checked, otherwise unused)
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        tiles = (C.c_int32 * 4)()
        prm = capi.DecodeParams(RRGGBB_LE, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        assert L.hm_plan_view(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(view), C.byref(tiles)) == 0
        assert tiles[1] * tiles[3] < 4, list(tiles)  # fewer tiles than the grid has
    finally:
        L.hm_file_close(h)
    pq = light_of(capi, 16, 9)  # (a grid canvas carries no nclx: what the image reports is the default, so the codes are given)
    rc, msg, s, out = decode_stats(capi, L, data, RRGGBB_LE, pq, view=view)
    assert rc == 0, msg
    want = ref.stats(pixels, 10, lib.table(16, 10, 1.0, False), None, None, lib.thr(1.0, 10000.0), crop)
    ref.same(ref.of_struct(s), want, "grid under a crop")
    assert want["pixels"] == 51 * 47
    rc, msg, s, out = decode_stats(capi, L, data, RRGGBB_LE, pq)
    assert rc == 0, msg
    ref.same(ref.of_struct(s), ref.stats(pixels, 10, lib.table(16, 10, 1.0, False), None, None, lib.thr(1.0, 10000.0), None), "the whole grid")


def test_three_lin_tables_from_an_items_icc_profile(hm, capi, L, lib):
    """an 8-bit item whose ICC profile has three distinct curves (iccwriter): three lin tables in LDS, hm_icc_table's"""
    import test_device_icc_gpu as ig
    prof = ig.PROFILES["three"]
    data = heifwriter.write_heic([synthutil.picture(56100, width=96, height=64)], (96, 64), icc=(b"prof", prof))
    rows, w, h = base.host_rows(hm, data, RGB, THREADS)
    pixels = rows.reshape(h, w, 3)
    lin3 = []
    for c in range(3):
        out = (C.c_float * 256)()
        assert L.hm_icc_table(prof, len(prof), c, 8, 1.0, out) == 256, L.hm_last_error().decode()
        lin3.append(np.frombuffer(out, F).copy())
    lin3 = np.stack(lin3)
    assert not np.array_equal(lin3[0], lin3[1])
    m = (C.c_float * 9)()
    assert L.hm_icc_matrix(prof, len(prof), 1, C.byref(m)) == 0
    for to_primaries, mm in ((0, None), (1, np.frombuffer(m, F).copy())):
        rc, msg, s, out = decode_stats(capi, L, data, RGB, light_of(capi, -1, -1, 8, to_primaries), unit=203.0)
        assert rc == 0, msg
        ref.same(ref.of_struct(s), ref.stats(pixels, 8, lin3, mm, None, lib.thr(1.0, 203.0), None, 203.0), f"three curves to {to_primaries}")
    rc, msg, s, out = decode_stats(capi, L, data, RGB, light_of(capi, -1, -1, 8, 0), unit=0.0)  # (no profile says what 1.0 stands for)
    assert rc == -1 and "unit_nits must be given" in msg


def measured(capi, L, data, fmt, view, lt, oo, tn, fraction, d, with_stats=True):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out, s = capi.Decoded(), capi.LightStatsC()
        C.memset(C.byref(s), 0xA5, C.sizeof(s))
        rc = L.hm_decode_item_to_device_measured(h, L.hm_file_primary_item(h), C.byref(prm), ref_of(view), C.byref(lt), ref_of(oo), C.byref(tn), fraction, C.byref(d),
                                                 C.byref(out), C.byref(s) if with_stats else None)
        return rc, L.hm_last_error().decode(), s, out
    finally:
        L.hm_file_close(h)


def explicit(capi, L, data, fmt, view, lt, oo, tn, d):
    """hm_decode_item_to_device_ootf (without an OOTF step: the _tone entry's rule) with the peak given"""
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        if oo is None:
            rc = L.hm_decode_item_to_device_tone(h, L.hm_file_primary_item(h), C.byref(prm), ref_of(view), C.byref(lt), C.byref(tn), C.byref(d), C.byref(out))
        else:
            rc = L.hm_decode_item_to_device_ootf(h, L.hm_file_primary_item(h), C.byref(prm), ref_of(view), C.byref(lt), C.byref(oo), C.byref(tn), None, C.byref(d), C.byref(out))
        return rc, L.hm_last_error().decode(), out
    finally:
        L.hm_file_close(h)


# (view, to_transfer, to_primaries, layout, dtype, out_bits)
MEASURED = {
    "whole, linear f32": (None, 8, 1, CHW, F32, 0),
    "whole, PQ codes u16": (None, 16, 0, HWC, U16, 0),
    "the thumbnail": ((None, (50, 37), TRIANGLE), 13, 1, HWC, U8, 8),
    "a crop resized": (((7, 5, 133, 81), (64, 40), TRIANGLE), 13, 1, CHW, F16, 0),
}
DST = 100.0
FRACTION = 0.9999


@pytest.mark.parametrize("name", list(MEASURED))
def test_measured_equals_the_tone_entry_with_the_measured_peak(capi, L, lib, images, name):
    """the file with neither property: byte for byte hm_decode_item_to_device_tone with src_peak = the measured value, different from
    what the 1000 default gives, and *stats the stats call's (of the view's crop at source resolution)"""
    files, pixels = images
    data = files["neither"]
    view, to_transfer, to_primaries, layout, dtype, out_bits = MEASURED[name]
    v = dv.make_view(capi, *view) if view else None
    lt = light_of(capi, to_transfer=to_transfer, to_primaries=to_primaries)
    ow, oh = (view[1] if view and view[1] else (160, 96))
    dfmt = RGB if out_bits == 8 else RRGGBB_LE
    rc, msg, s_alone, _ = decode_stats(capi, L, data, RRGGBB_LE, lt, view=v)
    assert rc == 0, msg
    crop = view[0] if view else None
    m = lib.matrix(9, 1) if to_primaries == 1 else None
    ref.same(ref.of_struct(s_alone), ref.stats(pixels, 10, lib.table(16, 10, 1.0, False), m, None, lib.thr(1.0, 10000.0), crop), name)
    code, peak = ref.percentile(s_alone.hist, s_alone.pixels, FRACTION)
    assert 0.0 < peak <= 10000.0 and peak != 1000.0
    got = []
    for which in ("measured", "explicit", "default"):
        d, g, row, plane = base.make_dest(capi, L, dfmt, layout, dtype, ow, oh, ONE, ZERO, 0, 0)
        if which == "measured":
            rc, msg, s, out = measured(capi, L, data, RRGGBB_LE, v, lt, None, tone_of(capi, DST, out_bits=out_bits), FRACTION, d)
            assert rc == 0, msg
            assert bytes(s) == bytes(s_alone)
            assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, RRGGBB_LE)
        else:
            rc, msg, out = explicit(capi, L, data, RRGGBB_LE, v, lt, None, tone_of(capi, DST, src_peak=peak if which == "explicit" else 0.0, out_bits=out_bits), d)
            assert rc == 0, msg
        got.append(g.host())
    assert np.array_equal(got[0], got[1]), name
    assert not np.array_equal(got[0], got[2]), name  # (the 1000 cd/m2 default gives other bytes)
    assert (got[0][:base.GUARD] == 0xA5).all() and (got[0][-base.GUARD:] == 0xA5).all()
    # stats may be NULL
    d, g, _, _ = base.make_dest(capi, L, dfmt, layout, dtype, ow, oh, ONE, ZERO, 0, 0)
    rc, msg, _, _ = measured(capi, L, data, RRGGBB_LE, v, lt, None, tone_of(capi, DST, out_bits=out_bits), FRACTION, d, with_stats=False)
    assert rc == 0 and np.array_equal(g.host(), got[0]), msg


@pytest.fixture(scope="module")
def hlg(hm):
    pic = synthutil.picture(48411, width=64, height=64, bit_depth=10, full_range=0, matrix=9, primaries=9, qp=40)
    data = hdrwriter.write_hdr_heic([pic], (64, 64), colr=(9, 18, 9, 0))
    rows, w, h = base.host_rows(hm, data, RRGGBB_LE, THREADS)
    return data, rows.view("<u2").reshape(h, w, 3)


def test_measured_behind_an_ootf_step(capi, L, lib, hlg):
    """an HLG picture rendered for a 1000 cd/m2 display, its peak measured behind the OOTF step: the _ootf entry's bytes with that peak
    (src_peak 0 there would mean display_peak: other bytes)"""
    data, pixels = hlg
    peak_of_display = 1000.0
    oo = ootf_of(capi, peak_of_display)
    lt = light_of(capi, to_transfer=13, to_primaries=1)
    rc, msg, s_alone, _ = decode_stats(capi, L, data, RRGGBB_LE, lt, oo=oo)
    assert rc == 0, msg
    model_oo = (ootf_ref.luma(9),) + ootf_ref.tables(1.0, peak_of_display)
    ref.same(ref.of_struct(s_alone), ref.stats(pixels, 10, lib.table(18, 10, 1.0, False), lib.matrix(9, 1), model_oo, lib.thr(1.0, peak_of_display), None, peak_of_display), "HLG")
    code, peak = ref.percentile(s_alone.hist, s_alone.pixels, 0.99)
    assert peak != peak_of_display
    got = []
    for which in ("measured", "explicit", "default"):
        d, g, row, plane = base.make_dest(capi, L, RGB, HWC, U8, 64, 64, ONE, ZERO, 0, 0)
        if which == "measured":
            rc, msg, s, out = measured(capi, L, data, RRGGBB_LE, None, lt, oo, tone_of(capi, DST, out_bits=8), 0.99, d)
            assert rc == 0 and bytes(s) == bytes(s_alone), msg
        else:
            rc, msg, out = explicit(capi, L, data, RRGGBB_LE, None, lt, oo, tone_of(capi, DST, src_peak=peak if which == "explicit" else 0.0, out_bits=8), d)
            assert rc == 0, msg
        got.append(g.host())
    assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


def test_refusals_behind_the_decode_leave_the_destination_unwritten(capi, L, images):
    """a dst_peak whose knee lies below black for the measured peak (KS < 0: PQ(dst) / PQ(src) < 1 / 3), and a missing unit_nits on a
    picture that is not PQ: refused behind the decode, every byte of the pre-filled destination as it was"""
    files, pixels = images
    d, g, _, _ = base.make_dest(capi, L, RRGGBB_LE, HWC, F32, 160, 96, ONE, ZERO, 0, 0)
    rc, msg, s, out = measured(capi, L, files["neither"], RRGGBB_LE, None, light_of(capi), None, tone_of(capi, 0.05), 1.0, d)
    assert rc == -1 and "KS < 0" in msg, (rc, msg)
    assert (g.host() == 0xA5).all() and bytes(s) == b"\xA5" * C.sizeof(s)
    sdr = heifwriter.write_heic([synthutil.picture(61016, width=16, height=16)], (16, 16))
    d, g, _, _ = base.make_dest(capi, L, RGB, HWC, F32, 16, 16, ONE, ZERO, 0, 0)
    rc, msg, s, out = measured(capi, L, sdr, RGB, None, light_of(capi), None, tone_of(capi, 100.0), 1.0, d)
    assert rc == -1 and "unit_nits must be given" in msg, (rc, msg)
    assert (g.host() == 0xA5).all() and bytes(s) == b"\xA5" * C.sizeof(s)
    rc, msg, s, out = decode_stats(capi, L, sdr, RGB, light_of(capi))
    assert rc == -1 and "unit_nits must be given" in msg, (rc, msg)


def test_the_python_calls_give_the_c_calls_numbers_and_bytes(pkg, capi, L, images):
    import torch
    files, pixels = images
    data = files["neither"]
    rc, msg, s, _ = decode_stats(capi, L, data, RRGGBB_LE, light_of(capi, to_primaries=1))
    assert rc == 0, msg
    want = ref.of_struct(s)
    st = pkg.measure_light(data, light=dict(to_primaries="bt709"))
    assert isinstance(st, pkg.LightStats) and st.histogram.dtype == np.uint32 and st.histogram.shape == (2048,)
    py = dict(pixels=st.pixels, hist=st.histogram, max_norm=F(st.max_norm), max_code=st.max_code, max_nits=st.max_nits, average_nits=st.average_nits)
    ref.same(py, want, "measure_light")
    assert st.percentile(0.9999) == ref.percentile(want["hist"], want["pixels"], 0.9999) and st.percentile(1.0)[0] == st.max_code
    # a crop, and the tensor form on the host decode's pixels - uint16, int16, and a row stride of the tensor's own
    crop = (7, 5, 133, 81)
    rc, msg, s, _ = decode_stats(capi, L, data, RRGGBB_LE, light_of(capi), view=capi.DeviceView(*crop, 0, 0, TRIANGLE))
    assert rc == 0, msg
    st = pkg.measure_light(data, crop=crop, out_format="rrggbb_le", unit_nits=10000.0)
    assert st.pixels == 133 * 81 and np.array_equal(st.histogram, ref.of_struct(s)["hist"]) and st.max_nits == s.max_nits and st.average_nits == s.average_nits
    host = np.zeros((96, 200, 3), np.uint16)
    host[:, :160] = pixels
    wide = torch.from_numpy(host.view(np.int16)).cuda()
    for t in (wide.view(torch.uint16)[:, :160], wide[:, :160]):
        assert not t.is_contiguous()
        st2 = pkg.measure_light_of_tensor(t, 10, dict(from_transfer="pq", from_primaries="bt2020"), crop=crop)
        assert np.array_equal(st2.histogram, st.histogram) and (st2.max_norm, st2.max_code, st2.max_nits, st2.average_nits) == (st.max_norm, st.max_code, st.max_nits, st.average_nits)
    # decode_to_tensor with a measured peak: hm_decode_item_to_device_measured's bytes
    d, g, _, _ = base.make_dest(capi, L, RGB, HWC, U8, 50, 37, ONE, ZERO, 0, 0)
    lt = light_of(capi, to_transfer=13, to_primaries=1)
    rc, msg, _, _ = measured(capi, L, data, RRGGBB_LE, dv.make_view(capi, None, (50, 37), TRIANGLE), lt, None, tone_of(capi, DST, out_bits=8), 0.9999, d)
    assert rc == 0, msg
    t = pkg.decode_to_tensor(data, out_format="rrggbb_le", layout="hwc", dtype=torch.uint8, size=(50, 37), light=dict(to_transfer="srgb", to_primaries="bt709"),
                             tone=dict(dst_peak=DST, src_peak="measured", out_bits=8))
    assert t.shape == (37, 50, 3) and t.cpu().numpy().tobytes() == g.host()[g.start:g.start + 37 * 50 * 3].tobytes()
    t2 = pkg.decode_to_tensor(data, out_format="rrggbb_le", layout="hwc", dtype=torch.uint8, size=(50, 37), light=dict(to_transfer="srgb", to_primaries="bt709"),
                              tone=dict(dst_peak=DST, src_peak="measured", percentile=0.5, out_bits=8))
    assert not torch.equal(t, t2)  # (another percentile, another peak)


def test_the_new_instances_use_no_scratch_and_ask_for_lds_within_the_bound(hm_hooks):
    """every instance of k_light_stats as the loaded code object has it (test hook hm_debug_kernel_regs, code 13): no scratch; what the
    launcher asks for as dynamic LDS (hm_debug_light_lds, pass 3) stays within 64 KB for every table combination the host can resolve
    with one lin table - three tables fit at 8 and 10 bits (3 x 4 KB + 8 + 8 KB and the counters), not at 12, where the check refuses"""
    T = hm_hooks
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(13, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 128, (n, out[0], out[1])
        n += 1
    assert n == 8
    T.hm_debug_light_lds.argtypes, T.hm_debug_light_lds.restype = [C.c_int] * 5, C.c_longlong
    for bits in (8, 9, 10, 11, 12):
        for steps in (0, 1, 2, 3):
            for encode, eb in ((0, bits), (1, bits), (1, 8)):
                asked = T.hm_debug_light_lds(bits, eb, encode, steps, 3)
                assert 0 < asked <= 64 * 1024, (bits, eb, encode, steps, asked)
                assert asked + 2 * 4 * (1 << bits) <= 64 * 1024 or bits == 12  # ... and two more lin tables beside it
