"""GPU: an ICC profile as the source of the light step (HM_LIGHT_FROM_ICC: hm_icc_to_tensor, hm_decode_item_to_device_light / _gain,
hm_pipeline_submit_to_device_light and light={"from": "icc"} of the Python calls).  Everything is bit-exact: the expected image of
every case is the pixel pipeline of tests/light_ref.py (with tone_ref, alpha_ref and gain_ref on top), fed with the library's own
host tables (hm_icc_table, hm_light_table, hm_tone_table, hm_gain_table), matrix (hm_icc_matrix) and taps (hm_view_filter_taps) -
those are held to their models by the CPU tests; only the device arithmetic is under test here.  Every destination sits in a guarded
buffer pre-filled with 0xA5 and the WHOLE buffer is compared.  The profiles are writer-made (tests/icc_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import gain_ref
import gainwriter
import heifwriter
import icc_cases
import light_ref
import synthutil
import test_device_gain_gpu as dg
import test_device_out_gpu as base
import test_device_view_gpu as dv
import tone_ref
import view_filters_ref
from heifwriter import _box
from test_device_gain_gpu import lib as gain_lib  # noqa: F401  (fixtures: the library's tables, matrices and taps, each result once)
from test_device_light_gpu import lib as light_lib  # noqa: F401
from test_device_tone_gpu import lib as tone_lib  # noqa: F401

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST = 0, 1
STRAIGHT, PREMULTIPLIED, MATTE = 1, 2, 3
ICC = -1
ONE, ZERO = [1.0] * 4, [0.0] * 4
SCALE, BIAS = [2.0, 0.75, 16.0, 1.0 / 255.0], [-1.0, 0.125, 0.5, -0.25]
THREADS = 2
W, H = 40, 24
PROFILES = {"one": icc_cases.display_p3(), "three": icc_cases.three_curves(), "gray": icc_cases.gray(), "cicp": icc_cases.with_cicp(12, 13)}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


class Lin3:
    """lin of a profile as the model's lookups take it: channel c of a pixel in table c"""

    def __init__(self, tables):
        self.t = tables

    def __getitem__(self, idx):
        idx = np.asarray(idx)
        assert idx.shape[-1] == 3
        return np.stack([self.t[c][idx[..., c]] for c in range(3)], axis=-1)


@pytest.fixture(scope="module")
def lib(gain_lib, L):
    cache = {}

    class Lib(gain_lib):
        @staticmethod
        def icc_tables(name, bits, gain=1.0):
            key = ("t", name, bits, gain)
            if key not in cache:
                data, got = PROFILES[name], []
                for c in range(3):
                    out = (C.c_float * (1 << bits))()
                    assert L.hm_icc_table(data, len(data), c, bits, gain, out) == 1 << bits, L.hm_last_error().decode()
                    got.append(np.frombuffer(out, np.float32).copy())
                cache[key] = got
            return cache[key]

        @staticmethod
        def icc_matrix(name, to):
            key = ("m", name, to)
            if key not in cache:
                m = (C.c_float * 9)()
                data = PROFILES[name]
                assert L.hm_icc_matrix(data, len(data), to, C.byref(m)) == 0, L.hm_last_error().decode()
                cache[key] = np.frombuffer(m, np.float32).copy()
            return cache[key]
    return Lib


def same(got, exp, start, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - start} from the destination's start (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def light_of(capi, to_transfer=8, to_primaries=0, gain=1.0, from_transfer=ICC, from_primaries=ICC):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def pixels_of(fmt, bits, w=W, h=H, seed=0):
    """random codes with 0 and the peak in every channel, and (16-bit samples) a few words above the peak, which are read as the peak"""
    c = 3 if base.OBPP[fmt] in (3, 6) else 4
    wide = base.OBPP[fmt] >= 6
    rng = np.random.default_rng(1000 * fmt + bits + seed)
    px = rng.integers(0, 1 << bits, (h, w, c), dtype=np.uint16 if wide else np.uint8)
    for ch in range(c):
        px[1 + ch, 3, ch] = 0
        px[2 + ch, w - 2, ch] = (1 << bits) - 1
    if wide:
        px[h - 1, 5, 0], px[h - 2, 7, 1], px[h - 3, 9, 2] = 65535, 1 << bits, (1 << bits) + 77
    return px


def model(lin, bits, pixels, view, taps, enc, m, tone, alpha, dtype, sc, bi):
    """the destination's values: light_ref's sums and tone_ref's finish; alpha = (mode, background): alpha_ref's sums and rule in front
    of that finish, the background's channel c through table c"""
    if alpha is None or (alpha[0] == STRAIGHT and (view is None or view[1] is None or view[2] == NEAREST)):  # (STRAIGHT without sums: the write without the step)
        r, a, resampled = light_ref.light_sums(pixels, bits, lin, view, taps)
        return tone_ref.finish(r, a, resampled, enc, m, tone, dtype, sc, bi)
    mode, background = alpha
    x, S, Sa, moved_alpha, summed = alpha_ref.sums(pixels, bits, lin, view, taps)
    b = [lin.t[c][background[c]] for c in range(3)] if mode == MATTE else None
    r = alpha_ref.rule(mode, x, S, Sa, summed, float((1 << bits) - 1), b)
    integer = dtype in (np.uint8, np.uint16)
    none = np.zeros(r.shape[:2] + (0,), np.float32)
    colour = tone_ref.finish(r, none, summed, enc, m, tone, np.float32 if not integer else dtype, sc, bi)
    if mode != MATTE:
        scf, bif = np.asarray(sc, np.float32), np.asarray(bi, np.float32)
        if summed:
            a_out = view_filters_ref.to_integer(Sa, 255 if dtype == np.uint8 else 65535) if integer else Sa * scf[3] + bif[3]
        else:
            a_out = moved_alpha.astype(np.int64) if integer else moved_alpha.astype(np.float32) * scf[3] + bif[3]
        colour = np.concatenate([colour, a_out[..., None]], axis=2)
    return colour.astype(dtype)


DOWN2 = ((3, 1, 36, 22), (18, 11), TRIANGLE)  # a triangle view down by 2, the crop at odd offsets
# name: (out_format, bits, profile, view, to_transfer, to_primaries, tone out_bits (None: no tone step), alpha (mode, background), layout, dtype, scale, bias, pad)
ALONE = {
    "rgb8_one_linear": (RGB, 8, "one", None, 8, 0, None, None, CHW, F32, SCALE, BIAS, 0),
    "rgb8_one_matrix_f16": (RGB, 8, "one", None, 8, 1, None, None, HWC, F16, SCALE, BIAS, 2),
    "rgb8_three_linear": (RGB, 8, "three", None, 8, 0, None, None, CHW, F32, ONE, ZERO, 0),
    "rgb8_three_matrix": (RGB, 8, "three", None, 8, 1, None, None, HWC, F32, SCALE, BIAS, 1),
    "rgb8_three_srgb_u8": (RGB, 8, "three", None, 13, 1, None, None, HWC, U8, ONE, ZERO, 0),
    "rgb8_three_down2": (RGB, 8, "three", DOWN2, 8, 9, None, None, CHW, F32, ONE, ZERO, 0),
    "rgb8_three_nearest": (RGB, 8, "three", (None, (29, 50), NEAREST), 13, 0, None, None, CHW, U8, ONE, ZERO, 1),
    "rgb8_three_crop_alone": (RGB, 8, "three", ((5, 3, 21, 17), None, TRIANGLE), 8, 1, None, None, HWC, F32, ONE, ZERO, 0),
    "rgb8_gray_matrix": (RGB, 8, "gray", None, 8, 1, None, None, CHW, F32, ONE, ZERO, 0),
    "rr10_one_matrix": (RRGGBB_LE, 10, "one", None, 8, 1, None, None, CHW, F32, ONE, ZERO, 0),
    "rr10_three_srgb_u16": (RRGGBB_LE, 10, "three", None, 13, 1, None, None, CHW, U16, ONE, ZERO, 0),
    "rr10_three_down2_u16": (RRGGBB_LE, 10, "three", DOWN2, 1, 0, None, None, HWC, U16, ONE, ZERO, 0),
    "rr10_three_nearest_linear": (RRGGBB_LE, 10, "three", (None, (17, 9), NEAREST), 8, 9, None, None, HWC, F16, SCALE, BIAS, 0),
    "rr10_three_tone_finish8": (RRGGBB_LE, 10, "three", None, 13, 1, 8, None, HWC, U8, ONE, ZERO, 0),
    "rr10_one_tone_finish8_nearest": (RRGGBB_LE, 10, "one", (None, (29, 50), NEAREST), 13, 1, 8, None, CHW, U8, ONE, ZERO, 0),
    "rr10_three_tone_down2": (RRGGBB_LE, 10, "three", DOWN2, 13, 1, 0, None, CHW, U16, ONE, ZERO, 0),
    "rgba8_three_premultiplied": (RGBA, 8, "three", None, 8, 1, None, (PREMULTIPLIED, None), CHW, F32, SCALE, BIAS, 0),
    "rgba8_three_matte_u8": (RGBA, 8, "three", None, 13, 0, None, (MATTE, (10, 200, 255)), HWC, U8, ONE, ZERO, 0),
    "rgba8_three_straight": (RGBA, 8, "three", None, 8, 1, None, (STRAIGHT, None), HWC, F32, SCALE, BIAS, 0),
    "rgba8_three_matte_nearest": (RGBA, 8, "three", (None, (29, 50), NEAREST), 8, 1, None, (MATTE, (0, 128, 255)), CHW, F32, ONE, ZERO, 0),
    "rrggbbaa10_three_straight_down2": (RRGGBBAA_LE, 10, "three", DOWN2, 8, 1, None, (STRAIGHT, None), CHW, F32, SCALE, BIAS, 0),
    "rrggbbaa10_three_matte_down2_u16": (RRGGBBAA_LE, 10, "three", DOWN2, 13, 0, None, (MATTE, (100, 700, 1023)), HWC, U16, ONE, ZERO, 0),
    "rrggbbaa10_three_premultiplied_down2": (RRGGBBAA_LE, 10, "three", DOWN2, 8, 0, None, (PREMULTIPLIED, None), HWC, F16, SCALE, BIAS, 1),
    "rrggbbaa10_one_matte": (RRGGBBAA_LE, 10, "one", None, 13, 1, None, (MATTE, (100, 700, 1023)), CHW, U16, ONE, ZERO, 0),
    "rr12_three_linear": (RRGGBB_LE, 12, "three", None, 8, 1, None, None, CHW, F32, ONE, ZERO, 0),   # 48 KB of tables: inside the 64 KB
    "rr12_three_srgb_u16": (RRGGBB_LE, 12, "three", None, 13, 0, None, None, HWC, U16, ONE, ZERO, 0),  # 48 + 16 KB: exactly the 64 KB
    "rr12_three_down2": (RRGGBB_LE, 12, "three", DOWN2, 13, 1, 0, None, CHW, U16, ONE, ZERO, 0),     # passes of 48 and 32 KB
}
TONE = dict(src_peak=1000.0, dst_peak=203.0, unit_nits=1000.0, out_unit_nits=203.0)


def alone_expected(lib, case, pixels, red_only=False):
    fmt, bits, prof, view, to_transfer, to_primaries, tone_bits, alpha, layout, dtype, sc, bi, pad = case
    tables = lib.icc_tables(prof, bits)
    lin = Lin3([tables[0]] * 3 if red_only else tables)
    ebits = 8 if tone_bits == 8 else bits
    enc = None if to_transfer == 8 else lib.table(to_transfer, ebits, 1.0, True)
    m = lib.icc_matrix(prof, to_primaries) if to_primaries else None
    tone = lib.tone(1.0, TONE["src_peak"], TONE["dst_peak"], TONE["unit_nits"], TONE["out_unit_nits"]) if tone_bits is not None else None
    return model(lin, bits, pixels, view, lib.taps, enc, m, tone, alpha, NP[dtype], sc, bi)


def dest_format(fmt, tone_bits, alpha):
    if alpha is not None and alpha[0] == MATTE:
        return RGB if fmt == RGBA or tone_bits == 8 else RRGGBB_LE
    return RGB if tone_bits == 8 and fmt == RRGGBB_LE else fmt


def upload(pixels, fmt):
    import torch
    h, w, _ = pixels.shape
    stride = (w * base.OBPP[fmt] + 63) // 64 * 64 + 64
    src = np.zeros((h, stride), np.uint8)
    src[:, :w * base.OBPP[fmt]] = pixels.reshape(h, -1).view(np.uint8)
    return torch.from_numpy(src).cuda(), stride


@pytest.mark.parametrize("name", list(ALONE))
def test_the_step_alone_equals_the_model(capi, L, lib, name):
    import torch
    case = ALONE[name]
    fmt, bits, prof, view, to_transfer, to_primaries, tone_bits, alpha, layout, dtype, sc, bi, pad = case
    pixels = pixels_of(fmt, bits)
    peak = (1 << bits) - 1
    assert all((pixels[..., c] == 0).any() and (pixels[..., c] == peak).any() for c in range(3)), name
    vals = alone_expected(lib, case, pixels)
    if prof == "three":
        # the census, on the model alone: looking all three channels up in the red table gives another result, in every output channel
        # that can differ - all three behind a matrix, green and blue without one.  A kernel that ignores the per-channel tables cannot pass.
        wrong = alone_expected(lib, case, pixels, red_only=True)
        t = lib.icc_tables(prof, bits)
        assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[0], t[2]) and not np.array_equal(t[1], t[2])
        for c in ((0, 1, 2) if to_primaries else (1, 2)):
            differing = np.count_nonzero(vals[..., c] != wrong[..., c])
            assert differing > vals[..., c].size // 4, (name, c, differing)
        if not to_primaries:
            assert np.array_equal(vals[..., 0], wrong[..., 0]) or alpha is not None
    oh, ow, _ = vals.shape
    dfmt = dest_format(fmt, tone_bits, alpha)
    d, g, row, plane = base.make_dest(capi, L, dfmt, layout, dtype, ow, oh, sc, bi, pad, 0)
    dsrc, stride = upload(pixels, fmt)
    data = PROFILES[prof]
    lt = light_of(capi, to_transfer=to_transfer, to_primaries=to_primaries)
    v = dv.make_view(capi, *view) if view is not None else None
    tn = capi.DeviceTone(1, tone_bits, TONE["src_peak"], TONE["dst_peak"], TONE["unit_nits"], TONE["out_unit_nits"], (C.c_int32 * 2)(0, 0)) if tone_bits is not None else None
    al = None
    if alpha is not None:
        al = capi.DeviceAlpha()
        al.mode = alpha[0]
        for c in range(3):
            al.background[c] = alpha[1][c] if alpha[1] else 0
    rc = L.hm_icc_to_tensor(fmt, bits, W, H, dsrc.data_ptr(), stride, C.byref(v) if v is not None else None, data, len(data), C.byref(lt),
                            C.byref(tn) if tn is not None else None, C.byref(al) if al is not None else None, C.byref(d), None)
    assert rc == 0, f"{name}: {L.hm_last_error().decode()}"
    torch.cuda.synchronize()
    same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, name)


def test_a_known_cicp_tag_runs_the_path_of_the_codes(capi, L, lib):
    """primaries 12 and transfer 13 in the cicp tag stand for the profile, whose curves (three distinct ones) and colorants are not read:
    the bytes are hm_light_to_tensor's with from_transfer 13 and from_primaries 12"""
    import torch
    pixels = pixels_of(RGB, 8)
    dsrc, stride = upload(pixels, RGB)
    data = PROFILES["cicp"]
    vals = light_ref.render(pixels, 8, lib.table(13, 8, 1.0, False), None, lib.matrix(12, 1), None, lib.taps, np.float32, ONE, ZERO)
    got = []
    for icc in (True, False):
        d, g, row, plane = base.make_dest(capi, L, RGB, CHW, F32, W, H, ONE, ZERO, 0, 0)
        lt = light_of(capi, to_primaries=1) if icc else light_of(capi, to_primaries=1, from_transfer=13, from_primaries=12)
        rc = (L.hm_icc_to_tensor(RGB, 8, W, H, dsrc.data_ptr(), stride, None, data, len(data), C.byref(lt), None, None, C.byref(d), None) if icc else
              L.hm_light_to_tensor(RGB, 8, W, H, dsrc.data_ptr(), stride, None, C.byref(lt), C.byref(d), None))
        assert rc == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        same(g.host(), dv.place(vals, CHW, F32, row, plane, g.size, g.start), g.start, f"cicp, through the profile: {icc}")
        got.append(g.host())
    assert np.array_equal(got[0], got[1])


def test_a_refused_request_leaves_every_byte_unwritten(capi, L):
    """the local memory of a launch, refused with real device memory behind the destination: not a byte of it is written"""
    import torch
    pixels = pixels_of(RRGGBB_LE, 12)
    dsrc, stride = upload(pixels, RRGGBB_LE)
    data = PROFILES["three"]
    d, g, _, _ = base.make_dest(capi, L, RRGGBB_LE, HWC, U16, W, H, ONE, ZERO, 0, 0)
    lt = light_of(capi, to_transfer=13)
    tn = capi.DeviceTone(1, 0, 1000.0, 203.0, 1000.0, 203.0, (C.c_int32 * 2)(0, 0))
    rc = L.hm_icc_to_tensor(RRGGBB_LE, 12, W, H, dsrc.data_ptr(), stride, None, data, len(data), C.byref(lt), C.byref(tn), None, C.byref(d), None)
    assert rc == -2 and "12-bit" in L.hm_last_error().decode(), L.hm_last_error().decode()
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()


# ---- from files ----

NCLX = (9, 16, 1, 0)  # beside the profile: it keeps deciding the YCbCr -> RGB chain (matrix 1, limited range), and only that


def _single(icc=None, colr=None):
    return heifwriter.write_heic([synthutil.picture(56100, width=96, height=64)], (96, 64), icc=icc, colr=colr)


def _grid(icc=None, colr=None):
    tiles = [synthutil.picture(56200 + t, width=64, height=64) for t in range(4)]
    return heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 128, 128), icc=icc, colr=colr)


@pytest.fixture(scope="module")
def files(hm):
    """name -> (file bytes, the host decode's pixels h x w x 3, the same file without any profile box)"""
    out = {}
    prof = PROFILES["three"]
    for name, make, kind, colr in (("single", _single, b"prof", None), ("single_nclx", _single, b"rICC", NCLX), ("grid", _grid, b"prof", None), ("grid_nclx", _grid, b"prof", NCLX)):
        data = make(icc=(kind, prof), colr=colr)
        rows, w, h = base.host_rows(hm, data, RGB, THREADS)
        out[name] = (data, rows.reshape(h, w, 3), make(colr=colr))
    assert out["single"][1].shape == (64, 96, 3) and out["grid"][1].shape == (128, 128, 3)
    assert not np.array_equal(out["single"][1], out["single_nclx"][1])  # (the nclx does decide the chain)
    return out


def item_to_device(capi, L, data, view, lt, d, fmt=RGB):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_light(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(view) if view is not None else None, C.byref(lt), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def file_expected(lib, pixels, view, to_transfer=8, to_primaries=1, dtype=np.float32, sc=ONE, bi=ZERO):
    lin = Lin3(lib.icc_tables("three", 8))
    enc = None if to_transfer == 8 else lib.table(to_transfer, 8, 1.0, True)
    return model(lin, 8, pixels, view, lib.taps, enc, lib.icc_matrix("three", to_primaries) if to_primaries else None, None, None, dtype, sc, bi)


@pytest.mark.parametrize("name", ["single", "single_nclx", "grid", "grid_nclx"])
def test_items_equal_the_model_on_the_host_decodes(capi, L, lib, files, name):
    """linear BT.709 float32 from the item's profile - whole, and under a view -, with and without an nclx beside the profile; and the
    same files with from_* = 0 give the bytes of a file without any profile box: nothing that was valid before changes"""
    data, pixels, bare = files[name]
    h, w, _ = pixels.shape
    views = (None, ((3, 1, w - 4, h - 6), ((w - 4) // 2, (h - 6) // 2), TRIANGLE), (None, (29, 50), NEAREST))
    for k, view in enumerate(views):
        layout, dtype, sc, bi, pad = ((CHW, F32, ONE, ZERO, 0), (HWC, F32, SCALE, BIAS, 1), (CHW, F16, SCALE, BIAS, 0))[k]
        vals = file_expected(lib, pixels, view, dtype=NP[dtype], sc=sc, bi=bi)
        oh, ow, _ = vals.shape
        d, g, row, plane = base.make_dest(capi, L, RGB, layout, dtype, ow, oh, sc, bi, pad, 0)
        rc, msg, out = item_to_device(capi, L, data, dv.make_view(capi, *view) if view else None, light_of(capi, to_primaries=1), d)
        assert rc == 0, f"{name}: {msg}"
        assert (out.width, out.height, out.used_ext_dst, out.out_format) == (ow, oh, 1, RGB), name
        # what the image reports is its nclx or the default, as before (a grid canvas carries none: the tiles' nclx decides their chain only)
        assert (out.transfer, out.primaries) == ((16, 9) if name == "single_nclx" else (13, 1))
        same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, f"{name} view {view}")
    # re-encoded to sRGB codes
    vals = file_expected(lib, pixels, None, to_transfer=13, dtype=np.uint8)
    d, g, row, plane = base.make_dest(capi, L, RGB, HWC, U8, w, h, ONE, ZERO, 0, 0)
    rc, msg, _ = item_to_device(capi, L, data, None, light_of(capi, to_transfer=13, to_primaries=1), d)
    assert rc == 0, msg
    same(g.host(), dv.place(vals, HWC, U8, row, plane, g.size, g.start), g.start, f"{name} re-encoded")
    # from_* = 0: the profile is not read
    got = []
    for file in (data, bare):
        d, g, row, plane = base.make_dest(capi, L, RGB, CHW, F32, w, h, ONE, ZERO, 0, 0)
        rc, msg, _ = item_to_device(capi, L, file, None, light_of(capi, to_primaries=1, from_transfer=0, from_primaries=0), d)
        assert rc == 0, msg
        got.append(g.host())
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(got[0], dv.place(file_expected(lib, pixels, None), CHW, F32, row, plane, g.size, g.start))  # (and the profile does say something else)


def test_the_pipeline_and_the_python_calls(pkg, capi, L, lib, files):
    """two files in flight through hm_pipeline_submit_to_device_light; decode_to_tensor and decode_batch_to_tensor with light={"from": "icc"};
    decode_sequence_to_tensor raises the library's refusal"""
    import moovwriter
    lt = light_of(capi, to_primaries=1)
    cfg = capi.PipelineConfig(4, 4, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        jobs = [("single_nclx", None), ("grid", ((3, 1, 124, 122), (62, 61), TRIANGLE))]
        want = [file_expected(lib, files[n][1], v) for n, v in jobs]
        dests = [base.make_dest(capi, L, RGB, CHW, F32, e.shape[1], e.shape[0], ONE, ZERO, 0, 0) for e in want]
        for k, (n, v) in enumerate(jobs):
            view = dv.make_view(capi, *v) if v else None
            data = files[n][0]
            assert L.hm_pipeline_submit_to_device_light(pipe, data, len(data), 0, k, C.byref(view) if view is not None else None, C.byref(lt), C.byref(dests[k][0])) == 0, \
                L.hm_last_error().decode()
        for k in range(2):
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0 and r.status == 0 and r.tag == k, L.hm_last_error().decode()
            d, g, row, plane = dests[k]
            same(g.host(), dv.place(want[k], CHW, F32, row, plane, g.size, g.start), g.start, f"pipeline job {k}")
            L.hm_pipeline_release(pipe, C.byref(r))
        # an item without a profile is refused at the submit: nothing is queued
        bare = files["single"][2]
        assert L.hm_pipeline_submit_to_device_light(pipe, bare, len(bare), 0, 9, None, C.byref(lt), C.byref(dests[0][0])) == -1
        assert "no ICC profile" in L.hm_last_error().decode() and L.hm_pipeline_pending(pipe) == 0
    finally:
        L.hm_pipeline_destroy(pipe)
    spec = {"from": "icc", "to_primaries": "bt709"}
    data, pixels, bare = files["single"]
    t1 = pkg.decode_to_tensor(data, light=spec)
    assert np.array_equal(t1.cpu().numpy(), file_expected(lib, pixels, None).transpose(2, 0, 1))
    gdata, gpixels, _ = files["grid_nclx"]
    t2 = pkg.decode_batch_to_tensor([gdata, gdata], size=(62, 61), crops=[(3, 1, 124, 122)] * 2, light=spec)
    e2 = file_expected(lib, gpixels, ((3, 1, 124, 122), (62, 61), TRIANGLE)).transpose(2, 0, 1)
    assert tuple(t2.shape) == (2, 3, 61, 62) and all(np.array_equal(t2[k].cpu().numpy(), e2) for k in range(2))
    with pytest.raises(pkg.HmError, match="no ICC profile"):
        pkg.decode_to_tensor(bare, light=spec)
    clip = moovwriter.write_movie([synthutil.picture(56300 + i, width=96, height=64) for i in range(2)], (96, 64))
    with pytest.raises(pkg.HmError, match="frames"):
        pkg.decode_sequence_to_tensor(clip, light=spec)


def test_a_gain_map_base_with_a_profile(hm, capi, L, lib):
    """hm_decode_item_to_device_gain on a 'tmap' file whose base image carries the profile: the base's light comes from the profile's three
    curves and colorants, the update and everything behind it is as it was - pointwise and under a triangle view"""
    w = gainwriter.Writer()
    b = w.hvc1(synthutil.picture(56401, width=64, height=64), (64, 64))
    w.assoc[b].append(w._prop(_box(b"colr", b"prof" + PROFILES["three"])))
    m = w.hvc1(synthutil.picture(56402, width=32, height=32, chroma_format=0), (32, 32), chroma_format=0, hidden=True)
    t = w.tmap(b, m, dg.GOOD_PAYLOAD, (64, 64), colr=(9, 16, 0, 1), clli=(600, 200))
    data = w.finish(primary=b)
    rows, bw, bh = base.host_rows(hm, data, RGB, THREADS, item=b)
    pixels = rows.reshape(bh, bw, 3)
    gmap, bd = dg.map_item_pixels(hm, data, m)
    assert bd == 8
    p = dg.params_of(capi, **dg.GOOD)
    kb, ka = gain_ref.offsets(dg.model_params(p), dg.SDR_GAIN)
    lin = Lin3(lib.icc_tables("three", 8, dg.SDR_GAIN))
    red = Lin3([lib.icc_tables("three", 8, dg.SDR_GAIN)[0]] * 3)
    mat = lib.icc_matrix("three", 9)
    for view, headroom, layout, dtype, sc, bi in ((None, 1.5, CHW, F32, ONE, ZERO), ((None, (30, 20), TRIANGLE), float("inf"), HWC, F16, SCALE, BIAS),
                                                  ((None, (40, 70), NEAREST), 1.0, CHW, F32, SCALE, BIAS)):
        tabs = lib.gain(p, headroom, 8)
        vals = gain_ref.render(pixels, 8, lin, gmap, 8, tabs, kb, ka, view, lib.taps, None, mat, None, NP[dtype], sc, bi)
        assert not np.array_equal(vals, gain_ref.render(pixels, 8, red, gmap, 8, tabs, kb, ka, view, lib.taps, None, mat, None, NP[dtype], sc, bi))
        oh, ow, _ = vals.shape
        d, g, row, plane = base.make_dest(capi, L, RGB, layout, dtype, ow, oh, sc, bi, 0, 0)
        lt = light_of(capi, to_primaries=9, gain=dg.SDR_GAIN)
        rc, msg, out = dg.gain_to_device(capi, L, data, t, dv.make_view(capi, *view) if view else None, lt, None, dg.gain_of(capi, capi.GainParams(), headroom, 0), d)
        assert rc == 0, msg
        same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, f"gain view {view}")
