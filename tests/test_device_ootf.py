"""The OOTF step (hm_device_ootf), the part that needs no GPU: the system gamma, the tables and the luminance weights the library
hands out against the model (tests/ootf_ref.py, written from the header's text and BT.2100), every refusal that is decided on the
host - through hm_ootf_to_tensor and through the decode entry -, the ABI, and the Python argument."""
import ctypes as C
import inspect
import math
import subprocess

import numpy as np
import pytest

import hdrwriter
import ootf_ref
import synthutil

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_NO_DEVICE = -1, -2, -4
RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 14, 15
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)
NEW_SYMBOLS = ("hm_decode_item_to_device_ootf", "hm_decode_frames_to_device_ootf", "hm_pipeline_submit_to_device_ootf", "hm_ootf_to_tensor", "hm_ootf_gamma",
               "hm_ootf_table", "hm_ootf_luma")
W, H = 64, 64


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def ootf(capi, display_peak=1000.0, gamma=0.0, kind=1, reserved=(0, 0, 0, 0, 0)):
    return capi.DeviceOotf(kind, display_peak, gamma, (C.c_int32 * 5)(*reserved))


def tone(capi, dst_peak=203.0, src_peak=0.0, unit_nits=0.0, out_unit_nits=0.0, out_bits=0):
    return capi.DeviceTone(1, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(0, 0))


def light(capi, to_transfer=8, to_primaries=0, gain=1.0, from_transfer=18, from_primaries=9):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def alpha(capi, mode, background=(0, 0, 0)):
    return capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*background, 0), (C.c_int32 * 3)(0, 0, 0))


def dest(capi, layout, dtype, length, ptr=FAKE):
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = ptr, length, layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    return d


def ref(s):
    return C.byref(s) if s is not None else None


def lib_gamma(L, o):
    g = C.c_double(-1.0)
    assert L.hm_ootf_gamma(C.byref(o), C.byref(g)) == 0, L.hm_last_error().decode()
    return g.value


def lib_tables(L, o, gain):
    out = []
    for which in (0, 1):
        buf = (C.c_float * 1024)()
        assert L.hm_ootf_table(C.byref(o), gain, which, buf) == 1024, L.hm_last_error().decode()
        out.append(np.frombuffer(buf, np.float32).copy())
    return out


def test_the_system_gamma(capi, L):
    """BT.2100 Table 5: note 5e inside 400 .. 2000 cd/m2, note 5f outside, both 1.2 at 1000; an explicit gamma is returned as it is"""
    e = lambda p: 1.2 + 0.42 * math.log10(p / 1000.0)
    f = lambda p: 1.2 * math.pow(1.111, math.log2(p / 1000.0))
    assert e(1000.0) == 1.2 and f(1000.0) == 1.2 and lib_gamma(L, ootf(capi, 1000.0)) == 1.2
    for peak, rule in ((400.0, e), (2000.0, e), (399.0, f), (2001.0, f), (203.0, f), (4000.0, f), (600.0, e)):
        got = lib_gamma(L, ootf(capi, peak))
        assert got == rule(peak) == ootf_ref.gamma(peak), (peak, got)
    assert e(399.0) != f(399.0) and e(2001.0) != f(2001.0) and e(400.0) != f(400.0) and e(2000.0) != f(2000.0)  # (the rule that was taken shows)
    for g in (1.0, 1.2, 1.5, 0.75):
        assert lib_gamma(L, ootf(capi, 1000.0, g)) == float(np.float32(g)) == ootf_ref.gamma(1000.0, g)
    g = C.c_double()
    ok = ootf(capi)
    assert L.hm_ootf_gamma(None, C.byref(g)) == HM_ERR_INVALID_ARG and L.hm_ootf_gamma(C.byref(ok), None) == HM_ERR_INVALID_ARG
    for bad, word in ((ootf(capi, 0.0), "display_peak"), (ootf(capi, gamma=-1.0), "gamma"), (ootf(capi, kind=2), "kind")):
        assert L.hm_ootf_gamma(C.byref(bad), C.byref(g)) == HM_ERR_INVALID_ARG and word in L.hm_last_error().decode()


def test_tables_against_the_model(capi, L):
    """bit for bit: both sides evaluate the same expressions in double with the C library's functions and round once"""
    for peak, gamma in ((1000.0, 0.0), (203.0, 0.0), (400.0, 0.0), (4000.0, 0.0), (1000.0, 1.5)):
        for gain in (1.0, 0.5, 12.0):
            got = lib_tables(L, ootf(capi, peak, gamma), gain)
            want = ootf_ref.tables(gain, peak, gamma)
            for name, a, b in zip(("thr", "sg"), got, want):
                assert a.shape == b.shape == (1024,) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (peak, gamma, gain, name, np.flatnonzero(a != b)[:4])
            thr, sg = got
            assert thr[0] == 0.0 and (np.diff(thr) > 0).all() and sg[0] == sg[1] and np.isfinite(sg).all() and (sg > 0).all(), (peak, gain)
            if ootf_ref.gamma(peak, gamma) > 1.0:
                assert (np.diff(sg[1:]) > 0).all() and sg[1023] == 1.0  # (F(1) = 1: the peak of the scene is the peak of the display)
    # gamma = 1: the identity
    assert (lib_tables(L, ootf(capi, 1000.0, 1.0), 1.0)[1] == 1.0).all() and (ootf_ref.tables(1.0, 1000.0, 1.0)[1] == 1.0).all()
    # the accuracy the header states: one step above E' = 0.5 changes the factor by about 0.11 % at gamma - 1 = 0.2
    sg = lib_tables(L, ootf(capi, 1000.0), 1.0)[1].astype(np.float64)
    steps = sg[513:] / sg[512:-1] - 1.0
    assert 0.0010 < steps.max() < 0.0012, steps.max()
    out = (C.c_float * 1024)()
    ok = ootf(capi)
    assert L.hm_ootf_table(None, 1.0, 0, out) == HM_ERR_INVALID_ARG and L.hm_ootf_table(C.byref(ok), 1.0, 0, None) == HM_ERR_INVALID_ARG
    assert L.hm_ootf_table(C.byref(ok), 1.0, 2, out) == HM_ERR_INVALID_ARG
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert L.hm_ootf_table(C.byref(ok), g, 0, out) == HM_ERR_INVALID_ARG, g
    for bad, word in ((ootf(capi, float("nan")), "display_peak"), (ootf(capi, 10001.0), "display_peak"), (ootf(capi, gamma=float("inf")), "gamma"),
                      (ootf(capi, reserved=(0, 0, 0, 0, 1)), "reserved"), (ootf(capi, kind=0), "kind")):
        assert L.hm_ootf_table(C.byref(bad), 1.0, 1, out) == HM_ERR_INVALID_ARG and word in L.hm_last_error().decode(), word


def test_luminance_weights(capi, L):
    for primaries in (1, 9, 12, 5, 6):
        y = (C.c_float * 3)()
        assert L.hm_ootf_luma(primaries, C.byref(y)) == 0
        got, want = np.array(list(y), np.float32), ootf_ref.luma(primaries)
        assert np.array_equal(got, want), (primaries, got, want)
        assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6  # (the white has Y = 1)
    y = (C.c_float * 3)()
    assert L.hm_ootf_luma(9, C.byref(y)) == 0
    assert np.abs(np.array(list(y)) - np.array([0.2627, 0.6780, 0.0593])).max() < 1e-4
    assert L.hm_ootf_luma(1, C.byref(y)) == 0
    assert np.abs(np.array(list(y)) - np.array([0.2126, 0.7152, 0.0722])).max() < 1e-4
    for bad in (0, 2, 3, 22):
        assert L.hm_ootf_luma(bad, C.byref(y)) == HM_ERR_UNSUPPORTED and "primaries" in L.hm_last_error().decode()
    assert L.hm_ootf_luma(9, None) == HM_ERR_INVALID_ARG


def refusal_cases(capi, explicit):
    """(out_format, light, ootf, tone, alpha, dest, status, word): what both kinds of entry refuse before any work is queued.
    explicit: from_transfer / from_primaries are given (the step on its own needs them)"""
    big = 1 << 28
    nan, inf = float("nan"), float("inf")
    f32, u8 = dest(capi, CHW, F32, big), dest(capi, HWC, U8, big)
    lt = lambda **kw: light(capi, **kw) if explicit else light(capi, from_transfer=0, from_primaries=0, **kw)
    cases = [
        (RRGGBB_LE, None, ootf(capi), None, None, f32, HM_ERR_INVALID_ARG, "null light step"),
        (RRGGBB_LE, lt(), ootf(capi, kind=0), None, None, f32, HM_ERR_INVALID_ARG, "kind"),
        (RRGGBB_LE, lt(), ootf(capi, kind=2), None, None, f32, HM_ERR_INVALID_ARG, "kind"),
        (RRGGBB_LE, lt(), ootf(capi, reserved=(1, 0, 0, 0, 0)), None, None, f32, HM_ERR_INVALID_ARG, "reserved"),
        (RRGGBB_LE, lt(), ootf(capi, reserved=(0, 0, 0, 0, -3)), None, None, f32, HM_ERR_INVALID_ARG, "reserved"),
    ]
    for bad in (nan, inf, -inf, 0.0, -1.0, 10000.5):
        cases.append((RRGGBB_LE, lt(), ootf(capi, bad), None, None, f32, HM_ERR_INVALID_ARG, "display_peak"))
    for bad in (nan, inf, -0.5):
        cases.append((RRGGBB_LE, lt(), ootf(capi, gamma=bad), None, None, f32, HM_ERR_INVALID_ARG, "gamma"))
    cases += [
        (RRGGBB_LE, light(capi, from_transfer=16), ootf(capi), None, None, f32, HM_ERR_INVALID_ARG, "from_transfer"),
        (RRGGBB_LE, light(capi, from_transfer=13, from_primaries=1), ootf(capi), tone(capi), None, f32, HM_ERR_INVALID_ARG, "from_transfer"),
        (RRGGBB_LE, lt(to_transfer=18), ootf(capi), None, None, dest(capi, HWC, U16, big), HM_ERR_INVALID_ARG, "to_transfer"),
        (RRGGBBAA_LE, lt(), ootf(capi), None, alpha(capi, 2), f32, HM_ERR_INVALID_ARG, "HM_ALPHA_PREMULTIPLIED"),
        (RGBA, lt(), ootf(capi), None, alpha(capi, 2), f32, HM_ERR_INVALID_ARG, "HM_ALPHA_PREMULTIPLIED"),
        # a tone step behind it: its zeros stand for display_peak, and the knee is judged against that
        (RRGGBB_LE, lt(), ootf(capi, 4000.0), tone(capi, dst_peak=1.0), None, f32, HM_ERR_INVALID_ARG, "KS"),
        (RRGGBB_LE, lt(), ootf(capi), tone(capi, dst_peak=0.0), None, f32, HM_ERR_INVALID_ARG, "dst_peak"),
        (RRGGBB_LE, lt(), ootf(capi), tone(capi, src_peak=nan), None, f32, HM_ERR_INVALID_ARG, "src_peak"),
        (RRGGBB_LE, lt(to_transfer=13), ootf(capi), tone(capi, out_bits=8), None, dest(capi, HWC, U16, big), HM_ERR_INVALID_ARG, "HM_DEV_U16"),
        (RRGGBBAA_LE, lt(to_transfer=13), ootf(capi), tone(capi, out_bits=8), None, u8, HM_ERR_UNSUPPORTED, "four-channel"),
        # everything the light, alpha and destination checks refuse
        (RRGGBB_LE, lt(gain=0.0), ootf(capi), None, None, f32, HM_ERR_INVALID_ARG, "gain"),
        (RRGGBB_LE, lt(to_transfer=11), ootf(capi), None, None, f32, HM_ERR_UNSUPPORTED, "transfer"),
        (RRGGBB_LE, lt(), ootf(capi), None, None, dest(capi, HWC, U16, big), HM_ERR_INVALID_ARG, "float dtype"),
        (RRGGBB_LE, lt(), ootf(capi), None, alpha(capi, 1), f32, HM_ERR_INVALID_ARG, "carries no alpha"),
        (RRGGBBAA_LE, lt(), ootf(capi), None, alpha(capi, 4), f32, HM_ERR_INVALID_ARG, "mode"),
        (RRGGBB_LE, lt(), ootf(capi), None, None, dest(capi, CHW, F32, W * H * 12 - 1), HM_ERR_INVALID_ARG, "len"),
    ]
    return cases


def test_refusals_of_the_step_alone(capi, L):
    for fmt, lt, oo, tn, al, d, status, word in refusal_cases(capi, True):
        rc = L.hm_ootf_to_tensor(fmt, 10, W, H, FAKE, W * 8, None, ref(lt), ref(oo), ref(tn), ref(al), C.byref(d), None)
        assert rc == status and word in L.hm_last_error().decode(), (rc, L.hm_last_error().decode(), word)
    f32 = dest(capi, CHW, F32, 1 << 28)
    # from_* must be explicit, as in hm_tone_to_tensor
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6, None, C.byref(light(capi, from_transfer=0)), C.byref(ootf(capi)), None, None, C.byref(f32), None)
    assert rc == HM_ERR_INVALID_ARG and "must be given" in L.hm_last_error().decode()
    # samples deeper than the tables, a short stride, null arguments
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 14, W, H, FAKE, W * 6, None, C.byref(light(capi)), C.byref(ootf(capi)), None, None, C.byref(f32), None)
    assert rc == HM_ERR_UNSUPPORTED and "bits" in L.hm_last_error().decode()
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6 - 1, None, C.byref(light(capi)), C.byref(ootf(capi)), None, None, C.byref(f32), None)
    assert rc == HM_ERR_INVALID_ARG and "src_stride" in L.hm_last_error().decode()
    assert L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, None, W * 6, None, C.byref(light(capi)), C.byref(ootf(capi)), None, None, C.byref(f32), None) == HM_ERR_INVALID_ARG
    assert L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6, None, C.byref(light(capi)), C.byref(ootf(capi)), None, None, None, None) == HM_ERR_INVALID_ARG
    # a request that passes every check of the host reaches the device check (or, with a GPU, the pointer check)
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6, None, C.byref(light(capi, to_transfer=13, to_primaries=1)), C.byref(ootf(capi)),
                             C.byref(tone(capi, out_bits=8)), None, C.byref(dest(capi, HWC, U8, W * H * 3)), None)
    msg = L.hm_last_error().decode()
    assert (rc == HM_ERR_NO_DEVICE) if L.hm_device_count() == 0 else (rc == HM_ERR_INVALID_ARG and "ptr" in msg), msg
    # ootf == NULL is the same call through the existing entries: their refusals, with their words
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6, None, C.byref(light(capi, from_transfer=16)), None, C.byref(tone(capi)), None, C.byref(f32), None)
    assert rc == HM_ERR_INVALID_ARG and "src_peak" in L.hm_last_error().decode()  # (hm_tone_to_tensor: src_peak must be explicit)
    rc = L.hm_ootf_to_tensor(RRGGBB_LE, 10, W, H, FAKE, W * 6, None, C.byref(light(capi)), None, None, C.byref(alpha(capi, 1)), C.byref(f32), None)
    assert rc == HM_ERR_INVALID_ARG and "carries no alpha" in L.hm_last_error().decode()  # (hm_alpha_to_tensor)


@pytest.fixture(scope="module")
def hlg_file():
    pic = synthutil.picture(48410, width=W, height=H, bit_depth=10, full_range=0, matrix=9, primaries=9)
    return hdrwriter.write_hdr_heic([pic], (W, H), colr=(9, 18, 9, 0))


def test_refusals_of_the_decode_entries(capi, L, hlg_file):
    def call(fmt, lt, oo, tn, al, d):
        fh = C.c_void_p()
        assert L.hm_file_open(hlg_file, len(hlg_file), C.byref(fh)) == 0
        try:
            prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
            out = capi.Decoded()
            rc = L.hm_decode_item_to_device_ootf(fh, L.hm_file_primary_item(fh), C.byref(prm), None, ref(lt), ref(oo), ref(tn), ref(al), C.byref(d), C.byref(out))
            assert not out.plane[0]
            return rc, L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
    for explicit in (False, True):
        for fmt, lt, oo, tn, al, d, status, word in refusal_cases(capi, explicit):
            rc, msg = call(fmt, lt, oo, tn, al, d)
            assert rc == status and word in msg, (explicit, fmt, rc, msg, word)
    f32 = dest(capi, CHW, F32, 1 << 28)
    missing = (lambda rc, msg: rc == HM_ERR_NO_DEVICE) if L.hm_device_count() == 0 else (lambda rc, msg: rc == HM_ERR_INVALID_ARG and "ptr" in msg)
    # a request the host accepts: from_* == 0 and the tone step's zeros pass (they resolve behind the decode and to display_peak)
    assert missing(*call(RRGGBB_LE, light(capi, from_transfer=0, from_primaries=0), ootf(capi), tone(capi), None, f32))
    assert missing(*call(RRGGBB_LE, light(capi), ootf(capi, 203.0, 1.1), None, None, f32))
    # ootf == NULL: the existing entries' own refusals
    rc, msg = call(RRGGBB_LE, None, None, tone(capi), None, f32)
    assert rc == HM_ERR_INVALID_ARG and "tone: null light step" in msg
    rc, msg = call(RRGGBB_LE, light(capi), None, None, alpha(capi, 1), f32)
    assert rc == HM_ERR_INVALID_ARG and "carries no alpha" in msg
    # the pipeline and the frames form: NULL arguments and the null light step
    ok = ootf(capi)
    assert L.hm_pipeline_submit_to_device_ootf(None, hlg_file, len(hlg_file), 0, 0, None, C.byref(light(capi)), C.byref(ok), None, None, C.byref(f32)) == HM_ERR_INVALID_ARG
    fh = C.c_void_p()
    assert L.hm_file_open(hlg_file, len(hlg_file), C.byref(fh)) == 0
    prm = capi.DecodeParams(RRGGBB_LE, 1, 0, 0, None, None, 0, 0, 0, 0)
    out, failed, ids = capi.Decoded(), C.c_int32(5), (C.c_uint32 * 1)(1)
    assert L.hm_decode_frames_to_device_ootf(fh, ids, 1, C.byref(prm), None, None, C.byref(ok), None, C.byref(f32), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
    assert failed.value == -1 and "ootf: null light step" in L.hm_last_error().decode()
    failed = C.c_int32(5)
    assert L.hm_decode_frames_to_device_ootf(fh, ids, 1, C.byref(prm), None, C.byref(light(capi)), C.byref(ok), None, C.byref(f32), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
    assert failed.value == -1 and "not an image sequence" in L.hm_last_error().decode()
    L.hm_file_close(fh)


def test_abi_and_exports(pkg, capi, L):
    T = capi.DeviceOotf
    assert C.sizeof(T) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("kind", 0), ("display_peak", 4), ("gamma", 8), ("reserved", 12)]
    assert (capi.HM_OOTF_HLG, capi.HM_OOTF_STEPS) == (1, 1024)
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in names and hasattr(L, name), name
    assert not [n for n in names if n.startswith("hm_debug")]
    for fn in (pkg.decode_to_tensor, pkg.decode_batch_to_tensor, pkg.decode_sequence_to_tensor):
        assert inspect.signature(fn).parameters["ootf"].default is None


def test_python_ootf_argument(pkg, hlg_file):
    from heif_decoder_lib_amd import decode
    lit = decode._light_of(True)
    assert decode._ootf_of(None, lit) is None and decode._ootf_of(None, None) is None and decode._ootf_of(False, lit) is None
    for arg in (1000, 1000.0, dict(display_peak=1000), dict(display_peak=1000.0, gamma=None)):
        d = decode._ootf_of(arg, lit)
        assert (d.kind, d.display_peak, d.gamma, tuple(d.reserved)) == (1, 1000.0, 0.0, (0, 0, 0, 0, 0)), arg
    d = decode._ootf_of(dict(display_peak=400, gamma=1.25), lit)
    assert (d.kind, d.display_peak, d.gamma) == (1, 400.0, 1.25)
    for bad in (dict(display_peak=1000, peak=5), dict(gamma=1.2), dict(display_peak=None), "hlg", True, dict(display_peak=1000, gamma=0), (1000,)):
        with pytest.raises(ValueError):
            decode._ootf_of(bad, lit)
    with pytest.raises(ValueError, match="unknown keys"):
        decode._ootf_of(dict(display_peak=1000, system_gamma=1.2), lit)
    with pytest.raises(ValueError, match="light"):
        decode._ootf_of(1000, None)
    # through the public calls: a missing light=, and the pair the plan refuses
    for fn, arg in ((pkg.decode_to_tensor, hlg_file), (pkg.decode_batch_to_tensor, [hlg_file]), (pkg.decode_sequence_to_tensor, hlg_file)):
        with pytest.raises((ValueError, pkg.HmError), match="light|sequence"):
            fn(arg, ootf=1000)
    with pytest.raises(pkg.HmError, match="gain step beside the OOTF"):
        pkg.decode_to_tensor(hlg_file, light=True, ootf=1000, gain=dict(headroom=1.0))
