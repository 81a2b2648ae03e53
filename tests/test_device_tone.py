"""The tone step (hm_device_tone), the part that needs no GPU: the model's own anchors (tests/tone_ref.py, written from BT.2390 and
ST 2084), the tables hm_tone_table hands out against it, every refusal that is decided on the host, the light levels the box reader
finds (clli / mdcv) and the peak rule on them, the ABI, the Python argument and the facade's decode of an mdcv."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import hdrwriter
import heifwriter
import synthutil
import tone_ref

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_BITSTREAM, HM_ERR_NO_DEVICE = -1, -2, -3, -4
RGB, RGBA, RRGGBB_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 14, 15
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)
CURVES = ((1000.0, 203.0), (4000.0, 100.0), (10000.0, 100.0), (1000.0, 1000.0))
GAINS = (1.0, 0.5)
NEW_SYMBOLS = ("hm_decode_item_to_device_tone", "hm_decode_frames_to_device_tone", "hm_pipeline_submit_to_device_tone", "hm_tone_to_tensor", "hm_tone_table",
               "hm_file_item_light_levels")


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def tone(capi, dst_peak=203.0, src_peak=1000.0, unit_nits=10000.0, out_unit_nits=0.0, out_bits=0, curve=1, reserved=(0, 0)):
    return capi.DeviceTone(curve, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(*reserved))


def light(capi, to_transfer=8, to_primaries=0, gain=1.0, from_transfer=0, from_primaries=0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def dest(capi, layout, dtype, length, ptr=FAKE):
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = ptr, length, layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    return d


def lib_tables(L, t, gain):
    out = []
    for which in (0, 1):
        buf = (C.c_float * 2048)()
        assert L.hm_tone_table(C.byref(t), gain, which, buf) == 2048, L.hm_last_error().decode()
        out.append(np.frombuffer(buf, np.float32).copy())
    return out


def test_the_models_anchors():
    """derived from the formulas: below the knee and at k = 0 the gain is U / Uo exactly; the code of src_peak maps to dst_peak; the
    output luminance does not fall as the code rises; thr rises strictly; a display at least as bright as the content changes nothing
    below src_peak"""
    for src, dst in CURVES:
        for U, Uo in ((10000.0, dst), (203.0, 100.0), (10000.0, 10000.0)):
            sg = tone_ref.gains(src, dst, U, Uo)
            out, curved = tone_ref.mapped_codes(src, dst)
            pw, max_lum, ks = tone_ref.knee(src, dst)
            e = np.arange(2048) / 2047.0
            below = e / pw < ks
            assert not curved[0] and not curved[below].any()
            assert (sg.astype(np.float32)[~curved] == np.float32(U / Uo)).all(), (src, dst, U, Uo)
            assert (np.diff(tone_ref.eotf(out)) >= 0).all(), (src, dst)
            # the entry at e * 10000 == src_peak: E1 = 1, T = 1, E2 = maxLum, so the output is EOTF(PQ(dst_peak)) = dst_peak
            top = tone_ref.eotf(np.float64(max_lum * pw if max_lum < 1.0 else pw)) * 10000.0
            assert abs(float(top) - min(src, dst)) <= 1e-9 * src, (src, dst, float(top))
            if max_lum < 1.0:  # ... and every code at or above src_peak maps there too: no channel rises above the display's peak
                above = e >= pw
                assert above.any() and np.abs(tone_ref.eotf(out[above]) * 10000.0 - dst).max() <= 1e-9 * src
            else:
                assert not curved.any() and (sg == U / Uo).all()
    assert abs(float(tone_ref.pq(tone_ref.eotf(np.float64(0.37)))) - 0.37) < 1e-12  # the two functions are inverses
    assert abs(float(tone_ref.pq(0.01)) - 0.508078421517399) < 1e-9                  # ST 2084: 100 cd/m2
    for g in GAINS:
        for U in (10000.0, 203.0):
            thr = tone_ref.thresholds(g, U).astype(np.float32)
            assert thr[0] == 0.0 and (np.diff(thr) > 0).all(), (g, U)


def test_tables_against_the_model(capi, L):
    """every entry within 1 float32 ulp of the model's (two correct double evaluations may round apart, and no more)"""
    for src, dst in CURVES:
        for g in GAINS:
            for U, Uo in ((10000.0, dst), (203.0, 100.0)):
                got = lib_tables(L, tone(capi, dst, src, U, Uo), g)
                want = tone_ref.tables(g, src, dst, U, Uo)
                for name, a, b in zip(("thr", "sg"), got, want):
                    assert a.shape == b.shape == (2048,) and (a >= 0).all(), (src, dst, g, name)
                    ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
                    assert ulps.max() <= 1, (src, dst, g, U, name, int(ulps.argmax()), a[ulps.argmax()], b[ulps.argmax()])
                assert got[0][0] == 0.0 and (np.diff(got[0]) > 0).all()
                _, curved = tone_ref.mapped_codes(src, dst)
                assert (got[1][~curved] == np.float32(U / Uo)).all(), (src, dst, g)  # ratio 1, exactly


def test_tone_table_refusals(capi, L):
    out = (C.c_float * 2048)()
    ok = tone(capi, 203.0, 1000.0, 10000.0, 203.0)
    assert L.hm_tone_table(C.byref(ok), 1.0, 0, out) == 2048
    assert L.hm_tone_table(None, 1.0, 0, out) == HM_ERR_INVALID_ARG and L.hm_tone_table(C.byref(ok), 1.0, 0, None) == HM_ERR_INVALID_ARG
    assert L.hm_tone_table(C.byref(ok), 1.0, 2, out) == HM_ERR_INVALID_ARG
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert L.hm_tone_table(C.byref(ok), g, 0, out) == HM_ERR_INVALID_ARG, g
    for bad, word in ((tone(capi, 203.0, 0.0, 10000.0, 203.0), "src_peak"), (tone(capi, 203.0, 1000.0, 0.0, 203.0), "unit_nits"),
                      (tone(capi, 203.0, 1000.0, 10000.0, 0.0), "out_unit_nits"), (tone(capi, 0.0, 1000.0, 10000.0, 203.0), "dst_peak"),
                      (tone(capi, 10.0, 10000.0, 10000.0, 10.0), "KS"), (tone(capi, 203.0, 1000.0, 10000.0, 203.0, curve=2), "curve")):
        assert L.hm_tone_table(C.byref(bad), 1.0, 1, out) == HM_ERR_INVALID_ARG and word in L.hm_last_error().decode(), (word, L.hm_last_error().decode())


@pytest.fixture(scope="module")
def files():
    """name -> file bytes: one 10-bit PQ BT.2020 picture with the light-level properties the name says"""
    hdr = synthutil.picture(48300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)
    w = lambda **kw: hdrwriter.write_hdr_heic([hdr], (160, 96), **kw)
    return {"clli": w(clli=(1000, 400)), "mdcv": w(mdcv=(40000000, 50)), "both": w(clli=(600, 120), mdcv=(10000000, 1)), "neither": w(),
            "mdcv_low": w(mdcv=(49999, 1)), "mdcv_high": w(mdcv=(100000001, 1)), "clli_zero": w(clli=(0, 90), mdcv=(20000000, 1)),
            "clli_huge": w(clli=(20000, 0)), "truncated": w(clli=b"\x03\xe8\x01")}


def levels(capi, L, data):
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0, L.hm_last_error().decode()
    try:
        ll = capi.LightLevels()
        assert L.hm_file_item_light_levels(fh, L.hm_file_primary_item(fh), C.byref(ll)) == 0
        return ll
    finally:
        L.hm_file_close(fh)


def test_light_levels_of_a_file(capi, L, files):
    want = {"clli": (1, 0, 1000, 400, 0, 0), "mdcv": (0, 1, 0, 0, 40000000, 50), "both": (1, 1, 600, 120, 10000000, 1), "neither": (0, 0, 0, 0, 0, 0),
            "mdcv_low": (0, 1, 0, 0, 49999, 1), "mdcv_high": (0, 1, 0, 0, 100000001, 1), "clli_zero": (1, 1, 0, 90, 20000000, 1),
            "clli_huge": (1, 0, 20000, 0, 0, 0)}
    peaks = {"clli": 1000.0, "mdcv": 4000.0, "both": 600.0, "neither": 1000.0, "mdcv_low": 1000.0, "mdcv_high": 1000.0, "clli_zero": 2000.0,
             "clli_huge": 10000.0}
    for name, exp in want.items():
        ll = levels(capi, L, files[name])
        got = (ll.has_clli, ll.has_mdcv, ll.max_content_light_level, ll.max_pic_average_light_level, ll.max_display_mastering_luminance,
               ll.min_display_mastering_luminance)
        assert got == exp, name
        if ll.has_mdcv:
            assert (tuple(ll.display_primaries_x), tuple(ll.display_primaries_y)) == (tuple(x for x, _ in hdrwriter.BT2020_XY), tuple(y for _, y in hdrwriter.BT2020_XY))
            assert (ll.white_point_x, ll.white_point_y) == hdrwriter.D65_XY
        # the peak rule, restated: clli's maximum if non-zero (at most 10000: PQ codes no more); else mdcv's maximum * 0.0001 if the raw
        # value lies in 50000 .. 100000000; else 1000
        if ll.has_clli and ll.max_content_light_level:
            peak = float(min(ll.max_content_light_level, 10000))
        elif ll.has_mdcv and 50000 <= ll.max_display_mastering_luminance <= 100000000:
            peak = ll.max_display_mastering_luminance * 0.0001
        else:
            peak = 1000.0
        assert peak == peaks[name] == tone_ref.peak_of(ll.has_clli, ll.max_content_light_level, ll.has_mdcv, ll.max_display_mastering_luminance), name
    # a grid: the properties are the grid item's; a tile carries none
    tiles = [synthutil.picture(48310 + t, width=64, height=64, bit_depth=10) for t in range(2)]
    grid = hdrwriter.write_hdr_heic(tiles, (64, 64), grid=(1, 2, 128, 64), clli=(1234, 0))
    assert levels(capi, L, grid).max_content_light_level == 1234
    fh = C.c_void_p()
    assert L.hm_file_open(grid, len(grid), C.byref(fh)) == 0
    ll = capi.LightLevels()
    assert L.hm_file_item_light_levels(fh, 1, C.byref(ll)) == 0 and (ll.has_clli, ll.has_mdcv) == (0, 0)
    assert L.hm_file_item_light_levels(fh, 99, C.byref(ll)) == HM_ERR_INVALID_ARG
    assert L.hm_file_item_light_levels(fh, 1, None) == HM_ERR_INVALID_ARG and L.hm_file_item_light_levels(None, 1, C.byref(ll)) == HM_ERR_INVALID_ARG
    L.hm_file_close(fh)
    # a truncated property fails the file as a truncated ispe does
    fh = C.c_void_p()
    assert L.hm_file_open(files["truncated"], len(files["truncated"]), C.byref(fh)) == HM_ERR_BITSTREAM and "clli" in L.hm_last_error().decode()
    message = L.hm_last_error().decode()
    hdr = synthutil.picture(48300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)
    cut = hdrwriter.write_hdr_heic([hdr], (160, 96), ispe=b"\0\0\0\0\0\0\0\xa0\0\0")
    assert L.hm_file_open(cut, len(cut), C.byref(fh)) == HM_ERR_BITSTREAM and L.hm_last_error().decode() == message.replace("clli", "ispe")


def test_tone_host_side_refusals(capi, L, files):
    big = 1 << 28
    sdr = heifwriter.write_heic([synthutil.picture(48100, width=96, height=64)], (96, 64))  # BT.709-class source: no unit of its own
    f32, u8, u16 = dest(capi, CHW, F32, big), dest(capi, HWC, U8, big), dest(capi, HWC, U16, big)
    nan, inf = float("nan"), float("inf")

    def call(data, fmt, lt, tn, d):
        fh = C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
        try:
            prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
            out = capi.Decoded()
            rc = L.hm_decode_item_to_device_tone(fh, L.hm_file_primary_item(fh), C.byref(prm), None, C.byref(lt) if lt is not None else None,
                                                 C.byref(tn) if tn is not None else None, C.byref(d), C.byref(out))
            assert not out.plane[0]
            return rc, L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
    hdr = files["clli"]
    cases = [
        (hdr, RRGGBB_LE, None, tone(capi), f32, HM_ERR_INVALID_ARG, "null light step"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, curve=0), f32, HM_ERR_INVALID_ARG, "curve"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, curve=2), f32, HM_ERR_INVALID_ARG, "curve"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, reserved=(0, 1)), f32, HM_ERR_INVALID_ARG, "reserved"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, reserved=(3, 0)), f32, HM_ERR_INVALID_ARG, "reserved"),
    ]
    for bad in (nan, inf, -1.0, 10000.5):
        cases += [(hdr, RRGGBB_LE, light(capi), tone(capi, src_peak=bad), f32, HM_ERR_INVALID_ARG, "src_peak"),
                  (hdr, RRGGBB_LE, light(capi), tone(capi, dst_peak=bad), f32, HM_ERR_INVALID_ARG, "dst_peak"),
                  (hdr, RRGGBB_LE, light(capi), tone(capi, unit_nits=bad), f32, HM_ERR_INVALID_ARG, "unit_nits"),
                  (hdr, RRGGBB_LE, light(capi), tone(capi, out_unit_nits=bad), f32, HM_ERR_INVALID_ARG, "out_unit_nits")]
    cases += [
        (hdr, RRGGBB_LE, light(capi), tone(capi, dst_peak=0.0), f32, HM_ERR_INVALID_ARG, "dst_peak"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, dst_peak=10.0, src_peak=10000.0), f32, HM_ERR_INVALID_ARG, "KS"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, dst_peak=1.0, src_peak=0.0), f32, HM_ERR_INVALID_ARG, "KS"),  # (the file's own 1000)
        (hdr, RRGGBB_LE, light(capi), tone(capi, out_bits=10), f32, HM_ERR_INVALID_ARG, "out_bits"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, out_bits=-8), f32, HM_ERR_INVALID_ARG, "out_bits"),
        (hdr, RRGGBB_LE, light(capi, to_transfer=13), tone(capi, out_bits=8), u16, HM_ERR_INVALID_ARG, "HM_DEV_U16"),
        (hdr, RRGGBBAA_LE, light(capi, to_transfer=13), tone(capi, out_bits=8), u8, HM_ERR_UNSUPPORTED, "four-channel"),
        (hdr, RGBA, light(capi, to_transfer=13), tone(capi, out_bits=8), u8, HM_ERR_UNSUPPORTED, "four-channel"),
        # everything the light and destination checks refuse
        (hdr, RRGGBB_LE, light(capi, gain=0.0), tone(capi), f32, HM_ERR_INVALID_ARG, "gain"),
        (hdr, RRGGBB_LE, light(capi, to_transfer=11), tone(capi), f32, HM_ERR_UNSUPPORTED, "transfer"),
        (hdr, RRGGBB_LE, light(capi), tone(capi), u16, HM_ERR_INVALID_ARG, "float dtype"),
        (hdr, RRGGBB_LE, light(capi), tone(capi, out_bits=8), u8, HM_ERR_INVALID_ARG, "float dtype"),  # (linear light: no code to store)
        (hdr, RRGGBB_LE, light(capi, to_transfer=13), tone(capi), u8, HM_ERR_INVALID_ARG, "dtype"),     # (8-bit integers need out_bits = 8)
        (hdr, RRGGBB_BE, light(capi, to_transfer=13), tone(capi, out_bits=8), u8, HM_ERR_INVALID_ARG, "_LE"),
        (hdr, RRGGBB_LE, light(capi), tone(capi), dest(capi, CHW, F32, 160 * 96 * 12 - 1), HM_ERR_INVALID_ARG, "len"),
        (hdr, RRGGBB_LE, light(capi, to_transfer=13), tone(capi, out_bits=8), dest(capi, HWC, U8, 160 * 96 * 3 - 1), HM_ERR_INVALID_ARG, "len"),
        (hdr, RRGGBB_LE, light(capi), tone(capi), dest(capi, CHW, F32, big, ptr=None), HM_ERR_INVALID_ARG, "null ptr"),
    ]
    for data, fmt, lt, tn, d, status, word in cases:
        rc, msg = call(data, fmt, lt, tn, d)
        assert rc == status and word in msg, (fmt, rc, msg, word)
    assert call(hdr, RRGGBB_LE, light(capi), None, f32)[0] == HM_ERR_INVALID_ARG
    # a clli above what PQ can code counts as 10000: the file decodes with src_peak = 0, and the knee is judged against 10000 (10000 -> 10
    # lies below black, the 1000 -> 10 of the other file does not)
    missing = (lambda rc, msg: rc == HM_ERR_NO_DEVICE) if L.hm_device_count() == 0 else (lambda rc, msg: rc == HM_ERR_INVALID_ARG and "ptr" in msg)
    assert missing(*call(files["clli_huge"], RRGGBB_LE, light(capi), tone(capi, src_peak=0.0), f32))
    rc, msg = call(files["clli_huge"], RRGGBB_LE, light(capi), tone(capi, dst_peak=10.0, src_peak=0.0), f32)
    assert rc == HM_ERR_INVALID_ARG and "KS" in msg and "10000" in msg, msg
    assert missing(*call(hdr, RRGGBB_LE, light(capi), tone(capi, dst_peak=10.0, src_peak=0.0), f32))
    # the 8-bit finish is sized as the 8-bit sibling target: exactly its bytes are enough to pass the len check
    need = L.hm_device_dest_bytes(RGB, 160, 96, C.byref(u8))
    assert need == 160 * 96 * 3
    rc, msg = call(hdr, RRGGBB_LE, light(capi, to_transfer=13), tone(capi, out_bits=8), dest(capi, HWC, U8, need))
    assert (rc == HM_ERR_NO_DEVICE) if L.hm_device_count() == 0 else (rc == HM_ERR_INVALID_ARG and "ptr" in msg), msg
    # the step on its own: src_peak, unit_nits and the light step's from_* must be explicit
    explicit = light(capi, from_transfer=16, from_primaries=9)
    for lt, tn, fmt, bits, d, status, word in ((light(capi), tone(capi), RRGGBB_LE, 10, f32, HM_ERR_INVALID_ARG, "must be given"),
                                               (explicit, tone(capi, src_peak=0.0), RRGGBB_LE, 10, f32, HM_ERR_INVALID_ARG, "src_peak"),
                                               (explicit, tone(capi, unit_nits=0.0), RRGGBB_LE, 10, f32, HM_ERR_INVALID_ARG, "unit_nits"),
                                               (explicit, tone(capi, dst_peak=10.0, src_peak=10000.0), RRGGBB_LE, 10, f32, HM_ERR_INVALID_ARG, "KS"),
                                               (explicit, tone(capi), RRGGBB_LE, 14, f32, HM_ERR_UNSUPPORTED, "bits"),
                                               (explicit, tone(capi, out_bits=8), RRGGBB_LE, 10, u16, HM_ERR_INVALID_ARG, "HM_DEV_U16")):
        rc = L.hm_tone_to_tensor(fmt, bits, 16, 16, FAKE, 128, None, C.byref(lt), C.byref(tn), C.byref(d), None)
        assert rc == status and word in L.hm_last_error().decode(), (rc, L.hm_last_error().decode(), word)
    ok = tone(capi)
    assert L.hm_tone_to_tensor(RRGGBB_LE, 10, 16, 16, FAKE, 128, None, None, C.byref(ok), C.byref(f32), None) == HM_ERR_INVALID_ARG
    assert "null light step" in L.hm_last_error().decode()
    assert L.hm_tone_to_tensor(RRGGBB_LE, 10, 16, 16, FAKE, 128, None, C.byref(explicit), None, C.byref(f32), None) == HM_ERR_INVALID_ARG
    assert L.hm_tone_to_tensor(RRGGBB_LE, 10, 16, 16, FAKE, 95, None, C.byref(explicit), C.byref(ok), C.byref(f32), None) == HM_ERR_INVALID_ARG
    assert "src_stride" in L.hm_last_error().decode()
    # the other entry points: NULL arguments
    assert L.hm_pipeline_submit_to_device_tone(None, hdr, len(hdr), 0, 0, None, C.byref(explicit), C.byref(ok), C.byref(f32)) == HM_ERR_INVALID_ARG
    fh = C.c_void_p()
    assert L.hm_file_open(hdr, len(hdr), C.byref(fh)) == 0
    prm = capi.DecodeParams(RRGGBB_LE, 1, 0, 0, None, None, 0, 0, 0, 0)
    out, failed, ids = capi.Decoded(), C.c_int32(5), (C.c_uint32 * 1)(1)
    assert L.hm_decode_frames_to_device_tone(fh, ids, 1, C.byref(prm), None, None, C.byref(ok), C.byref(f32), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
    assert failed.value == -1 and "null light step" in L.hm_last_error().decode()
    L.hm_file_close(fh)
    # unit_nits == 0 needs a PQ source: known once the image's profile is - without a GPU the missing device is reported first
    rc, msg = call(sdr, RGB, light(capi), tone(capi, unit_nits=0.0, src_peak=203.0, dst_peak=100.0), f32)
    if L.hm_device_count() == 0:
        assert rc == HM_ERR_NO_DEVICE, msg
    rc = L.hm_tone_to_tensor(RGB, 8, 16, 16, FAKE, 128, None, C.byref(light(capi, from_transfer=13, from_primaries=1)),
                             C.byref(tone(capi, unit_nits=0.0, src_peak=203.0, dst_peak=100.0)), C.byref(f32), None)
    assert rc == HM_ERR_INVALID_ARG and "unit_nits" in L.hm_last_error().decode()


def test_abi_and_exports(pkg, capi, L):
    T, LL = capi.DeviceTone, capi.LightLevels
    assert C.sizeof(T) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("curve", 0), ("out_bits", 4), ("src_peak", 8), ("dst_peak", 12), ("unit_nits", 16),
                                                                  ("out_unit_nits", 20), ("reserved", 24)]
    assert C.sizeof(LL) == 36
    assert [(n, getattr(LL, n).offset) for n, _ in LL._fields_] == [("has_clli", 0), ("has_mdcv", 4), ("max_content_light_level", 8), ("max_pic_average_light_level", 10),
                                                                    ("display_primaries_x", 12), ("display_primaries_y", 18), ("white_point_x", 24), ("white_point_y", 26),
                                                                    ("max_display_mastering_luminance", 28), ("min_display_mastering_luminance", 32)]
    assert (capi.HM_TONE_BT2390, capi.HM_TONE_STEPS) == (1, 2048)
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in names and hasattr(L, name), name
    assert not [n for n in names if n.startswith("hm_debug")]
    api = subprocess.run(["nm", "-D", "--defined-only", os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libheif_mi355x_api.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in ("heif_image_has_content_light_level", "heif_image_get_content_light_level", "heif_image_set_content_light_level",
                 "heif_image_has_mastering_display_colour_volume", "heif_image_get_mastering_display_colour_volume",
                 "heif_image_set_mastering_display_colour_volume", "heif_mastering_display_colour_volume_decode"):
        assert f" T {name}\n" in api, name
    assert "hm_debug" not in api
    for fn in (pkg.decode_to_tensor, pkg.decode_batch_to_tensor, pkg.decode_sequence_to_tensor):
        assert inspect.signature(fn).parameters["tone"].default is None


def test_python_tone_argument(pkg):
    from heif_decoder_lib_amd import decode
    lit = decode._light_of(True)
    assert decode._tone_of(None, lit) is None and decode._tone_of(None, None) is None
    d = decode._tone_of(dict(dst_peak=203), lit)
    assert (d.curve, d.out_bits, d.src_peak, d.dst_peak, d.unit_nits, d.out_unit_nits, tuple(d.reserved)) == (1, 0, 0.0, 203.0, 0.0, 0.0, (0, 0))
    d = decode._tone_of(dict(dst_peak=100.0, src_peak=4000, unit_nits=203.0, out_unit_nits=100.0, out_bits=8), lit)
    assert (d.out_bits, d.src_peak, d.dst_peak, d.unit_nits, d.out_unit_nits) == (8, 4000.0, 100.0, 203.0, 100.0)
    d = decode._tone_of(dict(dst_peak=100.0, src_peak=None, unit_nits=None, out_unit_nits=None, out_bits=None), lit)
    assert (d.out_bits, d.src_peak, d.unit_nits, d.out_unit_nits) == (0, 0.0, 0.0, 0.0)
    for bad in (dict(dst_peak=100.0, peak=5), dict(src_peak=1000.0), dict(dst_peak=None), "bt2390", dict(dst_peak=100.0, src_peak=0)):
        with pytest.raises(ValueError):
            decode._tone_of(bad, lit)
    with pytest.raises(ValueError, match="light"):
        decode._tone_of(dict(dst_peak=100.0), None)


def test_the_facade_decodes_an_mdcv(pkg):
    """heif_mastering_display_colour_volume_decode against the reference's rule, restated: coordinates * 0.00002 unless x is outside
    5 .. 37000 or y outside 5 .. 42000, luminances * 0.0001 unless the maximum is outside 50000 .. 100000000 or the minimum outside
    1 .. 50000 - what is out of range decodes to 0"""
    class Err(C.Structure):
        _fields_ = [("code", C.c_int), ("subcode", C.c_int), ("message", C.c_char_p)]

    class Raw(C.Structure):
        _fields_ = [("x", C.c_uint16 * 3), ("y", C.c_uint16 * 3), ("wx", C.c_uint16), ("wy", C.c_uint16), ("hi", C.c_uint32), ("lo", C.c_uint32)]

    class Dec(C.Structure):
        _fields_ = [("x", C.c_float * 3), ("y", C.c_float * 3), ("wx", C.c_float), ("wy", C.c_float), ("hi", C.c_double), ("lo", C.c_double)]
    assert (C.sizeof(Raw), C.sizeof(Dec)) == (24, 48)
    pkg.lib()
    api = C.CDLL(os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "libheif_mi355x_api.so"))
    fn = api.heif_mastering_display_colour_volume_decode
    fn.restype, fn.argtypes = Err, [C.POINTER(Raw), C.POINTER(Dec)]
    cx = lambda v, most: np.float32(0.0) if v < 5 or v > most else np.float32(v * 0.00002)
    for x, y, w, hi, lo in (((35400, 8500, 6550), (14600, 39850, 2300), (15635, 16450), 10000000, 50), ((4, 5, 37000), (42001, 42000, 4), (37001, 5), 49999, 0),
                            ((0, 65535, 100), (0, 65535, 100), (5, 42000), 50000, 50001), ((1, 2, 3), (1, 2, 3), (0, 0), 100000000, 50000),
                            ((34000, 13250, 7500), (16000, 34500, 3000), (15635, 16450), 100000001, 1)):
        raw, dec = Raw((C.c_uint16 * 3)(*x), (C.c_uint16 * 3)(*y), w[0], w[1], hi, lo), Dec()
        assert fn(C.byref(raw), C.byref(dec)).code == 0
        assert [np.float32(v) for v in dec.x] == [cx(v, 37000) for v in x] and [np.float32(v) for v in dec.y] == [cx(v, 42000) for v in y]
        assert (np.float32(dec.wx), np.float32(dec.wy)) == (cx(w[0], 37000), cx(w[1], 42000))
        assert dec.hi == (0.0 if hi < 50000 or hi > 100000000 else hi * 0.0001) and dec.lo == (0.0 if lo < 1 or lo > 50000 else lo * 0.0001)
    assert fn(None, C.byref(Dec())).code != 0 and fn(C.byref(Raw()), None).code != 0
