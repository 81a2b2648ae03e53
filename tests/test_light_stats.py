"""The light statistics (hm_light_stats, include/heif_mi355x.h "Light statistics"), the part that needs no GPU: the new symbols and
their bindings, the struct's layout, the three host functions against the model (tests/light_stats_ref.py) on hand-made histograms,
every refusal that is decided before anything is queued - through all three entries, with a device pointer that is never
dereferenced and *stats / *out filled with 0xA5 beforehand and still so afterwards -, and the Python argument errors."""
import ctypes as C

import numpy as np
import pytest

import hdrwriter
import heifwriter
import light_stats_ref as ref
import overlaywriter
import synthutil
import target_cases

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_NO_DEVICE = -1, -2, -4
RGB, RGBA, RRGGBB_BE, RRGGBB_LE, RRGGBBAA_BE = 10, 11, 12, 14, 13
HWC, F32 = 0, 3
FAKE = target_cases.FAKE  # (never dereferenced on the host: every call below is refused, or finds no device)
NEW_SYMBOLS = ("hm_light_stats_code_nits", "hm_light_stats_percentile", "hm_light_stats_average", "hm_light_stats_of_tensor", "hm_decode_item_light_stats",
               "hm_decode_item_to_device_measured")
FRACTIONS = (1e-9, 0.5, 0.9999, 1.0)
W, H = 160, 96


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def files():
    """name -> file bytes: a 10-bit PQ picture without light-level properties, an 8-bit sRGB one, and an 'iden' item over it"""
    hdr = synthutil.picture(48300, width=W, height=H, bit_depth=10, full_range=0, matrix=1, primaries=1)
    sdr = synthutil.picture(61016, width=16, height=16)
    w = overlaywriter.Writer()
    w_id = w.iden([w.hvc1(sdr, (16, 16))], (16, 16))
    return {"pq": hdrwriter.write_hdr_heic([hdr], (W, H)), "sdr": heifwriter.write_heic([sdr], (16, 16)), "iden": w.finish(primary=w_id)}


def light(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=0, gain=1.0, reserved=(0, 0, 0)):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(*reserved))


def tone(capi, dst_peak=203.0, src_peak=0.0, unit_nits=0.0, out_unit_nits=0.0, out_bits=0, curve=1, reserved=(0, 0)):
    return capi.DeviceTone(curve, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(*reserved))


def ootf(capi, display_peak=1000.0, gamma=0.0, kind=1, reserved=(0,) * 5):
    return capi.DeviceOotf(kind, display_peak, gamma, (C.c_int32 * 5)(*reserved))


def dest(capi, L, fmt, w, h, dtype=F32, ptr=FAKE):
    d = capi.DeviceDest()
    d.layout, d.dtype = HWC, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    d.ptr, d.len = ptr, max(int(L.hm_device_dest_bytes(fmt, w, h, C.byref(d))), 1)
    return d


def ref_of(x):
    return C.byref(x) if x is not None else None


def filled(struct):
    s = struct()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    return s


def untouched(s):
    return bytes(s) == b"\xA5" * C.sizeof(s)


def test_symbols_and_bindings(capi, L, hm, pkg):
    for name in NEW_SYMBOLS:
        assert hasattr(hm, name), name
        assert getattr(L, name).argtypes is not None, name
    for name in ("measure_light", "measure_light_of_tensor", "LightStats"):
        assert hasattr(pkg, name), name
    assert capi.HM_LIGHT_STATS_BINS == capi.HM_TONE_STEPS == 2048


def test_struct_layout(capi):
    """hm_light_stats as the header declares it: uint64, 2048 x uint32, float, int32, float, float, int32[2] - no padding"""
    S = capi.LightStatsC
    assert C.sizeof(S) == 8 + 4 * 2048 + 4 * 4 + 8 == 8224
    assert [(getattr(S, n).offset, getattr(S, n).size) for n in ("pixels", "hist", "max_norm", "max_code", "max_nits", "average_nits", "reserved")] == \
        [(0, 8), (8, 8192), (8200, 4), (8204, 4), (8208, 4), (8212, 4), (8216, 8)]


def test_code_nits_against_the_model(L):
    """every code, both edges: the double the model computes with the C library's pow, bit for bit; the anchors of ST 2084"""
    v = C.c_double()
    for edge in (0, 1):
        last = -1.0
        for k in range(2048):
            assert L.hm_light_stats_code_nits(k, edge, C.byref(v)) == 0
            assert v.value == ref.code_nits(k, edge), (k, edge, v.value, ref.code_nits(k, edge))
            assert v.value >= last and (v.value > last or (edge == 1 and k == 2047))
            last = v.value
    assert ref.code_nits(0, 0) == 0.0 and ref.code_nits(2047, 0) == 10000.0 == ref.code_nits(2047, 1) == ref.code_nits(2046, 1) * 0 + 10000.0
    assert 0.0 < ref.code_nits(0, 1) < ref.code_nits(1, 0) < ref.code_nits(1, 1)  # the upper edge of bin 0 is above 0
    for k, edge in ((-1, 0), (2048, 0), (0, 2), (0, -1)):
        assert L.hm_light_stats_code_nits(k, edge, C.byref(v)) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_code_nits(0, 0, None) == HM_ERR_INVALID_ARG


def hand_made():
    """name -> histogram: empty except bin 0, a single pixel, all in bin 2047, two bins with a rank exactly on the boundary (10000 pixels,
    fraction 0.5 -> rank 5000 = the last pixel of the lower bin; 0.9999 -> rank 9999), a spread over many bins"""
    out = {}
    h = np.zeros(2048, np.uint32); h[0] = 1000; out["bin 0 only"] = h
    h = np.zeros(2048, np.uint32); h[777] = 1; out["a single pixel"] = h
    h = np.zeros(2048, np.uint32); h[2047] = 123457; out["all in bin 2047"] = h
    h = np.zeros(2048, np.uint32); h[100] = 5000; h[1500] = 5000; out["two bins, the rank on the boundary"] = h
    h = np.zeros(2048, np.uint32); h[100] = 4999; h[1500] = 5001; out["two bins, the rank one behind the boundary"] = h
    h = np.zeros(2048, np.uint32); h[1200] = 9999; h[1900] = 1; out["one bright pixel in ten thousand"] = h
    rng = np.random.default_rng(77)
    out["random"] = rng.integers(0, 5000, 2048).astype(np.uint32)
    out["a full picture"] = np.full(2048, (4032 * 3024) // 2048, np.uint32)
    return out


def test_percentile_and_average_against_the_model(capi, L):
    for name, hist in hand_made().items():
        s = capi.LightStatsC()
        s.pixels = int(hist.sum(dtype=np.uint64))
        for k in np.flatnonzero(hist):
            s.hist[int(k)] = int(hist[k])
        s.max_code = int(np.flatnonzero(hist)[-1])
        for fraction in FRACTIONS:
            code, nits = C.c_int32(-1), C.c_float(-1.0)
            assert L.hm_light_stats_percentile(C.byref(s), fraction, C.byref(code), C.byref(nits)) == 0, L.hm_last_error().decode()
            want = ref.percentile(hist, s.pixels, fraction)
            assert (code.value, nits.value) == want, (name, fraction, code.value, nits.value, want)
            assert 0.0 < nits.value <= 10000.0
            if fraction == 1.0:
                assert code.value == s.max_code, name
            assert L.hm_light_stats_percentile(C.byref(s), fraction, None, None) == 0
        got = C.c_float(-1.0)
        assert L.hm_light_stats_average(C.byref(s), C.byref(got)) == 0
        a = ref.average(hist, s.pixels)
        assert got.value == a, (name, got.value, a)
        assert ref.code_nits(int(np.flatnonzero(hist)[0]), 0) <= a * (1 + 1e-6) and a <= ref.code_nits(s.max_code, 0) * (1 + 1e-6), name
    # the hand-made boundary, spelled out
    two = hand_made()["two bins, the rank on the boundary"]
    assert ref.percentile(two, 10000, 0.5)[0] == 100 and ref.percentile(two, 10000, 0.50001)[0] == 1500 and ref.percentile(two, 10000, 1e-9)[0] == 100
    assert ref.percentile(hand_made()["one bright pixel in ten thousand"], 10000, 0.9999)[0] == 1200


def test_percentile_refusals(capi, L):
    s = capi.LightStatsC()
    s.pixels, s.hist[5] = 10, 10
    code, nits = C.c_int32(-7), C.c_float(-7.0)
    for fraction in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert L.hm_light_stats_percentile(C.byref(s), fraction, C.byref(code), C.byref(nits)) == HM_ERR_INVALID_ARG, fraction
        assert "fraction" in L.hm_last_error().decode()
    assert L.hm_light_stats_percentile(None, 0.5, C.byref(code), C.byref(nits)) == HM_ERR_INVALID_ARG
    empty = capi.LightStatsC()
    assert L.hm_light_stats_percentile(C.byref(empty), 0.5, C.byref(code), C.byref(nits)) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_average(C.byref(empty), C.byref(nits)) == HM_ERR_INVALID_ARG and L.hm_light_stats_average(None, C.byref(nits)) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_average(C.byref(s), None) == HM_ERR_INVALID_ARG
    assert (code.value, nits.value) == (-7, -7.0)


# ---- the refusals before anything is queued, through all three entries ----
# name -> (what changes in the request, status, a word of the message).  The request: a 10-bit PQ picture, out_format rrggbb_le, the
# light step with explicit PQ / BT.2020 codes (the stand-alone entry needs them), no view, no OOTF step, unit_nits 0 (PQ: 10000),
# fraction 0.9999, dst_peak 203
REFUSALS = {
    "null light": (dict(light=None), HM_ERR_INVALID_ARG, "null argument"),
    "light: reserved": (dict(light=dict(reserved=(0, 1, 0))), HM_ERR_INVALID_ARG, "reserved"),
    "light: gain 0": (dict(light=dict(gain=0.0)), HM_ERR_INVALID_ARG, "gain"),
    "light: unknown from_transfer": (dict(light=dict(from_transfer=3)), HM_ERR_UNSUPPORTED, "transfer"),
    "light: unknown to_primaries": (dict(light=dict(to_primaries=3)), HM_ERR_UNSUPPORTED, "primaries"),
    "light: ICC in one field only": (dict(light=dict(from_transfer=-1)), HM_ERR_INVALID_ARG, "HM_LIGHT_FROM_ICC"),
    "a _BE target": (dict(fmt=RRGGBB_BE), HM_ERR_INVALID_ARG, "big-endian"),
    "a four-channel _BE target": (dict(fmt=RRGGBBAA_BE), HM_ERR_INVALID_ARG, "big-endian"),
    "unit_nits negative": (dict(unit_nits=-1.0), HM_ERR_INVALID_ARG, "unit_nits"),
    "unit_nits above 10000": (dict(unit_nits=10001.0), HM_ERR_INVALID_ARG, "unit_nits"),
    "unit_nits not finite": (dict(unit_nits=float("nan")), HM_ERR_INVALID_ARG, "unit_nits"),
    "ootf: reserved": (dict(ootf=dict(reserved=(0, 0, 1, 0, 0)), light=dict(from_transfer=18)), HM_ERR_INVALID_ARG, "reserved"),
    "ootf: unknown kind": (dict(ootf=dict(kind=2), light=dict(from_transfer=18)), HM_ERR_INVALID_ARG, "kind"),
    "ootf: display_peak 0": (dict(ootf=dict(display_peak=0.0), light=dict(from_transfer=18)), HM_ERR_INVALID_ARG, "display_peak"),
    "ootf: from PQ": (dict(ootf=dict()), HM_ERR_INVALID_ARG, "18"),
    "view: crop outside": (dict(view=((150, 90, 20, 20), (0, 0), 0)), HM_ERR_INVALID_ARG, "crop"),
    "view: unknown filter": (dict(view=((0, 0, 16, 16), (8, 8), 5)), HM_ERR_INVALID_ARG, "filter"),
    "view: an output size out of range (unused, and checked as the view entry checks it)": (dict(view=((0, 0, 160, 96), (40000, 96), 0)), HM_ERR_INVALID_ARG, "view"),
    # the measured entry alone
    "fraction 0": (dict(fraction=0.0), HM_ERR_INVALID_ARG, "fraction"),
    "fraction above 1": (dict(fraction=1.5), HM_ERR_INVALID_ARG, "fraction"),
    "fraction not finite": (dict(fraction=float("nan")), HM_ERR_INVALID_ARG, "fraction"),
    "null tone": (dict(tone=None), HM_ERR_INVALID_ARG, "null argument"),
    "tone: an explicit src_peak": (dict(tone=dict(src_peak=1000.0)), HM_ERR_INVALID_ARG, "hm_decode_item_to_device_tone"),
    "tone: a negative src_peak": (dict(tone=dict(src_peak=-1.0)), HM_ERR_INVALID_ARG, "src_peak"),
    "tone: reserved": (dict(tone=dict(reserved=(1, 0))), HM_ERR_INVALID_ARG, "reserved"),
    "tone: dst_peak 0": (dict(tone=dict(dst_peak=0.0)), HM_ERR_INVALID_ARG, "dst_peak"),
    "tone: unknown curve": (dict(tone=dict(curve=9)), HM_ERR_INVALID_ARG, "curve"),
    "tone: out_bits 8 with u16": (dict(tone=dict(out_bits=8), dtype=1), HM_ERR_INVALID_ARG, "out_bits"),
    "null destination": (dict(dest=None), HM_ERR_INVALID_ARG, "null argument"),
    "destination: len one byte short": (dict(short=1), HM_ERR_INVALID_ARG, "len"),
    "destination: linear light into integers": (dict(dtype=1), HM_ERR_INVALID_ARG, "float"),
}
MEASURED_ONLY = {n for n in REFUSALS if n.startswith(("fraction", "null tone", "tone:", "null destination", "destination:"))}


def request(capi, L, over):
    lt = None if "light" in over and over["light"] is None else light(capi, **dict(dict(from_transfer=16, from_primaries=9), **(over.get("light") or {})))
    oo = ootf(capi, **over["ootf"]) if over.get("ootf") is not None else None
    # (the measured entry has no unit_nits of its own: the tone step's)
    tn = None if "tone" in over and over["tone"] is None else tone(capi, **dict(dict(unit_nits=over.get("unit_nits", 0.0)), **(over.get("tone") or {})))
    vw = target_cases.make_view(capi, over["view"]) if over.get("view") else None
    fmt = over.get("fmt", RRGGBB_LE)
    ow, oh = (over["view"][1] if over.get("view") and over["view"][1] != (0, 0) else (over["view"][0][2:] if over.get("view") else (W, H)))
    dfmt = RGB if tn is not None and tn.out_bits == 8 and fmt == RRGGBB_LE else fmt
    d = None
    if not ("dest" in over and over["dest"] is None):
        d = dest(capi, L, dfmt, ow, oh, dtype=over.get("dtype", F32))
        d.len -= over.get("short", 0)
    return fmt, vw, lt, oo, tn, d, over.get("unit_nits", 0.0), over.get("fraction", 0.9999)


def call(capi, L, entry, data, over):
    """one request through one entry -> (status, message, *stats untouched, *out untouched)"""
    fmt, vw, lt, oo, tn, d, unit, fraction = request(capi, L, over)
    stats, out = filled(capi.LightStatsC), filled(capi.Decoded)
    if entry == "tensor":
        rc = L.hm_light_stats_of_tensor(fmt, 10, W, H, FAKE, W * 6, ref_of(vw), ref_of(lt), ref_of(oo), unit, C.byref(stats), None)
        return rc, L.hm_last_error().decode(), untouched(stats), True
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
        iid = L.hm_file_primary_item(h)
        if entry == "stats":
            rc = L.hm_decode_item_light_stats(h, iid, C.byref(prm), ref_of(vw), ref_of(lt), ref_of(oo), unit, C.byref(stats), C.byref(out))
        else:
            rc = L.hm_decode_item_to_device_measured(h, iid, C.byref(prm), ref_of(vw), ref_of(lt), ref_of(oo), ref_of(tn), fraction, ref_of(d), C.byref(out), C.byref(stats))
        return rc, L.hm_last_error().decode(), untouched(stats), untouched(out)
    finally:
        L.hm_file_close(h)


@pytest.mark.parametrize("entry", ["tensor", "stats", "measured"])
def test_refusals_before_anything_is_queued(capi, L, files, entry):
    for name, (over, status, word) in REFUSALS.items():
        if name in MEASURED_ONLY and entry != "measured":
            continue
        rc, msg, stats_kept, out_kept = call(capi, L, entry, files["pq"], over)
        assert rc == status and word in msg, (entry, name, rc, msg)
        assert stats_kept and out_kept, (entry, name)
    # what passes every check reaches the device probe (and there, without a GPU, finds none): the request itself is sound
    rc, msg, _, _ = call(capi, L, entry, files["pq"], {})
    assert rc in (0, HM_ERR_NO_DEVICE), (entry, rc, msg)


def test_null_out_and_stats(capi, L, files):
    fmt, vw, lt, oo, tn, d, unit, fraction = request(capi, L, {})
    stats, out = filled(capi.LightStatsC), filled(capi.Decoded)
    assert L.hm_light_stats_of_tensor(fmt, 10, W, H, FAKE, W * 6, None, C.byref(lt), None, 0.0, None, None) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_of_tensor(fmt, 10, W, H, None, W * 6, None, C.byref(lt), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    h = C.c_void_p()
    data = files["pq"]
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
        iid = L.hm_file_primary_item(h)
        assert L.hm_decode_item_light_stats(h, iid, C.byref(prm), None, C.byref(lt), None, 0.0, None, C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_light_stats(h, iid, C.byref(prm), None, C.byref(lt), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_light_stats(None, iid, C.byref(prm), None, C.byref(lt), None, 0.0, C.byref(stats), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device_measured(h, iid, C.byref(prm), None, C.byref(lt), None, C.byref(tn), 0.9999, C.byref(d), None, C.byref(stats)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_light_stats(h, 4242, C.byref(prm), None, C.byref(lt), None, 0.0, C.byref(stats), C.byref(out)) == HM_ERR_INVALID_ARG
        assert untouched(stats) and untouched(out)
    finally:
        L.hm_file_close(h)


def test_unit_nits_must_be_explicit_outside_pq(capi, L, files):
    """the stand-alone entry knows the transfer: sRGB without unit_nits is refused at once; with it the request reaches the device probe"""
    stats = filled(capi.LightStatsC)
    lt = light(capi, from_transfer=13, from_primaries=1)
    assert L.hm_light_stats_of_tensor(RGB, 8, 16, 16, FAKE, 48, None, C.byref(lt), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    assert "unit_nits must be given" in L.hm_last_error().decode() and untouched(stats)
    assert L.hm_light_stats_of_tensor(RGB, 8, 16, 16, FAKE, 48, None, C.byref(lt), None, 100.0, C.byref(stats), None) in (0, HM_ERR_NO_DEVICE)
    # from_* == 0 in the stand-alone form: the pixels carry no profile
    lt0 = light(capi)
    assert L.hm_light_stats_of_tensor(RGB, 8, 16, 16, FAKE, 48, None, C.byref(lt0), None, 100.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    assert "must be given" in L.hm_last_error().decode()
    # ... and no item whose profile HM_LIGHT_FROM_ICC could read
    icc = light(capi, from_transfer=-1, from_primaries=-1)
    assert L.hm_light_stats_of_tensor(RGB, 8, 16, 16, FAKE, 48, None, C.byref(icc), None, 100.0, C.byref(stats), None) == HM_ERR_UNSUPPORTED
    # a stride below the row, an odd stride of 16-bit samples
    pq = light(capi, from_transfer=16, from_primaries=9)
    assert L.hm_light_stats_of_tensor(RRGGBB_LE, 10, 16, 16, FAKE, 95, None, C.byref(pq), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_of_tensor(RRGGBB_LE, 10, 16, 16, FAKE, 97, None, C.byref(pq), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_of_tensor(RRGGBB_LE, 10, 0, 16, FAKE, 96, None, C.byref(pq), None, 0.0, C.byref(stats), None) == HM_ERR_INVALID_ARG
    assert L.hm_light_stats_of_tensor(RRGGBB_LE, 13, 16, 16, FAKE, 96, None, C.byref(pq), None, 0.0, C.byref(stats), None) == HM_ERR_UNSUPPORTED
    assert untouched(stats)


def test_derived_items_and_icc_without_a_profile_are_refused(capi, L, files):
    for entry in ("stats", "measured"):
        rc, msg, stats_kept, out_kept = call(capi, L, entry, files["iden"], dict(fmt=RGB, light=dict(from_transfer=0, from_primaries=0), tone=dict(unit_nits=100.0), unit_nits=100.0))
        assert rc == HM_ERR_UNSUPPORTED and "derived" in msg and stats_kept and out_kept, (entry, rc, msg)
        rc, msg, stats_kept, out_kept = call(capi, L, entry, files["pq"], dict(light=dict(from_transfer=-1, from_primaries=-1), tone=dict(unit_nits=100.0), unit_nits=100.0))
        assert rc == HM_ERR_INVALID_ARG and "ICC" in msg and stats_kept and out_kept, (entry, rc, msg)


def test_the_statistics_pass_asks_for_its_own_lds(hm_hooks):
    """what the launcher asks for as dynamic LDS (test hook hm_debug_light_lds, pass 3: the function the launch itself sizes its LDS
    with): lin, thr alone of the tone step - whatever the request says of enc and sg -, the OOTF tables, 2048 + 4 counters"""
    T = hm_hooks
    T.hm_debug_light_lds.argtypes, T.hm_debug_light_lds.restype = [C.c_int] * 5, C.c_longlong
    for bits in (8, 10, 12):
        for steps in (0, 1, 2, 3):
            for encode, eb in ((0, bits), (1, bits), (1, 8)):
                want = 4 * ((1 << bits) + 2048 + (2048 if steps & 2 else 0) + 2048 + 4)
                assert T.hm_debug_light_lds(bits, eb, encode, steps, 3) == want <= 64 * 1024, (bits, eb, encode, steps)


def test_python_argument_errors(pkg, files):
    """refused by the Python layer itself, before the library (or a device) is asked"""
    data = files["pq"]
    with pytest.raises(ValueError, match="only beside src_peak='measured'"):
        pkg.decode_to_tensor(data, out_format="rrggbb_le", light=True, tone=dict(dst_peak=203.0, percentile=0.5))
    with pytest.raises(ValueError, match="'measured'"):
        pkg.decode_to_tensor(data, out_format="rrggbb_le", light=True, tone=dict(dst_peak=203.0, src_peak="measure"))
    for bad in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            pkg.decode_to_tensor(data, out_format="rrggbb_le", light=True, tone=dict(dst_peak=203.0, src_peak="measured", percentile=bad))
    with pytest.raises(ValueError, match="unknown keys"):
        pkg.decode_to_tensor(data, out_format="rrggbb_le", light=True, tone=dict(dst_peak=203.0, src_peak="measured", percentil=0.5))
    with pytest.raises(ValueError, match="needs light="):
        pkg.decode_to_tensor(data, out_format="rrggbb_le", tone=dict(dst_peak=203.0, src_peak="measured"))
    with pytest.raises(ValueError, match="alpha= or gain="):
        pkg.decode_to_tensor(data, out_format="rrggbbaa_le", light=True, alpha="straight", tone=dict(dst_peak=203.0, src_peak="measured"))
    with pytest.raises(ValueError, match="only the single-item call"):
        pkg.decode_batch_to_tensor([data], out_format="rrggbb_le", light=True, tone=dict(dst_peak=203.0, src_peak="measured"))
    with pytest.raises(ValueError, match="only the single-item call"):
        pkg.decode_sequence_to_tensor(target_cases.files()["seq"], light=True, tone=dict(dst_peak=203.0, src_peak="measured", percentile=0.99))
    with pytest.raises(ValueError, match="needs light="):
        pkg.measure_light(data, light=None)
    with pytest.raises(ValueError, match="unit_nits"):
        pkg.measure_light(data, unit_nits=0)
    with pytest.raises(ValueError, match="crop"):
        pkg.measure_light(data, crop=(0, 0, 0, 5))
    with pytest.raises(ValueError, match="CUDA tensor"):
        pkg.measure_light_of_tensor(np.zeros((4, 4, 3), np.uint8), 8, dict(from_transfer="srgb", from_primaries="bt709"), unit_nits=100.0)
