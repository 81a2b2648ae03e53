"""The gain step (hm_device_gain) and the 'tmap' item, the part that needs no GPU: the new symbols, the payload reader against
tests/gainwriter.py, the file layer's answers (item kind, top-level list, hm_file_gain_map_of, hm_file_item_aux_type), the tables
hm_gain_table hands out against tests/gain_ref.py (written from the header's text), every refusal that is decided on the host - with
a pointer that is never dereferenced -, and the Python argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import gain_ref
import gainwriter
import synthutil

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_BITSTREAM, HM_ERR_NO_DEVICE = -1, -2, -3, -4
RGB, RGBA, RRGGBB_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 14, 15
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
TRIANGLE, NEAREST = 0, 1
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)
NEW_SYMBOLS = ("hm_file_gain_map_info", "hm_file_gain_map_of", "hm_file_item_aux_type", "hm_decode_item_to_device_gain", "hm_pipeline_submit_to_device_gain",
               "hm_gain_to_tensor", "hm_gain_table")
VENDOR_URN = "urn:com:example:hdr:aux:hdrgainmap"
inf, nan = float("inf"), float("nan")


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def pictures():
    """coded pictures for the items of the files below: a 64 x 64 4:2:0 base, a 32 x 32 4:0:0 map, a 32 x 32 4:2:0 picture"""
    return dict(base=synthutil.picture(51001, width=64, height=64), map=synthutil.picture(51002, width=32, height=32, chroma_format=0),
                colour=synthutil.picture(51003, width=32, height=32))


def params_of(capi, hb=0.0, ha=2.0, lo=0.0, hi=2.0, gamma=1.0, kb=1.0 / 64, ka=1.0 / 64, use_base=1, reserved=0):
    """hm_gain_params; lo, hi, gamma, kb, ka: a number for all three channels or three numbers"""
    p = capi.GainParams()
    p.base_headroom, p.alternate_headroom, p.use_base_primaries, p.reserved = hb, ha, use_base, reserved
    for name, v in (("map_min", lo), ("map_max", hi), ("gamma", gamma), ("base_offset", kb), ("alternate_offset", ka)):
        for c in range(3):
            getattr(p, name)[c] = v[c] if isinstance(v, (tuple, list)) else v
    return p


def model_params(p):
    return {short: [getattr(p, name)[c] for c in range(3)] for short, name in
            (("min", "map_min"), ("max", "map_max"), ("gamma", "gamma"), ("base_offset", "base_offset"), ("alternate_offset", "alternate_offset"))}


def gain_of(capi, p, headroom=1.0, map_item=0, reserved=(0, 0, 0, 0)):
    return capi.DeviceGain(map_item, headroom, p, (C.c_int32 * 4)(*reserved))


def light(capi, to_transfer=8, to_primaries=0, gain=1.0, from_transfer=13, from_primaries=1):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def dest(capi, layout, dtype, length, ptr=FAKE):
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = ptr, length, layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    return d


def lib_table(L, p, headroom, c, bits):
    buf = (C.c_float * (1 << bits))()
    assert L.hm_gain_table(C.byref(p), headroom, c, bits, buf) == 1 << bits, L.hm_last_error().decode()
    return np.frombuffer(buf, np.float32).copy()


def tmap_file(pictures, payload, refs=None, colr=(9, 16, 0, 1), map_kw=None, base_colr=None, hidden=True):
    """(file bytes, base id, map id, tmap id)"""
    w = gainwriter.Writer()
    base = w.hvc1(pictures["base"], (64, 64), colr=base_colr)
    kw = dict(chroma_format=0, hidden=hidden)
    kw.update(map_kw or {})
    gmap = w.hvc1(pictures["colour" if kw["chroma_format"] else "map"], (32, 32), **kw)
    t = w.tmap(base, gmap, payload, (64, 64), colr=colr, clli=(1000, 400), refs=refs)
    return w.finish(primary=base), base, gmap, t


def opened(L, data):
    h = C.c_void_p()
    rc = L.hm_file_open(data, len(data), C.byref(h))
    assert rc == 0, L.hm_last_error().decode()
    return h


def info_of(capi, L, data, tmap):
    h = opened(L, data)
    try:
        info = capi.GainMapInfo()
        rc = L.hm_file_gain_map_info(h, tmap, C.byref(info))
        return rc, L.hm_last_error().decode(), info
    finally:
        L.hm_file_close(h)


def test_the_new_symbols_exist(hm):
    for name in NEW_SYMBOLS:
        assert hasattr(hm, name), name


CHANNELS = {
    "one": [gainwriter.channel(min=(-3, 4), max=(7, 2), gamma=(11, 5), base_offset=(1, 64), alternate_offset=(-1, 32))],
    "three": [gainwriter.channel(min=(-1, 2), max=(5, 2), gamma=(1, 1), base_offset=(1, 64), alternate_offset=(1, 64)),
              gainwriter.channel(min=(0, 1), max=(-2147483648, 1073741824), gamma=(22, 10), base_offset=(-5, 1000), alternate_offset=(3, 7)),
              gainwriter.channel(min=(-7, 8), max=(2147483647, 536870912), gamma=(4294967295, 2147483648), base_offset=(0, 9), alternate_offset=(-2147483648, 4294967295))],
}


@pytest.mark.parametrize("name", sorted(CHANNELS))
@pytest.mark.parametrize("use_base", (False, True))
def test_payload_round_trip(capi, L, pictures, name, use_base):
    """negative numerators, is_multichannel 0 and 1, both flag bits, denominators up to 2^32 - 1: every fraction as n / d in double"""
    chans = CHANNELS[name]
    heads = dict(base_headroom=(1, 3), alternate_headroom=(4000000000, 1000000000))
    data, base, gmap, t = tmap_file(pictures, gainwriter.tmap_payload(chans, use_base=use_base, writer_version=7, **heads))
    rc, msg, info = info_of(capi, L, data, t)
    assert rc == 0, msg
    hb, ha, want = gainwriter.as_doubles(chans, **heads)
    p = info.params
    assert (info.base_item, info.map_item) == (base, gmap)
    assert (p.base_headroom, p.alternate_headroom, p.use_base_primaries, p.reserved) == (hb, ha, int(use_base), 0)
    got = model_params(p)
    assert got == want, (got, want)
    assert any(v < 0 for f in want.values() for v in f)
    assert (info.alt_has_nclx, info.alt_primaries, info.alt_transfer) == (1, 9, 16)
    assert gain_ref.channels(got) == (1 if name == "one" else 3)


def test_payload_refusals(capi, L, pictures):
    ok = gainwriter.channel()
    good = gainwriter.tmap_payload([ok])
    assert info_of(capi, L, tmap_file(pictures, good)[0], 3)[0] == 0
    three = gainwriter.tmap_payload([ok, ok, ok])
    cases = [(gainwriter.tmap_payload([gainwriter.channel(gamma=(0, 5))]), HM_ERR_BITSTREAM, "gamma"),
             (gainwriter.tmap_payload([ok, ok, gainwriter.channel(gamma=(0, 1))]), HM_ERR_BITSTREAM, "gamma"),
             (gainwriter.tmap_payload([ok], base_headroom=(1, 0)), HM_ERR_BITSTREAM, "denominator"),
             (gainwriter.tmap_payload([ok], alternate_headroom=(0, 0)), HM_ERR_BITSTREAM, "denominator"),
             (good[:-1], HM_ERR_BITSTREAM, "truncated"), (good[:5], HM_ERR_BITSTREAM, "truncated"), (good[:22], HM_ERR_BITSTREAM, "truncated"),
             (three[:len(good)], HM_ERR_BITSTREAM, "truncated"), (three[:-4], HM_ERR_BITSTREAM, "truncated"),
             (gainwriter.tmap_payload([ok], multichannel=True), HM_ERR_BITSTREAM, "truncated"),
             (gainwriter.tmap_payload([ok], version=1), HM_ERR_UNSUPPORTED, "version"),
             (gainwriter.tmap_payload([ok], minimum_version=1), HM_ERR_UNSUPPORTED, "minimum_version"),
             (gainwriter.tmap_payload([ok], version=255, minimum_version=65535), HM_ERR_UNSUPPORTED, "version")]
    for field in ("min", "max", "gamma", "base_offset", "alternate_offset"):
        cases.append((gainwriter.tmap_payload([gainwriter.channel(**{field: (1, 0)})]), HM_ERR_BITSTREAM, "denominator"))
    for payload, status, word in cases:
        rc, msg, _ = info_of(capi, L, tmap_file(pictures, payload)[0], 3)
        assert rc == status and word in msg, (rc, msg, word, len(payload))
    # flag bits other than the two, and a writer_version, change nothing; bytes behind the payload are not looked at
    rc, msg, info = info_of(capi, L, tmap_file(pictures, gainwriter.tmap_payload([ok], writer_version=65535, extra_flags=0x3F) + b"\0\1\2")[0], 3)
    assert rc == 0 and info.params.use_base_primaries == 0, msg
    # the references: exactly two, base and map
    for refs in ([1], [1, 2, 1], [], [3, 2], [1, 3], [1, 1], [1, 9], [0, 2]):
        rc, msg, _ = info_of(capi, L, tmap_file(pictures, good, refs=refs)[0], 3)
        assert rc == HM_ERR_BITSTREAM and "reference" in msg, (refs, rc, msg)
    rc, msg, _ = info_of(capi, L, tmap_file(pictures, good)[0], 1)
    assert rc == HM_ERR_INVALID_ARG and "tmap" in msg
    assert info_of(capi, L, tmap_file(pictures, good)[0], 9)[0] == HM_ERR_INVALID_ARG


def test_file_level_answers(capi, L, pictures):
    """the kind of a 'tmap' item; the base stays a top-level image, the 'tmap' item is never listed, the map as its hidden flag says;
    hm_file_gain_map_of; hm_file_item_aux_type; hm_decode_item's refusal names the entry point"""
    payload = gainwriter.tmap_payload([gainwriter.channel()])
    for hidden in (True, False):
        data, base, gmap, t = tmap_file(pictures, payload, hidden=hidden)
        h = opened(L, data)
        try:
            assert [L.hm_file_item_kind(h, i) for i in (base, gmap, t)] == [capi.HM_ITEM_HVC1, capi.HM_ITEM_HVC1, capi.HM_ITEM_TMAP] and capi.HM_ITEM_TMAP == 5
            ids = (C.c_uint32 * 8)()
            n = L.hm_file_top_level_images(h, ids, 8)
            assert list(ids[:n]) == ([base] if hidden else [base, gmap])
            assert (L.hm_file_gain_map_of(h, base), L.hm_file_gain_map_of(h, gmap), L.hm_file_gain_map_of(h, t), L.hm_file_gain_map_of(h, 77)) == (t, 0, 0, 0)
            prm, out = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
            assert L.hm_decode_item(h, t, C.byref(prm), C.byref(out)) == HM_ERR_UNSUPPORTED
            assert "hm_decode_item_to_device_gain" in L.hm_last_error().decode()
            levels = capi.LightLevels()
            assert L.hm_file_item_light_levels(h, t, C.byref(levels)) == 0 and (levels.has_clli, levels.max_content_light_level) == (1, 1000)
        finally:
            L.hm_file_close(h)
    # two 'tmap' items over one base: the first in item order; a vendor gain map among the 'auxl' items, found by its URN
    w = gainwriter.Writer()
    base = w.hvc1(pictures["base"], (64, 64))
    aux = w.aux(pictures["map"], (32, 32), base, VENDOR_URN)
    alpha = w.alpha(pictures["map"], (32, 32), base)
    t1 = w.tmap(base, aux, payload, (64, 64))
    t2 = w.tmap(base, alpha, payload, (64, 64))
    other = w.tmap(aux, base, payload, (32, 32))
    h = opened(L, w.finish(primary=base))
    try:
        assert (L.hm_file_gain_map_of(h, base), L.hm_file_gain_map_of(h, aux)) == (t1, other) and t1 < t2
        ids = (C.c_uint32 * 8)()
        assert L.hm_file_top_level_images(h, ids, 8) == 1 and ids[0] == base  # (auxiliary images stay sub-images)
        buf = C.create_string_buffer(64)
        assert L.hm_file_item_aux_type(h, aux, buf, 64) == len(VENDOR_URN) and buf.value.decode() == VENDOR_URN
        assert L.hm_file_item_aux_type(h, alpha, buf, 64) > 0 and buf.value.decode() == "urn:mpeg:hevc:2015:auxid:1"
        assert L.hm_file_item_aux_type(h, base, buf, 64) == 0 and buf.value == b""
        small = C.create_string_buffer(b"\xff" * 8, 8)
        assert L.hm_file_item_aux_type(h, aux, small, 8) == len(VENDOR_URN) and small.raw == VENDOR_URN[:7].encode() + b"\0"
        assert L.hm_file_item_aux_type(h, aux, None, 0) == len(VENDOR_URN)
        assert L.hm_file_item_aux_type(h, 99, buf, 64) == HM_ERR_INVALID_ARG and L.hm_file_item_aux_type(h, aux, None, 4) == HM_ERR_INVALID_ARG
        found = [i for i in range(1, 8) if L.hm_file_item_kind(h, i) == capi.HM_ITEM_HVC1 and L.hm_file_item_aux_type(h, i, buf, 64) > 0 and b"gainmap" in buf.value]
        assert found == [aux]
    finally:
        L.hm_file_close(h)


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


TABLE_PARAMS = (dict(), dict(gamma=2.2), dict(lo=-1.5, hi=3.25, gamma=0.7), dict(hb=0.5, ha=4.0, lo=-2.0, hi=0.0, gamma=1.0),
                dict(lo=(0.0, -1.0, 0.25), hi=(2.0, 2.5, 3.0), gamma=(1.0, 2.2, 0.5)), dict(hb=3.0, ha=1.0, lo=-1.0, hi=2.0, gamma=1.8))


def test_tables_against_the_model(capi, L):
    """every entry within 1 float32 ulp of the model's: two correct double evaluations may round apart, and no more"""
    for kw in TABLE_PARAMS:
        p = params_of(capi, **kw)
        mp = model_params(p)
        for headroom in (0.0, 0.75, 1.0, 2.5, 5.0, inf):
            for bits in (8, 10, 12):
                w = gain_ref.weight(headroom, p.base_headroom, p.alternate_headroom)
                for c in range(3):
                    got = lib_table(L, p, headroom, c, bits)
                    want = gain_ref.table(w, mp["min"][c], mp["max"][c], mp["gamma"][c], bits)
                    assert got.shape == want.shape == (1 << bits,) and (got > 0).all()
                    d = ulps(got, want)
                    assert d.max() <= 1, (kw, headroom, bits, c, int(d.argmax()), got[d.argmax()], want[d.argmax()])


def test_table_anchors(capi, L):
    """exact: wgt = 0 gives 1.0f everywhere; a headroom at or below Hb, at or above Ha clamps; Ha < Hb reverses; +inf is wgt = 1;
    with gamma = 1 the ends of the table are exp2 of whole numbers"""
    p = params_of(capi, hb=1.0, ha=3.0, lo=-1.0, hi=2.0, gamma=2.2)
    ones = np.ones(256, np.float32)
    for headroom in (0.0, 0.5, 1.0):
        assert np.array_equal(lib_table(L, p, headroom, 1, 8), ones), headroom
    full = lib_table(L, p, 3.0, 0, 8)
    assert full[0] == np.float32(0.5) and full[255] == np.float32(4.0) and (np.diff(full) > 0).all()
    for headroom in (3.0, 3.5, 100.0, inf):
        assert np.array_equal(lib_table(L, p, headroom, 2, 8), full), headroom
    half = lib_table(L, p, 2.0, 0, 8)  # wgt = 0.5, exactly
    assert half[0] == np.float32(2.0 ** -0.5) and half[255] == np.float32(2.0) and not np.array_equal(half, full)
    # Ha < Hb: the alternate rendition is the darker one - the weight falls as the headroom rises
    r = params_of(capi, hb=3.0, ha=1.0, lo=-1.0, hi=2.0, gamma=2.2)
    for headroom in (0.0, 1.0):
        assert np.array_equal(lib_table(L, r, headroom, 0, 8), full), headroom
    for headroom in (3.0, 4.0, inf):
        assert np.array_equal(lib_table(L, r, headroom, 0, 8), ones), headroom
    assert np.array_equal(lib_table(L, r, 2.0, 0, 8), half)
    assert (gain_ref.weight(inf, 1.0, 3.0), gain_ref.weight(inf, 3.0, 1.0), gain_ref.weight(2.0, 3.0, 1.0), gain_ref.weight(0.0, 1.0, 3.0)) == (1.0, 0.0, 0.5, 0.0)
    # gamma = 1 takes no pow: u = v / mpeak as it is - the entries at v = 0, 51 * k of an 8-bit table with min 0, max 5 are exp2(k)
    g1 = params_of(capi, hb=0.0, ha=1.0, lo=0.0, hi=5.0, gamma=1.0)
    t = lib_table(L, g1, 1.0, 0, 8)
    assert [float(t[51 * k]) for k in range(6)] == [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    for bits in (10, 12):
        t = lib_table(L, g1, 1.0, 0, bits)
        assert (t[0], t[-1]) == (1.0, 32.0) and t.shape == (1 << bits,)


def test_gain_table_refusals(capi, L):
    out = (C.c_float * 4096)()
    ok = params_of(capi)
    assert L.hm_gain_table(C.byref(ok), 1.0, 0, 8, out) == 256
    assert L.hm_gain_table(None, 1.0, 0, 8, out) == HM_ERR_INVALID_ARG and L.hm_gain_table(C.byref(ok), 1.0, 0, 8, None) == HM_ERR_INVALID_ARG
    for c in (-1, 3):
        assert L.hm_gain_table(C.byref(ok), 1.0, c, 8, out) == HM_ERR_INVALID_ARG
    for bits in (7, 13, 16):
        assert L.hm_gain_table(C.byref(ok), 1.0, 0, bits, out) == HM_ERR_UNSUPPORTED and "bits" in L.hm_last_error().decode()
    for h in (nan, -0.5, -inf):
        assert L.hm_gain_table(C.byref(ok), h, 0, 8, out) == HM_ERR_INVALID_ARG and "headroom" in L.hm_last_error().decode(), h
    for bad, word in BAD_PARAMS:
        assert L.hm_gain_table(C.byref(params_of(capi, **bad)), 1.0, 0, 8, out) == HM_ERR_INVALID_ARG and word in L.hm_last_error().decode(), (bad, L.hm_last_error().decode())


BAD_PARAMS = ((dict(hb=2.0, ha=2.0), "alternate_headroom"), (dict(gamma=0.0), "gamma"), (dict(gamma=-1.0), "gamma"), (dict(gamma=(1.0, nan, 1.0)), "gamma"),
              (dict(gamma=(1.0, 1.0, inf)), "gamma"), (dict(lo=nan), "finite"), (dict(hi=(0.0, inf, 0.0)), "finite"), (dict(kb=-inf), "finite"),
              (dict(ka=(0.0, 0.0, nan)), "finite"), (dict(hb=nan), "finite"), (dict(ha=inf), "finite"), (dict(reserved=1), "reserved"))


def step_alone(capi, L, gn, fmt=RGB, bits=8, size=(64, 48), map_size=(32, 24), map_bits=8, view=None, lt="default", tone=None, layout=CHW, dtype=F32, out_size=None,
               length=None, map_stride=None):
    """hm_gain_to_tensor on pointers that are never dereferenced"""
    w, h = size
    ow, oh = out_size or size
    obpp = {RGB: 3, RGBA: 4, RRGGBB_LE: 6, RRGGBBAA_LE: 8, RRGGBB_BE: 6}.get(fmt, 3)
    c = 3 if obpp in (3, 6) else 4
    d = dest(capi, layout, dtype, length if length is not None else ow * oh * c * {U8: 1, U16: 2, F16: 2, F32: 4}[dtype])
    if lt == "default":
        lt = light(capi)
    ms = map_stride if map_stride is not None else map_size[0] * (2 if map_bits > 8 else 1)
    rc = L.hm_gain_to_tensor(fmt, bits, w, h, FAKE, w * obpp, FAKE + 0x100000, ms, map_size[0], map_size[1], map_bits, C.byref(view) if view is not None else None,
                             C.byref(lt) if lt is not None else None, C.byref(tone) if tone is not None else None, C.byref(gn) if gn is not None else None, C.byref(d), None)
    return rc, L.hm_last_error().decode()


def test_the_steps_refusals(capi, L):
    """decided on the host, before a device is looked for: the call that passes them all finds no device here, or on a GPU machine
    refuses the pointer"""
    ok = gain_of(capi, params_of(capi))
    rc, msg = step_alone(capi, L, ok)
    assert rc in (HM_ERR_NO_DEVICE, HM_ERR_INVALID_ARG) and "gain" not in msg, msg
    rc, msg = step_alone(capi, L, ok, lt=None)
    assert rc == HM_ERR_INVALID_ARG and "gain: null light step" in msg
    assert step_alone(capi, L, None)[0] == HM_ERR_INVALID_ARG
    for bad, word in BAD_PARAMS:
        rc, msg = step_alone(capi, L, gain_of(capi, params_of(capi, **bad)))
        assert rc == HM_ERR_INVALID_ARG and word in msg, (bad, rc, msg)
    for h in (nan, -1.0, -inf):
        rc, msg = step_alone(capi, L, gain_of(capi, params_of(capi), headroom=h))
        assert rc == HM_ERR_INVALID_ARG and "headroom" in msg, (h, rc, msg)
    for k in range(4):
        rc, msg = step_alone(capi, L, gain_of(capi, params_of(capi), reserved=[int(i == k) for i in range(4)]))
        assert rc == HM_ERR_INVALID_ARG and "reserved" in msg, (k, rc, msg)
    # (+inf and 0 are headrooms like any other)
    for h in (inf, 0.0):
        assert "gain" not in step_alone(capi, L, gain_of(capi, params_of(capi), headroom=h))[1]
    # the geometry: a whole factor per axis, the crop on the map's raster
    for map_size, status in (((33, 24), HM_ERR_UNSUPPORTED), ((32, 25), HM_ERR_UNSUPPORTED), ((65, 48), HM_ERR_UNSUPPORTED), ((31, 24), HM_ERR_UNSUPPORTED),
                             ((64, 48), None), ((32, 48), None), ((22, 16), None), ((1, 1), None)):
        rc, msg = step_alone(capi, L, ok, map_size=map_size)
        assert (rc == status and "map" in msg) if status else "gain" not in msg, (map_size, rc, msg)
    V = capi.DeviceView
    rc, msg = step_alone(capi, L, ok, view=V(1, 0, 32, 32, 16, 16, TRIANGLE), out_size=(16, 16))
    assert rc == HM_ERR_INVALID_ARG and "crop_x 1" in msg, msg
    rc, msg = step_alone(capi, L, ok, view=V(2, 3, 32, 32, 0, 0, TRIANGLE), out_size=(32, 32))
    assert rc == HM_ERR_INVALID_ARG and "crop_y 3" in msg, msg
    rc, msg = step_alone(capi, L, ok, view=V(2, 4, 31, 33, 16, 16, NEAREST), out_size=(16, 16))
    assert "gain" not in msg, msg
    rc, msg = step_alone(capi, L, ok, map_size=(64, 48), view=V(1, 3, 31, 33, 16, 16, TRIANGLE), out_size=(16, 16))  # (sx = sy = 1: any origin)
    assert "gain" not in msg, msg
    # the map's depth, its stride; targets; what the light, tone and destination checks refuse stays refused
    for bits in (7, 13, 16):
        rc, msg = step_alone(capi, L, ok, map_bits=bits)
        assert rc == HM_ERR_UNSUPPORTED and "bits" in msg, (bits, msg)
    rc, msg = step_alone(capi, L, ok, map_stride=31)
    assert rc == HM_ERR_INVALID_ARG and "map_stride" in msg, msg
    rc, msg = step_alone(capi, L, ok, map_bits=10, map_stride=65)
    assert rc == HM_ERR_INVALID_ARG and "odd" in msg, msg
    rc, msg = step_alone(capi, L, ok, fmt=RRGGBB_BE, bits=10, dtype=F32)
    assert rc == HM_ERR_INVALID_ARG and "_LE" in msg, msg
    rc, msg = step_alone(capi, L, ok, fmt=0x101)
    assert rc == HM_ERR_UNSUPPORTED and "planar" in msg, msg
    rc, msg = step_alone(capi, L, ok, dtype=U8)
    assert rc == HM_ERR_INVALID_ARG and "float dtype" in msg, msg
    rc, msg = step_alone(capi, L, ok, lt=light(capi, from_transfer=0))
    assert rc == HM_ERR_INVALID_ARG and "from_transfer" in msg, msg
    rc, msg = step_alone(capi, L, ok, length=64 * 48 * 12 - 1)
    assert rc == HM_ERR_INVALID_ARG and "len" in msg, msg
    tn = capi.DeviceTone(1, 0, 0.0, 203.0, 203.0, 0.0, (C.c_int32 * 2)(0, 0))
    rc, msg = step_alone(capi, L, ok, tone=tn)
    assert rc == HM_ERR_INVALID_ARG and "src_peak" in msg, msg
    for fmt, bits in ((RGBA, 8), (RRGGBB_LE, 10), (RRGGBBAA_LE, 12)):
        assert "gain" not in step_alone(capi, L, ok, fmt=fmt, bits=bits)[1]


def decode_gain(capi, L, data, item, gn, fmt=RGB, view=None, size=(64, 64)):
    h = opened(L, data)
    try:
        prm, out = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
        d = dest(capi, CHW, F32, size[0] * size[1] * 12)
        lt = light(capi, from_transfer=0, from_primaries=0)
        rc = L.hm_decode_item_to_device_gain(h, item, C.byref(prm), C.byref(view) if view is not None else None, C.byref(lt), None, C.byref(gn), C.byref(d), C.byref(out))
        return rc, L.hm_last_error().decode()
    finally:
        L.hm_file_close(h)


def test_the_decodes_refusals(capi, L, pictures):
    """what the file says about the map is judged before anything is queued (no device is needed to be refused)"""
    good, other_space = gainwriter.tmap_payload([gainwriter.channel()], use_base=True), gainwriter.tmap_payload([gainwriter.channel()])
    data, base, gmap, t = tmap_file(pictures, good)
    from_file = gain_of(capi, capi.GainParams(), headroom=1.0)
    rc, msg = decode_gain(capi, L, data, t, from_file)
    assert rc in (HM_ERR_NO_DEVICE, HM_ERR_INVALID_ARG) and "gain" not in msg, msg
    rc, msg = decode_gain(capi, L, data, base, from_file)
    assert rc == HM_ERR_INVALID_ARG and "not a 'tmap' item" in msg, msg
    rc, msg = decode_gain(capi, L, data, t, gain_of(capi, params_of(capi), map_item=gmap))
    assert rc == HM_ERR_INVALID_ARG and "brings its own" in msg, msg
    explicit = gain_of(capi, params_of(capi), map_item=gmap)
    assert "gain" not in decode_gain(capi, L, data, base, explicit)[1]
    rc, msg = decode_gain(capi, L, data, base, gain_of(capi, params_of(capi), map_item=9))
    assert rc == HM_ERR_INVALID_ARG and "no item 9" in msg, msg
    rc, msg = decode_gain(capi, L, data, base, gain_of(capi, params_of(capi), map_item=base))
    assert rc == HM_ERR_INVALID_ARG and "itself" in msg, msg
    rc, msg = decode_gain(capi, L, data, base, gain_of(capi, params_of(capi), map_item=t))
    assert rc == HM_ERR_UNSUPPORTED and "tmap" in msg, msg
    rc, msg = decode_gain(capi, L, data, base, gain_of(capi, params_of(capi, gamma=0.0), map_item=gmap))
    assert rc == HM_ERR_INVALID_ARG and "gamma" in msg, msg
    # parameters from the payload that the step cannot use are the file's fault
    rc, msg = decode_gain(capi, L, tmap_file(pictures, gainwriter.tmap_payload([gainwriter.channel()], base_headroom=(2, 1), alternate_headroom=(4, 2)))[0], t, from_file)
    assert rc == HM_ERR_BITSTREAM and "alternate_headroom" in msg, msg
    rc, msg = decode_gain(capi, L, data, t, gain_of(capi, capi.GainParams(), headroom=nan))
    assert rc == HM_ERR_INVALID_ARG and "headroom" in msg, msg
    rc, msg = decode_gain(capi, L, data, t, gain_of(capi, capi.GainParams(), reserved=(0, 0, 0, 5)))
    assert rc == HM_ERR_INVALID_ARG and "reserved" in msg, msg
    # the open steps, each named: a colour map, a map deeper than 12 bits, the gain in the alternate primaries
    rc, msg = decode_gain(capi, L, tmap_file(pictures, good, map_kw=dict(chroma_format=1))[0], t, from_file)
    assert rc == HM_ERR_UNSUPPORTED and "4:0:0" in msg and "open step" in msg, msg
    rc, msg = decode_gain(capi, L, tmap_file(pictures, good, map_kw=dict(bit_depth=14))[0], t, from_file)
    assert rc == HM_ERR_UNSUPPORTED and "14 bits" in msg and "open step" in msg, msg
    for base_colr in ((1, 13, 6, 1), None):  # (a base without a colr: BT.709)
        rc, msg = decode_gain(capi, L, tmap_file(pictures, other_space, colr=(9, 16, 0, 1), base_colr=base_colr)[0], t, from_file)
        assert rc == HM_ERR_UNSUPPORTED and "alternate primaries" in msg and "open step" in msg, msg
    for payload, colr in ((good, (9, 16, 0, 1)), (other_space, (1, 16, 0, 1)), (other_space, None)):
        assert "gain" not in decode_gain(capi, L, tmap_file(pictures, payload, colr=colr, base_colr=(1, 13, 6, 1))[0], t, from_file)[1]
    # the geometry against the declared sizes: a 24 x 24 map (clap) for the 64 x 64 base; a crop off the map's raster
    w = gainwriter.Writer()
    b = w.hvc1(pictures["base"], (64, 64))
    m = w.hvc1(pictures["map"], (32, 32), chroma_format=0, hidden=True, transforms=[("clap", (24, 1, 24, 1, 0, 1, 0, 1))])
    tt = w.tmap(b, m, good, (64, 64))
    rc, msg = decode_gain(capi, L, w.finish(primary=b), tt, from_file)
    assert rc == HM_ERR_UNSUPPORTED and "24 x 24 map" in msg, msg
    rc, msg = decode_gain(capi, L, data, t, from_file, view=capi.DeviceView(3, 0, 32, 32, 0, 0, TRIANGLE), size=(32, 32))
    assert rc == HM_ERR_INVALID_ARG and "crop_x 3" in msg, msg
    # the pipeline refuses at submission
    cfg = capi.PipelineConfig(1, 2, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    if L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0:
        try:
            colour = tmap_file(pictures, good, map_kw=dict(chroma_format=1))[0]
            d = dest(capi, CHW, F32, 64 * 64 * 12)
            lt = light(capi, from_transfer=0, from_primaries=0)
            assert L.hm_pipeline_submit_to_device_gain(pipe, colour, len(colour), t, 0, None, C.byref(lt), None, C.byref(from_file), C.byref(d)) == HM_ERR_UNSUPPORTED
            assert "4:0:0" in L.hm_last_error().decode() and L.hm_pipeline_pending(pipe) == 0
            assert L.hm_pipeline_submit_to_device_gain(pipe, colour, len(colour), t, 0, None, None, None, C.byref(from_file), C.byref(d)) == HM_ERR_INVALID_ARG
        finally:
            L.hm_pipeline_destroy(pipe)


def decode_module(pkg):
    import sys
    return sys.modules[pkg.__name__ + ".decode"]


def test_python_argument_checks(pkg, capi, pictures):
    good = gainwriter.tmap_payload([gainwriter.channel()])
    data, base, gmap, t = tmap_file(pictures, good)
    plain = gainwriter.Writer()
    only = plain.hvc1(pictures["base"], (64, 64))
    plain = plain.finish(primary=only)
    for call, arg in ((pkg.decode_to_tensor, data), (pkg.decode_batch_to_tensor, [data])):
        with pytest.raises(ValueError, match="needs light"):
            call(arg, gain=dict(headroom=1.0))
        with pytest.raises(ValueError, match="headroom"):
            call(arg, light=True, gain=dict())
        with pytest.raises(ValueError, match="unknown keys"):
            call(arg, light=True, gain=dict(headroom=1.0, gama=2.2))
        with pytest.raises(ValueError, match="a dict"):
            call(arg, light=True, gain=2.0)
        with pytest.raises(ValueError, match="without map_item"):
            call(arg, light=True, gain=dict(headroom=1.0, gamma=2.2))
        with pytest.raises(ValueError, match="alternate_headroom"):
            call(arg, light=True, gain=dict(headroom=1.0, map_item=gmap))
        with pytest.raises(ValueError, match="map_max"):
            call(arg, light=True, gain=dict(headroom=1.0, map_item=gmap, alternate_headroom=2.0))
        with pytest.raises(ValueError, match="one number or three"):
            call(arg, light=True, gain=dict(headroom=1.0, map_item=gmap, alternate_headroom=2.0, map_max=(1.0, 2.0)))
        with pytest.raises(pkg.HmError, match="alpha step beside"):
            call(arg, light=True, out_format="rgba", alpha="straight", gain=dict(headroom=math.inf))
    with pytest.raises(ValueError, match="no 'tmap' item"):
        pkg.decode_to_tensor(plain, light=True, gain=dict(headroom=1.0))
    with pytest.raises(ValueError, match="no 'tmap' item"):
        pkg.decode_batch_to_tensor([data, plain], light=True, gain=dict(headroom=1.0))
    with pytest.raises(ValueError, match="no 'tmap' item"):
        pkg.decode_to_tensor(data, item_id=gmap, light=True, gain=dict(headroom=1.0))
    g = decode_module(pkg)._gain_of(dict(headroom=math.inf, map_item=gmap, alternate_headroom=3.0, map_max=(1.0, 2.0, 3.0), gamma=2.2, use_base_primaries=False), object())
    assert (g.map_item, g.headroom, g.params.alternate_headroom, list(g.params.map_max), list(g.params.gamma), g.params.use_base_primaries) == \
        (gmap, inf, 3.0, [1.0, 2.0, 3.0], [2.2] * 3, 0)
    assert list(g.params.base_offset) == [1.0 / 64] * 3 and list(g.params.map_min) == [0.0] * 3
    assert C.sizeof(capi.GainParams) == 17 * 8 + 8 and C.sizeof(capi.DeviceGain) == 8 + C.sizeof(capi.GainParams) + 16
