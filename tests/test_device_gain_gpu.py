"""GPU: the gain step (hm_gain_to_tensor, hm_decode_item_to_device_gain, hm_pipeline_submit_to_device_gain and gain= of the Python
calls).  Everything is bit-exact: the expected image of every case is the model of tests/gain_ref.py on top of light_ref and tone_ref,
fed with the library's tables (hm_light_table, hm_tone_table, hm_gain_table - held to their models within 1 ulp by the CPU tests),
hm_light_matrix's matrix and hm_view_filter_taps' weights, so only the device arithmetic is under test.  Every destination sits in a
guarded buffer pre-filled with 0xA5 and the WHOLE buffer is compared, as in test_device_alpha_gpu.py.  Where the arrays of the
step-alone tests are made, a census is asserted: map codes 0 and mpeak and base codes 0 and peak are present (and, at 10 bits, codes
above the peak, which are read as the peak)."""
import ctypes as C
import math

import numpy as np
import pytest

import gain_ref
import gainwriter
import light_ref
import pipeline
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv
import tone_ref
from test_device_light_gpu import lib as light_lib  # noqa: F401  (a fixture: hm_light_table, hm_light_matrix, hm_view_filter_taps, each result once)
from test_device_tone_gpu import lib as tone_lib  # noqa: F401  (a fixture on top of it: hm_tone_table)

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
ONE, ZERO = [1.0] * 4, [0.0] * 4
SCALE, BIAS = [2.0, 0.75, 16.0, 1.0 / 255.0], [-1.0, 0.125, 0.5, -0.25]
THREADS = 2
inf = float("inf")
# SDR white at 203 cd/m2 in units of 10000 cd/m2: what an sRGB base needs to land on PQ codes
SDR_GAIN = 0.0203
VENDOR_URN = "urn:com:example:hdr:aux:hdrgainmap"

# parameter sets (hm_gain_params): gamma 1 and 2.2, a negative min (darkening), offsets zero and non-zero, one table and three
PARAMS = {
    "plain": dict(hb=0.0, ha=2.0, lo=0.0, hi=2.0, gamma=1.0, kb=1.0 / 64, ka=1.0 / 64),
    "dark_gamma": dict(hb=0.0, ha=3.0, lo=-1.0, hi=3.0, gamma=2.2, kb=1.0 / 64, ka=1.0 / 128),
    "no_offsets": dict(hb=1.0, ha=2.0, lo=-0.5, hi=1.5, gamma=1.0, kb=0.0, ka=0.0),
    "three": dict(hb=0.5, ha=2.5, lo=(-0.5, 0.0, -1.0), hi=(2.0, 2.5, 1.5), gamma=(1.0, 2.2, 0.8), kb=(1.0 / 64, 0.0, 1.0 / 32), ka=(1.0 / 64, 1.0 / 16, 0.0)),
}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def params_of(capi, hb, ha, lo, hi, gamma, kb, ka):
    p = capi.GainParams()
    p.base_headroom, p.alternate_headroom, p.use_base_primaries = hb, ha, 1
    for name, v in (("map_min", lo), ("map_max", hi), ("gamma", gamma), ("base_offset", kb), ("alternate_offset", ka)):
        for c in range(3):
            getattr(p, name)[c] = v[c] if isinstance(v, tuple) else v
    return p


def model_params(p):
    return {short: [getattr(p, name)[c] for c in range(3)] for short, name in
            (("min", "map_min"), ("max", "map_max"), ("gamma", "gamma"), ("base_offset", "base_offset"), ("alternate_offset", "alternate_offset"))}


@pytest.fixture(scope="module")
def lib(tone_lib, L, capi):
    """what the model is fed with, each computed once: the light and tone tests' tables, matrices and taps, and gain(params, headroom,
    map_bits) -> the nch tables of hm_gain_table (nch: the model's count of distinct parameter sets)"""
    gains = {}

    class Lib(tone_lib):
        @staticmethod
        def gain(p, headroom, bits):
            key = (bytes(p), headroom, bits)
            if key not in gains:
                got = []
                for c in range(gain_ref.channels(model_params(p))):
                    out = (C.c_float * (1 << bits))()
                    assert L.hm_gain_table(C.byref(p), headroom, c, bits, out) == 1 << bits, L.hm_last_error().decode()
                    got.append(np.frombuffer(out, np.float32).copy())
                gains[key] = got
            return gains[key]
    return Lib


def light_of(capi, from_transfer=13, from_primaries=1, to_transfer=8, to_primaries=0, gain=1.0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def tone_of(capi, dst_peak=203.0, src_peak=1000.0, unit_nits=10000.0, out_unit_nits=0.0, out_bits=0):
    return capi.DeviceTone(1, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(0, 0))


def gain_of(capi, p, headroom, map_item=0):
    return capi.DeviceGain(map_item, headroom, p, (C.c_int32 * 4)(0, 0, 0, 0))


def same(got, exp, start, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - start} from the destination's start (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def pitched_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, aligned):
    """a guarded destination with an explicit row and plane pitch: rounded up to 16 bytes (the 16-byte stores run, with their ragged
    last groups), or one element more than that, which no 16-byte store can follow"""
    c = 3 if base.OBPP[fmt] in (3, 6) else 4
    tight = w * base.ELEM[dtype] * (c if layout == HWC else 1)
    row = (tight + 15) // 16 * 16 + (0 if aligned else base.ELEM[dtype])
    plane = row * h
    d = capi.DeviceDest()
    d.layout, d.dtype, d.row_pitch, d.plane_pitch = layout, dtype, row, plane if layout == CHW else 0
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    need = L.hm_device_dest_bytes(fmt, w, h, C.byref(d))
    assert need > 0, L.hm_last_error().decode()
    g = base.Guarded(need)
    d.ptr, d.len = g.ptr, need
    return d, g, row, plane


class Arrays:
    """a base image and its gain map on the device, with the census asserted"""

    def __init__(self, seed, w, h, mw, mh, bits, mbits, channels):
        import torch
        rng = np.random.default_rng(seed)
        peak, mpeak = (1 << bits) - 1, (1 << mbits) - 1
        wide, mwide = bits > 8, mbits > 8
        px = rng.integers(0, peak + 1, (h, w, channels), dtype=np.uint16 if wide else np.uint8)
        gm = rng.integers(0, mpeak + 1, (mh, mw), dtype=np.uint16 if mwide else np.uint8)
        px[0, 0, :3], px[h - 1, w - 1, :3], px[h // 2, w // 2, 1] = 0, peak, peak
        gm[0, 0], gm[mh - 1, mw - 1], gm[mh // 2, mw // 2] = 0, mpeak, mpeak
        gm[0, mw - 1], gm[mh - 1, 0] = mpeak, 0
        if wide:  # codes above the peak are read as the peak
            px[1, 1, 0], px[h - 2, 2, 2] = 65535, peak + 1
        if mwide:
            gm[1, 1], gm[mh - 2, 0] = 65535, mpeak + 1
        assert (px[..., :3] == 0).any() and (px[..., :3] == peak).any() and (gm == 0).any() and (gm == mpeak).any()
        assert (not wide or (px[..., :3] > peak).any()) and (not mwide or (gm > mpeak).any())
        self.pixels, self.gmap, self.bits, self.mbits, self.w, self.h, self.mw, self.mh = px, gm, bits, mbits, w, h, mw, mh
        obpp = channels * (2 if wide else 1)
        self.fmt = {3: RGB, 4: RGBA, 6: RRGGBB_LE, 8: RRGGBBAA_LE}[obpp]
        self.src_stride = (w * obpp + 63) // 64 * 64 + 64  # (16-byte aligned rows: the vector instance can run)
        src = np.zeros((h, self.src_stride), np.uint8)
        src[:, :w * obpp] = px.reshape(h, -1).view(np.uint8)
        self.map_stride = mw * (2 if mwide else 1) + 6
        mp = np.full((mh, self.map_stride), 0x5A, np.uint8)
        mp[:, :mw * (2 if mwide else 1)] = gm.view(np.uint8)
        self.dsrc, self.dmap = torch.from_numpy(src).cuda(), torch.from_numpy(mp).cuda()

    def call(self, L, view, lt, tn, gn, d):
        import torch
        rc = L.hm_gain_to_tensor(self.fmt, self.bits, self.w, self.h, self.dsrc.data_ptr(), self.src_stride, self.dmap.data_ptr(), self.map_stride, self.mw, self.mh,
                                 self.mbits, C.byref(view) if view is not None else None, C.byref(lt), C.byref(tn) if tn is not None else None, C.byref(gn), C.byref(d), None)
        msg = L.hm_last_error().decode()
        torch.cuda.synchronize()
        return rc, msg


def views_of(w, h, sx, sy):
    """name -> (crop, size, filter): none, the crop alone, nearest, and the three resampling filters reducing and enlarging; every crop
    origin on the map's raster"""
    small = (sx, 2 * sy, min(20, w - sx), min(15, h - 2 * sy))
    return {"none": None, "crop_alone": ((2 * sx, sy, w - 2 * sx - 3, h - sy - 2), None, TRIANGLE),
            "nearest_down": (None, (w * 2 // 3, h // 2 + 1), NEAREST), "nearest_up": (small, (33, 29), NEAREST),
            "triangle_down": (None, (w // 2 + 1, h // 3 + 1), TRIANGLE), "triangle_up": (small, (41, 37), TRIANGLE),
            "cubic_down": ((0, sy, w, h - sy), (w * 3 // 5, h * 2 // 3), CUBIC), "cubic_up": (small, (33, 30), CUBIC),
            "lanczos_down": (None, (w // 2, h // 2), LANCZOS3), "lanczos_up": (small, (37, 21), LANCZOS3)}


# (view, params, headroom, layout, dtype, aligned, to_transfer, to_primaries, tone, out_bits, scale, bias); dtype "int": the target's own
# integer type.  Every view with both layouts somewhere; F32, F16, the integer types and the 8-bit finish; aligned pitches and pitches
# one element off; wgt 0 (headroom at Hb), fractional and 1 (headroom +inf); the gamut matrix, the tone step
MODES = [
    ("none", "plain", 1.0, CHW, F32, True, 8, 0, False, 0, ONE, ZERO),
    ("none", "dark_gamma", inf, HWC, F16, True, 8, 9, False, 0, SCALE, BIAS),
    ("none", "three", 1.25, HWC, "int", False, 16, 9, False, 0, ONE, ZERO),
    ("none", "three", inf, CHW, "int", True, 16, 0, True, 8, ONE, ZERO),
    ("none", "no_offsets", 1.5, CHW, F16, False, 16, 0, True, 0, SCALE, BIAS),
    ("crop_alone", "dark_gamma", 2.0, CHW, F32, False, 8, 9, True, 0, SCALE, BIAS),
    ("crop_alone", "plain", inf, HWC, "int", True, 13, 0, False, 0, ONE, ZERO),
    ("nearest_down", "three", 2.0, HWC, F32, True, 8, 0, False, 0, SCALE, BIAS),
    ("nearest_up", "dark_gamma", 1.0, CHW, "int", False, 16, 9, True, 8, ONE, ZERO),
    ("triangle_down", "plain", 0.5, CHW, F32, True, 8, 0, False, 0, ONE, ZERO),
    ("triangle_down", "three", inf, HWC, F16, False, 16, 9, True, 0, SCALE, BIAS),
    ("triangle_up", "dark_gamma", 1.75, HWC, "int", True, 16, 0, False, 0, ONE, ZERO),
    ("cubic_down", "no_offsets", 1.25, CHW, F16, True, 8, 9, False, 0, SCALE, BIAS),
    ("cubic_up", "three", 2.25, HWC, F32, False, 13, 0, False, 0, ONE, ZERO),
    ("lanczos_down", "dark_gamma", inf, CHW, "int", True, 16, 9, True, 8, ONE, ZERO),
    ("lanczos_up", "plain", 1.0, CHW, F32, False, 8, 0, True, 0, SCALE, BIAS),
    ("triangle_down", "plain", 0.0, HWC, F32, True, 8, 0, False, 0, ONE, ZERO),
]

# base w, h, map w, h (sx, sy): 3 x 3 on odd sizes, 2 x 2, 1 x 1, 2 x 1 - then base bits, map bits, channels of the base
SHAPES = [(37, 23, 13, 8, 8, 8, 3), (37, 23, 13, 8, 10, 10, 4), (64, 48, 32, 24, 8, 10, 4), (64, 48, 32, 24, 10, 8, 3), (64, 48, 64, 48, 10, 10, 3),
          (64, 48, 64, 48, 8, 8, 4), (64, 48, 32, 48, 8, 8, 3), (64, 48, 32, 48, 10, 8, 4)]


@pytest.mark.parametrize("w,h,mw,mh,bits,mbits,channels", SHAPES)
def test_the_step_alone_equals_the_model(capi, L, lib, w, h, mw, mh, bits, mbits, channels):
    A = Arrays(52000 + w * 7 + mw + bits * 3 + mbits + channels, w, h, mw, mh, bits, mbits, channels)
    sx, sy = gain_ref.factor(w, mw), gain_ref.factor(h, mh)
    views = views_of(w, h, sx, sy)
    ran = 0
    for name, pname, headroom, layout, dtype, aligned, to_transfer, to_primaries, tone, out_bits, sc, bi in MODES:
        if out_bits == 8 and (channels == 4 or bits == 8):
            out_bits = 0  # (the 8-bit finish is for deeper three-channel targets: here the mode runs at the target's depth)
        if dtype == "int":
            dtype = U8 if bits == 8 or out_bits == 8 else U16
        view = views[name]
        p = params_of(capi, **PARAMS[pname])
        mp = model_params(p)
        lin = lib.table(13, bits, SDR_GAIN, False)
        enc = None if to_transfer == 8 else lib.table(to_transfer, 8 if out_bits == 8 else bits, SDR_GAIN, True)
        m = lib.matrix(1, to_primaries) if to_primaries else None
        tn_tables = lib.tone(SDR_GAIN, 1000.0, 203.0, 10000.0, 203.0) if tone else None
        kb, ka = gain_ref.offsets(mp, SDR_GAIN)
        wgt = gain_ref.weight(headroom, p.base_headroom, p.alternate_headroom)
        if wgt == 0.0:  # the write without the step
            vals = tone_ref.finish(*light_ref.light_sums(A.pixels, bits, lin, view, lib.taps), enc, m, tn_tables, NP[dtype], sc, bi)
        else:
            vals = gain_ref.render(A.pixels, bits, lin, A.gmap, mbits, lib.gain(p, headroom, mbits), kb, ka, view, lib.taps, enc, m, tn_tables, NP[dtype], sc, bi)
        oh, ow, oc = vals.shape
        assert oc == channels
        dfmt = RGB if out_bits == 8 else A.fmt
        d, g, row, plane = pitched_dest(capi, L, dfmt, layout, dtype, ow, oh, sc, bi, aligned)
        lt = light_of(capi, to_transfer=to_transfer, to_primaries=to_primaries, gain=SDR_GAIN)
        tn = tone_of(capi, out_bits=out_bits) if tone or out_bits else None
        rc, msg = A.call(L, dv.make_view(capi, *view) if view is not None else None, lt, tn, gain_of(capi, p, headroom), d)
        what = f"{name} {pname} headroom {headroom} layout {layout} dtype {dtype} aligned {aligned} to {to_transfer}/{to_primaries} tone {tone} out_bits {out_bits}"
        assert rc == 0, f"{what}: {msg}"
        same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
        ran += 1
    assert ran == len(MODES)


def test_weight_zero_writes_the_light_steps_bytes_and_alpha_is_untouched(capi, L, lib):
    """wgt == 0: byte for byte hm_light_to_tensor; and with any weight the alpha element of an RGBA target is the one of the call
    without the step"""
    A = Arrays(52900, 64, 48, 32, 24, 8, 8, 4)
    p = params_of(capi, **PARAMS["dark_gamma"])
    for view, layout, dtype, to_transfer in ((None, CHW, F32, 8), (((2, 2, 40, 30), None, TRIANGLE), HWC, U8, 13), ((None, (31, 22), TRIANGLE), CHW, F16, 8),
                                             ((None, (50, 60), NEAREST), HWC, U8, 16)):
        import torch
        ow, oh = (view[1] or view[0][2:]) if view else (64, 48)
        v = dv.make_view(capi, *view) if view else None
        lt = light_of(capi, to_transfer=to_transfer, gain=SDR_GAIN)
        outs = {}
        for headroom in (None, 0.0, 2.0):
            d, g, row, plane = pitched_dest(capi, L, RGBA, layout, dtype, ow, oh, SCALE, BIAS, True)
            if headroom is None:
                rc = L.hm_light_to_tensor(RGBA, 8, 64, 48, A.dsrc.data_ptr(), A.src_stride, C.byref(v) if v is not None else None, C.byref(lt), C.byref(d), None)
                msg = L.hm_last_error().decode()
                torch.cuda.synchronize()
            else:
                rc, msg = A.call(L, v, lt, None, gain_of(capi, p, headroom), d)
            assert rc == 0, msg
            outs[headroom] = g.host()
        assert np.array_equal(outs[0.0], outs[None]) and not np.array_equal(outs[2.0], outs[None]), (view, layout, dtype)
        e = base.ELEM[dtype]
        inner = [outs[k][g.start:g.start + (plane * 4 if layout == CHW else row * oh)] for k in (None, 2.0)]
        if layout == CHW:
            alpha = [b[3 * plane:4 * plane] for b in inner]
        else:
            alpha = [b.reshape(oh, row)[:, :ow * 4 * e].reshape(oh, ow, 4, e)[:, :, 3] for b in inner]
        assert np.array_equal(alpha[0], alpha[1]) and not (alpha[0] == 0xA5).all()


def map_item_pixels(hm, data, item):
    """the Y plane of item `item` as hm_decode_item hands it out (its own transformations applied): h x w codes, and its depth"""
    f = pipeline.HeifFile(hm, data)
    try:
        planes, meta = f.decode(item, 0, threads=THREADS)
    finally:
        f.close()
    w, h, bd = meta["width"], meta["height"], meta["bit_depth"]
    assert meta["chroma"] == 0
    y = planes[0][:h, :w * (2 if bd > 8 else 1)]
    return (np.ascontiguousarray(y).view("<u2") if bd > 8 else np.ascontiguousarray(y)).reshape(h, w), bd


GOOD = dict(hb=0.0, ha=2.0, lo=-0.5, hi=2.0, gamma=2.2, kb=1.0 / 64, ka=1.0 / 64)
GOOD_PAYLOAD = gainwriter.tmap_payload([gainwriter.channel(min=(-1, 2), max=(2, 1), gamma=(22, 10), base_offset=(1, 64), alternate_offset=(1, 64))], use_base=True)


@pytest.fixture(scope="module")
def files(hm):
    """name -> (file bytes, the item the decode is asked for, base id, map id, map_item of the request (0: a 'tmap' item), base pixels, map codes)"""
    out = {}

    def add(name, w, item, b, m, map_item):
        data = w.finish(primary=b)
        rows, bw, bh = base.host_rows(hm, data, RGB, THREADS, item=b)
        gm, bd = map_item_pixels(hm, data, m)
        assert bd == 8
        out[name] = (data, item, b, m, map_item, rows.reshape(bh, bw, 3), gm)

    w = gainwriter.Writer()
    b = w.hvc1(synthutil.picture(53001, width=64, height=64), (64, 64))
    m = w.hvc1(synthutil.picture(53002, width=32, height=32, chroma_format=0), (32, 32), chroma_format=0, hidden=True)
    add("tmap", w, w.tmap(b, m, GOOD_PAYLOAD, (64, 64), colr=(9, 16, 0, 1), clli=(600, 200)), b, m, 0)
    w = gainwriter.Writer()
    tiles = [w.hvc1(synthutil.picture(53010 + k, width=64, height=64), (64, 64)) for k in range(4)]
    b = w.grid(tiles, 2, 2, 128, 128)
    m = w.hvc1(synthutil.picture(53015, width=64, height=64, chroma_format=0), (64, 64), chroma_format=0, hidden=True)
    add("grid_base", w, w.tmap(b, m, GOOD_PAYLOAD, (128, 128)), b, m, 0)
    w = gainwriter.Writer()
    b = w.hvc1(synthutil.picture(53020, width=64, height=48), (64, 48))
    m = w.hvc1(synthutil.picture(53021, width=24, height=32, chroma_format=0), (24, 32), chroma_format=0, hidden=True, transforms=[("irot", 1)])
    add("irot_map", w, w.tmap(b, m, GOOD_PAYLOAD, (64, 48)), b, m, 0)
    w = gainwriter.Writer()
    b = w.hvc1(synthutil.picture(53030, width=64, height=64), (64, 64))
    m = w.aux(synthutil.picture(53031, width=32, height=64, chroma_format=0), (32, 64), b, VENDOR_URN)
    add("auxl", w, b, b, m, m)
    assert out["irot_map"][6].shape == (24, 32) and out["grid_base"][5].shape == (128, 128, 3) and out["auxl"][6].shape == (64, 32)
    return out


def gain_to_device(capi, L, data, item, view, lt, tn, gn, d, fmt=RGB):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, THREADS, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_gain(h, item, C.byref(prm), C.byref(view) if view is not None else None, C.byref(lt), C.byref(tn) if tn is not None else None,
                                             C.byref(gn), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def expected(capi, lib, pixels, gmap, headroom, view, to_transfer, to_primaries, tone, dtype, sc, bi):
    p = params_of(capi, **GOOD)
    lin = lib.table(13, 8, SDR_GAIN, False)
    enc = None if to_transfer == 8 else lib.table(to_transfer, 8, SDR_GAIN, True)
    m = lib.matrix(1, to_primaries) if to_primaries else None
    kb, ka = gain_ref.offsets(model_params(p), SDR_GAIN)
    return gain_ref.render(pixels, 8, lin, gmap, 8, lib.gain(p, headroom, 8), kb, ka, view, lib.taps, enc, m, tone, NP[dtype], sc, bi)


# (file, view, headroom, to_transfer, to_primaries, tone, layout, dtype, scale, bias, pad)
DECODES = {
    "tmap": ("tmap", None, inf, 8, 9, False, CHW, F32, SCALE, BIAS, 0),
    "tmap_view_u8": ("tmap", ((2, 4, 50, 40), (31, 27), CUBIC), 1.0, 16, 9, True, HWC, U8, ONE, ZERO, 1),
    "tmap_nearest": ("tmap", (None, (40, 70), NEAREST), 1.5, 8, 0, False, HWC, F16, SCALE, BIAS, 2),
    "grid_base": ("grid_base", None, 1.0, 8, 0, False, HWC, F32, ONE, ZERO, 0),
    "grid_base_crop": ("grid_base", ((62, 60, 40, 30), (55, 41), TRIANGLE), inf, 13, 0, False, CHW, U8, ONE, ZERO, 0),
    "irot_map": ("irot_map", None, 1.25, 8, 0, False, CHW, F32, ONE, ZERO, 1),
    "irot_map_triangle": ("irot_map", (None, (30, 20), TRIANGLE), inf, 8, 9, False, CHW, F16, SCALE, BIAS, 0),
    "auxl": ("auxl", None, 2.0, 16, 9, True, CHW, U8, ONE, ZERO, 0),
    "auxl_crop_alone": ("auxl", ((4, 7, 33, 21), None, TRIANGLE), 0.75, 8, 0, False, HWC, F32, SCALE, BIAS, 2),
}


@pytest.mark.parametrize("name", list(DECODES))
def test_decodes_equal_the_model_on_the_host_decodes(capi, L, lib, files, name):
    """a 'tmap' file; a 2 x 2 grid base with a single-picture map; a map carrying an irot; an explicit map_item on an 'auxl' image.
    hm_decoded reports the base image's fields; the tone step's src_peak == 0 reads the 'tmap' item's clli (600)"""
    fname, view, headroom, to_transfer, to_primaries, tone, layout, dtype, sc, bi, pad = DECODES[name]
    data, item, b, m, map_item, pixels, gmap = files[fname]
    src_peak = 600.0 if fname == "tmap" else 1000.0
    tn_tables = lib.tone(SDR_GAIN, src_peak, 203.0, 10000.0, 203.0) if tone else None
    vals = expected(capi, lib, pixels, gmap, headroom, view, to_transfer, to_primaries, tn_tables, dtype, sc, bi)
    oh, ow, _ = vals.shape
    d, g, row, plane = base.make_dest(capi, L, RGB, layout, dtype, ow, oh, sc, bi, pad, 0)
    lt = light_of(capi, from_transfer=0, from_primaries=0, to_transfer=to_transfer, to_primaries=to_primaries, gain=SDR_GAIN)
    tn = tone_of(capi, src_peak=0.0, unit_nits=10000.0) if tone else None
    gn = gain_of(capi, params_of(capi, **GOOD) if map_item else capi.GainParams(), headroom, map_item)
    rc, msg, out = gain_to_device(capi, L, data, item, dv.make_view(capi, *view) if view else None, lt, tn, gn, d)
    assert rc == 0, f"{name}: {msg}"
    assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format, out.bit_depth, out.transfer, out.primaries) == (ow, oh, 1, row, RGB, 8, 13, 1), name
    same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, name)


def test_weight_zero_decodes_to_the_light_steps_bytes(capi, L, files):
    import test_device_light_gpu as dl
    data, item, b, m, _, pixels, gmap = files["tmap"]
    lt = light_of(capi, from_transfer=0, from_primaries=0, to_transfer=16, to_primaries=9, gain=SDR_GAIN)
    view = dv.make_view(capi, (0, 0, 64, 32), (40, 30), TRIANGLE)  # (crop_y etc. on the map's raster)
    d1, g1, _, _ = base.make_dest(capi, L, RGB, CHW, U8, 40, 30, ONE, ZERO, 0, 0)
    d2, g2, _, _ = base.make_dest(capi, L, RGB, CHW, U8, 40, 30, ONE, ZERO, 0, 0)
    rc, msg, _ = gain_to_device(capi, L, data, item, view, lt, None, gain_of(capi, capi.GainParams(), 0.0), d1)
    assert rc == 0, msg
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm, out = capi.DecodeParams(RGB, THREADS, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
        assert L.hm_decode_item_to_device_light(h, b, C.byref(prm), C.byref(view), C.byref(lt), C.byref(d2), C.byref(out)) == 0, L.hm_last_error().decode()
    finally:
        L.hm_file_close(h)
    assert dl is not None and np.array_equal(g1.host(), g2.host()) and not (g1.host()[g1.start:g1.start + 64] == 0xA5).all()


def test_the_pipeline_and_the_python_calls(pkg, capi, L, lib, files):
    """two files in flight through hm_pipeline_submit_to_device_gain (a 'tmap' item, and an explicit map_item), then gain= of
    decode_to_tensor (by 'tmap' id, by base id, by map_item) and decode_batch_to_tensor"""
    import torch
    size = (48, 36)
    view = (None, size, TRIANGLE)
    v = dv.make_view(capi, *view)
    lt = light_of(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=9, gain=SDR_GAIN)
    want = {k: expected(capi, lib, files[k][5], files[k][6], 1.5, view, 8, 9, None, F32, ONE, ZERO) for k in ("tmap", "auxl")}
    assert not np.array_equal(want["tmap"], want["auxl"])
    cfg = capi.PipelineConfig(2, 2, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        dests = []
        for k, name in enumerate(("tmap", "auxl")):
            data, item, b, m, map_item, _, _ = files[name]
            d, g, row, plane = base.make_dest(capi, L, RGB, CHW, F32, size[0], size[1], ONE, ZERO, 0, 0)
            gn = gain_of(capi, params_of(capi, **GOOD) if map_item else capi.GainParams(), 1.5, map_item)
            assert L.hm_pipeline_submit_to_device_gain(pipe, data, len(data), item, k, C.byref(v), C.byref(lt), None, C.byref(gn), C.byref(d)) == 0, L.hm_last_error().decode()
            dests.append((name, g, row, plane))
        assert L.hm_pipeline_pending(pipe) == 2
        for k, (name, g, row, plane) in enumerate(dests):
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0 and r.status == 0 and r.tag == k, L.hm_last_error().decode()
            assert (r.image.out_format, r.image.width, r.image.height) == (RGB, size[0], size[1])
            L.hm_pipeline_release(pipe, C.byref(r))
            same(g.host(), dv.place(want[name], CHW, F32, row, plane, g.size, g.start), g.start, f"pipeline {name}")
    finally:
        L.hm_pipeline_destroy(pipe)
    spec = dict(to_transfer="linear", to_primaries="bt2020", gain=SDR_GAIN)
    data, tmap, b, m, _, _, _ = files["tmap"]
    kw = dict(layout="hwc", dtype=torch.float32, size=size, light=spec)
    for item_id in (tmap, b, 0):  # (0: the primary item, which is the base)
        t = pkg.decode_to_tensor(data, item_id=item_id, gain=dict(headroom=1.5), **kw)
        assert tuple(t.shape) == (size[1], size[0], 3) and t.cpu().numpy().tobytes() == want["tmap"].tobytes(), item_id
    aux = files["auxl"]
    explicit = dict(headroom=1.5, map_item=aux[3], base_headroom=GOOD["hb"], alternate_headroom=GOOD["ha"], map_min=GOOD["lo"], map_max=GOOD["hi"], gamma=GOOD["gamma"],
                    base_offset=GOOD["kb"], alternate_offset=GOOD["ka"])
    t = pkg.decode_to_tensor(aux[0], gain=explicit, **kw)
    assert t.cpu().numpy().tobytes() == want["auxl"].tobytes()
    t2 = pkg.decode_batch_to_tensor([data, data], gain=dict(headroom=1.5), **kw)
    assert tuple(t2.shape) == (2, size[1], size[0], 3) and all(t2[k].cpu().numpy().tobytes() == want["tmap"].tobytes() for k in range(2))
    full = pkg.decode_to_tensor(data, light=spec, gain=dict(headroom=math.inf), layout="chw")
    assert tuple(full.shape) == (3, 64, 64)
    assert full.cpu().numpy().transpose(1, 2, 0).tobytes() == expected(capi, lib, files["tmap"][5], files["tmap"][6], inf, None, 8, 9, None, F32, ONE, ZERO).tobytes()


def test_refusals_leave_every_byte_unwritten(capi, L, files):
    import torch
    data, item, b, m, _, _, _ = files["tmap"]
    lt = light_of(capi, from_transfer=0, from_primaries=0, gain=SDR_GAIN)

    def refused(view, gn, status, word, w=64, h=64, light=lt, shrink=0):
        d, g, _, _ = base.make_dest(capi, L, RGB, CHW, F32, w, h, ONE, ZERO, 0, 0, shrink=shrink)
        rc, msg, _ = gain_to_device(capi, L, data, item, view, light, None, gn, d)
        assert rc == status and word in msg, (rc, msg, word)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"
    from_file = capi.GainParams()
    refused(None, gain_of(capi, from_file, float("nan")), -1, "headroom")
    refused(None, gain_of(capi, from_file, -1.0), -1, "headroom")
    refused(dv.make_view(capi, (1, 0, 32, 32), None, TRIANGLE), gain_of(capi, from_file, 1.0), -1, "crop_x 1", 32, 32)
    refused(dv.make_view(capi, (0, 5, 32, 32), (16, 16), NEAREST), gain_of(capi, from_file, 1.0), -1, "crop_y 5", 16, 16)
    refused(None, gain_of(capi, from_file, 1.0), -1, "len", shrink=1)
    refused(None, gain_of(capi, from_file, 1.0), -1, "gain", light=light_of(capi, from_transfer=0, from_primaries=0, gain=0.0))
    refused(None, gain_of(capi, from_file, 1.0, map_item=m), -1, "brings its own")
    # ... and the library still renders after all of that
    d, g, _, _ = base.make_dest(capi, L, RGB, CHW, F32, 64, 64, ONE, ZERO, 0, 0)
    rc, msg, _ = gain_to_device(capi, L, data, item, None, lt, None, gain_of(capi, from_file, 1.0), d)
    assert rc == 0 and not (g.host()[g.start:g.start + 64] == 0xA5).all(), msg


def test_gain_kernels_use_no_scratch(pkg):
    """every instance of the gain kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 12): no scratch"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(12, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 128, (n, out[0], out[1])
        n += 1
    # 26 pointwise (sample width x dtype x channels x store width, the layout being a kernel argument, plus the two of the 8-bit finish),
    # 13 nearest, 3 of the map's two passes, 16 vertical
    assert n == 58
