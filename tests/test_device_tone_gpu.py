"""GPU: the tone step (hm_decode_item_to_device_tone, hm_decode_frames_to_device_tone, hm_pipeline_submit_to_device_tone,
hm_tone_to_tensor and tone= of the Python calls).  Everything is bit-exact: the expected image of every case is the model of
tests/tone_ref.py on top of tests/light_ref.py, fed with the library's tables (hm_light_table, hm_tone_table - held to the model
within 1 ulp by test_device_tone.py), hm_light_matrix's matrix and hm_view_filter_taps' weights.  Every destination sits in a guarded
buffer pre-filled with 0xA5 and the WHOLE buffer is compared, as in test_device_light_gpu.py.  A census of the norm's three arms -
below the knee, between knee and src_peak, above src_peak - is asserted in the step-alone test on random samples and in every case of
the picture test (each arm holds at least 5 % of the pixels): no arm goes untested.  The peak-rule, no-op-curve and routes tests
compare pixels of the same picture without a census of their own."""
import ctypes as C

import numpy as np
import pytest

import hdrwriter
import light_ref
import moovwriter
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv
import test_facade_gpu as fg
import tone_ref
from test_device_light_gpu import lib as light_lib  # noqa: F401  (a fixture: hm_light_table, hm_light_matrix, hm_view_filter_taps, each result once)
from test_facade_gpu import api  # noqa: F401  (the facade's bound library: a fixture)

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
ONE, ZERO = [1.0] * 4, [0.0] * 4
SCALE, BIAS = [2.0, 0.75, 16.0, 1.0], [-1.0, 0.125, 0.5, 0.0]
THREADS = 2
W, H = 160, 96
# the picture: coarse enough (qp 40) that its PQ codes spread over the whole range - with clli 1000 and a 203 cd/m2 display about
# 18 % / 52 % / 30 % of its pixels fall below the knee, between knee and peak, and above the peak (CPU oracle decode)
PICTURE = dict(width=W, height=H, bit_depth=10, full_range=0, matrix=1, primaries=1, qp=40)
SEED = 48302
DST = 203.0


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def lib(light_lib, L, capi):
    """what the model is fed with, each computed once: the light tests' tables, matrices and taps, and tone(gain, src_peak, dst_peak,
    unit_nits, out_unit_nits) -> (thr, sg) of hm_tone_table"""
    tones = {}

    class Lib(light_lib):
        @staticmethod
        def tone(gain, src, dst, unit, out_unit):
            key = (gain, src, dst, unit, out_unit)
            if key not in tones:
                t = capi.DeviceTone(1, 0, src, dst, unit, out_unit, (C.c_int32 * 2)(0, 0))
                got = []
                for which in (0, 1):
                    out = (C.c_float * 2048)()
                    assert L.hm_tone_table(C.byref(t), gain, which, out) == 2048, L.hm_last_error().decode()
                    got.append(np.frombuffer(out, np.float32).copy())
                tones[key] = tuple(got)
            return tones[key]
    return Lib


@pytest.fixture(scope="module")
def images(hm):
    """name -> file bytes, and the host decode's pixels (h x w x 3 samples of 10 bits): one picture, three sets of light levels"""
    pic = synthutil.picture(SEED, **PICTURE)
    files = {"clli": hdrwriter.write_hdr_heic([pic], (W, H), clli=(1000, 300)), "mdcv": hdrwriter.write_hdr_heic([pic], (W, H), mdcv=(6000000, 50)),
             "neither": hdrwriter.write_hdr_heic([pic], (W, H))}
    rows, w, h = base.host_rows(hm, files["clli"], RRGGBB_LE, THREADS)
    pixels = rows.view("<u2").reshape(h, w, 3)
    assert (w, h) == (W, H) and pixels.max() <= 1023
    for name in ("mdcv", "neither"):  # (the properties change no pixel)
        assert np.array_equal(base.host_rows(hm, files[name], RRGGBB_LE, THREADS)[0], rows)
    return files, pixels


def light_of(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=0, gain=1.0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def tone_of(capi, dst_peak=DST, src_peak=0.0, unit_nits=0.0, out_unit_nits=0.0, out_bits=0):
    return capi.DeviceTone(1, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits, (C.c_int32 * 2)(0, 0))


def tone_to_device(capi, L, data, fmt, view, lt, tn, d, threads=THREADS):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device_tone(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(view) if view is not None else None, C.byref(lt), C.byref(tn),
                                             C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def same(got, exp, start, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - start} from the destination's start (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def sibling(fmt, out_bits):
    """the target the destination is judged, sized and written as"""
    return RGB if out_bits == 8 and fmt == RRGGBB_LE else fmt


def census(thr, r, m, src, dst, what):
    arms = tone_ref.arms(thr, r, m, src, dst, 1.0, 10000.0)
    print(f"{what}: below the knee {arms[0]:.3f}, knee to src_peak {arms[1]:.3f}, above src_peak {arms[2]:.3f}")
    assert min(arms) >= 0.05, (what, arms)


def check_item(capi, L, data, fmt, view, lt, tn, vals, layout, dtype, scale, bias, pad, what):
    """decode under (view, lt, tn) into a guarded destination and compare the whole buffer with `vals`"""
    oh, ow, _ = vals.shape
    d, g, row, plane = base.make_dest(capi, L, sibling(fmt, tn.out_bits), layout, dtype, ow, oh, scale, bias, pad, 0)
    v = dv.make_view(capi, *view) if view is not None else None
    rc, msg, out = tone_to_device(capi, L, data, fmt, v, lt, tn, d)
    assert rc == 0, f"{what}: {msg}"
    assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, fmt), what
    same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
    return out


def pitched_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, aligned):
    """make_dest with an explicit row and plane pitch.  aligned: rounded up to 16 bytes - no tight row of the sizes below is a multiple of
    16 bytes, so only an explicit pitch lets the 16-byte stores run, with their ragged last groups; else one element more than that,
    which no 16-byte store can follow (make_dest's padded pitches are aligned for some of these sizes and dtypes, by accident)"""
    tight = w * base.ELEM[dtype] * (3 if layout == HWC else 1)
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


def takes_vector_instance(src_ptr, src_stride, d, layout, row, plane):
    """k_light_tensor's launcher picks the 16-byte instance exactly when both sides allow it: this is its rule, restated"""
    return src_ptr % 16 == 0 and src_stride % 16 == 0 and d.ptr % 16 == 0 and row % 16 == 0 and (layout != CHW or plane % 16 == 0)


@pytest.mark.parametrize("bits,w,h", [(10, 1043, 5), (12, 131, 37), (12, 1043, 5), (10, 131, 37)])
def test_the_step_alone_on_random_samples(capi, L, lib, bits, w, h):
    """hm_tone_to_tensor on uniform random codes, peaks 1000 -> 203.  With pitches rounded up to 16 bytes the vector instances run:
    1043 x 5 is then more than one wave of 64 x 16 pixels and leaves a ragged last group in the second column of workgroups, 131 x 37
    gives a ragged last group for every dtype (131 is no multiple of 4, 8 or 16) and rows that are no multiple of 4.  Beside each, a
    pitch one element wider, which forces the scalar instance; which of the two a launch takes is asserted.  Both layouts, the target's depth (u16 / f16 / f32) and the 8-bit finish
    (u8 / f32); linear, re-encoded, and behind the 2020 -> 709 matrix; 12 bits re-encoded with a tone step is the 48 KB of LDS."""
    import torch
    rng = np.random.default_rng(bits * 10000 + w)
    pixels = rng.integers(0, 1 << bits, (h, w, 3), dtype=np.uint16)
    pixels[rng.integers(0, h, 20), rng.integers(0, w, 20), rng.integers(0, 3, 20)] = rng.integers(1 << bits, 65536, 20, dtype=np.uint16)  # (read as the peak)
    src_stride = (w * 6 + 63) // 64 * 64 + 64
    src = np.zeros((h, src_stride), np.uint8)
    src[:, :w * 6] = pixels.reshape(h, -1).view(np.uint8)
    dsrc = torch.from_numpy(src).cuda()
    gain, srcp, dst = 1.0, 1000.0, 203.0
    lin, m = lib.table(16, bits, gain, False), lib.matrix(9, 1)
    tn_tables = lib.tone(gain, srcp, dst, 10000.0, dst)
    r, alpha, resampled = light_ref.light_sums(pixels, bits, lin, None, lib.taps)
    census(tn_tables[0], r, None, srcp, dst, f"random {bits}-bit codes")
    census(tn_tables[0], r, m, srcp, dst, f"random {bits}-bit codes behind the matrix")
    # (to_transfer, matrix, dtype, out_bits, scale, bias)
    modes = ((13, None, U16, 0, ONE, ZERO), (8, None, F16, 0, SCALE, BIAS), (13, m, F32, 0, SCALE, BIAS), (8, m, F32, 0, ONE, ZERO),
             (13, m, U8, 8, ONE, ZERO), (13, None, F32, 8, SCALE, BIAS), (8, None, F32, 8, SCALE, BIAS))
    for to_transfer, mm, dtype, out_bits, sc, bi in modes:
        enc = None if to_transfer == 8 else lib.table(to_transfer, 8 if out_bits == 8 else bits, gain, True)
        vals = tone_ref.finish(r, alpha, resampled, enc, mm, tn_tables, NP[dtype], sc, bi)
        for layout in (HWC, CHW):
            for aligned in (True, False):
                dfmt = sibling(RRGGBB_LE, out_bits)
                d, g, row, plane = pitched_dest(capi, L, dfmt, layout, dtype, w, h, sc, bi, aligned)
                assert takes_vector_instance(dsrc.data_ptr(), src_stride, d, layout, row, plane) == aligned, (layout, dtype, aligned, row, plane)
                lt = light_of(capi, from_transfer=16, from_primaries=9, to_transfer=to_transfer, to_primaries=0 if mm is None else 1, gain=gain)
                tn = tone_of(capi, dst, srcp, 10000.0, dst, out_bits)
                rc = L.hm_tone_to_tensor(RRGGBB_LE, bits, w, h, dsrc.data_ptr(), src_stride, None, C.byref(lt), C.byref(tn), C.byref(d), None)
                assert rc == 0, L.hm_last_error().decode()
                torch.cuda.synchronize()
                same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start,
                     f"{bits} bits to {to_transfer} matrix {mm is not None} dtype {dtype} out_bits {out_bits} layout {layout} aligned {aligned}")


def test_the_step_alone_on_8_bit_srgb(capi, L, lib):
    """HM_OUT_RGB from sRGB, where 1.0 is the 203 cd/m2 of an SDR white, to a 100 cd/m2 display; out_bits = 8 changes nothing here"""
    import torch
    w, h = 131, 37
    pixels = np.random.default_rng(77).integers(0, 256, (h, w, 3), dtype=np.uint8)
    dsrc = torch.from_numpy(pixels.reshape(h, w * 3).copy()).cuda()
    lin, enc = lib.table(13, 8, 1.0, False), lib.table(13, 8, 1.0, True)
    tn_tables = lib.tone(1.0, 203.0, 100.0, 203.0, 100.0)
    r, alpha, resampled = light_ref.light_sums(pixels, 8, lin, None, lib.taps)
    vals = tone_ref.finish(r, alpha, resampled, enc, None, tn_tables, np.uint8, ONE, ZERO)
    assert not np.array_equal(vals, pixels)
    lt = light_of(capi, from_transfer=13, from_primaries=1, to_transfer=13)
    for out_bits in (0, 8):
        d, g, row, plane = base.make_dest(capi, L, RGB, HWC, U8, w, h, ONE, ZERO, 0, 0)
        tn = tone_of(capi, 100.0, 203.0, 203.0, 100.0, out_bits)
        assert L.hm_tone_to_tensor(RGB, 8, w, h, dsrc.data_ptr(), w * 3, None, C.byref(lt), C.byref(tn), C.byref(d), None) == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        same(g.host(), dv.place(vals, HWC, U8, row, plane, g.size, g.start), g.start, f"sRGB 203 -> 100, out_bits {out_bits}")


# (view, to_transfer, to_primaries, layout, dtype, out_bits, scale, bias, pad)
CASES = {
    "no_view": (None, 8, 0, CHW, F32, 0, SCALE, BIAS, 0),
    "triangle": ((None, (50, 37), TRIANGLE), 16, 0, HWC, U16, 0, ONE, ZERO, 0),
    "cubic": (((3, 5, 150, 80), (64, 40), CUBIC), 8, 1, CHW, F32, 0, ONE, ZERO, 1),
    "lanczos3": ((None, (77, 45), LANCZOS3), 13, 1, HWC, U8, 8, ONE, ZERO, 0),
    "nearest": ((None, (77, 201), NEAREST), 13, 0, CHW, U8, 8, ONE, ZERO, 2),
    "crop_alone": (((7, 5, 133, 81), None, TRIANGLE), 16, 0, CHW, U16, 0, ONE, ZERO, 0),
    "thumbnail": ((None, (40, 24), TRIANGLE), 13, 1, HWC, U8, 8, ONE, ZERO, 0),
    "srgb_u8_whole": (None, 13, 1, HWC, U8, 8, ONE, ZERO, 0),
    "linear_f16_chw": (None, 8, 0, CHW, F16, 0, SCALE, BIAS, 0),
}


def expected(lib, pixels, case, src_peak, dst_peak=DST, what=None):
    view, to_transfer, to_primaries, layout, dtype, out_bits, sc, bi, pad = case
    lin = lib.table(16, 10, 1.0, False)
    enc = None if to_transfer == 8 else lib.table(to_transfer, 8 if out_bits == 8 else 10, 1.0, True)
    m = lib.matrix(9, 1) if to_primaries == 1 else None
    tn_tables = lib.tone(1.0, src_peak, dst_peak, 10000.0, dst_peak)
    r, alpha, resampled = light_ref.light_sums(pixels, 10, lin, view, lib.taps)
    if what:
        census(tn_tables[0], r, m, src_peak, dst_peak, what)
    return tone_ref.finish(r, alpha, resampled, enc, m, tn_tables, NP[dtype], sc, bi)


@pytest.mark.parametrize("name", list(CASES))
def test_a_pq_picture_with_clli_equals_the_model(capi, L, lib, images, name):
    """a 160 x 96 10-bit PQ BT.2020 picture with clli 1000 and src_peak = 0: the expected pixels are the model on the host decode's"""
    files, pixels = images
    case = CASES[name]
    view, to_transfer, to_primaries, layout, dtype, out_bits, sc, bi, pad = case
    vals = expected(lib, pixels, case, 1000.0, what=name)
    out = check_item(capi, L, files["clli"], RRGGBB_LE, view, light_of(capi, to_transfer=to_transfer, to_primaries=to_primaries), tone_of(capi, out_bits=out_bits),
                     vals, layout, dtype, sc, bi, pad, name)
    assert (out.transfer, out.primaries, out.bit_depth) == (16, 9, 10)


def test_the_peak_rule_end_to_end(capi, L, lib, images):
    """mdcv only: its maximum of 600 cd/m2; neither property: 1000 - the same bytes as the clli 1000 file gives"""
    files, pixels = images
    case = CASES["no_view"]
    by_peak = {peak: expected(lib, pixels, case, peak) for peak in (600.0, 1000.0)}
    assert not np.array_equal(by_peak[600.0], by_peak[1000.0])
    for name, peak in (("mdcv", 600.0), ("neither", 1000.0), ("clli", 1000.0)):
        check_item(capi, L, files[name], RRGGBB_LE, None, light_of(capi), tone_of(capi), by_peak[peak], CHW, F32, SCALE, BIAS, 0, f"peak of {name}")
    # an explicit src_peak overrides the file's
    check_item(capi, L, files["clli"], RRGGBB_LE, None, light_of(capi), tone_of(capi, src_peak=600.0), by_peak[600.0], CHW, F32, SCALE, BIAS, 0, "explicit peak")


def test_a_curve_that_does_nothing_gives_the_light_steps_bytes(capi, L, images):
    """dst_peak >= src_peak, Uo == U and a norm that stays below src_peak: byte for byte hm_decode_item_to_device_light"""
    import test_device_light_gpu as dl
    files, pixels = images
    for view, to_transfer, layout, dtype in ((None, 8, CHW, F32), (None, 16, HWC, U16), ((None, (50, 37), TRIANGLE), 13, CHW, F16), ((None, (77, 45), NEAREST), 8, HWC, F32)):
        ow, oh = view[1] if view else (W, H)
        v = dv.make_view(capi, *view) if view else None
        lt = light_of(capi, to_transfer=to_transfer, to_primaries=1)
        d1, g1, _, _ = base.make_dest(capi, L, RRGGBB_LE, layout, dtype, ow, oh, SCALE, BIAS, 0, 0)
        d2, g2, _, _ = base.make_dest(capi, L, RRGGBB_LE, layout, dtype, ow, oh, SCALE, BIAS, 0, 0)
        rc, msg, _ = tone_to_device(capi, L, files["clli"], RRGGBB_LE, v, lt, tone_of(capi, 10000.0, 10000.0, 10000.0, 10000.0), d1)
        assert rc == 0, msg
        rc, msg, _ = dl.light_to_device(capi, L, files["clli"], RRGGBB_LE, v, lt, d2)
        assert rc == 0, msg
        assert np.array_equal(g1.host(), g2.host()) and not (g1.host()[g1.start:g1.start + 64] == 0xA5).all(), (view, to_transfer)


def test_every_route_gives_the_item_calls_bytes(hm, pkg, capi, L, lib, images):
    """one request - the thumbnail: 2020 -> 709, sRGB, 8-bit codes, HWC uint8 under a triangle view - through the item call, the frames
    form (a two-frame clip), the pipeline, the step alone and the three Python calls"""
    import torch
    files, pixels = images
    size = (40, 24)
    case = (None, size, TRIANGLE), 13, 1, HWC, U8, 8, ONE, ZERO, 0
    vals = expected(lib, pixels, case, 1000.0)
    want = vals.tobytes()
    view = dv.make_view(capi, None, size, TRIANGLE)
    lt = light_of(capi, from_transfer=16, from_primaries=9, to_transfer=13, to_primaries=1)
    tn = tone_of(capi, src_peak=1000.0, out_bits=8)

    def fresh():
        return base.make_dest(capi, L, RGB, HWC, U8, size[0], size[1], ONE, ZERO, 0, 0)

    def inner(g):
        got = g.host()
        assert (got[:g.start] == 0xA5).all() and (got[g.size - base.GUARD:] == 0xA5).all()
        return got[g.start:g.size - base.GUARD].tobytes()
    d, g, _, _ = fresh()
    rc, msg, out = tone_to_device(capi, L, files["clli"], RRGGBB_LE, view, lt, tn, d)
    assert rc == 0 and inner(g) == want, msg
    # the step alone, on the host decode's pixels
    dsrc = torch.from_numpy(pixels.reshape(H, W * 3).view(np.uint8).copy()).cuda()
    d, g, _, _ = fresh()
    alone = tone_of(capi, src_peak=1000.0, unit_nits=10000.0, out_bits=8)  # (nothing is resolved for the step alone: the unit is explicit)
    assert L.hm_tone_to_tensor(RRGGBB_LE, 10, W, H, dsrc.data_ptr(), W * 6, C.byref(view), C.byref(lt), C.byref(alone), C.byref(d), None) == 0, L.hm_last_error().decode()
    torch.cuda.synchronize()
    assert inner(g) == want
    # the pipeline: src_peak = 0 is the file's own there too
    cfg = capi.PipelineConfig(2, 2, RRGGBB_LE, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        dests = [fresh(), fresh()]
        for k, t in enumerate((tn, tone_of(capi, out_bits=8))):
            assert L.hm_pipeline_submit_to_device_tone(pipe, files["clli"], len(files["clli"]), 0, k, C.byref(view), C.byref(lt), C.byref(t), C.byref(dests[k][0])) == 0
        for k in range(2):
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0 and r.status == 0 and r.tag == k, L.hm_last_error().decode()
            assert (r.image.out_format, r.image.width, r.image.height, r.image.stride[0]) == (RRGGBB_LE, size[0], size[1], size[0] * 3)
            assert inner(dests[k][1]) == want, k
            L.hm_pipeline_release(pipe, C.byref(r))
    finally:
        L.hm_pipeline_destroy(pipe)
    # the frames form: a two-frame clip of the picture (a frame carries no light levels: src_peak = 0 is 1000)
    pic = synthutil.picture(SEED, **PICTURE)
    clip = moovwriter.write_movie([pic, pic], (W, H), bit_depth=10)
    per = size[0] * size[1] * 3
    for t in (tn, tone_of(capi, out_bits=8)):
        g = base.Guarded(per * 2)
        dests = (capi.DeviceDest * 2)()
        for k in range(2):
            dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = g.ptr + k * per, per, HWC, U8
            for c in range(4):
                dests[k].scale[c], dests[k].bias[c] = 1.0, 0.0
        fh = C.c_void_p()
        assert L.hm_file_open(clip, len(clip), C.byref(fh)) == 0
        try:
            prm = capi.DecodeParams(RRGGBB_LE, 2, 0, 0, None, None, 0, 0, 0, 0)
            res = (capi.Decoded * 2)()
            failed = C.c_int32(-2)
            rc = L.hm_decode_frames_to_device_tone(fh, (C.c_uint32 * 2)(2, 1), 2, C.byref(prm), C.byref(view), C.byref(lt), C.byref(t), dests, res, C.byref(failed))
            assert rc == 0 and failed.value == -1, L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
        assert inner(g) == want + want
    # the Python calls
    spec = dict(from_transfer="pq", from_primaries="bt2020", to_transfer="srgb", to_primaries="bt709")
    kw = dict(out_format="rrggbb_le", layout="hwc", dtype=torch.uint8, size=size, light=spec)
    t1 = pkg.decode_to_tensor(files["clli"], tone=dict(dst_peak=DST, out_bits=8), **kw)
    assert t1.dtype == torch.uint8 and tuple(t1.shape) == (size[1], size[0], 3) and t1.cpu().numpy().tobytes() == want
    t2 = pkg.decode_batch_to_tensor([files["clli"], files["neither"]], tone=dict(dst_peak=DST, src_peak=None, out_bits=8), **kw)
    assert tuple(t2.shape) == (2, size[1], size[0], 3) and all(t2[k].cpu().numpy().tobytes() == want for k in range(2))
    t3 = pkg.decode_sequence_to_tensor(clip, frames=[1, 2], tone=dict(dst_peak=DST, src_peak=1000.0, out_bits=8), **kw)
    assert tuple(t3.shape) == (2, size[1], size[0], 3) and all(t3[k].cpu().numpy().tobytes() == want for k in range(2))
    with pytest.raises(ValueError, match="light"):
        pkg.decode_to_tensor(files["clli"], tone=dict(dst_peak=DST))
    with pytest.raises(pkg.HmError, match="dtype"):  # (8-bit integers of a deeper image need out_bits = 8)
        pkg.decode_to_tensor(files["clli"], tone=dict(dst_peak=DST), **kw)


def test_refusals_leave_every_byte_unwritten(capi, L, images):
    import heifwriter
    import torch
    files, pixels = images
    hdr = files["clli"]
    sdr = heifwriter.write_heic([synthutil.picture(48100, width=96, height=64)], (96, 64))
    nan, inf = float("nan"), float("inf")

    def refused(file, fmt, view, lt, tn, d, g, status, word):
        rc, msg, _ = tone_to_device(capi, L, file, fmt, view, lt, tn, d)
        assert rc == status and word in msg, (rc, msg, word)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"

    def fresh(fmt, layout, dtype, w=W, h=H, shrink=0):
        d, g, _, _ = base.make_dest(capi, L, fmt, layout, dtype, w, h, ONE, ZERO, 0, 0, shrink=shrink)
        return d, g
    T = capi.DeviceTone
    two = C.c_int32 * 2
    srgb = light_of(capi, to_transfer=13)
    cases = [(T(0, 0, 0.0, DST, 0.0, 0.0, two(0, 0)), "curve"), (T(3, 0, 0.0, DST, 0.0, 0.0, two(0, 0)), "curve"), (T(1, 0, 0.0, DST, 0.0, 0.0, two(1, 0)), "reserved"),
             (T(1, 0, 0.0, DST, 0.0, 0.0, two(0, -1)), "reserved"), (tone_of(capi, out_bits=10), "out_bits"), (tone_of(capi, out_bits=16), "out_bits"),
             (tone_of(capi, dst_peak=10.0, src_peak=10000.0), "KS"), (tone_of(capi, dst_peak=2.0), "KS"), (tone_of(capi, dst_peak=0.0), "dst_peak")]
    for bad in (nan, inf, -5.0, 10001.0):
        cases += [(tone_of(capi, src_peak=bad), "src_peak"), (tone_of(capi, dst_peak=bad), "dst_peak"), (tone_of(capi, unit_nits=bad), "unit_nits"),
                  (tone_of(capi, out_unit_nits=bad), "out_unit_nits")]
    for tn, word in cases:
        d, g = fresh(RRGGBB_LE, CHW, F32)
        refused(hdr, RRGGBB_LE, None, light_of(capi), tn, d, g, -1, word)
    d, g = fresh(RRGGBB_LE, CHW, F32)  # a null light step
    fh = C.c_void_p()
    assert L.hm_file_open(hdr, len(hdr), C.byref(fh)) == 0
    prm, out = capi.DecodeParams(RRGGBB_LE, THREADS, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
    assert L.hm_decode_item_to_device_tone(fh, L.hm_file_primary_item(fh), C.byref(prm), None, None, C.byref(tone_of(capi)), C.byref(d), C.byref(out)) == -1
    assert "null light step" in L.hm_last_error().decode()
    L.hm_file_close(fh)
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()
    d, g = fresh(RRGGBB_LE, HWC, U16)
    refused(hdr, RRGGBB_LE, None, srgb, tone_of(capi, out_bits=8), d, g, -1, "HM_DEV_U16")
    d, g = fresh(RRGGBBAA_LE, HWC, F32)
    refused(hdr, RRGGBBAA_LE, None, srgb, tone_of(capi, out_bits=8), d, g, -2, "four-channel")
    d, g = fresh(RGB, HWC, U8)  # (the 8-bit sibling's size: the request would fit)
    refused(hdr, RRGGBB_LE, None, srgb, tone_of(capi), d, g, -1, "dtype")
    refused(hdr, RRGGBB_LE, None, light_of(capi), tone_of(capi, out_bits=8), d, g, -1, "float dtype")
    refused(hdr, RRGGBB_BE, None, srgb, tone_of(capi, out_bits=8), d, g, -1, "_LE")
    d, g = fresh(RGB, HWC, U8, shrink=1)
    refused(hdr, RRGGBB_LE, None, srgb, tone_of(capi, out_bits=8), d, g, -1, "len")
    d, g = fresh(RGB, HWC, U8, 50, 37, shrink=1)
    refused(hdr, RRGGBB_LE, dv.make_view(capi, None, (50, 37), TRIANGLE), srgb, tone_of(capi, out_bits=8), d, g, -1, "len")
    d, g = fresh(RRGGBB_LE, CHW, F32)
    refused(hdr, RRGGBB_LE, None, light_of(capi, gain=0.0), tone_of(capi), d, g, -1, "gain")
    refused(hdr, RRGGBB_LE, None, light_of(capi, to_transfer=11), tone_of(capi), d, g, -2, "transfer")
    refused(hdr, RRGGBB_LE, dv.make_view(capi, (100, 50, 80, 60), (16, 16), TRIANGLE), light_of(capi), tone_of(capi), d, g, -1, "not inside")
    # a BT.709-class source says nothing about what 1.0 stands for: known once the image's profile is, before a byte is written
    for view, (ow, oh) in ((None, (96, 64)), (dv.make_view(capi, None, (40, 30), TRIANGLE), (40, 30))):
        d, g = fresh(RGB, CHW, F32, ow, oh)
        refused(sdr, RGB, view, light_of(capi), tone_of(capi, dst_peak=100.0, src_peak=203.0), d, g, -1, "unit_nits")
        rc, msg, _ = tone_to_device(capi, L, sdr, RGB, view, light_of(capi), tone_of(capi, dst_peak=100.0, src_peak=203.0, unit_nits=203.0), d)
        assert rc == 0, msg
        assert not (g.host()[g.start:g.start + 64] == 0xA5).all()
    # the pipeline and the frames form refuse at submission / before anything is queued
    cfg = capi.PipelineConfig(2, 2, RRGGBB_LE, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0
    try:
        d, g = fresh(RRGGBB_LE, CHW, F32)
        bad = tone_of(capi, dst_peak=2.0)  # (KS < 0 against the file's own peak)
        assert L.hm_pipeline_submit_to_device_tone(pipe, hdr, len(hdr), 0, 0, None, C.byref(light_of(capi)), C.byref(bad), C.byref(d)) == -1
        assert "KS" in L.hm_last_error().decode() and L.hm_pipeline_pending(pipe) == 0
    finally:
        L.hm_pipeline_destroy(pipe)
    pic = synthutil.picture(SEED, **PICTURE)
    clip = moovwriter.write_movie([pic, pic], (W, H), bit_depth=10)
    fh = C.c_void_p()
    assert L.hm_file_open(clip, len(clip), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(RRGGBB_LE, 2, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        bad = tone_of(capi, out_bits=7)
        assert L.hm_decode_frames_to_device_tone(fh, (C.c_uint32 * 1)(2), 1, C.byref(prm), None, C.byref(light_of(capi, from_transfer=16, from_primaries=9)), C.byref(bad),
                                                 C.byref(d), C.byref(out), None) == -1
    finally:
        L.hm_file_close(fh)
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()
    # ... and the library still decodes after all of that
    d, g, row, plane = base.make_dest(capi, L, RRGGBB_LE, HWC, U16, W, H, ONE, ZERO, 0, 0)
    rc, msg, _ = tone_to_device(capi, L, hdr, RRGGBB_LE, None, light_of(capi, to_transfer=16), tone_of(capi, 10000.0, 10000.0, 10000.0, 10000.0), d)
    assert rc == 0, msg
    same(g.host(), dv.place(pixels, HWC, U16, row, plane, g.size, g.start), g.start, "a decode after the refusals")


def test_the_new_kernel_instances_use_no_scratch(pkg):
    """the instances of the 8-bit finish from 16-bit samples as the loaded code object has them (test hook hm_debug_kernel_regs, code 10):
    no scratch.  LDS is dynamic, so the code object does not show it: the bound is held on what the launchers ask for (test hook
    hm_debug_light_lds, the functions the launches themselves size their LDS with) over every table combination the host can resolve -
    48 KB at the most, reached by 12-bit samples re-encoded at 12 bits with a tone step in the pointwise kernels."""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(10, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 128, (n, out[0], out[1])
        n += 1
    assert n == 5  # k_light_tensor<2, 3, uint8_t> x layout x store width, k_light_nearest<uint16_t, 3, uint8_t>
    T.hm_debug_light_lds.argtypes, T.hm_debug_light_lds.restype = [C.c_int] * 5, C.c_longlong
    asked = {(bits, eb, enc, tone, p): T.hm_debug_light_lds(bits, eb, enc, tone, p)
             for bits in range(8, 13) for eb in {bits, 8} for enc in (0, 1) for tone in (0, 1) for p in (0, 1, 2)}
    assert max(asked.values()) == asked[(12, 12, 1, 1, 0)] == 48 * 1024 and min(asked.values()) >= 0
    assert (asked[(12, 8, 1, 1, 0)], asked[(10, 10, 1, 1, 2)], asked[(12, 12, 1, 1, 1)], asked[(8, 8, 0, 0, 2)]) == (33 * 1024, 20 * 1024, 16 * 1024, 0)


def test_the_facade_reports_light_levels_on_decoded_images(api, images):
    """heif_image_has / get / set_content_light_level and ..._mastering_display_colour_volume: a decoded image carries the properties of
    the item that was decoded (the reference: context.cc:2087-2103), the setters replace them"""
    files, _ = images

    class Clli(C.Structure):
        _fields_ = [("max_cll", C.c_uint16), ("max_pall", C.c_uint16)]

    class Mdcv(C.Structure):
        _fields_ = [("x", C.c_uint16 * 3), ("y", C.c_uint16 * 3), ("wx", C.c_uint16), ("wy", C.c_uint16), ("hi", C.c_uint32), ("lo", C.c_uint32)]
    for name in ("heif_image_has_content_light_level", "heif_image_has_mastering_display_colour_volume"):
        getattr(api, name).argtypes = [C.c_void_p]
    for name, T in (("content_light_level", Clli), ("mastering_display_colour_volume", Mdcv)):
        for verb in ("get", "set"):
            fn = getattr(api, f"heif_image_{verb}_{name}")
            fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(T)], None
    want = {"clli": (1, (1000, 300), 0, (0, 0)), "mdcv": (0, (0, 0), 1, (6000000, 50)), "neither": (0, (0, 0), 0, (0, 0))}
    for name, (has_c, clli, has_m, lum) in want.items():
        ctx, h, img, e = fg._decode(api, files[name], 0, 1, RRGGBB_LE)  # heif_colorspace_RGB
        assert e.code == 0, e.message
        c, m = Clli(7, 7), Mdcv()
        api.heif_image_get_content_light_level(img, C.byref(c))
        api.heif_image_get_mastering_display_colour_volume(img, C.byref(m))
        assert (api.heif_image_has_content_light_level(img), (c.max_cll, c.max_pall)) == (has_c, clli), name
        assert (api.heif_image_has_mastering_display_colour_volume(img), (m.hi, m.lo)) == (has_m, lum), name
        if has_m:
            assert (tuple(zip(m.x, m.y)), (m.wx, m.wy)) == (hdrwriter.BT2020_XY, hdrwriter.D65_XY)
        api.heif_image_set_content_light_level(img, C.byref(Clli(0, 250)))  # (either field non-zero: pixelimage.h:167)
        api.heif_image_set_mastering_display_colour_volume(img, C.byref(Mdcv((C.c_uint16 * 3)(1, 2, 3), (C.c_uint16 * 3)(4, 5, 6), 7, 8, 9, 10)))
        api.heif_image_get_content_light_level(img, C.byref(c))
        api.heif_image_get_mastering_display_colour_volume(img, C.byref(m))
        assert api.heif_image_has_content_light_level(img) == 1 and (c.max_cll, c.max_pall) == (0, 250)
        assert api.heif_image_has_mastering_display_colour_volume(img) == 1 and (tuple(m.x), tuple(m.y), m.wx, m.wy, m.hi, m.lo) == ((1, 2, 3), (4, 5, 6), 7, 8, 9, 10)
        api.heif_image_set_content_light_level(img, None)  # (a null argument changes nothing)
        assert api.heif_image_has_content_light_level(img) == 1
        api.heif_image_release(img); api.heif_image_handle_release(h); api.heif_context_free(ctx)
