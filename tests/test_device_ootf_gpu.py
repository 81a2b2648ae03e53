"""GPU: the OOTF step (hm_decode_item_to_device_ootf, hm_decode_frames_to_device_ootf, hm_pipeline_submit_to_device_ootf,
hm_ootf_to_tensor and ootf= of the Python calls).  Everything is bit-exact: the expected image of every case is the model of
tests/ootf_ref.py on top of light_ref / tone_ref / alpha_ref, fed with the library's light and tone tables (held to their models by
the light and tone tests), the model's own OOTF tables and luminance weights (test_device_ootf.py holds the library's to them bit for
bit), hm_light_matrix's matrix and hm_view_filter_taps' weights.  Every destination sits in a guarded buffer pre-filled with 0xA5 and
the WHOLE buffer is compared.  A census of the model's k is asserted on every input set: pixels with k == 0, 1 <= k <= 511 (the
square-law part), 512 <= k <= 1022 and k == 1023 must all be there.  The file tests take the library's host decode as the decoded
picture (the suite holds it to the oracle elsewhere), as the tone tests do."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import hdrwriter
import light_ref
import moovwriter
import ootf_ref
import synthutil
import test_device_out_gpu as base
import test_device_tone_gpu as tg
import test_device_view_gpu as dv
from test_device_light_gpu import lib as light_lib  # noqa: F401  (a fixture: hm_light_table, hm_light_matrix, hm_view_filter_taps, each result once)
from test_device_tone_gpu import lib as tone_lib  # noqa: F401  (a fixture: ... and hm_tone_table)

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = tg.NP
TRIANGLE, NEAREST, LANCZOS3 = 0, 1, 17
ONE, ZERO, SCALE, BIAS = tg.ONE, tg.ZERO, tg.SCALE, tg.BIAS
PEAK, DST = 1000.0, 203.0
THREADS = 2


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def lib(tone_lib):
    """what the model is fed with, each computed once: the tone tests' tables, matrices and taps, and ootf(gain, primaries, peak,
    gamma) -> (y, thr, sg) of the model"""
    made = {}

    class Lib(tone_lib):
        @staticmethod
        def ootf(gain, primaries=9, peak=PEAK, gamma=0.0):
            key = (gain, primaries, peak, gamma)
            if key not in made:
                made[key] = (ootf_ref.luma(primaries),) + ootf_ref.tables(gain, peak, gamma)
            return made[key]
    return Lib


def ootf_of(capi, peak=PEAK, gamma=0.0):
    return capi.DeviceOotf(1, peak, gamma, (C.c_int32 * 5)(0, 0, 0, 0, 0))


def light_of(capi, to_transfer=8, to_primaries=0, gain=1.0, from_transfer=18, from_primaries=9):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def alpha_of(capi, mode, background=(0, 0, 0)):
    return capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*background, 0), (C.c_int32 * 3)(0, 0, 0))


def ref(s):
    return C.byref(s) if s is not None else None


def census(oo, r, what, negative=False):
    """every arm of the model's k holds pixels - and, where the case is about them, some luminances are negative"""
    arms = ootf_ref.arms(oo[0], oo[1], r)
    print(f"{what}: k == 0: {arms[0]}, 1 .. 511: {arms[1]}, 512 .. 1022: {arms[2]}, k == 1023: {arms[3]}")
    assert min(arms) > 0, (what, arms)
    if negative:
        ys = (oo[0][0] * r[..., 0] + oo[0][1] * r[..., 1]) + oo[0][2] * r[..., 2]
        assert (ys < 0).any(), what


def ramp_image(bits, w, h, channels, seed):
    """a grey ramp over all codes in row 0, a black row, a peak row (some samples above the peak of a deeper container: read as the
    peak), random colours below; with four channels a random alpha with zeros and the peak in it"""
    rng = np.random.default_rng(seed)
    peak = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    px = rng.integers(0, peak + 1, (h, w, channels)).astype(dt)
    px[0, :, :3] = np.linspace(0, peak, w).round().astype(dt)[:, None]
    px[1, :, :3] = 0
    px[2, :, :3] = peak
    if bits > 8:
        px[2, ::5, :3] = 65535
    if channels == 4:
        px[0:3, :, 3] = peak
        px[3, ::3, 3] = 0
        px[0, 5, 3] = 0
    return px


def upload(pixels):
    """the pixels in device memory with a 64-byte aligned stride: (tensor, stride)"""
    import torch
    h = pixels.shape[0]
    row = pixels.reshape(h, -1).view(np.uint8)
    stride = (row.shape[1] + 63) // 64 * 64 + 64
    src = np.zeros((h, stride), np.uint8)
    src[:, :row.shape[1]] = row
    return torch.from_numpy(src).cuda(), stride


@pytest.mark.parametrize("bits,w,h", [(8, 67, 5), (10, 67, 5), (12, 67, 5), (8, 131, 9), (10, 131, 9), (12, 131, 9)])
def test_the_step_alone_pointwise(capi, L, lib, bits, w, h):
    """hm_ootf_to_tensor without a view: 67 x 5 and 131 x 9 leave a ragged last 16-byte group for every dtype and more than one group
    of four rows; pitches rounded up to 16 bytes take the vector instance, one element more the scalar one (asserted); both layouts;
    float32, float16 and the target's integer dtype; linear and re-encoded (13); with and without the 2020 -> 709 matrix; with and
    without a tone step (its zeros: display_peak); the 8-bit finish.  12 bits re-encoded with a tone step is the 56 KB of LDS."""
    import torch
    fmt = RGB if bits == 8 else RRGGBB_LE
    pixels = ramp_image(bits, w, h, 3, bits * 1000 + w)
    dsrc, stride = upload(pixels)
    gain = 1.0 if bits != 10 else 0.5
    lin, m, oo = lib.table(18, bits, gain, False), lib.matrix(9, 1), lib.ootf(gain)
    tone_tables = lib.tone(gain, PEAK, DST, PEAK, DST)
    r, a, resampled = light_ref.light_sums(pixels, bits, lin, None, lib.taps)
    census(oo, r, f"{bits}-bit ramp {w} x {h}")
    own = U8 if bits == 8 else U16
    # (to_transfer, matrix, dtype, tone, out_bits, scale, bias)
    modes = [(8, None, F32, False, 0, SCALE, BIAS), (13, m, own, False, 0, ONE, ZERO), (8, m, F16, True, 0, SCALE, BIAS), (13, None, F32, True, 0, ONE, ZERO),
             (13, m, own, True, 0, ONE, ZERO)]
    if bits > 8:
        modes += [(13, m, U8, True, 8, ONE, ZERO), (13, None, F16, True, 8, SCALE, BIAS)]
    for to_transfer, mm, dtype, with_tone, out_bits, sc, bi in modes:
        enc = None if to_transfer == 8 else lib.table(to_transfer, 8 if out_bits == 8 else bits, gain, True)
        vals = ootf_ref.finish(r, a, resampled, enc, mm, oo, tone_tables if with_tone else None, NP[dtype], sc, bi)
        for layout in (HWC, CHW):
            for aligned in (True, False):
                d, g, row, plane = tg.pitched_dest(capi, L, tg.sibling(fmt, out_bits), layout, dtype, w, h, sc, bi, aligned)
                assert tg.takes_vector_instance(dsrc.data_ptr(), stride, d, layout, row, plane) == aligned
                lt = light_of(capi, to_transfer, 0 if mm is None else 1, gain)
                tn = tg.tone_of(capi, DST, 0.0, 0.0, 0.0, out_bits) if with_tone else None
                rc = L.hm_ootf_to_tensor(fmt, bits, w, h, dsrc.data_ptr(), stride, None, C.byref(lt), C.byref(ootf_of(capi)), ref(tn), None, C.byref(d), None)
                assert rc == 0, L.hm_last_error().decode()
                torch.cuda.synchronize()
                tg.same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start,
                        f"{bits} bits to {to_transfer} matrix {mm is not None} dtype {dtype} tone {with_tone} out_bits {out_bits} layout {layout} aligned {aligned}")


def view_image(bits=10, w=64, h=48):
    """the ramp image with blocks of black and peak below it: hard edges, so that Lanczos-3 undershoots below zero"""
    px = ramp_image(bits, w, h, 3, 4711)
    peak = (1 << bits) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = (((yy // 8) + (xx // 8)) % 2 * peak).astype(px.dtype)
    px[16:, :, :] = blocks[16:, :, None]
    return px


@pytest.mark.parametrize("name", ["crop", "nearest", "triangle", "lanczos3"])
def test_views(capi, L, lib, name):
    """the crop alone, HM_VIEW_NEAREST, and triangle and Lanczos-3 from 64 x 48 to 23 x 17: the sums are over scene light, the step
    follows them; Lanczos-3 produces negative sums (k == 0 with a negative Ys)"""
    import torch
    bits, w, h = 10, 64, 48
    pixels = view_image(bits, w, h)
    dsrc, stride = upload(pixels)
    view = {"crop": ((3, 0, 57, 40), None, TRIANGLE), "nearest": (None, (23, 17), NEAREST), "triangle": (None, (23, 17), TRIANGLE),
            "lanczos3": (None, (23, 17), LANCZOS3)}[name]
    gain = 1.0
    lin, m, oo = lib.table(18, bits, gain, False), lib.matrix(9, 1), lib.ootf(gain)
    tone_tables = lib.tone(gain, PEAK, DST, PEAK, DST)
    r, a, resampled = light_ref.light_sums(pixels, bits, lin, view, lib.taps)
    census(oo, r, name, negative=name == "lanczos3")
    oh, ow, _ = r.shape
    for to_transfer, mm, dtype, with_tone, out_bits, layout, sc, bi, pad in ((8, None, F32, False, 0, CHW, SCALE, BIAS, 0), (13, m, U16, False, 0, HWC, ONE, ZERO, 1),
                                                                           (13, m, U8, True, 8, HWC, ONE, ZERO, 0), (8, m, F16, True, 0, CHW, SCALE, BIAS, 2)):
        enc = None if to_transfer == 8 else lib.table(to_transfer, 8 if out_bits == 8 else bits, gain, True)
        vals = ootf_ref.finish(r, a, resampled, enc, mm, oo, tone_tables if with_tone else None, NP[dtype], sc, bi)
        d, g, row, plane = base.make_dest(capi, L, tg.sibling(RRGGBB_LE, out_bits), layout, dtype, ow, oh, sc, bi, pad, 0)
        lt = light_of(capi, to_transfer, 0 if mm is None else 1, gain)
        tn = tg.tone_of(capi, DST, 0.0, 0.0, 0.0, out_bits) if with_tone else None
        v = dv.make_view(capi, *view)
        rc = L.hm_ootf_to_tensor(RRGGBB_LE, bits, w, h, dsrc.data_ptr(), stride, C.byref(v), C.byref(lt), C.byref(ootf_of(capi)), ref(tn), None, C.byref(d), None)
        assert rc == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        tg.same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, f"{name} to {to_transfer} dtype {dtype} tone {with_tone}")


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("summed", [False, True])
def test_alpha_beside_it(capi, L, lib, bits, summed):
    """straight and matte, pointwise and resampled, on four-channel 8- and 10-bit sources: the step acts on the alpha step's r_c"""
    import torch
    fmt = RGBA if bits == 8 else RRGGBBAA_LE
    w, h = 67, 21
    pixels = ramp_image(bits, w, h, 4, 99 + bits)
    pixels[4:10], pixels[10:15, :, :3], pixels[10:15, :, 3] = (1 << bits) - 1, 0, (1 << bits) - 1  # (opaque peak and black bands a reduction keeps pure)
    dsrc, stride = upload(pixels)
    view = (None, (23, 9), TRIANGLE) if summed else None
    gain = 1.0
    lin, m, oo = lib.table(18, bits, gain, False), lib.matrix(9, 1), lib.ootf(gain)
    tone_tables = lib.tone(gain, PEAK, DST, PEAK, DST)
    own = U8 if bits == 8 else U16
    bg = (3, 10, 5) if bits == 8 else (12, 40, 20)  # (a dark matte: the transparent parts stay in the square-law arm)
    for mode, to_transfer, mm, dtype, with_tone, layout, sc, bi in ((alpha_ref.STRAIGHT, 8, None, F32, False, CHW, SCALE, BIAS), (alpha_ref.STRAIGHT, 13, m, own, True, HWC, ONE, ZERO),
                                                                  (alpha_ref.MATTE, 8, m, F32, True, HWC, SCALE, BIAS), (alpha_ref.MATTE, 13, None, own, False, CHW, ONE, ZERO)):
        enc = None if to_transfer == 8 else lib.table(to_transfer, bits, gain, True)
        vals, r = ootf_ref.render_alpha(pixels, bits, mode, bg, view, lib.taps, NP[dtype], sc, bi, lin, enc, mm, oo, tone_tables if with_tone else None)
        census(oo, r, f"alpha mode {mode} on {bits} bits, summed {summed}")
        oh, ow, _ = vals.shape
        al = alpha_of(capi, mode, bg if mode == alpha_ref.MATTE else (0, 0, 0))
        dfmt = L.hm_alpha_dest_format(fmt, C.byref(al), None)
        d, g, row, plane = base.make_dest(capi, L, dfmt, layout, dtype, ow, oh, sc, bi, 0, 0)
        lt = light_of(capi, to_transfer, 0 if mm is None else 1, gain)
        tn = tg.tone_of(capi, DST, 0.0, 0.0, 0.0, 0) if with_tone else None
        v = dv.make_view(capi, *view) if view else None
        rc = L.hm_ootf_to_tensor(fmt, bits, w, h, dsrc.data_ptr(), stride, ref(v), C.byref(lt), C.byref(ootf_of(capi)), ref(tn), C.byref(al), C.byref(d), None)
        assert rc == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        tg.same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, f"alpha mode {mode} {bits} bits summed {summed} to {to_transfer}")


def test_identity(capi, L, lib):
    """gamma = 1 writes the bytes of the same call without the step; a NULL ootf through the new entry is the old entry"""
    import torch
    bits, w, h = 10, 131, 9
    pixels = ramp_image(bits, w, h, 3, 5)
    dsrc, stride = upload(pixels)
    census(lib.ootf(1.0), light_ref.light_sums(pixels, bits, lib.table(18, bits, 1.0, False), None, lib.taps)[0], "identity")
    tn = tg.tone_of(capi, DST, PEAK, PEAK, DST, 0)
    for view, to_transfer, dtype, with_tone in ((None, 8, F32, False), (None, 13, U16, True), ((None, (23, 7), TRIANGLE), 13, F16, True), ((None, (40, 5), NEAREST), 8, F32, False)):
        ow, oh = view[1] if view else (w, h)
        v = dv.make_view(capi, *view) if view else None
        lt = light_of(capi, to_transfer, 1)
        got = []
        for call in ("gamma 1", "null", "old"):
            d, g, _, _ = base.make_dest(capi, L, RRGGBB_LE, HWC, dtype, ow, oh, SCALE, BIAS, 0, 0)
            t = ref(tn) if with_tone else None
            if call == "old":
                if with_tone:
                    rc = L.hm_tone_to_tensor(RRGGBB_LE, bits, w, h, dsrc.data_ptr(), stride, ref(v), C.byref(lt), t, C.byref(d), None)
                else:
                    rc = L.hm_light_to_tensor(RRGGBB_LE, bits, w, h, dsrc.data_ptr(), stride, ref(v), C.byref(lt), C.byref(d), None)
            elif call == "null" and not with_tone:
                continue  # (a NULL ootf goes through hm_tone_to_tensor, which wants its tone step)
            else:
                oo = ootf_of(capi, PEAK, 1.0) if call == "gamma 1" else None
                rc = L.hm_ootf_to_tensor(RRGGBB_LE, bits, w, h, dsrc.data_ptr(), stride, ref(v), C.byref(lt), ref(oo), t, None, C.byref(d), None)
            assert rc == 0, (call, L.hm_last_error().decode())
            torch.cuda.synchronize()
            got.append(g.host())
        assert all(np.array_equal(x, got[-1]) for x in got) and not (got[-1][base.GUARD:base.GUARD + 64] == 0xA5).all(), (view, to_transfer)


W, H = 64, 64
PICTURE = dict(width=W, height=H, bit_depth=10, full_range=0, matrix=9, primaries=9, qp=40)
SEED = 48411


@pytest.fixture(scope="module")
def hlg(hm):
    """a 10-bit 4:2:0 HLG BT.2020 HEIC (colr nclx 9 / 18 / 9) of 64 x 64, its host decode (h x w x 3 samples), a PQ twin, a two-frame clip"""
    pic = synthutil.picture(SEED, **PICTURE)
    data = hdrwriter.write_hdr_heic([pic], (W, H), colr=(9, 18, 9, 0))
    rows, w, h = base.host_rows(hm, data, RRGGBB_LE, THREADS)
    pixels = rows.view("<u2").reshape(h, w, 3)
    assert (w, h) == (W, H) and pixels.max() <= 1023
    return data, pixels, hdrwriter.write_hdr_heic([pic], (W, H), colr=(9, 16, 9, 0)), moovwriter.write_movie([pic, pic], (W, H), bit_depth=10)


def test_from_a_file_every_route(pkg, capi, L, lib, hlg):
    """ootf{1000}, tone{dst_peak 203, out_bits 8}, to_transfer 13, to_primaries 1: uint8 RGB in one call - the item call, the pipeline,
    decode_to_tensor, and a two-frame track through the frames form"""
    import torch
    data, pixels, _, clip = hlg
    lin, enc, m, oo = lib.table(18, 10, 1.0, False), lib.table(13, 8, 1.0, True), lib.matrix(9, 1), lib.ootf(1.0)
    r, a, resampled = light_ref.light_sums(pixels, 10, lin, None, lib.taps)
    census(oo, r, "the HLG picture")
    vals = ootf_ref.finish(r, a, resampled, enc, m, oo, lib.tone(1.0, PEAK, DST, PEAK, DST), np.uint8, ONE, ZERO)
    want = vals.tobytes()
    assert vals.shape == (H, W, 3) and len(np.unique(vals)) > 50
    lt, oo_c, tn = light_of(capi, 13, 1, 1.0, 0, 0), ootf_of(capi), tg.tone_of(capi, DST, 0.0, 0.0, 0.0, 8)

    def fresh():
        return base.make_dest(capi, L, RGB, HWC, U8, W, H, ONE, ZERO, 0, 0)

    def inner(g):
        got = g.host()
        assert (got[:g.start] == 0xA5).all() and (got[g.size - base.GUARD:] == 0xA5).all()
        return got[g.start:g.size - base.GUARD].tobytes()
    d, g, _, _ = fresh()
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        prm, out = capi.DecodeParams(RRGGBB_LE, THREADS, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
        rc = L.hm_decode_item_to_device_ootf(fh, L.hm_file_primary_item(fh), C.byref(prm), None, C.byref(lt), C.byref(oo_c), C.byref(tn), None, C.byref(d), C.byref(out))
        assert rc == 0, L.hm_last_error().decode()
        assert (out.width, out.height, out.transfer, out.primaries, out.bit_depth, out.out_format, out.stride[0]) == (W, H, 18, 9, 10, RRGGBB_LE, W * 3)
    finally:
        L.hm_file_close(fh)
    assert inner(g) == want
    # the pipeline
    cfg = capi.PipelineConfig(2, 2, RRGGBB_LE, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        d, g, _, _ = fresh()
        assert L.hm_pipeline_submit_to_device_ootf(pipe, data, len(data), 0, 7, None, C.byref(lt), C.byref(oo_c), C.byref(tn), None, C.byref(d)) == 0, L.hm_last_error().decode()
        res = capi.PipelineResult()
        assert L.hm_pipeline_next(pipe, C.byref(res)) == 0 and res.status == 0 and res.tag == 7, L.hm_last_error().decode()
        L.hm_pipeline_release(pipe, C.byref(res))
        assert inner(g) == want
    finally:
        L.hm_pipeline_destroy(pipe)
    # the frames form: a track carries no profile of its own, so from_* is explicit
    explicit = light_of(capi, 13, 1)
    g = base.Guarded(len(want) * 2)
    dests = (capi.DeviceDest * 2)()
    for k in range(2):
        dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = g.ptr + k * len(want), len(want), HWC, U8
        for c in range(4):
            dests[k].scale[c], dests[k].bias[c] = 1.0, 0.0
    fh = C.c_void_p()
    assert L.hm_file_open(clip, len(clip), C.byref(fh)) == 0
    try:
        prm, res, failed = capi.DecodeParams(RRGGBB_LE, 2, 0, 0, None, None, 0, 0, 0, 0), (capi.Decoded * 2)(), C.c_int32(-2)
        rc = L.hm_decode_frames_to_device_ootf(fh, (C.c_uint32 * 2)(2, 1), 2, C.byref(prm), None, C.byref(explicit), C.byref(oo_c), C.byref(tn), dests, res, C.byref(failed))
        assert rc == 0 and failed.value == -1, L.hm_last_error().decode()
    finally:
        L.hm_file_close(fh)
    assert inner(g) == want + want
    # the Python calls
    kw = dict(out_format="rrggbb_le", layout="hwc", dtype=torch.uint8, light=dict(to_transfer="srgb", to_primaries="bt709"), tone=dict(dst_peak=DST, out_bits=8))
    t1 = pkg.decode_to_tensor(data, ootf=1000, **kw)
    assert t1.dtype == torch.uint8 and tuple(t1.shape) == (H, W, 3) and t1.cpu().numpy().tobytes() == want
    t2 = pkg.decode_batch_to_tensor([data, data], ootf=dict(display_peak=1000.0), **kw)
    assert tuple(t2.shape) == (2, H, W, 3) and all(t2[k].cpu().numpy().tobytes() == want for k in range(2))
    kw["light"] = dict(from_transfer="hlg", from_primaries="bt2020", to_transfer="srgb", to_primaries="bt709")
    t3 = pkg.decode_sequence_to_tensor(clip, frames=[1, 2], ootf=1000, **kw)
    assert tuple(t3.shape) == (2, H, W, 3) and all(t3[k].cpu().numpy().tobytes() == want for k in range(2))


def test_a_pq_file_is_refused_behind_the_decode(capi, L, hlg):
    """from_transfer == 0 on a PQ file: known once the image reports its profile - HM_ERR_INVALID_ARG, and the destination, pre-filled
    with a sentinel, is unchanged"""
    import torch
    _, _, pq, _ = hlg
    d, g, _, _ = base.make_dest(capi, L, RRGGBB_LE, CHW, F32, W, H, ONE, ZERO, 0, 0)
    fh = C.c_void_p()
    assert L.hm_file_open(pq, len(pq), C.byref(fh)) == 0
    try:
        prm, out = capi.DecodeParams(RRGGBB_LE, THREADS, 0, 0, None, None, 0, 0, 0, 0), capi.Decoded()
        rc = L.hm_decode_item_to_device_ootf(fh, L.hm_file_primary_item(fh), C.byref(prm), None, C.byref(light_of(capi, 8, 0, 1.0, 0, 0)), C.byref(ootf_of(capi)), None, None,
                                             C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
    finally:
        L.hm_file_close(fh)
    assert rc == -1 and "from_transfer 16" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (g.host() == 0xA5).all()


def test_the_launchers_lds(pkg):
    """what the launchers ask for as dynamic LDS (test hook hm_debug_light_lds; bit 1 of its tone argument: an OOTF step): 56 KB at the
    most - 12-bit samples re-encoded at 12 bits with tone and OOTF in the pointwise kernels -, and for a call without the step what
    it asked for before"""
    pkg.lib()
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_light_lds.argtypes, T.hm_debug_light_lds.restype = [C.c_int] * 5, C.c_longlong
    asked = {(bits, eb, enc, steps, p): T.hm_debug_light_lds(bits, eb, enc, steps, p)
             for bits in range(8, 13) for eb in {bits, 8} for enc in (0, 1) for steps in (0, 1, 2, 3) for p in (0, 1, 2)}
    assert max(asked.values()) == asked[(12, 12, 1, 3, 0)] == 56 * 1024 <= 64 * 1024
    for (bits, eb, enc, steps, p), v in asked.items():
        assert v == asked[(bits, eb, enc, steps & 1, p)] + (8 * 1024 if steps & 2 and p != 1 else 0)
    assert max(v for k, v in asked.items() if not k[3] & 2) == 48 * 1024
