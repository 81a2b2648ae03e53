"""GPU: the alpha step (hm_alpha_to_tensor, hm_decode_item_to_device_alpha, hm_pipeline_submit_to_device_alpha and alpha= of the
Python calls).  Everything is bit-exact, with no tolerance anywhere: the expected image of every case is the model of
tests/alpha_ref.py - written from the header's text -, fed with the library's tables (hm_light_table, hm_tone_table), hm_light_matrix's
matrix and hm_view_filter_taps' weights; __fdiv_rn and numpy's float32 division are both correctly rounded.  Every destination sits in
a guarded buffer pre-filled with 0xA5 and the WHOLE buffer is compared, as in test_device_light_gpu.py.  The crafted arrays hold alpha
0, 1, peak - 1 and peak and colour 0 and peak (a census asserted where they are made), and a hard edge between opaque and transparent
columns, so that the cubic and Lanczos sums leave [0, P]: asserted on the model in the view test."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref
import heifwriter
import synthutil
import test_device_out_gpu as base
import test_device_view_gpu as dv
from test_device_light_gpu import lib as light_lib  # noqa: F401  (a fixture: hm_light_table, hm_light_matrix, hm_view_filter_taps, each result once)
from test_device_tone_gpu import lib  # noqa: F401  (a fixture: the same with hm_tone_table)

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 13, 14, 15
HWC, CHW = base.HWC, base.CHW
U8, U16, F16, F32 = base.U8, base.U16, base.F16, base.F32
NP = {U8: np.uint8, U16: np.uint16, F16: np.float16, F32: np.float32}
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
STRAIGHT, PREMULTIPLIED, MATTE = alpha_ref.STRAIGHT, alpha_ref.PREMULTIPLIED, alpha_ref.MATTE
MODES = (STRAIGHT, PREMULTIPLIED, MATTE)
ONE, ZERO = [1.0] * 4, [0.0] * 4
SCALE, BIAS = [2.0, 0.75, 16.0, 1.0], [-1.0, 0.125, 0.5, 0.0]
THREADS = 2


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def alpha_of(capi, mode, background=(0, 0, 0), reserved=(0, 0, 0)):
    bg = tuple(background) + (0,) * (4 - len(background))
    return capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*bg), (C.c_int32 * 3)(*reserved))


def light_of(capi, from_transfer=0, from_primaries=0, to_transfer=8, to_primaries=0, gain=1.0):
    return capi.DeviceLight(from_transfer, from_primaries, to_transfer, to_primaries, gain, (C.c_int32 * 3)(0, 0, 0))


def same(got, exp, start, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - start} from the destination's start (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")


def background(bits):
    peak = (1 << bits) - 1
    return (peak, peak // 3, 1)


def sibling(fmt, mode, out_bits=0):
    """the target the destination is judged, sized and written as"""
    if mode != MATTE:
        return fmt
    return RGB if fmt == RGBA or out_bits == 8 else RRGGBB_LE


def crafted(bits, w, h):
    """h x w x 4 samples of `bits` bits: columns [0, w / 3) opaque, [w / 3, 2 w / 3) transparent - a hard edge on either side -, the
    rest random alpha with 0, 1, peak - 1 and peak frequent; random colour with 0 and peak frequent, also under alpha 0"""
    rng = np.random.default_rng(bits * 100000 + w * 100 + h)
    peak = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    px = rng.integers(0, peak + 1, (h, w, 4), dtype=dt)
    pick = rng.integers(0, 8, (h, w, 4))
    px[pick == 0] = 0
    px[pick == 1] = peak
    a = px[..., 3]
    a[pick[..., 3] == 2] = 1
    a[pick[..., 3] == 3] = peak - 1
    a[:, :w // 3] = peak
    a[:, w // 3:2 * w // 3] = 0
    a[h // 2, :] = rng.choice(np.array([0, 1, peak - 1, peak], dt), w)  # (one row where the edge is broken up)
    for v in (0, 1, peak - 1, peak):
        assert (a == v).sum() >= 4, (bits, w, h, v)
    for v in (0, peak):
        assert (px[..., :3] == v).sum() >= 12 and (px[..., :3][a == 0] == v).any() and (px[..., :3][a == peak] == v).any(), (bits, w, h, v)
    return px


def upload(px, offset_samples=0):
    """the array in device memory, rows 64-byte aligned (offset_samples: the first sample that many samples behind an aligned address) ->
    (tensor that owns the memory, pointer, stride)"""
    import torch
    h, w, c = px.shape
    sb = px.dtype.itemsize
    stride = (w * c * sb + 63) // 64 * 64 + 64
    buf = np.zeros(h * stride + 64, np.uint8)
    off = offset_samples * sb
    rows = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w * c * sb), strides=(stride, 1))
    rows[...] = px.reshape(h, -1).view(np.uint8)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 64 == 0
    return t, t.data_ptr() + off, stride


def pitched_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, aligned):
    """a destination with explicit pitches: rounded up to 16 bytes (the 16-byte instance runs, with its ragged last group), or one
    element more than that (no 16-byte store can follow: the scalar instance)"""
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


def to_tensor(capi, L, fmt, bits, w, h, ptr, stride, view, lt, tn, al, d):
    import torch
    v = dv.make_view(capi, *view) if view is not None else None
    rc = L.hm_alpha_to_tensor(fmt, bits, w, h, ptr, stride, C.byref(v) if v is not None else None, C.byref(lt) if lt is not None else None,
                              C.byref(tn) if tn is not None else None, C.byref(al), C.byref(d), None)
    msg = L.hm_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg


@pytest.mark.parametrize("bits,w,h", [(8, 1029, 5), (12, 1029, 5), (8, 37, 23), (12, 37, 23)])
def test_the_step_alone_on_crafted_arrays(capi, L, lib, bits, w, h):
    """hm_alpha_to_tensor without a view: every mode, both layouts, every dtype the mode admits - the integers round half up -, with
    pitches rounded up to 16 bytes (the 16-byte instance: 1029 x 5 is a full wave of 16-pixel groups, a ragged group and a ragged row
    group) and one element wider (the scalar instance).  STRAIGHT moves nothing but the samples: the bytes of hm_to_tensor."""
    fmt = RGBA if bits == 8 else RRGGBBAA_LE
    px = crafted(bits, w, h)
    keep, ptr, stride = upload(px)
    bg = background(bits)
    for mode in MODES:
        al = alpha_of(capi, mode, bg if mode == MATTE else (0, 0, 0))
        dfmt = sibling(fmt, mode)
        for dtype, sc, bi in ((U8 if bits == 8 else U16, ONE, ZERO), (F16, SCALE, BIAS), (F32, SCALE, BIAS)):
            vals, _, _ = alpha_ref.render(px, bits, mode, bg, None, lib.taps, NP[dtype], sc, bi)
            assert vals.shape == (h, w, 3 if mode == MATTE else 4)
            for layout in (HWC, CHW):
                for aligned in (True, False):
                    what = f"{bits} bits {w} x {h} mode {mode} dtype {dtype} layout {layout} aligned {aligned}"
                    d, g, row, plane = pitched_dest(capi, L, dfmt, layout, dtype, w, h, sc, bi, aligned)
                    rc, msg = to_tensor(capi, L, fmt, bits, w, h, ptr, stride, None, None, None, al, d)
                    assert rc == 0, f"{what}: {msg}"
                    got = g.host()
                    same(got, dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
                    if mode == STRAIGHT:
                        d2, g2, _, _ = pitched_dest(capi, L, fmt, layout, dtype, w, h, sc, bi, aligned)
                        assert L.hm_to_tensor(fmt, w, h, ptr, stride, C.byref(d2), None) == 0, L.hm_last_error().decode()
                        import torch
                        torch.cuda.synchronize()
                        assert np.array_equal(got, g2.host()), what
    del keep


VIEWS = [(None, (11, 7), TRIANGLE), (None, (37, 23), TRIANGLE), (None, (11, 7), CUBIC), (None, (37, 23), CUBIC), (None, (11, 7), LANCZOS3), (None, (37, 23), LANCZOS3),
         ((2, 1, 33, 21), (11, 7), CUBIC), (None, (11, 7), NEAREST), (None, (50, 9), NEAREST), ((5, 3, 29, 17), None, TRIANGLE)]


@pytest.mark.parametrize("bits", [8, 12])
def test_views_of_the_crafted_arrays(capi, L, lib, bits):
    """37 x 23 -> 11 x 7 and -> 37 x 23 under all three filters, nearest and the crop alone, every mode.  Where sums are formed the
    products are summed; the cubic and Lanczos cases hold outputs with S_a <= 0 or cov outside [0, 1] (asserted on the model), the
    reductions among them true overshoot: S_a < 0 and S_a > P.  STRAIGHT without sums: the bytes of hm_resample_to_tensor.  One source
    sits one sample behind an aligned address: at 8 bits the horizontal pass then loads sample by sample."""
    import torch
    w, h = 37, 23
    fmt = RGBA if bits == 8 else RRGGBBAA_LE
    px = crafted(bits, w, h)
    P = float((1 << bits) - 1)
    bg = background(bits)
    sources = [upload(px), upload(px, 1)]
    integer = U8 if bits == 8 else U16
    n = 0
    for view in VIEWS:
        crop, size, filt = view
        summed = size is not None and filt != NEAREST
        for mode in MODES:
            al = alpha_of(capi, mode, bg if mode == MATTE else (0, 0, 0))
            dfmt = sibling(fmt, mode)
            for layout, dtype, sc, bi, pad in ((HWC, integer, ONE, ZERO, 0), (CHW, F32, SCALE, BIAS, 1), (CHW, integer, ONE, ZERO, 2), (HWC, F16, SCALE, BIAS, 2)):
                n += 1
                what = f"{bits} bits view {view} mode {mode} layout {layout} dtype {dtype} pad {pad}"
                vals, S, Sa = alpha_ref.render(px, bits, mode, bg, view, lib.taps, NP[dtype], sc, bi)
                if filt in (CUBIC, LANCZOS3):
                    cov = Sa / np.float32(P)
                    assert (Sa <= 0).any() or (cov < 0).any() or (cov > 1).any(), what
                    if size == (11, 7):
                        assert (Sa < 0).any() and (Sa > P).any(), what
                oh, ow, _ = vals.shape
                d, g, row, plane = base.make_dest(capi, L, dfmt, layout, dtype, ow, oh, sc, bi, pad, 0)
                keep, ptr, stride = sources[n % 2]
                rc, msg = to_tensor(capi, L, fmt, bits, w, h, ptr, stride, view, None, None, al, d)
                assert rc == 0, f"{what}: {msg}"
                got = g.host()
                same(got, dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
                if mode == STRAIGHT and not summed:
                    d2, g2, _, _ = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, sc, bi, pad, 0)
                    v = dv.make_view(capi, *view)
                    assert L.hm_resample_to_tensor(fmt, w, h, ptr, stride, C.byref(v), C.byref(d2), None) == 0, L.hm_last_error().decode()
                    torch.cuda.synchronize()
                    assert np.array_equal(got, g2.host()), what


LIGHT_VIEWS = [None, (None, (11, 7), TRIANGLE), ((2, 1, 33, 21), (13, 9), LANCZOS3), (None, (20, 30), NEAREST), ((5, 3, 29, 17), None, TRIANGLE)]


@pytest.mark.parametrize("bits", [8, 12])
def test_beside_the_light_step(capi, L, lib, bits):
    """sRGB to linear float in each mode, and re-encoded through a P3 matrix for STRAIGHT and MATTE: x_c = lin[v_c], the background
    b_c = lin[background[c]], and r takes the place of the resampled light.  STRAIGHT without sums: the bytes of hm_light_to_tensor.
    At 12 bits both tables of a pointwise kernel are 16 KB, and a few colour words lie above the peak: they are read as the peak."""
    import torch
    w, h = 37, 23
    fmt = RGBA if bits == 8 else RRGGBBAA_LE
    px = crafted(bits, w, h)
    if bits > 8:
        rng = np.random.default_rng(3)
        px[rng.integers(0, h, 12), rng.integers(0, w, 12), rng.integers(0, 3, 12)] = rng.integers(1 << bits, 65536, 12, dtype=np.uint16)
    keep, ptr, stride = upload(px)
    bg = background(bits)
    gain = 2.0
    lin, enc, m = lib.table(13, bits, gain, False), lib.table(13, bits, gain, True), lib.matrix(1, 12)
    integer = U8 if bits == 8 else U16
    # (to_transfer, matrix, modes, layout, dtype, scale, bias, pad)
    plans = ((8, None, MODES, CHW, F32, SCALE, BIAS, 0), (8, None, MODES, HWC, F16, SCALE, BIAS, 2), (13, m, (STRAIGHT, MATTE), HWC, integer, ONE, ZERO, 0),
             (13, m, (STRAIGHT, MATTE), CHW, F32, SCALE, BIAS, 1))
    for view in LIGHT_VIEWS:
        summed = view is not None and view[1] is not None and view[2] != NEAREST
        for to_transfer, mm, modes, layout, dtype, sc, bi, pad in plans:
            lt = light_of(capi, from_transfer=13, from_primaries=1, to_transfer=to_transfer, to_primaries=0 if mm is None else 12, gain=gain)
            for mode in modes:
                what = f"view {view} to {to_transfer} matrix {mm is not None} mode {mode} layout {layout} dtype {dtype}"
                al = alpha_of(capi, mode, bg if mode == MATTE else (0, 0, 0))
                vals, _, _ = alpha_ref.render(px, bits, mode, bg, view, lib.taps, NP[dtype], sc, bi, lin=lin, enc=enc if to_transfer != 8 else None, m=mm)
                oh, ow, _ = vals.shape
                d, g, row, plane = base.make_dest(capi, L, sibling(fmt, mode), layout, dtype, ow, oh, sc, bi, pad, 0)
                rc, msg = to_tensor(capi, L, fmt, bits, w, h, ptr, stride, view, lt, None, al, d)
                assert rc == 0, f"{what}: {msg}"
                got = g.host()
                same(got, dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
                if mode == STRAIGHT and not summed:
                    d2, g2, _, _ = base.make_dest(capi, L, fmt, layout, dtype, ow, oh, sc, bi, pad, 0)
                    v = dv.make_view(capi, *view) if view is not None else None
                    assert L.hm_light_to_tensor(fmt, bits, w, h, ptr, stride, C.byref(v) if v is not None else None, C.byref(lt), C.byref(d2), None) == 0
                    torch.cuda.synchronize()
                    assert np.array_equal(got, g2.host()), what


def test_beside_the_tone_step(capi, L, lib):
    """a 10-bit RRGGBBAA_LE array, PQ BT.2020 to sRGB BT.709 under the BT.2390 curve, out_bits = 8, MATTE over white, into uint8 RGB: the
    one four-channel request the 8-bit finish takes.  12 bits re-encoded with a tone step is the most LDS a kernel asks for."""
    for bits, w, h in ((10, 37, 23), (12, 131, 9)):
        fmt = RRGGBBAA_LE
        px = crafted(bits, w, h)
        keep, ptr, stride = upload(px)
        peak = (1 << bits) - 1
        bg = (peak, peak, peak)
        gain, srcp, dst = 1.0, 1000.0, 203.0
        lin, enc8, m = lib.table(16, bits, gain, False), lib.table(13, 8, gain, True), lib.matrix(9, 1)
        tables = lib.tone(gain, srcp, dst, 10000.0, dst)
        lt = light_of(capi, from_transfer=16, from_primaries=9, to_transfer=13, to_primaries=1, gain=gain)
        tn = capi.DeviceTone(1, 8, srcp, dst, 10000.0, dst, (C.c_int32 * 2)(0, 0))
        al = alpha_of(capi, MATTE, bg)
        assert L.hm_alpha_dest_format(fmt, C.byref(al), C.byref(tn)) == RGB
        for view in (None, (None, (11, 7), TRIANGLE), ((2, 1, 33, 8), (13, 5), CUBIC), (None, (20, 30), NEAREST)):
            for layout, dtype, sc, bi, aligned in ((HWC, U8, ONE, ZERO, True), (CHW, U8, ONE, ZERO, False), (CHW, F32, SCALE, BIAS, True)):
                what = f"{bits} bits view {view} layout {layout} dtype {dtype} aligned {aligned}"
                vals, _, _ = alpha_ref.render(px, bits, MATTE, bg, view, lib.taps, NP[dtype], sc, bi, lin=lin, enc=enc8, m=m, tone=tables)
                oh, ow, c = vals.shape
                assert c == 3
                d, g, row, plane = pitched_dest(capi, L, RGB, layout, dtype, ow, oh, sc, bi, aligned)
                rc, msg = to_tensor(capi, L, fmt, bits, w, h, ptr, stride, view, lt, tn, al, d)
                assert rc == 0, f"{what}: {msg}"
                same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
        # the target's own depth beside the tone step: 16-bit codes, three channels
        tn0 = capi.DeviceTone(1, 0, srcp, dst, 10000.0, dst, (C.c_int32 * 2)(0, 0))
        enc = lib.table(13, bits, gain, True)
        vals, _, _ = alpha_ref.render(px, bits, MATTE, bg, (None, (11, 7), TRIANGLE), lib.taps, np.uint16, ONE, ZERO, lin=lin, enc=enc, m=m, tone=tables)
        d, g, row, plane = base.make_dest(capi, L, RRGGBB_LE, HWC, U16, 11, 7, ONE, ZERO, 0, 0)
        rc, msg = to_tensor(capi, L, fmt, bits, w, h, ptr, stride, (None, (11, 7), TRIANGLE), lt, tn0, al, d)
        assert rc == 0, msg
        same(g.host(), dv.place(vals, HWC, U16, row, plane, g.size, g.start), g.start, f"{bits} bits, out_bits 0")
        del keep


@pytest.fixture(scope="module")
def files(hm):
    """name -> (file bytes, the host decode's RGBA pixels as h x w x 4 samples): the alpha_aux construction (a 96 x 64 image with a
    48 x 32 alpha image), a 2 x 2 grid whose tiles 0 and 3 carry alpha images, an image without alpha"""
    main = synthutil.picture(49400, width=96, height=64, vui=1, full_range=1, matrix=6)
    tiles = [synthutil.picture(49410 + i, width=64, height=64, vui=1, full_range=1, matrix=6) for i in range(4)]
    data = {"alpha_aux": heifwriter.write_heic([main], (96, 64), aux=[(synthutil.picture(49401, width=48, height=32), (48, 32), base.ALPHA_URN)]),
            "grid": heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 120, 100),
                                          aux=[(synthutil.picture(49420, width=64, height=64, chroma_format=0), (64, 64), base.ALPHA_URN, 0, 8, 1),
                                               (synthutil.picture(49421, width=32, height=32), (32, 32), base.ALPHA_URN, 1, 8, 4)]),
            "no_alpha": heifwriter.write_heic([main], (96, 64))}
    out = {}
    for name, d in data.items():
        rows, w, h = base.host_rows(hm, d, RGBA, THREADS)
        out[name] = (d, rows.reshape(h, w, 4))
    assert out["alpha_aux"][1].shape == (64, 96, 4) and out["grid"][1].shape == (100, 120, 4)
    assert len(np.unique(out["alpha_aux"][1][..., 3])) > 8 and len(np.unique(out["grid"][1][..., 3])) > 8
    assert (out["no_alpha"][1][..., 3] == 255).all()
    return out


def alpha_to_device(capi, L, data, fmt, view, lt, tn, al, d, threads=THREADS):
    import torch
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        v = dv.make_view(capi, *view) if view is not None else None
        rc = L.hm_decode_item_to_device_alpha(h, L.hm_file_primary_item(h), C.byref(prm), C.byref(v) if v is not None else None, C.byref(lt) if lt is not None else None,
                                              C.byref(tn) if tn is not None else None, C.byref(al), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        torch.cuda.synchronize()
        return rc, msg, out
    finally:
        L.hm_file_close(h)


FILE_CASES = [(None, STRAIGHT, HWC, U8, ONE, ZERO), (None, PREMULTIPLIED, CHW, F32, SCALE, BIAS), (None, MATTE, HWC, U8, ONE, ZERO),
              ((None, (40, 30), TRIANGLE), STRAIGHT, CHW, F32, SCALE, BIAS), ((None, (40, 30), TRIANGLE), MATTE, CHW, U8, ONE, ZERO),
              (((10, 6, 80, 50), (33, 21), LANCZOS3), PREMULTIPLIED, HWC, U8, ONE, ZERO), (((10, 6, 80, 50), (33, 21), CUBIC), MATTE, HWC, F16, SCALE, BIAS)]


@pytest.mark.parametrize("name", ["alpha_aux", "grid", "no_alpha"])
def test_files_equal_the_model_on_the_host_decodes_pixels(capi, L, lib, files, name):
    """hm_decode_item_to_device_alpha with and without a view, alone and beside a light step"""
    data, px = files[name]
    h, w, _ = px.shape
    bg = (255, 255, 255)
    for view, mode, layout, dtype, sc, bi in FILE_CASES:
        al = alpha_of(capi, mode, bg if mode == MATTE else (0, 0, 0))
        vals, _, _ = alpha_ref.render(px, 8, mode, bg, view, lib.taps, NP[dtype], sc, bi)
        oh, ow, _ = vals.shape
        d, g, row, plane = base.make_dest(capi, L, sibling(RGBA, mode), layout, dtype, ow, oh, sc, bi, 0, 0)
        rc, msg, out = alpha_to_device(capi, L, data, RGBA, view, None, None, al, d)
        what = f"{name} view {view} mode {mode} layout {layout} dtype {dtype}"
        assert rc == 0, f"{what}: {msg}"
        assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (ow, oh, 1, row, RGBA), what
        assert out.has_alpha == (0 if name == "no_alpha" else 1)
        same(g.host(), dv.place(vals, layout, dtype, row, plane, g.size, g.start), g.start, what)
    # beside a light step whose from_* are the image's own (a grid canvas reports the sRGB defaults)
    lin = lib.table(13, 8, 1.0, False)
    view = (None, (40, 30), TRIANGLE)
    vals, _, _ = alpha_ref.render(px, 8, MATTE, bg, view, lib.taps, np.float32, SCALE, BIAS, lin=lin)
    d, g, row, plane = base.make_dest(capi, L, RGB, CHW, F32, 40, 30, SCALE, BIAS, 0, 0)
    rc, msg, out = alpha_to_device(capi, L, data, RGBA, view, light_of(capi, from_transfer=13, from_primaries=1), None, alpha_of(capi, MATTE, bg), d)
    assert rc == 0, msg
    same(g.host(), dv.place(vals, CHW, F32, row, plane, g.size, g.start), g.start, f"{name} beside a light step")


def test_a_16_bit_target_from_a_file(hm, capi, L, lib, files):
    """RRGGBBAA_LE of the 8-bit alpha_aux image: 10-bit samples (hm_decoded.bit_depth), a background at that depth"""
    data, _ = files["alpha_aux"]
    rows, w, h = base.host_rows(hm, data, RRGGBBAA_LE, THREADS)
    px = rows.view("<u2").reshape(h, w, 4)
    assert px.max() <= 1023
    bg = (1023, 512, 0)
    view = (None, (40, 30), TRIANGLE)
    vals, _, _ = alpha_ref.render(px, 10, MATTE, bg, view, lib.taps, np.uint16, ONE, ZERO)
    d, g, row, plane = base.make_dest(capi, L, RRGGBB_LE, HWC, U16, 40, 30, ONE, ZERO, 0, 0)
    rc, msg, out = alpha_to_device(capi, L, data, RRGGBBAA_LE, view, None, None, alpha_of(capi, MATTE, bg), d)
    assert rc == 0, msg
    assert (out.bit_depth, out.out_format, out.stride[0]) == (10, RRGGBBAA_LE, row)
    same(g.host(), dv.place(vals, HWC, U16, row, plane, g.size, g.start), g.start, "RRGGBBAA_LE matte")


def test_the_pipeline_and_the_python_calls(pkg, capi, L, lib, files):
    import torch
    bg = (255, 255, 255)
    view = (None, (40, 30), TRIANGLE)
    names = ["alpha_aux", "no_alpha", "grid"]
    expected = {n: alpha_ref.render(files[n][1], 8, MATTE, bg, view, lib.taps, np.uint8, ONE, ZERO)[0] for n in names}
    straight = alpha_ref.render(files["alpha_aux"][1], 8, STRAIGHT, None, view, lib.taps, np.float32, SCALE, BIAS)[0]
    cfg = capi.PipelineConfig(4, 4, RGBA, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        v = dv.make_view(capi, *view)
        al = alpha_of(capi, MATTE, bg)
        dests = [base.make_dest(capi, L, RGB, HWC, U8, 40, 30, ONE, ZERO, 0, 0) for _ in names]
        for k, n in enumerate(names):
            data = files[n][0]
            assert L.hm_pipeline_submit_to_device_alpha(pipe, data, len(data), 0, k, C.byref(v), None, None, C.byref(al), C.byref(dests[k][0])) == 0, L.hm_last_error().decode()
        for k, n in enumerate(names):
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0 and r.status == 0 and r.tag == k, L.hm_last_error().decode()
            d, g, row, plane = dests[k]
            same(g.host(), dv.place(expected[n], HWC, U8, row, plane, g.size, g.start), g.start, f"pipeline {n}")
            L.hm_pipeline_release(pipe, C.byref(r))
        bad = alpha_of(capi, MATTE, (0, 300, 0))
        assert L.hm_pipeline_submit_to_device_alpha(pipe, files["grid"][0], len(files["grid"][0]), 0, 9, C.byref(v), None, None, C.byref(bad), C.byref(dests[0][0])) == -1
    finally:
        L.hm_pipeline_destroy(pipe)
    t = pkg.decode_to_tensor(files["alpha_aux"][0], out_format="rgba", layout="hwc", dtype=torch.uint8, size=(40, 30), alpha=dict(mode="matte", background=bg))
    assert tuple(t.shape) == (30, 40, 3) and np.array_equal(t.cpu().numpy(), expected["alpha_aux"])
    t = pkg.decode_to_tensor(files["alpha_aux"][0], out_format="rgba", size=(40, 30), scale=SCALE, bias=BIAS, alpha="straight")
    assert tuple(t.shape) == (4, 30, 40) and np.array_equal(t.cpu().numpy(), straight.transpose(2, 0, 1))
    t = pkg.decode_batch_to_tensor([files[n][0] for n in names], out_format="rgba", layout="hwc", dtype=torch.uint8, size=(40, 30),
                                   alpha=dict(mode="matte", background=bg))
    assert tuple(t.shape) == (3, 30, 40, 3)
    for k, n in enumerate(names):
        assert np.array_equal(t[k].cpu().numpy(), expected[n]), n
    with pytest.raises(ValueError, match="four-channel"):
        pkg.decode_to_tensor(files["alpha_aux"][0], out_format="rgb", alpha="straight")
    with pytest.raises(pkg.HmError, match="peak"):
        pkg.decode_to_tensor(files["alpha_aux"][0], out_format="rgba", alpha=dict(mode="matte", background=(256, 0, 0)))


def test_refusals_leave_every_byte_unwritten(capi, L, files):
    import torch
    data, px = files["alpha_aux"]

    def refused(fmt, view, lt, tn, al, d, g, status, word):
        rc, msg, _ = alpha_to_device(capi, L, data, fmt, view, lt, tn, al, d)
        assert rc == status and word in msg, (rc, msg, word)
        torch.cuda.synchronize()
        assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"

    def fresh(f, layout, dtype, w, h, shrink=0):
        d, g, _, _ = base.make_dest(capi, L, f, layout, dtype, w, h, ONE, ZERO, 0, 0, shrink=shrink)
        return d, g

    def tone(out_bits=0, unit_nits=203.0):
        return capi.DeviceTone(1, out_bits, 1000.0, 203.0, unit_nits, 0.0, (C.c_int32 * 2)(0, 0))
    d, g = fresh(RGBA, CHW, F32, 96, 64)
    for al, word in ((alpha_of(capi, 0), "mode"), (alpha_of(capi, 4), "mode"), (alpha_of(capi, STRAIGHT, reserved=(0, 1, 0)), "reserved"),
                     (alpha_of(capi, STRAIGHT, (0, 0, 7)), "background"), (alpha_of(capi, PREMULTIPLIED, (1, 0, 0)), "background"),
                     (capi.DeviceAlpha(MATTE, (C.c_uint16 * 4)(0, 0, 0, 9), (C.c_int32 * 3)(0, 0, 0)), "background[3]"), (alpha_of(capi, MATTE, (0, 256, 0)), "peak")):
        refused(RGBA, None, None, None, al, d, g, -1, word)
    # a background above the peak of a 16-bit target: known once the image reports its depth (10 bits here), refused before a byte is written
    d16, g16 = fresh(RRGGBB_LE, HWC, U16, 96, 64)
    refused(RRGGBBAA_LE, None, None, None, alpha_of(capi, MATTE, (0, 1024, 0)), d16, g16, -1, "peak")
    d16v, g16v = fresh(RRGGBB_LE, HWC, U16, 40, 30)
    refused(RRGGBBAA_LE, (None, (40, 30), TRIANGLE), None, None, alpha_of(capi, MATTE, (0, 0, 65535)), d16v, g16v, -1, "peak")
    # a three-channel target, a _BE target, a planar one
    d3, g3 = fresh(RGB, CHW, F32, 96, 64)
    refused(RGB, None, None, None, alpha_of(capi, STRAIGHT), d3, g3, -1, "three-channel")
    refused(RRGGBB_LE, None, None, None, alpha_of(capi, MATTE), d3, g3, -1, "three-channel")
    dbe, gbe = fresh(RRGGBBAA_BE, HWC, U16, 96, 64)
    refused(RRGGBBAA_BE, None, None, None, alpha_of(capi, STRAIGHT), dbe, gbe, -1, "_LE")
    refused(RRGGBBAA_BE, ((7, 5, 33, 21), None, TRIANGLE), None, None, alpha_of(capi, MATTE), dbe, gbe, -1, "_LE")
    refused(0x103, None, None, None, alpha_of(capi, STRAIGHT), d, g, -2, "planar")
    # PREMULTIPLIED beside a tone step, and beside a light step that re-encodes
    refused(RGBA, None, light_of(capi, to_transfer=13), tone(), alpha_of(capi, PREMULTIPLIED), d, g, -1, "tone")
    refused(RGBA, None, light_of(capi, to_transfer=13), None, alpha_of(capi, PREMULTIPLIED), d, g, -1, "re-encodes")
    # what the tone, light, view and destination checks refuse today; a matte is judged against the sibling target
    refused(RGBA, None, None, tone(), alpha_of(capi, MATTE), d3, g3, -1, "null light step")
    refused(RGBA, None, light_of(capi, to_transfer=13), tone(8), alpha_of(capi, STRAIGHT), d, g, -2, "four-channel")
    refused(RGBA, None, light_of(capi, to_transfer=11), None, alpha_of(capi, STRAIGHT), d, g, -2, "transfer")
    refused(RGBA, None, light_of(capi, gain=0.0), None, alpha_of(capi, MATTE), d3, g3, -1, "gain")
    du8, gu8 = fresh(RGB, HWC, U8, 96, 64)
    refused(RGBA, None, light_of(capi), None, alpha_of(capi, MATTE), du8, gu8, -1, "float dtype")
    refused(RGBA, None, light_of(capi, to_transfer=13), tone(0, 0.0), alpha_of(capi, MATTE), du8, gu8, -1, "unit_nits")  # (sRGB does not say what 1.0 stands for: behind the decode)
    refused(RGBA, ((90, 60, 30, 40), (16, 16), TRIANGLE), None, None, alpha_of(capi, STRAIGHT), d, g, -1, "not inside")
    refused(RGBA, (None, (96, 64), 5), None, None, alpha_of(capi, STRAIGHT), d, g, -1, "filter")
    dm, gm = fresh(RGB, HWC, U8, 96, 64, shrink=1)  # a matte's destination is sized as the three-channel sibling's
    refused(RGBA, None, None, None, alpha_of(capi, MATTE), dm, gm, -1, "len")
    d4, g4 = fresh(RGBA, HWC, U8, 96, 64, shrink=1)
    refused(RGBA, None, None, None, alpha_of(capi, PREMULTIPLIED), d4, g4, -1, "len")
    dv4, gv4 = fresh(RGBA, HWC, U8, 40, 30, shrink=1)
    refused(RGBA, (None, (40, 30), CUBIC), None, None, alpha_of(capi, STRAIGHT), dv4, gv4, -1, "len")
    du16, gu16 = fresh(RRGGBB_LE, HWC, U16, 96, 64)  # the 8-bit sibling takes no 16-bit words
    refused(RGBA, None, None, None, alpha_of(capi, MATTE), du16, gu16, -1, "dtype")
    # hm_alpha_to_tensor: the same refusals on pixels that are on the device already
    keep, ptr, stride = upload(np.ascontiguousarray(px))
    for al, word in ((alpha_of(capi, 9), "mode"), (alpha_of(capi, MATTE, (0, 0, 999)), "peak")):
        rc, msg = to_tensor(capi, L, RGBA, 8, 96, 64, ptr, stride, None, None, None, al, d)
        assert rc == -1 and word in msg and (g.host() == 0xA5).all(), msg
    rc, msg = to_tensor(capi, L, RRGGBBAA_LE, 12, 48, 64, ptr, stride, None, None, None, alpha_of(capi, MATTE, (0, 0, 4096)), d16)  # (known at once: bits is an argument)
    assert rc == -1 and "peak" in msg and (g16.host() == 0xA5).all(), msg
    del keep
    # ... and the library still decodes after all of that
    d, g, row, plane = base.make_dest(capi, L, RGBA, HWC, U8, 96, 64, ONE, ZERO, 0, 0)
    rc, msg, _ = alpha_to_device(capi, L, data, RGBA, None, None, None, alpha_of(capi, STRAIGHT), d)
    assert rc == 0, msg
    same(g.host(), dv.place(px, HWC, U8, row, plane, g.size, g.start), g.start, "a decode after the refusals")


def test_alpha_kernels_use_no_scratch(pkg):
    """every instance of the alpha kernels as the loaded code object has it (test hook hm_debug_kernel_regs, code 11): no scratch"""
    pkg.lib()  # (torch's HIP runtime first)
    T = C.CDLL(pkg.capi.TEST_LIB_PATH)
    T.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    n = 0
    while T.hm_debug_kernel_regs(11, n, 0, 0, C.byref(out)) == 0:
        assert out[1] == 0 and 0 < out[0] <= 128, (n, out[0], out[1])
        n += 1
    # 92 pointwise (sample width x dtype x channels written x layout x store width x with / without a light step, less the premultiplied
    # integers beside a light step, plus the 8-bit finish), 23 nearest, 8 horizontal, 32 vertical
    assert n == 155
