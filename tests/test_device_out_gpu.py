"""GPU: device-resident output (hm_decode_item_to_device, hm_decode_sequence_to_device, hm_pipeline_submit_to_device and the
Python decode_to_tensor / decode_batch_to_tensor).  Everything is bit-exact: the reference of every case is the same item decoded
by hm_decode_item to host memory (which the other GPU tests hold to the reference decoder); floats are restated in float32 numpy,
multiply and add rounded separately.  Every destination sits between two guard regions in a buffer pre-filled with 0xA5, and the
WHOLE buffer is compared with its expected image: the pixels, and 0xA5 in the guards, the pitch padding and - after a refused
call - everywhere."""
import ctypes as C

import numpy as np
import pytest

import heifwriter
import moovwriter
import pipeline
import synthutil

pytestmark = pytest.mark.gpu
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 13, 14, 15
OBPP = {RGB: 3, RGBA: 4, RRGGBB_BE: 6, RRGGBBAA_BE: 8, RRGGBB_LE: 6, RRGGBBAA_LE: 8}
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
ELEM = {U8: 1, U16: 2, F16: 2, F32: 4}
GUARD = 512
ALPHA_URN = "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"
# ImageNet statistics on samples of `peak`: (v / peak - mean) / std as v * scale + bias - values near zero around the mean
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


def imagenet(peak):
    return [1.0 / (peak * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)]


def _clap(cw, ch, dx2=0, dy2=0):
    return ("clap", (cw, 1, ch, 1, dx2, 2, dy2, 2))


# name -> (host threads, formats to decode to); the files themselves: the `inputs` fixture
PLAN = {"single_full_range": (2, (RGB, RGBA)), "single_limited_range": (2, (RGB,)),
        # four tile rows, two parsing threads: hm_decode_item takes the grid slab by slab; with sixteen threads as one batch
        "grid_4_rows_slabs": (2, (RGB, RGBA)), "grid_4_rows_one_batch": (16, (RGB,)), "grid_cropped": (2, (RGB, RRGGBB_LE)),
        "alpha_aux": (2, (RGBA,)), "ten_bit": (2, (RRGGBB_LE, RRGGBB_BE, RRGGBBAA_LE)), "irot_clap_odd_width": (2, (RGB, RRGGBBAA_LE))}
CASES = [(n, fmt) for n in sorted(PLAN) for fmt in PLAN[n][1]]


@pytest.fixture(scope="module")
def inputs():
    """name -> (file bytes, host threads, formats to decode to)"""
    files = {}
    full = synthutil.picture(42000, width=200, height=136, qp=30, vui=1, full_range=1, matrix=6)
    limited = synthutil.picture(42001, width=200, height=136, qp=30, vui=1, full_range=0, matrix=1, primaries=1)
    files["single_full_range"] = heifwriter.write_heic([full], (200, 136))
    files["single_limited_range"] = heifwriter.write_heic([limited], (200, 136))
    tiles = [synthutil.picture(42100 + t, width=64, height=64) for t in range(8)]
    files["grid_4_rows_slabs"] = heifwriter.write_heic(tiles, (64, 64), grid=(4, 2, 128, 256))
    files["grid_4_rows_one_batch"] = heifwriter.write_heic(tiles, (64, 64), grid=(4, 2, 128, 256))
    files["grid_cropped"] = heifwriter.write_heic(tiles[:6], (64, 64), grid=(3, 2, 117, 171))
    alpha = synthutil.picture(42201, width=48, height=32)
    main = synthutil.picture(42200, width=96, height=64, vui=1, full_range=1, matrix=6)
    files["alpha_aux"] = heifwriter.write_heic([main], (96, 64), aux=[(alpha, (48, 32), ALPHA_URN)])
    hdr = synthutil.picture(42300, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)
    files["ten_bit"] = heifwriter.write_heic([hdr], (160, 96), bit_depth=10)
    files["irot_clap_odd_width"] = heifwriter.write_heic([full], (200, 136), transforms=[_clap(121, 77, 7, -5), ("irot", 1)])
    assert sorted(files) == sorted(PLAN)
    return {n: (files[n],) + PLAN[n] for n in PLAN}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def host_rows(hm, data, fmt, threads, item=0):
    """hm_decode_item to host memory: the image's rows (h x w * obpp bytes), w, h"""
    f = pipeline.HeifFile(hm, data)
    try:
        planes, meta = f.decode(item or f.primary(), fmt, threads=threads)
    finally:
        f.close()
    w, h = meta["width"], meta["height"]
    return np.ascontiguousarray(planes[0][:h, :w * OBPP[fmt]]), w, h


def variant_pitches(fmt, layout, dtype, w, h, pad):
    c = 3 if OBPP[fmt] in (3, 6) else 4
    tight = w * ELEM[dtype] * (c if layout == HWC else 1)
    if not pad:
        return 0, 0, tight, tight * h
    # pad 1: 21 elements more (21, 42 or 84 bytes: a row that began 16-byte aligned is followed by one that does not, so no
    # 16-byte store is possible); pad 2: 64 bytes more (rows stay aligned where the tight row is: 16-byte stores beside padding)
    row = tight + (21 * ELEM[dtype] if pad == 1 else 64)
    return row, row * (h + 3), row, row * (h + 3)


def expected_image(rows, fmt, layout, dtype, w, h, scale, bias, row, plane, size, start):
    """the whole guarded buffer as it must look after the decode"""
    c = 3 if OBPP[fmt] in (3, 6) else 4
    buf = np.full(size, 0xA5, np.uint8)
    if layout == HWC and dtype in (U8, U16):  # the bytes of plane[0]
        view = np.lib.stride_tricks.as_strided(buf[start:], shape=(h, w * OBPP[fmt]), strides=(row, 1))
        view[...] = rows
        return buf
    vals = rows.reshape(h, w, c) if OBPP[fmt] <= 4 else rows.view("<u2").reshape(h, w, c)
    if dtype in (F16, F32):
        v = vals.astype(np.float32) * np.asarray(scale[:c], np.float32) + np.asarray(bias[:c], np.float32)
        assert v.dtype == np.float32
        if dtype == F16:
            v = v.astype(np.float16)
    else:
        v = vals.astype(np.uint8 if dtype == U8 else np.uint16)
    e = ELEM[dtype]
    typed = buf[start:start + (size - start) // e * e].view(v.dtype)
    if layout == CHW:
        view = np.lib.stride_tricks.as_strided(typed, shape=(c, h, w), strides=(plane, row, e))
        view[...] = v.transpose(2, 0, 1)
    else:
        view = np.lib.stride_tricks.as_strided(typed, shape=(h, w, c), strides=(row, c * e, e))
        view[...] = v
    return buf


class Guarded:
    """`need` bytes of device memory between two guards, everything pre-filled with 0xA5"""

    def __init__(self, need, offset=0):
        import torch
        self.size = GUARD + offset + need + GUARD
        self.t = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda")
        self.start = GUARD + offset
        self.ptr = self.t.data_ptr() + self.start
        assert self.t.data_ptr() % 256 == 0
        torch.cuda.synchronize()

    def host(self):
        return self.t.cpu().numpy()


def make_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, pad, offset_elems, shrink=0):
    row_arg, plane_arg, row, plane = variant_pitches(fmt, layout, dtype, w, h, pad)
    d = capi.DeviceDest()
    d.layout, d.dtype, d.row_pitch, d.plane_pitch = layout, dtype, row_arg, plane_arg
    for k in range(4):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    need = L.hm_device_dest_bytes(fmt, w, h, C.byref(d))
    assert need > 0, L.hm_last_error().decode()
    g = Guarded(need, offset_elems * ELEM[dtype])
    d.ptr, d.len = g.ptr, need - shrink
    return d, g, row, plane


def to_device(capi, L, data, fmt, d, threads, item=0, ext_dst=None):
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        prm = capi.DecodeParams(fmt, threads, 0, 0, None, ext_dst, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = L.hm_decode_item_to_device(h, item or L.hm_file_primary_item(h), C.byref(prm), C.byref(d), C.byref(out))
        msg = L.hm_last_error().decode()
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, msg, out
    finally:
        L.hm_file_close(h)


def variants(fmt):
    """(layout, dtype, scale, bias, pitches: 0 tight / 1 padded off 16-byte alignment / 2 padded by 64 bytes, ptr offset in elements)"""
    wide = OBPP[fmt] >= 6
    integer = U16 if wide else U8
    sc, bi = imagenet(65535.0 if wide else 255.0)
    one, zero = [1.0] * 4, [0.0] * 4
    v = [(HWC, integer, one, zero, False, 0), (HWC, integer, one, zero, True, 0), (HWC, integer, one, zero, True, 1)]
    if fmt not in (RRGGBB_BE, RRGGBBAA_BE):
        v += [(CHW, integer, one, zero, False, 0), (CHW, integer, one, zero, True, 1),
              (CHW, F32, sc, bi, False, 0), (CHW, F32, sc, bi, True, 0), (CHW, F32, sc, bi, 2, 0), (CHW, F32, sc, bi, False, 1),
              (CHW, integer, one, zero, 2, 0), (HWC, F16, sc, bi, 2, 0),
              (HWC, F32, sc, bi, False, 0), (HWC, F32, one, zero, True, 1),
              (CHW, F16, sc, bi, False, 0), (CHW, F16, sc, bi, True, 1), (HWC, F16, sc, bi, False, 0),
              # a scale small enough for float16 subnormals (below 2 ** -14): 8-bit samples times 2 ** -20, 16-bit times 2 ** -28
              (CHW, F16, [2.0 ** (-28 if wide else -20)] * 4, zero, False, 0)]
    return v


@pytest.mark.parametrize("name,fmt", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_item_to_device_equals_host_decode(hm, capi, L, inputs, name, fmt):
    data, threads, _ = inputs[name]
    rows, w, h = host_rows(hm, data, fmt, threads)
    if name == "irot_clap_odd_width":
        assert w % 2 == 1
    seen_subnormal = False
    for layout, dtype, scale, bias, pad, off in variants(fmt):
        what = f"{name} fmt {fmt} layout {layout} dtype {dtype} pad {pad} offset {off}"
        d, g, row, plane = make_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, pad, off)
        rc, msg, out = to_device(capi, L, data, fmt, d, threads)
        assert rc == 0, f"{what}: {msg}"
        assert (out.width, out.height, out.used_ext_dst, out.stride[0], out.out_format) == (w, h, 1, row, fmt), what
        exp = expected_image(rows, fmt, layout, dtype, w, h, scale, bias, row, plane, g.size, g.start)
        got = g.host()
        assert got.shape == exp.shape
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0] - g.start} from the destination's start "
                                 f"(got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})")
        if dtype == F16 and scale[0] < 1e-5:
            f16 = exp[g.start:g.start + w * h * 2].view(np.float16)
            seen_subnormal = bool(((f16 != 0) & (np.abs(f16) < 2.0 ** -14)).any())
    if fmt not in (RRGGBB_BE, RRGGBBAA_BE):
        assert seen_subnormal, "the small-scale case produced no float16 subnormal"


@pytest.mark.parametrize("fmt,w,h", [(RGB, 4032, 37), (RGB, 1001, 9), (RGBA, 130, 7), (RRGGBB_LE, 258, 5), (RRGGBBAA_LE, 67, 3)])
def test_to_tensor_on_random_pixels(capi, L, fmt, w, h):
    """hm_to_tensor alone: every sample value and wide rows (several blocks per row, a ragged last pixel group)"""
    import torch
    rng = np.random.default_rng(fmt * 1000 + w)
    src_stride = (w * OBPP[fmt] + 63) // 64 * 64 + 64
    src = rng.integers(0, 256, (h, src_stride), dtype=np.uint8)
    rows = np.ascontiguousarray(src[:, :w * OBPP[fmt]])
    dsrc = torch.from_numpy(src).cuda()
    for layout, dtype, scale, bias, pad, off in variants(fmt):
        d, g, row, plane = make_dest(capi, L, fmt, layout, dtype, w, h, scale, bias, pad, off)
        rc = L.hm_to_tensor(fmt, w, h, dsrc.data_ptr(), src_stride, C.byref(d), None)
        assert rc == 0, L.hm_last_error().decode()
        torch.cuda.synchronize()
        exp = expected_image(rows, fmt, layout, dtype, w, h, scale, bias, row, plane, g.size, g.start)
        assert np.array_equal(g.host(), exp), f"fmt {fmt} layout {layout} dtype {dtype} pad {pad} offset {off}"


def _keep_the_default_stream_busy():
    """queues some 15 ms of work on the default stream (60 passes over 512 MB) and returns its tensor, for more of the same"""
    import torch
    x = torch.ones(128 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(60):
        x.mul_(1.0)
    return x


@pytest.mark.parametrize("name,fmt", [("grid_4_rows_slabs", RGB), ("grid_4_rows_slabs", RRGGBBAA_LE), ("grid_4_rows_one_batch", RGB)])
def test_destination_with_work_pending_on_the_default_stream(hm, pkg, capi, L, inputs, name, fmt):
    """The caller still writes the destination on the default stream (params->stream NULL) when the decode is called: the
    decode's writes come behind that work, also where a grid's slabs run on streams of their own.  A decode that does not wait
    finishes long before the pending fill does, and the fill then wipes its pixels.  (RRGGBBAA: the colour step is a kernel of
    its own there and nothing on the way happens to wait for the default stream.)"""
    import torch
    data, threads, _ = inputs[name]
    rows, w, h = host_rows(hm, data, fmt, threads)
    wide = OBPP[fmt] >= 6
    c = 3 if OBPP[fmt] in (3, 6) else 4
    sc, bi = imagenet(65535.0 if wide else 255.0)
    # the C entry point, CHW float32 (k_to_tensor)
    d, g, row, plane = make_dest(capi, L, fmt, CHW, F32, w, h, sc, bi, True, 0)
    busy = _keep_the_default_stream_busy()
    g.t.fill_(0x11)
    g.t.fill_(0xA5)
    behind = torch.cuda.Event()
    behind.record()
    assert not behind.query(), "the pending work was over before the decode was called: the test shows nothing"
    rc, msg, _ = to_device(capi, L, data, fmt, d, threads)
    assert rc == 0, msg
    assert np.array_equal(g.host(), expected_image(rows, fmt, CHW, F32, w, h, sc, bi, row, plane, g.size, g.start))
    # decode_to_tensor, H x W x C integers (the 2-D device copy) into a tensor that is still being filled
    out = torch.empty((h, w, c), dtype=torch.uint16 if wide else torch.uint8, device="cuda")
    for _ in range(60):
        busy.mul_(1.0)
    out.view(torch.uint8).fill_(0x11)
    behind.record()
    assert not behind.query(), "the pending work was over before the decode was called: the test shows nothing"
    assert pkg.decode_to_tensor(data, out_format={RGB: "rgb", RRGGBBAA_LE: "rrggbbaa_le"}[fmt], layout="hwc", out=out, host_threads=threads) is out
    exp = rows.view("<u2").reshape(h, w, c) if wide else rows.reshape(h, w, c)
    assert np.array_equal(out.cpu().numpy(), exp)


def test_imagenet_values_land_near_zero(hm, inputs):
    """the float cases are not all far from zero: some samples sit within one step of a channel mean"""
    data, threads, _ = inputs["single_full_range"]
    rows, w, h = host_rows(hm, data, RGB, threads)
    sc, bi = imagenet(255.0)
    v = rows.reshape(h, w, 3).astype(np.float32) * np.asarray(sc[:3], np.float32) + np.asarray(bi[:3], np.float32)
    assert (np.abs(v) < 0.02).any()


def test_refusals_leave_the_destination_untouched(hm, capi, L, inputs):
    import torch
    data, threads, _ = inputs["single_full_range"]
    hdr = inputs["ten_bit"][0]
    rows, w, h = host_rows(hm, data, RGB, threads)
    one, zero = [1.0] * 4, [0.0] * 4

    def refused(file, fmt, d, g, status, word, ext_dst=None):
        rc, msg, _ = to_device(capi, L, file, fmt, d, threads, ext_dst=ext_dst)
        assert rc == status and word in msg, (rc, msg)
        if g is not None:
            torch.cuda.synchronize()
            assert (g.host() == 0xA5).all(), f"a refused call ({msg}) wrote to the destination"

    # short len, both kinds of write
    for layout, dtype in ((HWC, U8), (CHW, F32), (CHW, U8)):
        d, g, _, _ = make_dest(capi, L, RGB, layout, dtype, w, h, one, zero, False, 0, shrink=1)
        refused(data, RGB, d, g, -1, "len")
    # dtype mismatch
    d, g, _, _ = make_dest(capi, L, RGB, CHW, F32, w, h, one, zero, False, 0)
    d.dtype = U16
    refused(data, RGB, d, g, -1, "dtype")
    # _BE with CHW / float
    d, g, _, _ = make_dest(capi, L, RRGGBB_LE, CHW, U16, 160, 96, one, zero, False, 0)
    refused(hdr, RRGGBB_BE, d, g, -1, "_LE")
    d.dtype = F32
    refused(hdr, RRGGBB_BE, d, g, -1, "_LE")
    # planar YCbCr / as-decoded targets
    d, g, _, _ = make_dest(capi, L, RGB, HWC, U8, w, h, one, zero, False, 0)
    for fmt in (0, 0x101, 0x103):
        refused(data, fmt, d, g, -2, "not supported with a device destination")
    # ext_dst together with a destination
    host = np.full(w * h * 3, 0x5A, np.uint8)
    refused(data, RGB, d, g, -1, "ext_dst", ext_dst=host.ctypes.data)
    assert (host == 0x5A).all()
    # pitches below tight / not multiples of the element size, a misaligned pointer
    d2, g2, _, _ = make_dest(capi, L, RGB, CHW, F32, w, h, one, zero, False, 0)
    d2.row_pitch = w * 4 - 4
    refused(data, RGB, d2, g2, -1, "row_pitch")
    d2.row_pitch = w * 4 + 2
    refused(data, RGB, d2, g2, -1, "multiple of the element size")
    d2.row_pitch = 0
    d2.ptr += 2
    refused(data, RGB, d2, g2, -1, "ptr is not a multiple")
    # host memory: pageable and pinned
    d3, _, _, _ = make_dest(capi, L, RGB, HWC, U8, w, h, one, zero, False, 0)
    d3.ptr = host.ctypes.data
    refused(data, RGB, d3, None, -1, "ptr")
    pinned = torch.full((w * h * 3,), 0x5A, dtype=torch.uint8).pin_memory()
    d3.ptr = pinned.data_ptr()
    refused(data, RGB, d3, None, -1, "ptr")
    assert (host == 0x5A).all() and bool((pinned == 0x5A).all())
    # ... and the library still decodes after all of that
    d, g, row, plane = make_dest(capi, L, RGB, HWC, U8, w, h, one, zero, False, 0)
    assert to_device(capi, L, data, RGB, d, threads)[0] == 0
    assert np.array_equal(g.host(), expected_image(rows, RGB, HWC, U8, w, h, one, zero, row, plane, g.size, g.start))


def _movie(n=5):
    frames = [synthutil.picture(43000 + i, width=200, height=136, qp=30) for i in range(n)]
    return moovwriter.write_movie(frames, (200, 136)), 200, 136


@pytest.mark.parametrize("fmt,layout,dtype", [(RGB, CHW, F32), (RGB, HWC, U8), (RGBA, CHW, F16), (RRGGBB_LE, CHW, U16)])
def test_sequence_to_device_equals_per_frame_host_decodes(hm, capi, L, fmt, layout, dtype):
    """count frames into ONE N x C x H x W (N x H x W x C) allocation, passed as count destinations at offsets"""
    buf, w, h = _movie(5)
    n = 5
    sc, bi = imagenet(65535.0 if OBPP[fmt] >= 6 else 255.0) if dtype in (F16, F32) else ([1.0] * 4, [0.0] * 4)
    frames = [host_rows(hm, buf, fmt, 4, item=k)[0] for k in range(1, n + 1)]
    d0 = capi.DeviceDest()
    d0.layout, d0.dtype = layout, dtype
    per = L.hm_device_dest_bytes(fmt, w, h, C.byref(d0))
    g = Guarded(per * n)
    dests = (capi.DeviceDest * n)()
    for k in range(n):
        dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = g.ptr + k * per, per, layout, dtype
        for c in range(4):
            dests[k].scale[c], dests[k].bias[c] = sc[c], bi[c]
    fh = C.c_void_p()
    assert L.hm_file_open(buf, len(buf), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(fmt, 4, 0, 0, None, None, 0, 0, 0, 0)
        out = (capi.Decoded * n)()
        failed = C.c_int32(-2)
        rc = L.hm_decode_sequence_to_device(fh, 1, n, C.byref(prm), dests, out, C.byref(failed))
        assert rc == 0 and failed.value == -1, L.hm_last_error().decode()
        for k in range(n):
            assert (out[k].width, out[k].height, out[k].used_ext_dst) == (w, h, 1) and not out[k].plane[0]
        # a destination that is too short fails the call before anything is written
        g2 = Guarded(per * n)
        for k in range(n):
            dests[k].ptr = g2.ptr + k * per
        dests[n - 1].len = per - 1
        rc = L.hm_decode_sequence_to_device(fh, 1, n, C.byref(prm), dests, out, C.byref(failed))
        assert rc == -1 and failed.value == n - 1 and "len" in L.hm_last_error().decode()
        assert (g2.host() == 0xA5).all()
    finally:
        L.hm_file_close(fh)
    exp = np.full(g.size, 0xA5, np.uint8)
    tight_row = w * ELEM[dtype] * (1 if layout == CHW else OBPP[fmt] // (2 if OBPP[fmt] >= 6 else 1))
    for k in range(n):
        one = expected_image(frames[k], fmt, layout, dtype, w, h, sc, bi, tight_row, tight_row * h, per, 0)
        exp[g.start + k * per:g.start + (k + 1) * per] = one
    assert np.array_equal(g.host(), exp)


def _many_files():
    files = []
    for i in range(18):
        kind = i % 3
        if kind == 0:
            tiles = [synthutil.picture(44000 + 10 * i + t, width=64, height=64) for t in range(6)]
            files.append(heifwriter.write_heic(tiles, (64, 64), grid=(2, 3, 180, 120)))
        elif kind == 1:
            files.append(heifwriter.write_heic([synthutil.picture(44000 + 10 * i, width=200, height=136, slices=80, dependent=300)], (200, 136)))
        else:
            tiles = [synthutil.picture(44000 + 10 * i + t, width=128, height=64, vui=0) for t in range(4)]
            files.append(heifwriter.write_heic(tiles, (128, 64), grid=(2, 2, 250, 128)))
    return files


@pytest.mark.parametrize("layout,dtype", [(CHW, F32), (HWC, U8)])
def test_pipeline_to_device_equals_host_decodes_in_submission_order(hm, capi, L, layout, dtype):
    files = _many_files()
    assert len(files) >= 16
    sc, bi = imagenet(255.0) if dtype == F32 else ([1.0] * 4, [0.0] * 4)
    host = [host_rows(hm, data, RGB, 2) for data in files]
    cfg = capi.PipelineConfig(4, 4, RGB, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    dests, order, full_seen = [], [], 0
    try:
        def take():
            r = capi.PipelineResult()
            assert L.hm_pipeline_next(pipe, C.byref(r)) == 0
            assert r.status == 0, L.hm_last_error().decode()
            rows, w, h = host[r.tag]
            assert (r.image.width, r.image.height, r.image.used_ext_dst) == (w, h, 1) and not r.image.plane[0]
            # (the pixels are complete when the result is handed out: compared right here, before the release)
            d, g, row, plane = dests[r.tag]
            assert np.array_equal(g.host(), expected_image(rows, RGB, layout, dtype, w, h, sc, bi, row, plane, g.size, g.start)), f"file {r.tag}"
            order.append(r.tag)
            L.hm_pipeline_release(pipe, C.byref(r))
        for k, data in enumerate(files):
            _, w, h = host[k]
            dests.append(make_dest(capi, L, RGB, layout, dtype, w, h, sc, bi, k % 2 == 1, 0))
            while True:
                rc = L.hm_pipeline_submit_to_device(pipe, data, len(data), 0, k, C.byref(dests[k][0]))
                assert rc >= 0, L.hm_last_error().decode()
                if rc == 0:
                    break
                full_seen += 1
                take()
        # a destination that is refused fails the submit: nothing queued, nothing written
        d, g, _, _ = make_dest(capi, L, RGB, layout, dtype, host[0][1], host[0][2], sc, bi, False, 0, shrink=1)
        while L.hm_pipeline_pending(pipe) >= 4:
            take()
        assert L.hm_pipeline_submit_to_device(pipe, files[0], len(files[0]), 0, 99, C.byref(d)) == -1
        assert (g.host() == 0xA5).all()
        while L.hm_pipeline_pending(pipe):
            take()
    finally:
        L.hm_pipeline_destroy(pipe)
    assert order == list(range(len(files))) and full_seen > 0


def test_python_decode_to_tensor(hm, pkg, capi, L, inputs):
    import torch
    data, threads, _ = inputs["grid_cropped"]
    rows, w, h = host_rows(hm, data, RGB, threads)
    sc, bi = imagenet(255.0)
    # defaults: C x H x W float32, scale 1, bias 0
    t = pkg.decode_to_tensor(data)
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (3, h, w)
    assert np.array_equal(t.cpu().numpy(), rows.reshape(h, w, 3).transpose(2, 0, 1).astype(np.float32))
    # equal to the ctypes-level call, bit for bit
    d, g, row, plane = make_dest(capi, L, RGB, CHW, F16, w, h, sc, bi, False, 0)
    assert to_device(capi, L, data, RGB, d, threads)[0] == 0
    low = g.host()[g.start:g.start + 3 * h * w * 2].view(np.float16).reshape(3, h, w)
    t = pkg.decode_to_tensor(data, out_format="rgb", layout="chw", dtype=torch.float16, scale=sc[:3], bias=bi[:3], host_threads=threads)
    assert np.array_equal(t.cpu().numpy().view(np.uint16), low.view(np.uint16))
    t = pkg.decode_to_tensor(data, layout="hwc", dtype=torch.uint8)
    assert tuple(t.shape) == (h, w, 3) and np.array_equal(t.cpu().numpy(), rows.reshape(h, w, 3))
    hdr = inputs["ten_bit"][0]
    rows16, w16, h16 = host_rows(hm, hdr, RRGGBBAA_LE, 2)
    t = pkg.decode_to_tensor(hdr, out_format="rrggbbaa_le", dtype=torch.uint16)
    assert np.array_equal(t.cpu().numpy(), rows16.view("<u2").reshape(h16, w16, 4).transpose(2, 0, 1))
    # out= is honoured, its row stride too: the columns behind the image stay as they were
    big = torch.full((3, h + 2, w + 9), -7.0, dtype=torch.float32, device="cuda")
    view = big[:, 1:h + 1, :w]
    res = pkg.decode_to_tensor(data, out=view, scale=sc, bias=bi)
    assert res is view
    exp = rows.reshape(h, w, 3).astype(np.float32) * np.asarray(sc[:3], np.float32) + np.asarray(bi[:3], np.float32)
    got = big.cpu().numpy()
    assert np.array_equal(got[:, 1:h + 1, :w], exp.transpose(2, 0, 1))
    assert (got[:, :, w:] == -7.0).all() and (got[:, 0] == -7.0).all() and (got[:, h + 1] == -7.0).all()
    # a size mismatch raises, and so does a layout the strides cannot express
    with pytest.raises(ValueError, match="shape"):
        pkg.decode_to_tensor(data, out=torch.empty((3, h, w + 1), device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        pkg.decode_to_tensor(data, out=torch.empty((h, w, 3), device="cuda").permute(2, 0, 1))
    with pytest.raises(capi.HmError, match="dtype"):
        pkg.decode_to_tensor(data, dtype=torch.uint16)


def test_python_decode_batch_to_tensor(hm, pkg, inputs, tmp_path):
    import torch
    files = [heifwriter.write_heic([synthutil.picture(45000 + 10 * i + t, width=64, height=64) for t in range(6)], (64, 64), grid=(2, 3, 180, 120))
             for i in range(7)]
    sc, bi = imagenet(255.0)
    host = [host_rows(hm, data, RGB, 2)[0].reshape(120, 180, 3) for data in files]
    t = pkg.decode_batch_to_tensor(files, dtype=torch.float32, scale=sc, bias=bi, max_in_flight=3)
    assert tuple(t.shape) == (7, 3, 120, 180)
    got = t.cpu().numpy()
    for k in range(7):
        exp = host[k].astype(np.float32) * np.asarray(sc[:3], np.float32) + np.asarray(bi[:3], np.float32)
        assert np.array_equal(got[k], exp.transpose(2, 0, 1)), f"image {k}"
        single = pkg.decode_to_tensor(files[k], scale=sc, bias=bi)
        assert torch.equal(single, t[k])
    # N x H x W x C uint8 into a tensor of the caller, files given as paths
    paths = []
    for k, data in enumerate(files[:3]):
        paths.append(tmp_path / f"img{k}.heic")
        paths[-1].write_bytes(data)
    out = torch.zeros((3, 120, 180, 3), dtype=torch.uint8, device="cuda")
    assert pkg.decode_batch_to_tensor(paths, layout="hwc", out=out) is out
    assert np.array_equal(out.cpu().numpy(), np.stack(host[:3]))
    # a file of another size is refused by name
    odd = tmp_path / "other_size.heic"
    odd.write_bytes(inputs["single_full_range"][0])
    with pytest.raises(ValueError, match="other_size.heic"):
        pkg.decode_batch_to_tensor(paths + [odd])
    with pytest.raises(ValueError, match=r"files\[1\]"):
        pkg.decode_batch_to_tensor([files[0], inputs["single_full_range"][0]])
