"""GPU: image sequences (the fork's movie mode).  Every frame through hm_decode_item against libde265 + the oracle colour path;
hm_decode_sequence (all frames in one device batch) against the per-frame decodes; a damaged frame; the facade driven like the
fork's Android caller; the decoder plugin given a frame's byte string."""
import ctypes as C
import os

import numpy as np
import pytest

import moovwriter
import orc
import pipeline
import pluginapi
import synthutil
from test_sequence import p_slice

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BPP = {10: 3, 11: 4, 14: 6}


class FrameDest(C.Structure):
    _fields_ = [("ext_dst", C.c_void_p), ("ext_dst_len", C.c_uint32), ("ext_dst_stride", C.c_uint32)]


def basketball():
    return [open(os.path.join(HERE, "data", f"basketball_1080p_qp{q}.hevc"), "rb").read() for q in (1, 25, 32)]


def synth_frames(n, seed, **kw):
    return [synthutil.picture(seed + i, **kw) for i in range(n)]


def movies():
    """(name, file bytes, width, height): 8-bit 4:2:0 real 1080p content, synthesised 8-bit 4:2:0 with per-frame parameter sets
    and a short hvcC, a 10-bit 4:2:0 class"""
    bb = basketball()
    out = [("basketball_1080p", moovwriter.write_movie(bb, (1920, 1080)), 1920, 1080)]
    s8 = synth_frames(6, 31000, width=200, height=136, qp=30)
    out.append(("synth8_short_hvcc", moovwriter.write_movie(s8, (200, 136), hvcc_units=3, params_in="hvcc"), 200, 136))
    s10 = synth_frames(4, 32000, width=160, height=96, bit_depth=10, full_range=0, matrix=1, primaries=1)
    out.append(("synth10", moovwriter.write_movie(s10, (160, 96), bit_depth=10, params_in="sample"), 160, 96))
    return out


MOVIES = {m[0]: m for m in movies()} if os.path.exists(os.path.join(HERE, "data")) else {}


def bind_sequence(hm):
    pipeline.bind(hm)
    hm.hm_decode_sequence.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(pipeline.DecodeParams), C.POINTER(FrameDest),
                                      C.POINTER(pipeline.Decoded), C.POINTER(C.c_int32)]
    return hm


def take(hm, d, fmt):
    """the pixels of one hm_decoded (rows x stride arrays) + its fields; frees it"""
    planes = []
    for c in range(1 if fmt else 3):
        if d.plane[c]:
            planes.append(np.ctypeslib.as_array(d.plane[c], shape=(d.plane_height[c], d.stride[c])).copy())
    meta = {k: getattr(d, k) for k in "width height bit_depth chroma out_format has_nclx primaries transfer matrix full_range used_ext_dst warnings".split()}
    meta["stride"] = list(d.stride)
    hm.hm_decoded_free(C.byref(d))
    return planes, meta


def same_pixels(r1, r2, what=""):
    """two (planes, meta) results are the same image: equal fields, and equal planes - interleaved output up to the row width (the
    bytes behind a row are padding neither path writes), native planes whole (both paths clear them before the decode)"""
    (p1, m1), (p2, m2) = r1, r2
    assert m1 == m2, what
    assert len(p1) == len(p2), what
    for a, b in zip(p1, p2):
        if m1["out_format"]:
            row = m1["width"] * BPP[m1["out_format"]]
            a, b = a[:m1["height"], :row], b[:m1["height"], :row]
        np.testing.assert_array_equal(a, b, err_msg=what)


def decode_sequence(hm, f, first, count, fmt, threads=1, dests=None, strict=0):
    bind_sequence(hm)
    prm = pipeline.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, strict, 0)
    out = (pipeline.Decoded * count)()
    failed = C.c_int32(-2)
    darr = None
    if dests is not None:
        darr = (FrameDest * count)(*[FrameDest(b.ctypes.data, b.size, st) for b, st in dests])
    rc = hm.hm_decode_sequence(f.h, first, count, C.byref(prm), darr, out, C.byref(failed))
    msg = hm.hm_last_error().decode()
    res = [take(hm, out[k], fmt) for k in range(count)] if rc == 0 else []
    if rc:
        assert all(not out[k].plane[0] for k in range(count))
    return rc, msg, failed.value, res


def decode_item(hm, f, iid, fmt, threads=1, ext=None, strict=0):
    pipeline.bind(hm)
    prm = pipeline.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, strict, 0)
    if ext is not None:
        prm.ext_dst, prm.ext_dst_len, prm.ext_dst_stride = ext[0].ctypes.data, ext[0].size, ext[1]
    d = pipeline.Decoded()
    rc = hm.hm_decode_item(f.h, iid, C.byref(prm), C.byref(d))
    msg = hm.hm_last_error().decode()
    if rc:
        return rc, msg, None
    return rc, msg, take(hm, d, fmt)


@pytest.mark.parametrize("fmt", [0, 10, 11, 14], ids=["ycbcr", "RGB24", "RGBA32", "RRGGBB_LE"])
@pytest.mark.parametrize("name", sorted(MOVIES))
def test_frames_bit_exact_to_reference(hm, name, fmt):
    """hm_decode_item on every frame == libde265 (oracle/_ref) on the frame's byte string + the oracle colour path"""
    _, buf, w, h = MOVIES[name]
    f = pipeline.HeifFile(hm, buf)
    try:
        n = moovwriter.fork_movie_info(buf)["frame_count"]
        for k in range(1, n + 1):
            data = f.hevc_data(k)
            assert data == moovwriter.fork_sample_bytes(buf, k)
            rc, msg, (planes, meta) = decode_item(hm, f, k, fmt, threads=4)
            assert rc == 0, msg
            assert (meta["width"], meta["height"]) == (w, h)
            decoder = "ref" if orc.have_ref() else "oracle"
            exp, stride, canv = pipeline.cpu_decode(hm, [data], w, h, w, h, 1, False, fmt or 10, decoder=decoder)
            if fmt:
                np.testing.assert_array_equal(planes[0][:h, :w * BPP[fmt]], exp[:h, :w * BPP[fmt]], err_msg=f"{name} frame {k}")
            else:
                bps = 2 if meta["bit_depth"] > 8 else 1
                for c, (pw, ph) in enumerate(((w, h), ((w + 1) // 2, (h + 1) // 2), ((w + 1) // 2, (h + 1) // 2))):
                    np.testing.assert_array_equal(planes[c][:ph, :pw * bps], canv[c][0][:ph, :pw * bps], err_msg=f"{name} frame {k} plane {c}")
    finally:
        f.close()


@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("fmt", [0, 10, 11, 14], ids=["ycbcr", "RGB24", "RGBA32", "RRGGBB_LE"])
@pytest.mark.parametrize("name", sorted(MOVIES))
def test_sequence_equals_per_frame(hm, name, fmt, threads):
    """hm_decode_sequence over all frames == hm_decode_item frame by frame, byte for byte, with pinned results and with caller
    buffers; and a sub-range"""
    _, buf, w, h = MOVIES[name]
    f = pipeline.HeifFile(hm, buf)
    try:
        n = moovwriter.fork_movie_info(buf)["frame_count"]
        single = []
        for k in range(1, n + 1):
            rc, msg, r = decode_item(hm, f, k, fmt, threads=threads)
            assert rc == 0, msg
            single.append(r)
        rc, msg, failed, seq = decode_sequence(hm, f, 1, n, fmt, threads=threads)
        assert rc == 0 and failed == -1, msg
        for k in range(n):
            same_pixels(single[k], seq[k], f"{name} frame {k + 1}")
        rc, msg, failed, part = decode_sequence(hm, f, 2, n - 1, fmt, threads=threads)
        assert rc == 0, msg
        for k in range(n - 1):
            same_pixels(single[k + 1], part[k], f"{name} frame {k + 2} of the sub-range")
        if fmt:  # caller buffers: one per frame, a stride wider than the row
            stride = w * BPP[fmt] + 64
            bufs = [np.full((h, stride), 0xA5, np.uint8) for _ in range(n)]
            rc, msg, failed, res = decode_sequence(hm, f, 1, n, fmt, threads=threads, dests=[(b, stride) for b in bufs])
            assert rc == 0, msg
            for k in range(n):
                assert res[k][1]["used_ext_dst"] == 1 and not res[k][0]
                np.testing.assert_array_equal(bufs[k][:, :w * BPP[fmt]], single[k][0][0][:h, :w * BPP[fmt]])
                assert (bufs[k][:, w * BPP[fmt]:] == 0xA5).all()
            # ... the same as hm_decode_item with ext_dst
            one = np.zeros((h, stride), np.uint8)
            assert decode_item(hm, f, n, fmt, ext=(one, stride))[0] == 0
            np.testing.assert_array_equal(one[:, :w * BPP[fmt]], bufs[n - 1][:, :w * BPP[fmt]])
    finally:
        f.close()


def test_mixed_classes_share_a_call(hm):
    """frames of different sizes and depths (the writer's hvc1 declares one depth; each sample carries its own SPS) decode in one
    call as they do alone: groups of one colour description each"""
    pics = synth_frames(2, 33000, width=128, height=64) + synth_frames(2, 33100, width=96, height=80, vui=0) + \
        synth_frames(1, 33200, width=64, height=64, chroma_format=0)
    buf = moovwriter.write_movie(pics, (128, 64), params_in="sample")
    f = pipeline.HeifFile(hm, buf)
    try:
        for fmt in (0, 10, 11):
            single = [decode_item(hm, f, k, fmt, threads=2)[2] for k in range(1, 6)]
            rc, msg, failed, seq = decode_sequence(hm, f, 1, 5, fmt, threads=2)
            assert rc == 0, msg
            for k in range(5):
                same_pixels(single[k], seq[k], f"format {fmt} frame {k + 1}")
    finally:
        f.close()


def test_damaged_frame_fails_like_alone(hm):
    """a frame that fails (a P slice; a sample past the end of the file) fails the whole call with the status and message of
    hm_decode_item on that frame; the index is reported; no caller buffer is written"""
    pics = synth_frames(4, 34000, width=128, height=96)
    cases = []
    bad = list(pics)
    bad[2] = p_slice(bad[2])
    cases.append((moovwriter.write_movie(bad, (128, 96)), 3))
    info = moovwriter.fork_movie_info(moovwriter.write_movie(pics, (128, 96)))
    cases.append((moovwriter.write_movie(pics, (128, 96), stsz_entries=info["sizes"][:3] + [info["sizes"][3] + 5000]), 4))
    for buf, bad_id in cases:
        f = pipeline.HeifFile(hm, buf)
        try:
            rc1, msg1, _ = decode_item(hm, f, bad_id, 11)
            assert rc1 < 0 and msg1
            bufs = [np.full((96, 128 * 4), 0x5A, np.uint8) for _ in range(4)]
            for dests in (None, [(b, 128 * 4) for b in bufs]):
                rc2, msg2, failed, res = decode_sequence(hm, f, 1, 4, 11, threads=4, dests=dests)
                assert (rc2, msg2, failed) == (rc1, msg1, bad_id - 1)
            assert all((b == 0x5A).all() for b in bufs)
            assert decode_sequence(hm, f, 1, bad_id - 1, 11)[0] == 0  # the frames in front of it are fine
        finally:
            f.close()


@pytest.fixture(scope="module")
def api(pkg):
    from test_sequence import ImageParameters, LibheifParameters
    a = pluginapi.load_api(pkg)
    E = pluginapi.Err
    a.heif_context_alloc.restype = C.c_void_p
    a.heif_context_free.argtypes = [C.c_void_p]
    a.heif_context_read_from_memory.restype = E
    a.heif_context_read_from_memory.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
    a.heif_context_get_number_of_top_level_images.argtypes = [C.c_void_p]
    a.heif_context_get_list_of_top_level_image_IDs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    a.heif_context_get_heif_params.restype = E
    a.heif_context_get_heif_params.argtypes = [C.c_void_p, C.POINTER(LibheifParameters)]
    a.heif_context_get_image_handle.restype = E
    a.heif_context_get_image_handle.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    a.heif_image_handle_release.argtypes = [C.c_void_p]
    a.heif_decoding_options_alloc.restype = C.c_void_p
    a.heif_decoding_options_free.argtypes = [C.c_void_p]
    a.heif_decoding_options_add_external_dest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    a.heif_decode_image.restype = E
    a.heif_decode_image.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    return a


def test_facade_like_the_android_caller(api, hm):
    """heif_jni.cpp:150-215, 518-528: heif_context_get_heif_params, the list of top-level IDs, then heif_decode_image of frame i
    into an RGBA ext_dst - equal to hm_decode_item's RGBA pixels"""
    from test_sequence import ImageParameters, LibheifParameters
    _, buf, w, h = MOVIES["synth8_short_hvcc"]
    ctx = api.heif_context_alloc()
    f = pipeline.HeifFile(hm, buf)
    try:
        assert api.heif_context_read_from_memory(ctx, buf, len(buf), None).code == 0
        n = api.heif_context_get_number_of_top_level_images(ctx)
        arr = (ImageParameters * n)()
        params = LibheifParameters(False, 0, 0, arr)
        e = api.heif_context_get_heif_params(ctx, C.byref(params))
        assert e.code == 0 and params.movie_flag and params.frame_count == n == 6 and params.movie_duration == 3000
        ids = (C.c_uint32 * n)()
        assert api.heif_context_get_list_of_top_level_image_IDs(ctx, ids, n) == n
        for i in range(n):
            hdl = C.c_void_p()
            assert api.heif_context_get_image_handle(ctx, ids[i], C.byref(hdl)).code == 0
            stride = arr[i].img_width * 4
            ext = np.zeros((arr[i].img_height, stride), np.uint8)
            opt = api.heif_decoding_options_alloc()
            api.heif_decoding_options_add_external_dest(opt, ext.ctypes.data_as(C.c_void_p), ext.size, stride)
            img = C.c_void_p()
            e = api.heif_decode_image(hdl, C.byref(img), 1, 11, opt)  # heif_colorspace_RGB, heif_chroma_interleaved_RGBA
            assert e.code == 0, e.message
            rc, msg, (planes, _) = decode_item(hm, f, ids[i], 11)
            assert rc == 0, msg
            np.testing.assert_array_equal(ext[:h, :w * 4], planes[0][:h, :w * 4])
            api.heif_image_release(img)
            api.heif_decoding_options_free(opt)
            api.heif_image_handle_release(hdl)
    finally:
        f.close()
        api.heif_context_free(ctx)


def test_plugin_given_a_frame(pkg, api, hm):
    """a libheif fork hands its decoder plugin exactly the frame's byte string: the plugin's planes equal hm_decode_item's"""
    plugin = api.hm_get_decoder_plugin().contents
    for name in ("synth8_short_hvcc", "synth10"):
        _, buf, w, h = MOVIES[name]
        f = pipeline.HeifFile(hm, buf)
        try:
            for k in (1, 2, moovwriter.fork_movie_info(buf)["frame_count"]):
                img = pluginapi.decode_tile(plugin, moovwriter.fork_sample_bytes(buf, k))
                rc, msg, (planes, meta) = decode_item(hm, f, k, 0)
                assert rc == 0, msg
                bps = 2 if meta["bit_depth"] > 8 else 1
                for c, ch in enumerate((0, 1, 2)):  # heif_channel_Y / Cb / Cr
                    st = C.c_int()
                    p = api.heif_image_get_plane_readonly(img, ch, C.byref(st))
                    pw, ph = api.heif_image_get_width(img, ch), api.heif_image_get_height(img, ch)
                    got = np.ctypeslib.as_array(p, shape=(ph, st.value))[:, :pw * bps]
                    np.testing.assert_array_equal(got, planes[c][:ph, :pw * bps], err_msg=f"{name} frame {k} channel {c}")
                api.heif_image_release(img)
        finally:
            f.close()
