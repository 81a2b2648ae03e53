"""CPU: image sequences - the fork's movie mode (a 'moov' track whose samples are HEVC-intra pictures, file.cc:474-483,
context.cc:646-700 of the reference).  Container, sample byte strings, refusals, the facade's heif_context_get_heif_params."""
import ctypes as C
import os
import struct

import pytest

import heifwriter
import moovwriter
import orc
import pipeline
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_BITSTREAM = -1, -2, -3


class SequenceInfo(C.Structure):
    _fields_ = [("is_sequence", C.c_int32), ("frame_count", C.c_uint32), ("duration", C.c_uint64)]


def pictures(n, seed=100, **kw):
    kw = dict(dict(width=96, height=64), **kw)
    return [synthutil.picture(seed + i, **kw) for i in range(n)]


def open_rc(hm, data):
    """(status, message) of hm_file_open"""
    pipeline.bind(hm)
    h = C.c_void_p()
    rc = hm.hm_file_open(data, len(data), C.byref(h))
    if not rc:
        hm.hm_file_close(h)
    return rc, hm.hm_last_error().decode()


def seq_info(hm, f):
    hm.hm_file_sequence_info.argtypes = [C.c_void_p, C.POINTER(SequenceInfo)]
    i = SequenceInfo()
    assert hm.hm_file_sequence_info(f.h, C.byref(i)) == 0
    return i


def top_level(hm, f):
    hm.hm_file_top_level_images.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    n = hm.hm_file_top_level_images(f.h, None, 0)
    ids = (C.c_uint32 * max(n, 1))()
    assert hm.hm_file_top_level_images(f.h, ids, n) == n
    return list(ids[:n])


def hevc_data_rc(hm, f, iid):
    p = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    rc = hm.hm_file_item_hevc_data(f.h, iid, C.byref(p), C.byref(n))
    if not rc:
        hm.hm_free(p)
    return rc, hm.hm_last_error().decode()


@pytest.mark.parametrize("version", [0, 1])
def test_movie_structure(hm, version):
    """frame count, IDs 1..N, primary 1, handle size from tkhd (not the pictures' size), depth from hvcC, mvhd duration"""
    pics = pictures(5)
    duration = 7_000_000_000 if version == 1 else 4321
    buf = moovwriter.write_movie(pics, (120, 80), duration=duration, version=version)
    f = pipeline.HeifFile(hm, buf)
    try:
        si = seq_info(hm, f)
        assert (si.is_sequence, si.frame_count, si.duration) == (1, 5, duration)
        assert f.primary() == 1
        assert top_level(hm, f) == [1, 2, 3, 4, 5]
        for k in range(1, 6):
            i = f.info(k)
            assert (i.width, i.height, i.bit_depth, i.chroma) == (120, 80, 8, 1)
            assert (i.is_grid, i.has_alpha, i.has_transforms, i.has_nclx) == (0, 0, 0, 0)
        with pytest.raises(RuntimeError):
            f.info(6)
    finally:
        f.close()


def test_still_image_is_not_a_sequence(hm):
    data = open(os.path.join(HERE, "data", "example.heic"), "rb").read()
    f = pipeline.HeifFile(hm, data)
    try:
        si = seq_info(hm, f)
        assert (si.is_sequence, si.frame_count, si.duration) == (0, 0, 0)
    finally:
        f.close()


def _layouts():
    same = [synthutil.picture(300, width=96, height=64)] * 4
    ten = pictures(3, seed=400, bit_depth=10)
    return {
        "per_entry": dict(pics=pictures(6), kw={}),
        "constant": dict(pics=same, kw=dict(constant_size=True)),
        "params_in_sample": dict(pics=pictures(4, seed=200), kw=dict(params_in="sample")),
        "short_hvcc": dict(pics=pictures(5, seed=500), kw=dict(hvcc_units=2)),
        "ten_bit": dict(pics=ten, kw=dict(bit_depth=10)),
        "v1_boxes": dict(pics=pictures(3, seed=600), kw=dict(version=1)),
        "long_compressorname": dict(pics=pictures(2, seed=700), kw=dict(compressorname=b"x" * 31)),
    }


@pytest.mark.parametrize("layout", sorted(_layouts()))
def test_sample_bytes_equal_fork_restatement(hm, layout):
    """hm_file_item_hevc_data(k) == unit k-1 of each hvcC array (or its last) + the sample (codecs/hevc.cc:196-224, file.cc:1154-1244)"""
    L = _layouts()[layout]
    buf = moovwriter.write_movie(L["pics"], (96, 64), **L["kw"])
    f = pipeline.HeifFile(hm, buf)
    try:
        info = moovwriter.fork_movie_info(buf)
        assert info["frame_count"] == len(L["pics"])
        for k in range(1, len(L["pics"]) + 1):
            assert f.hevc_data(k) == moovwriter.fork_sample_bytes(buf, k, info), k
        if layout in ("per_entry", "constant", "ten_bit", "v1_boxes"):  # every frame's own parameter sets: its own picture
            for k, p in enumerate(L["pics"], 1):
                assert f.hevc_data(k) == p
    finally:
        f.close()


def test_meta_beside_moov_is_ignored(hm):
    """with the brand and a moov box, a meta box (here: a real single-image one) is not read (context.cc:435-437)"""
    still = heifwriter.write_heic([synthutil.picture(900, width=64, height=64)], (64, 64))
    meta = moovwriter.top_box(still, b"meta")
    pics = pictures(3)
    buf = moovwriter.write_movie(pics, (96, 64), meta=meta)
    f = pipeline.HeifFile(hm, buf)
    try:
        assert seq_info(hm, f).is_sequence == 1
        assert top_level(hm, f) == [1, 2, 3]
        assert [f.hevc_data(k) for k in (1, 2, 3)] == pics
    finally:
        f.close()


def test_plain_heic_with_moov_but_without_the_brand_reads_meta(hm):
    """no 'hevc' / 'hevx' compatible brand: a moov box changes nothing - the file is read through meta as before"""
    still = heifwriter.write_heic([synthutil.picture(901, width=64, height=64)], (64, 64))
    movie = moovwriter.write_movie(pictures(2), (96, 64))
    moov = moovwriter.top_box(movie, b"moov")
    for data in (still, still + moov):
        f = pipeline.HeifFile(hm, data)
        try:
            assert seq_info(hm, f).is_sequence == 0
            assert top_level(hm, f) == [1]
            assert f.info(1).width == 64
            assert heifwriter.split_nals(f.hevc_data(1))[-1] == heifwriter.split_nals(synthutil.picture(901, width=64, height=64))[-1]
        finally:
            f.close()
    # the brand as the MAJOR brand only does not count either (Box_ftyp::has_compatible_brand)
    buf = moovwriter.write_movie(pictures(2), (96, 64), major=b"hevc", brands=(b"mif1", b"heic"))
    assert open_rc(hm, buf)[0] == HM_ERR_BITSTREAM  # (no meta box)


def test_hevx_brand_selects_movie_mode(hm):
    buf = moovwriter.write_movie(pictures(2), (96, 64), brands=(b"msf1", b"hevx"))
    f = pipeline.HeifFile(hm, buf)
    try:
        assert seq_info(hm, f).frame_count == 2
    finally:
        f.close()


def test_frame_count_is_samples_per_chunk(hm):
    """frame_count = the stsc entry's samples_per_chunk, not the stsz count (context.cc:654-676)"""
    buf = moovwriter.write_movie(pictures(4), (96, 64), samples_per_chunk=3)
    f = pipeline.HeifFile(hm, buf)
    try:
        assert seq_info(hm, f).frame_count == 3
        assert top_level(hm, f) == [1, 2, 3]
    finally:
        f.close()


def test_refusals(hm):
    pics = pictures(3)
    # two stsc entries: the fork's own message
    rc, msg = open_rc(hm, moovwriter.write_movie(pics, (96, 64), stsc_entries=[(1, 2, 1), (2, 1, 1)]))
    assert rc == HM_ERR_BITSTREAM and msg == "'stsc' box more than one chunk"
    # stsz shorter than samples_per_chunk: the fork reads past its table
    rc, msg = open_rc(hm, moovwriter.write_movie(pics, (96, 64), samples_per_chunk=4))
    assert rc == HM_ERR_BITSTREAM and "stsz" in msg
    # missing hvcC and other required boxes
    rc, msg = open_rc(hm, moovwriter.write_movie(pics, (96, 64), omit=(b"hvcC",)))
    assert rc == HM_ERR_BITSTREAM and "hvcC" in msg
    for box in (b"stco", b"stsz", b"stsc", b"stsd"):
        rc, msg = open_rc(hm, moovwriter.write_movie(pics, (96, 64), omit=(box,)))
        assert rc == HM_ERR_BITSTREAM and box.decode() in msg, box
    # compressorname without a NUL in its 32 bytes (the fork's read fails)
    rc, msg = open_rc(hm, moovwriter.write_movie(pics, (96, 64), compressorname=b"y" * 40))
    assert rc == HM_ERR_BITSTREAM and "hvc1" in msg
    # a sample past the end of the file: the file opens, that frame fails (file.cc:1174-1189)
    good = moovwriter.write_movie(pics, (96, 64))
    info = moovwriter.fork_movie_info(good)
    big = info["sizes"][:2] + [info["sizes"][2] + 1000]
    buf = moovwriter.write_movie(pics, (96, 64), stsz_entries=big)
    f = pipeline.HeifFile(hm, buf)
    try:
        assert hevc_data_rc(hm, f, 2)[0] == 0
        rc, msg = hevc_data_rc(hm, f, 3)
        assert rc == HM_ERR_BITSTREAM and "outside the file" in msg
    finally:
        f.close()
    buf = moovwriter.write_movie(pics, (96, 64), chunk_offset_delta=1 << 20)
    f = pipeline.HeifFile(hm, buf)
    try:
        assert hevc_data_rc(hm, f, 1)[0] == HM_ERR_BITSTREAM
    finally:
        f.close()


def p_slice(picture):
    """the picture with its (IDR, first) slice's slice_type turned from I (ue 2 = '011') into P (ue 1 = '010')"""
    nals = heifwriter.split_nals(picture)
    k = next(i for i, n in enumerate(nals) if (n[0] >> 1) & 0x3F < 32)
    n = bytearray(nals[k])
    # first_slice_segment_in_pic_flag = 1, no_output_of_prior_pics_flag, slice_pic_parameter_set_id = ue(0) = '1', slice_type
    assert (n[2] >> 2) & 0x2F == 0x2B, hex(n[2])
    n[2] ^= 0x04
    nals[k] = bytes(n)
    return b"".join(struct.pack(">I", len(x)) + x for x in nals)


def test_p_slice_sample_is_refused(pkg, hm):
    pics = pictures(3)
    pics[1] = p_slice(pics[1])
    buf = moovwriter.write_movie(pics, (96, 64))
    f = pipeline.HeifFile(hm, buf)
    try:
        data = f.hevc_data(2)
        assert data == moovwriter.fork_sample_bytes(buf, 2)
        with pytest.raises(pkg.capi.HmError) as e:
            pkg.capi.parse_hevc(data)
        assert e.value.status == HM_ERR_UNSUPPORTED and "P/B slice" in str(e.value)
        pkg.capi.parse_hevc(f.hevc_data(3))  # the neighbours parse
    finally:
        f.close()


def test_reference_decodes_every_frame(hm):
    """libde265 (oracle/_ref) decodes each frame's byte string as the fork's decoder plugin would get it, to the picture's own pixels"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    pics = pictures(4, seed=800)
    for kw in (dict(), dict(hvcc_units=1), dict(params_in="sample")):
        buf = moovwriter.write_movie(pics, (96, 64), **kw)
        f = pipeline.HeifFile(hm, buf)
        try:
            for k, p in enumerate(pics, 1):
                got, _ = orc.ref_decode(f.hevc_data(k), 0)
                want, _ = orc.ref_decode(p, 0)
                for a, b in zip(got, want):
                    assert (a == b).all(), (kw, k)
        finally:
            f.close()


class ImageParameters(C.Structure):
    _fields_ = [("alpha_flag", C.c_bool), ("img_width", C.c_uint32), ("img_height", C.c_uint32), ("img_bitdepth", C.c_uint32)]


class LibheifParameters(C.Structure):
    _fields_ = [("movie_flag", C.c_bool), ("frame_count", C.c_uint32), ("movie_duration", C.c_uint32),
                ("img_params", C.POINTER(ImageParameters))]


class Err(C.Structure):
    _fields_ = [("code", C.c_int), ("subcode", C.c_int), ("message", C.c_char_p)]


@pytest.fixture(scope="module")
def api(pkg):
    pkg.lib()
    a = C.CDLL(os.path.join(ROOT, "heif-decoder-lib_amd", "libheif_mi355x_api.so"))
    a.heif_context_alloc.restype = C.c_void_p
    a.heif_context_free.argtypes = [C.c_void_p]
    a.heif_context_read_from_memory.restype = Err
    a.heif_context_read_from_memory.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
    a.heif_context_get_number_of_top_level_images.argtypes = [C.c_void_p]
    a.heif_context_get_list_of_top_level_image_IDs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    a.heif_context_get_heif_params.restype = Err
    a.heif_context_get_heif_params.argtypes = [C.c_void_p, C.POINTER(LibheifParameters)]
    return a


def heif_params(api, data):
    ctx = api.heif_context_alloc()
    try:
        e = api.heif_context_read_from_memory(ctx, data, len(data), None)
        assert e.code == 0, e.message
        n = api.heif_context_get_number_of_top_level_images(ctx)
        arr = (ImageParameters * max(n, 1))()
        p = LibheifParameters(False, 0, 0, arr)
        e = api.heif_context_get_heif_params(ctx, C.byref(p))
        assert e.code == 0, e.message
        ids = (C.c_uint32 * max(n, 1))()
        assert api.heif_context_get_list_of_top_level_image_IDs(ctx, ids, n) == n
        return p, [(a.alpha_flag, a.img_width, a.img_height, a.img_bitdepth) for a in arr[:n]], list(ids[:n])
    finally:
        api.heif_context_free(ctx)


def test_heif_params_of_a_movie(api):
    """heif_context_get_heif_params (heif.h:672-686, context.cc:459-491): movie flag, frame count, duration, per frame the
    tkhd size, the hvcC depth, no alpha"""
    assert C.sizeof(ImageParameters) == 16 and C.sizeof(LibheifParameters) == 24
    buf = moovwriter.write_movie(pictures(3, bit_depth=10), (100, 70), bit_depth=10, duration=(1 << 32) + 55, version=1)
    p, frames, ids = heif_params(api, buf)
    assert (p.movie_flag, p.frame_count, p.movie_duration) == (True, 3, 55)  # (the fork's field: 32 bits of mvhd's duration)
    assert frames == [(False, 100, 70, 10)] * 3
    assert ids == [1, 2, 3]


def test_heif_params_of_still_images(api):
    """non-movie files: movie_flag false, duration 0, one entry per top-level image with the handle's size, depth and alpha flag"""
    for name, want in (("colors-with-alpha.heic", True), ("colors-no-alpha.heic", False), ("example.heic", False)):
        data = open(os.path.join(HERE, "data", name), "rb").read()
        p, frames, ids = heif_params(api, data)
        assert (p.movie_flag, p.movie_duration) == (False, 0)
        assert p.frame_count == len(ids) >= 1
        assert all(f[0] == want and f[1] > 0 and f[2] > 0 and f[3] == 8 for f in frames), (name, frames)
