"""Device-resident planar YCbCr (hm_device_planes), the part that needs no GPU: hm_device_planes_bytes against a numpy restatement
and hand-computed values, every refusal that is decided on the host with a message that names the field, NULL arguments, and what a
box without a GPU answers."""
import ctypes as C
import itertools

import numpy as np
import pytest

import heifwriter
import synthutil

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_NO_DEVICE = -1, -2, -4
SEPARATE, SEMI = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
ELEM = {U8: 1, U16: 2, F16: 2, F32: 4}
YCBCR_420, YCBCR_444 = 0x101, 0x103
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def planes(capi, layout, dtype, pitches=(0, 0, 0, 0), ptrs=(None, None, None, None), lens=(0, 0, 0, 0), msb=0, reserved=0):
    d = capi.DevicePlanes()
    d.layout, d.dtype, d.msb_aligned, d.reserved = layout, dtype, msb, reserved
    for c in range(4):
        d.plane[c].ptr, d.plane[c].len, d.plane[c].row_pitch = ptrs[c], lens[c], pitches[c]
        d.scale[c], d.bias[c] = 1.0, 0.0
    return d


def plane_sizes(chroma, layout, w, h):
    """(elements per row, rows) of plane[0 .. 3]; None: the plane does not exist"""
    cw, ch = (w if chroma == 3 else (w + 1) // 2), ((h + 1) // 2 if chroma == 1 else h)
    if chroma == 0:
        return [(w, h), None, None, (w, h)]
    if layout == SEMI:
        return [(w, h), (2 * cw, ch), None, (w, h)]
    return [(w, h), (cw, ch), (cw, ch), (w, h)]


def expected_need(chroma, layout, dtype, w, h, pitches):
    need = np.zeros(4, np.int64)
    for c, size in enumerate(plane_sizes(chroma, layout, w, h)):
        if size is not None:
            tight = size[0] * ELEM[dtype]
            need[c] = (pitches[c] or tight) * (size[1] - 1) + tight
    return need


def allowed_dtype(dtype, bits):
    return dtype in (F16, F32) or (dtype == U8) == (bits == 8)


def test_planes_bytes_against_numpy(capi, L):
    for chroma, bits, w, h, layout, dtype, padded in itertools.product((0, 1, 2, 3), (8, 10, 12), (1, 2, 3, 17, 200), (1, 2, 5, 136), (SEPARATE, SEMI),
                                                                       (U8, U16, F16, F32), (False, True)):
        sizes = plane_sizes(chroma, layout, w, h)
        # padded: every plane that exists gets a pitch 64 bytes + one element above tight
        pitches = [0 if (s is None or not padded) else s[0] * ELEM[dtype] + 64 + ELEM[dtype] for s in sizes]
        for with_alpha in (False, True):
            d = planes(capi, layout, dtype, pitches, ptrs=(None, None, None, FAKE if with_alpha else None))
            need = (C.c_int64 * 4)(-1, -1, -1, -1)
            got = L.hm_device_planes_bytes(chroma, bits, w, h, C.byref(d), C.byref(need))
            what = (chroma, bits, w, h, layout, dtype, padded, with_alpha)
            if not allowed_dtype(dtype, bits):
                assert got == HM_ERR_INVALID_ARG and "dtype" in L.hm_last_error().decode(), what
                continue
            exp = expected_need(chroma, layout, dtype, w, h, pitches)
            assert list(need) == list(exp), (what, list(need), list(exp))
            assert got == exp[:3].sum() + (exp[3] if with_alpha else 0), what


def test_planes_bytes_known_values(capi, L):
    """a few written out by hand"""
    need = (C.c_int64 * 4)()
    # NV12 of a 200 x 136 8-bit 4:2:0 picture, tight: 200 * 136 luma, 100 pairs x 68 rows
    assert L.hm_device_planes_bytes(1, 8, 200, 136, C.byref(planes(capi, SEMI, U8)), C.byref(need)) == 27200 + 13600
    assert list(need) == [27200, 13600, 0, 27200]
    # I420 of the same
    assert L.hm_device_planes_bytes(1, 8, 200, 136, C.byref(planes(capi, SEPARATE, U8)), C.byref(need)) == 27200 + 6800 + 6800
    assert list(need) == [27200, 6800, 6800, 27200]
    # P010 of a 121 x 77 10-bit 4:2:0 picture: chroma 61 x 39, luma pitch 256: 256 * 76 + 242, chroma tight: 61 * 2 * 2 * 39
    assert L.hm_device_planes_bytes(1, 10, 121, 77, C.byref(planes(capi, SEMI, U16, (256, 0, 0, 0), msb=1)), C.byref(need)) == 256 * 76 + 242 + 244 * 39
    # 4:0:0 float32 with an alpha plane asked for: Y and A
    d = planes(capi, SEPARATE, F32, ptrs=(None, None, None, FAKE))
    assert L.hm_device_planes_bytes(0, 8, 3, 2, C.byref(d), C.byref(need)) == 24 + 24 and list(need) == [24, 0, 0, 24]
    # 4:2:2 float16 of 17 x 5, interleaved: 9 pairs x 5 rows
    assert L.hm_device_planes_bytes(2, 12, 17, 5, C.byref(planes(capi, SEMI, F16)), None) == 17 * 5 * 2 + 9 * 2 * 2 * 5
    assert L.hm_device_planes_bytes(3, 8, 17, 5, C.byref(planes(capi, SEPARATE, U8)), None) == 3 * 85


def test_planes_bytes_refusals_name_the_field(capi, L):
    def refused(d, status, word, chroma=1, bits=8, w=16, h=8):
        assert L.hm_device_planes_bytes(chroma, bits, w, h, C.byref(d), None) == status, word
        assert word in L.hm_last_error().decode(), (word, L.hm_last_error().decode())
    assert L.hm_device_planes_bytes(1, 8, 16, 8, None, None) == HM_ERR_INVALID_ARG
    refused(planes(capi, 2, U8), HM_ERR_INVALID_ARG, "layout")
    refused(planes(capi, SEPARATE, 4), HM_ERR_INVALID_ARG, "dtype")
    refused(planes(capi, SEPARATE, -1), HM_ERR_INVALID_ARG, "dtype")
    refused(planes(capi, SEPARATE, U8, reserved=1), HM_ERR_INVALID_ARG, "reserved")
    for dtype in (U8, F16, F32):
        refused(planes(capi, SEPARATE, dtype, msb=1), HM_ERR_INVALID_ARG, "msb_aligned")
    refused(planes(capi, SEPARATE, U16, msb=2), HM_ERR_INVALID_ARG, "msb_aligned", bits=10)
    # the integer dtype against the result's depth
    refused(planes(capi, SEPARATE, U8), HM_ERR_INVALID_ARG, "dtype", bits=10)
    refused(planes(capi, SEPARATE, U16), HM_ERR_INVALID_ARG, "dtype", bits=8)
    # pitches: below tight, not a multiple of the element size, negative - each names its plane
    refused(planes(capi, SEPARATE, U8, (15, 0, 0, 0)), HM_ERR_INVALID_ARG, "plane[0].row_pitch")
    refused(planes(capi, SEPARATE, U8, (0, 7, 0, 0)), HM_ERR_INVALID_ARG, "plane[1].row_pitch")
    refused(planes(capi, SEPARATE, U8, (0, 0, 7, 0)), HM_ERR_INVALID_ARG, "plane[2].row_pitch")
    refused(planes(capi, SEMI, U8, (0, 15, 0, 0)), HM_ERR_INVALID_ARG, "plane[1].row_pitch")  # (16 elements: 8 pairs)
    refused(planes(capi, SEPARATE, F32, (66, 0, 0, 0)), HM_ERR_INVALID_ARG, "multiple of the element size")
    refused(planes(capi, SEPARATE, U16, (0, 17, 0, 0)), HM_ERR_INVALID_ARG, "plane[1].row_pitch", bits=10)
    refused(planes(capi, SEPARATE, U8, (-16, 0, 0, 0)), HM_ERR_INVALID_ARG, "plane[0].row_pitch")
    refused(planes(capi, SEPARATE, U8, (0, 0, 0, 15), ptrs=(None, None, None, FAKE)), HM_ERR_INVALID_ARG, "plane[3].row_pitch")
    # pointers that are not multiples of the element size
    refused(planes(capi, SEPARATE, F32, ptrs=(FAKE + 2, None, None, None)), HM_ERR_INVALID_ARG, "plane[0].ptr")
    refused(planes(capi, SEPARATE, F16, ptrs=(None, FAKE + 1, None, None)), HM_ERR_INVALID_ARG, "plane[1].ptr")
    # semi-planar: plane[2] all zero; 4:0:0: plane[1] and plane[2] all zero
    refused(planes(capi, SEMI, U8, ptrs=(None, None, FAKE, None)), HM_ERR_INVALID_ARG, "plane[2]")
    refused(planes(capi, SEMI, U8, (0, 0, 16, 0)), HM_ERR_INVALID_ARG, "plane[2]")
    refused(planes(capi, SEMI, U8, lens=(0, 0, 1, 0)), HM_ERR_INVALID_ARG, "plane[2]")
    refused(planes(capi, SEPARATE, U8, ptrs=(None, FAKE, None, None)), HM_ERR_INVALID_ARG, "plane[1]", chroma=0)
    refused(planes(capi, SEPARATE, U8, (0, 0, 8, 0)), HM_ERR_INVALID_ARG, "plane[2]", chroma=0)
    # the format itself
    refused(planes(capi, SEPARATE, U8), HM_ERR_INVALID_ARG, "chroma", chroma=4)
    refused(planes(capi, SEPARATE, U8), HM_ERR_INVALID_ARG, "bit depth", bits=7)
    refused(planes(capi, SEPARATE, U8), HM_ERR_INVALID_ARG, "size", w=0)
    refused(planes(capi, SEPARATE, U8), HM_ERR_INVALID_ARG, "size", h=32769)


@pytest.fixture(scope="module")
def heic():
    pic = synthutil.picture(47000, width=96, height=64)
    return heifwriter.write_heic([pic], (96, 64))


class File:
    def __init__(self, L, data):
        self.L, self.h = L, C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(self.h)) == 0
        self.id = L.hm_file_primary_item(self.h)

    def to_planes(self, capi, fmt, d, ext_dst=None, to_8bit=0):
        prm = capi.DecodeParams(fmt, 1, 0, 0, None, ext_dst, 0, 0, 0, to_8bit)
        out = capi.Decoded()
        rc = self.L.hm_decode_item_to_device_planes(self.h, self.id, C.byref(prm), C.byref(d), C.byref(out))
        assert not out.plane[0] and not out.plane[1] and not out.plane[2] and not out.alpha
        return rc, self.L.hm_last_error().decode()

    def close(self):
        self.L.hm_file_close(self.h)


def i420(capi, **kw):
    """a destination that is in order for the 96 x 64 8-bit 4:2:0 file, at fake addresses"""
    args = dict(ptrs=(FAKE, FAKE + 0x10000, FAKE + 0x20000, None), lens=(96 * 64, 48 * 32, 48 * 32, 0))
    args.update(kw)
    return planes(capi, SEPARATE, U8, **args)


def test_decode_to_device_planes_host_side_refusals(capi, L, heic):
    f = File(L, heic)
    try:
        prm = capi.DecodeParams(0, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        d = i420(capi)
        # NULL arguments
        assert L.hm_decode_item_to_device_planes(None, f.id, C.byref(prm), C.byref(d), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device_planes(f.h, f.id, None, C.byref(d), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device_planes(f.h, f.id, C.byref(prm), None, C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device_planes(f.h, f.id, C.byref(prm), C.byref(d), None) == HM_ERR_INVALID_ARG
        host = (C.c_uint8 * 64)()
        cases = [
            # ext_dst together with planes; an interleaved RGB target
            (0, i420(capi), dict(ext_dst=C.cast(host, C.c_void_p)), HM_ERR_INVALID_ARG, "ext_dst"),
            (10, i420(capi), {}, HM_ERR_INVALID_ARG, "hm_decode_item_to_device"),
            (15, i420(capi), {}, HM_ERR_INVALID_ARG, "hm_decode_item_to_device"),
            (9, i420(capi), {}, HM_ERR_INVALID_ARG, "output format"),
            # the static refusals
            (0, planes(capi, 3, U8), {}, HM_ERR_INVALID_ARG, "layout"),
            (0, planes(capi, SEPARATE, 7), {}, HM_ERR_INVALID_ARG, "dtype"),
            (0, i420(capi, reserved=5), {}, HM_ERR_INVALID_ARG, "reserved"),
            (0, i420(capi, msb=1), {}, HM_ERR_INVALID_ARG, "msb_aligned"),
            (0, i420(capi, pitches=(95, 0, 0, 0)), {}, HM_ERR_INVALID_ARG, "plane[0].row_pitch"),
            (0, i420(capi, pitches=(0, 0, 47, 0)), {}, HM_ERR_INVALID_ARG, "plane[2].row_pitch"),
            (0, i420(capi, ptrs=(None, FAKE + 0x10000, FAKE + 0x20000, None)), {}, HM_ERR_INVALID_ARG, "plane[0].ptr"),
            (0, i420(capi, ptrs=(FAKE, None, FAKE + 0x20000, None)), {}, HM_ERR_INVALID_ARG, "plane[1].ptr"),
            # len below the last-row form, per plane (the sizes the file declares); a padded pitch counts
            (0, i420(capi, lens=(96 * 64 - 1, 48 * 32, 48 * 32, 0)), {}, HM_ERR_INVALID_ARG, "plane[0].len"),
            (0, i420(capi, lens=(96 * 64, 48 * 32, 48 * 32 - 1, 0)), {}, HM_ERR_INVALID_ARG, "plane[2].len"),
            (0, i420(capi, pitches=(128, 0, 0, 0)), {}, HM_ERR_INVALID_ARG, "plane[0].len"),
            (0, i420(capi, ptrs=(FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000)), {}, HM_ERR_INVALID_ARG, "plane[3].len"),
            # two planes whose bytes overlap
            (0, i420(capi, ptrs=(FAKE, FAKE + 96 * 64 - 1, FAKE + 0x20000, None)), {}, HM_ERR_INVALID_ARG, "overlap"),
            (0, i420(capi, ptrs=(FAKE, FAKE + 0x10000, FAKE + 0x10000 + 48 * 31, None)), {}, HM_ERR_INVALID_ARG, "overlap"),
            # what the file's hm_image_info decides: the depth class, the result's chroma format
            (0, planes(capi, SEPARATE, U16, ptrs=(FAKE, FAKE + 0x10000, FAKE + 0x20000, None), lens=(1 << 20,) * 3 + (0,)), {}, HM_ERR_INVALID_ARG, "dtype"),
            (YCBCR_444, i420(capi), {}, HM_ERR_INVALID_ARG, "plane[1].len"),  # (4:4:4 chroma planes are 96 x 64)
            (0, planes(capi, SEMI, U8, ptrs=(FAKE, FAKE + 0x10000, None, None), lens=(96 * 64, 96 * 32 - 1, 0, 0)), {}, HM_ERR_INVALID_ARG, "plane[1].len"),
        ]
        for fmt, dd, kw, status, word in cases:
            rc, msg = f.to_planes(capi, fmt, dd, **kw)
            assert rc == status and word in msg, (fmt, word, rc, msg)
        # requests that are in order: a box without a GPU says so; with one, the pointers are found not to be device memory
        for fmt, dd in ((0, i420(capi)), (YCBCR_420, i420(capi)),
                        (0, planes(capi, SEMI, F16, ptrs=(FAKE, FAKE + 0x10000, None, None), lens=(96 * 64 * 2, 96 * 32 * 2, 0, 0)))):
            rc, msg = f.to_planes(capi, fmt, dd)
            if L.hm_device_count() == 0:
                assert rc == HM_ERR_NO_DEVICE, msg
            else:
                assert rc == HM_ERR_INVALID_ARG and "plane[0].ptr" in msg
    finally:
        f.close()


def test_other_entry_points_null_arguments_and_refusals(capi, L, heic):
    f = File(L, heic)
    try:
        prm = capi.DecodeParams(0, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        failed = C.c_int32(7)
        d = i420(capi)
        ids = (C.c_uint32 * 1)(1)
        assert L.hm_decode_frames_to_device_planes(None, ids, 1, C.byref(prm), C.byref(d), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_frames_to_device_planes(f.h, None, 1, C.byref(prm), C.byref(d), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_frames_to_device_planes(f.h, ids, 1, C.byref(prm), None, C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_frames_to_device_planes(f.h, ids, 1, None, C.byref(d), C.byref(out), None) == HM_ERR_INVALID_ARG
        assert failed.value == -1
        # (a still image is not a sequence)
        assert L.hm_decode_frames_to_device_planes(f.h, ids, 1, C.byref(prm), C.byref(d), C.byref(out), None) == HM_ERR_INVALID_ARG
        assert "sequence" in L.hm_last_error().decode()
        assert L.hm_pipeline_submit_to_device_planes(None, heic, len(heic), 0, 0, C.byref(d)) == HM_ERR_INVALID_ARG
        # the step alone: NULL arguments, and a bad destination before a device is looked for
        srcs, strides = (C.c_void_p * 4)(FAKE, FAKE, FAKE, None), (C.c_int32 * 4)(128, 64, 64, 0)
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 0, None, C.byref(strides), C.byref(d), None) == HM_ERR_INVALID_ARG
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 0, C.byref(srcs), None, C.byref(d), None) == HM_ERR_INVALID_ARG
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 0, C.byref(srcs), C.byref(strides), None, None) == HM_ERR_INVALID_ARG
        short = i420(capi, lens=(96 * 64, 48 * 32 - 1, 48 * 32, 0))
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 0, C.byref(srcs), C.byref(strides), C.byref(short), None) == HM_ERR_INVALID_ARG
        assert "plane[1].len" in L.hm_last_error().decode()
        with_alpha = i420(capi, ptrs=(FAKE, FAKE + 0x10000, FAKE + 0x20000, FAKE + 0x30000), lens=(96 * 64, 48 * 32, 48 * 32, 96 * 64))
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 0, C.byref(srcs), C.byref(strides), C.byref(with_alpha), None) == HM_ERR_INVALID_ARG
        assert "no alpha" in L.hm_last_error().decode()
        srcs[3], strides[3] = FAKE, 128
        assert L.hm_planes_to_tensor(1, 8, 96, 64, 10, C.byref(srcs), C.byref(strides), C.byref(with_alpha), None) == HM_ERR_UNSUPPORTED
        assert "alpha plane of 10 bits" in L.hm_last_error().decode()
        rc = L.hm_planes_to_tensor(1, 8, 96, 64, 0, C.byref(srcs), C.byref(strides), C.byref(d), None)
        assert rc == (HM_ERR_NO_DEVICE if L.hm_device_count() == 0 else HM_ERR_INVALID_ARG)
    finally:
        f.close()


def test_planar_formats_stay_refused_by_the_rgb_destination(capi, L, heic):
    """hm_device_dest is an interleaved-RGB destination: hm_decode_item_to_device answers a planar format as it always did"""
    f = File(L, heic)
    try:
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = FAKE, 1 << 20, 0, U8
        for fmt in (0, 0x101, 0x102, 0x103):
            prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
            out = capi.Decoded()
            assert L.hm_decode_item_to_device(f.h, f.id, C.byref(prm), C.byref(d), C.byref(out)) == HM_ERR_UNSUPPORTED
            assert L.hm_last_error().decode() == f"planar YCbCr output (format {fmt}) is not supported with a device destination"
    finally:
        f.close()


def test_python_entry_points_are_exported(pkg):
    for name in ("decode_to_planes", "decode_sequence_to_planes", "decode_batch_to_planes"):
        assert callable(getattr(pkg, name)) and getattr(pkg.decode, name) is getattr(pkg, name)
    with pytest.raises(ValueError, match="layout"):
        pkg.decode_to_planes(b"", layout="nv12")
    with pytest.raises(ValueError, match="chroma"):
        pkg.decode_to_planes(b"", chroma="411")
