"""Device-resident output, the part that needs no GPU: hm_device_dest_bytes against hand-computed values for every
format x layout x dtype, every refusal that is decided on the host, NULL arguments, and what a box without a GPU answers."""
import ctypes as C
import itertools

import pytest

import heifwriter
import synthutil

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED, HM_ERR_NO_DEVICE = -1, -2, -4
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 13, 14, 15
FORMATS = {RGB: (3, 1), RGBA: (4, 1), RRGGBB_BE: (3, 2), RRGGBBAA_BE: (4, 2), RRGGBB_LE: (3, 2), RRGGBBAA_LE: (4, 2)}  # channels, bytes per sample
BIG_ENDIAN = (RRGGBB_BE, RRGGBBAA_BE)
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
ELEM = {U8: 1, U16: 2, F16: 2, F32: 4}


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def dest(capi, layout, dtype, row_pitch=0, plane_pitch=0, ptr=None, length=0):
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype, d.row_pitch, d.plane_pitch = ptr, length, layout, dtype, row_pitch, plane_pitch
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    return d


def allowed(fmt, layout, dtype):
    """the combinations the interface defines: HWC with the target's own integer type is the raw bytes (any byte order); CHW
    and float output take sample values - integer dtype = the target's width, no big-endian target"""
    sample_bytes = FORMATS[fmt][1]
    if dtype in (U8, U16) and ELEM[dtype] != sample_bytes:
        return False
    raw = layout == HWC and dtype in (U8, U16)
    return raw or fmt not in BIG_ENDIAN


def expected_bytes(fmt, layout, dtype, w, h, row_pitch=0, plane_pitch=0):
    c, e = FORMATS[fmt][0], ELEM[dtype]
    if layout == HWC:
        rp = row_pitch or w * c * e
        return rp * (h - 1) + w * c * e
    rp = row_pitch or w * e
    pp = plane_pitch or rp * h
    return pp * (c - 1) + rp * (h - 1) + w * e


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (4032, 3024)])
def test_dest_bytes_every_combination(capi, L, w, h):
    for fmt, layout, dtype in itertools.product(FORMATS, (HWC, CHW), (U8, U16, F16, F32)):
        got = L.hm_device_dest_bytes(fmt, w, h, C.byref(dest(capi, layout, dtype)))
        if not allowed(fmt, layout, dtype):
            assert got == HM_ERR_INVALID_ARG, (fmt, layout, dtype, got)
            assert L.hm_last_error()
            continue
        assert got == expected_bytes(fmt, layout, dtype, w, h), (fmt, layout, dtype)
        # padded pitches: a row pitch one 64-byte line wider than tight, a plane pitch three rows longer than tight
        c, e = FORMATS[fmt][0], ELEM[dtype]
        rp = w * e * (c if layout == HWC else 1) + 64
        pp = (rp * h + 3 * rp) if layout == CHW else 0
        got = L.hm_device_dest_bytes(fmt, w, h, C.byref(dest(capi, layout, dtype, rp, pp)))
        assert got == expected_bytes(fmt, layout, dtype, w, h, rp, pp), (fmt, layout, dtype, "padded")


def test_dest_bytes_known_values(capi, L):
    """a few written out by hand"""
    assert L.hm_device_dest_bytes(RGB, 4032, 3024, C.byref(dest(capi, HWC, U8))) == 4032 * 3024 * 3
    assert L.hm_device_dest_bytes(RGB, 4032, 3024, C.byref(dest(capi, CHW, F32))) == 4032 * 3024 * 3 * 4
    assert L.hm_device_dest_bytes(RGBA, 10, 4, C.byref(dest(capi, CHW, F16, 32, 256))) == 256 * 3 + 32 * 3 + 20
    assert L.hm_device_dest_bytes(RRGGBB_BE, 10, 4, C.byref(dest(capi, HWC, U16, 64))) == 64 * 3 + 60
    assert L.hm_device_dest_bytes(RRGGBBAA_LE, 3, 2, C.byref(dest(capi, HWC, F32))) == 3 * 4 * 4 * 2


def test_dest_bytes_refusals(capi, L):
    def refused(fmt, d, status, word, w=16, h=8):
        assert L.hm_device_dest_bytes(fmt, w, h, C.byref(d)) == status
        assert word in L.hm_last_error().decode(), L.hm_last_error().decode()
    assert L.hm_device_dest_bytes(RGB, 16, 8, None) == HM_ERR_INVALID_ARG
    # planar YCbCr / as-decoded targets
    for fmt in (0, 0x101, 0x102, 0x103, 0x301):
        refused(fmt, dest(capi, HWC, U8), HM_ERR_UNSUPPORTED, "not supported with a device destination")
    refused(9, dest(capi, HWC, U8), HM_ERR_UNSUPPORTED, "output format")
    # the integer dtype must be the target's
    refused(RGB, dest(capi, HWC, U16), HM_ERR_INVALID_ARG, "dtype")
    refused(RRGGBB_LE, dest(capi, CHW, U8), HM_ERR_INVALID_ARG, "dtype")
    refused(RGB, dest(capi, CHW, 4), HM_ERR_INVALID_ARG, "dtype")
    refused(RGB, dest(capi, 2, U8), HM_ERR_INVALID_ARG, "layout")
    # big-endian targets only as raw bytes
    refused(RRGGBB_BE, dest(capi, CHW, U16), HM_ERR_INVALID_ARG, "_LE")
    refused(RRGGBBAA_BE, dest(capi, HWC, F32), HM_ERR_INVALID_ARG, "_LE")
    # pitches below the tight value
    refused(RGB, dest(capi, HWC, U8, 16 * 3 - 1), HM_ERR_INVALID_ARG, "row_pitch")
    refused(RGB, dest(capi, CHW, F32, 16 * 4 - 4), HM_ERR_INVALID_ARG, "row_pitch")
    refused(RGB, dest(capi, CHW, F32, 64, 64 * 8 - 4), HM_ERR_INVALID_ARG, "plane_pitch")
    # pitches that are not multiples of the element size
    refused(RGB, dest(capi, CHW, F32, 66), HM_ERR_INVALID_ARG, "multiple of the element size")
    refused(RGB, dest(capi, CHW, F16, 64, 64 * 8 + 1), HM_ERR_INVALID_ARG, "multiple of the element size")
    refused(RRGGBB_LE, dest(capi, HWC, U16, 16 * 6 + 1), HM_ERR_INVALID_ARG, "multiple of the element size")
    refused(RGB, dest(capi, HWC, U8, -48), HM_ERR_INVALID_ARG, "pitch")
    refused(RGB, dest(capi, HWC, U8), HM_ERR_INVALID_ARG, "size", w=0)


@pytest.fixture(scope="module")
def heic():
    pic = synthutil.picture(41000, width=96, height=64)
    return heifwriter.write_heic([pic], (96, 64))


class File:
    def __init__(self, L, data):
        self.L, self.h = L, C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(self.h)) == 0
        self.id = L.hm_file_primary_item(self.h)

    def to_device(self, capi, fmt, d, ext_dst=None):
        prm = capi.DecodeParams(fmt, 1, 0, 0, None, ext_dst, 0, 0, 0, 0)
        out = capi.Decoded()
        rc = self.L.hm_decode_item_to_device(self.h, self.id, C.byref(prm), C.byref(d), C.byref(out))
        assert not out.plane[0]
        return rc, self.L.hm_last_error().decode()

    def close(self):
        self.L.hm_file_close(self.h)


FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused, or finds no device)


def test_decode_to_device_host_side_refusals(capi, L, heic):
    f = File(L, heic)
    try:
        need = 96 * 64 * 3
        prm = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        d = dest(capi, HWC, U8, ptr=FAKE, length=need)
        # NULL arguments
        assert L.hm_decode_item_to_device(None, f.id, C.byref(prm), C.byref(d), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device(f.h, f.id, None, C.byref(d), C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device(f.h, f.id, C.byref(prm), None, C.byref(out)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_item_to_device(f.h, f.id, C.byref(prm), C.byref(d), None) == HM_ERR_INVALID_ARG
        rc, msg = f.to_device(capi, RGB, dest(capi, HWC, U8, ptr=None, length=need))
        assert rc == HM_ERR_INVALID_ARG and "null ptr" in msg
        # ext_dst together with a destination
        host = (C.c_uint8 * need)()
        rc, msg = f.to_device(capi, RGB, d, ext_dst=C.cast(host, C.c_void_p))
        assert rc == HM_ERR_INVALID_ARG and "ext_dst" in msg
        # len below hm_device_dest_bytes (the size the file declares), for both layouts
        rc, msg = f.to_device(capi, RGB, dest(capi, HWC, U8, ptr=FAKE, length=need - 1))
        assert rc == HM_ERR_INVALID_ARG and "len" in msg
        rc, msg = f.to_device(capi, RGB, dest(capi, CHW, F32, ptr=FAKE, length=need * 4 - 1))
        assert rc == HM_ERR_INVALID_ARG and "len" in msg
        # pitch below tight, ptr / pitch not multiples of the element size, dtype mismatch, _BE with CHW, planar targets
        for fmt, dd, status, word in (
                (RGB, dest(capi, HWC, U8, 96 * 3 - 1, ptr=FAKE, length=1 << 20), HM_ERR_INVALID_ARG, "row_pitch"),
                (RGB, dest(capi, CHW, F32, ptr=FAKE + 2, length=1 << 20), HM_ERR_INVALID_ARG, "ptr is not a multiple"),
                (RGB, dest(capi, CHW, F16, 96 * 2 + 1, ptr=FAKE, length=1 << 20), HM_ERR_INVALID_ARG, "multiple of the element size"),
                (RGB, dest(capi, CHW, U16, ptr=FAKE, length=1 << 20), HM_ERR_INVALID_ARG, "dtype"),
                (RRGGBB_BE, dest(capi, CHW, U16, ptr=FAKE, length=1 << 20), HM_ERR_INVALID_ARG, "_LE"),
                (0, dest(capi, HWC, U8, ptr=FAKE, length=1 << 20), HM_ERR_UNSUPPORTED, "not supported with a device destination"),
                (0x101, dest(capi, HWC, U8, ptr=FAKE, length=1 << 20), HM_ERR_UNSUPPORTED, "not supported with a device destination")):
            rc, msg = f.to_device(capi, fmt, dd)
            assert rc == status and word in msg, (fmt, rc, msg)
        # a request that is in order: a box without a GPU says so; with one, the pointer is found not to be device memory
        rc, msg = f.to_device(capi, RGB, d)
        if L.hm_device_count() == 0:
            assert rc == HM_ERR_NO_DEVICE, msg
        else:
            assert rc == HM_ERR_INVALID_ARG and "ptr" in msg
    finally:
        f.close()


def test_sequence_and_pipeline_entry_points_null_arguments(capi, L, heic):
    f = File(L, heic)
    try:
        prm = capi.DecodeParams(RGB, 1, 0, 0, None, None, 0, 0, 0, 0)
        out = capi.Decoded()
        failed = C.c_int32(7)
        d = dest(capi, HWC, U8, ptr=FAKE, length=1 << 20)
        assert L.hm_decode_sequence_to_device(None, 1, 1, C.byref(prm), C.byref(d), C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_sequence_to_device(f.h, 1, 1, C.byref(prm), None, C.byref(out), C.byref(failed)) == HM_ERR_INVALID_ARG
        assert L.hm_decode_sequence_to_device(f.h, 1, 1, None, C.byref(d), C.byref(out), None) == HM_ERR_INVALID_ARG
        assert failed.value == -1
        # (a still image is not a sequence)
        assert L.hm_decode_sequence_to_device(f.h, 1, 1, C.byref(prm), C.byref(d), C.byref(out), None) == HM_ERR_INVALID_ARG
        assert "sequence" in L.hm_last_error().decode()
        assert L.hm_pipeline_submit_to_device(None, heic, len(heic), 0, 0, C.byref(d)) == HM_ERR_INVALID_ARG
    finally:
        f.close()


def test_python_entry_points_are_exported(pkg):
    assert callable(pkg.decode_to_tensor) and callable(pkg.decode_batch_to_tensor)
    assert pkg.decode.decode_to_tensor is pkg.decode_to_tensor
