"""Sequences under a view (hm_decode_frames_to_device_view, decode_sequence_to_tensor), the part that needs no GPU: the export and
its declaration, the argument checks, and every refusal that is decided before the device is needed - each with a message that
names the problem."""
import ctypes as C
import os

import pytest

import heifwriter
import moovwriter
import synthutil

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED = -1, -2
RGB, RRGGBB_BE = 10, 12
HWC, CHW = 0, 1
U8, U16, F32 = 0, 1, 3
TRIANGLE, NEAREST, CUBIC = 0, 1, 16
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused before the device is asked)
W, H, N = 200, 136, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


@pytest.fixture(scope="module")
def movie():
    return moovwriter.write_movie([synthutil.picture(48000 + i, width=W, height=H, qp=30) for i in range(N)], (W, H))


@pytest.fixture(scope="module")
def still():
    return heifwriter.write_heic([synthutil.picture(48100, width=64, height=64)], (64, 64))


def call(capi, L, data, frames, fmt=RGB, view=(0, 0, 0, 0, 50, 37, TRIANGLE), layout=CHW, dtype=F32, ext_dst=None, count=None, null=()):
    """hm_decode_frames_to_device_view with destinations at a fake address: (status, message, failed_frame)"""
    n = len(frames)
    h = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(h)) == 0
    try:
        ids = (C.c_uint32 * max(n, 1))(*frames)
        dests = (capi.DeviceDest * max(n, 1))()
        for d in dests:
            d.ptr, d.len, d.layout, d.dtype = FAKE, 1 << 30, layout, dtype
            for c in range(4):
                d.scale[c] = 1.0
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, ext_dst, 0, 0, 0, 0)
        out = (capi.Decoded * max(n, 1))()
        failed = C.c_int32(-2)
        v = capi.DeviceView(*view)
        rc = L.hm_decode_frames_to_device_view(None if "f" in null else h, None if "frames" in null else ids, n if count is None else count,
                                               None if "params" in null else C.byref(prm), C.byref(v), None if "dests" in null else dests,
                                               None if "out" in null else out, C.byref(failed))
        return rc, L.hm_last_error().decode(), failed.value
    finally:
        L.hm_file_close(h)


def test_the_entry_point_is_exported_declared_and_bound(hm, capi, L):
    assert hasattr(hm, "hm_decode_frames_to_device_view")
    with open(os.path.join(ROOT, "include", "heif_mi355x.h")) as fh:
        assert "HM_API int hm_decode_frames_to_device_view(" in fh.read()
    assert len(L.hm_decode_frames_to_device_view.argtypes) == 8


def test_null_arguments(capi, L, movie):
    for what in ("f", "frames", "params", "dests", "out"):
        rc, msg, failed = call(capi, L, movie, [1, 2], null=(what,))
        assert rc == HM_ERR_INVALID_ARG and "null" in msg and failed == -1, (what, rc, msg)


def test_frame_counts_and_ids(capi, L, movie):
    for count in (0, -1):
        rc, msg, _ = call(capi, L, movie, [1], count=count)
        assert rc == HM_ERR_INVALID_ARG and "count" in msg, (count, msg)
    for frames, k in (([0], 0), ([1, N + 1], 1), ([2, 1, 0], 2)):
        rc, msg, failed = call(capi, L, movie, frames)
        assert rc == HM_ERR_INVALID_ARG and f"frames[{k}] = {frames[k]}" in msg and f"1..{N}" in msg and failed == k, (frames, msg, failed)


@pytest.mark.parametrize("name,kw,status,word", [
    ("planar_target", dict(fmt=0x101, layout=HWC, dtype=U8), HM_ERR_UNSUPPORTED, "not supported with a device destination"),
    ("as_decoded_target", dict(fmt=0, layout=HWC, dtype=U8), HM_ERR_UNSUPPORTED, "not supported with a device destination"),
    ("big_endian_resampled", dict(fmt=RRGGBB_BE, layout=HWC, dtype=U16), HM_ERR_INVALID_ARG, "_LE"),
    ("unknown_filter", dict(view=(0, 0, 0, 0, 50, 37, 2)), HM_ERR_INVALID_ARG, "unknown filter 2"),
    ("reduction_beyond_the_filter", dict(view=(0, 0, 0, 0, 1, 1, CUBIC)), HM_ERR_INVALID_ARG, "more than 128"),
    ("output_extent_0x5", dict(view=(0, 0, 0, 0, 0, 5, TRIANGLE)), HM_ERR_INVALID_ARG, "output width 0"),
    ("crop_outside", dict(view=(150, 100, 60, 30, 16, 16, TRIANGLE)), HM_ERR_INVALID_ARG, "not inside"),
    ("ext_dst", dict(ext_dst=FAKE), HM_ERR_INVALID_ARG, "ext_dst"),
])
def test_refusals_decided_before_the_device_is_needed(capi, L, movie, name, kw, status, word):
    rc, msg, failed = call(capi, L, movie, [1, 3], **kw)
    assert rc == status and word in msg, (name, rc, msg)
    if name in ("unknown_filter", "reduction_beyond_the_filter", "output_extent_0x5", "crop_outside", "big_endian_resampled"):
        assert failed == 0  # (the view is judged frame by frame: the first frame already fails)


def test_a_short_destination_names_its_frame(capi, L, movie):
    n = 2
    h = C.c_void_p()
    assert L.hm_file_open(movie, len(movie), C.byref(h)) == 0
    try:
        dests = (capi.DeviceDest * n)()
        need = 50 * 37 * 3 * 4
        for k, d in enumerate(dests):
            d.ptr, d.len, d.layout, d.dtype = FAKE, need - (1 if k == 1 else 0), CHW, F32
        prm = capi.DecodeParams(RGB, 2, 0, 0, None, None, 0, 0, 0, 0)
        out = (capi.Decoded * n)()
        failed = C.c_int32(-2)
        v = capi.DeviceView(0, 0, 0, 0, 50, 37, TRIANGLE)
        rc = L.hm_decode_frames_to_device_view(h, (C.c_uint32 * n)(1, 2), n, C.byref(prm), C.byref(v), dests, out, C.byref(failed))
        assert rc == HM_ERR_INVALID_ARG and "len" in L.hm_last_error().decode() and failed.value == 1
    finally:
        L.hm_file_close(h)


def test_a_still_image_is_not_a_sequence(capi, L, still):
    rc, msg, failed = call(capi, L, still, [1])
    assert rc == HM_ERR_INVALID_ARG and "not an image sequence" in msg and failed == -1


def test_python_argument_checks(pkg, movie, still):
    import torch
    assert pkg.decode_sequence_to_tensor is pkg.decode.decode_sequence_to_tensor
    for frames, word in (([1, 0], r"frames\[1\] = 0"), ([N + 1], r"frames\[0\] = 4"), ([1, 2.5], r"frames\[1\]"), (["2"], r"frames\[0\]"), ([], "empty")):
        with pytest.raises(ValueError, match=word):
            pkg.decode_sequence_to_tensor(movie, frames=frames, size=(32, 32))
    with pytest.raises(ValueError, match="shape"):
        pkg.decode_sequence_to_tensor(movie, frames=range(1, N + 1, 2), size=(32, 24), out=torch.empty((2, 3, 24, 33)))
    with pytest.raises(ValueError, match="shape"):
        pkg.decode_sequence_to_tensor(movie, size=(32, 24), out=torch.empty((2, 3, 24, 32)))  # (all three frames asked for)
    with pytest.raises(ValueError, match="filter"):
        pkg.decode_sequence_to_tensor(movie, size=(32, 24), filter="lanczos")
    with pytest.raises(pkg.capi.HmError, match="not an image sequence"):
        pkg.decode_sequence_to_tensor(still, size=(32, 24))
