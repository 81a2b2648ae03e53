"""The alpha step (hm_device_alpha), the part that needs no GPU: what the model (tests/alpha_ref.py) is for - premultiplied sums keep
the colour of a cut-out up to its edge where plain sums darken it, a matte over an opaque picture is the picture, a matte over a
transparent one the background -, hm_alpha_dest_format over every target, mode and out_bits, the refusals that are decided on the
host, the ABI and the Python argument."""
import ctypes as C
import inspect

import numpy as np
import pytest

import alpha_ref
import view_filters_ref
import view_ref

HM_ERR_INVALID_ARG, HM_ERR_UNSUPPORTED = -1, -2
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 13, 14, 15
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
STRAIGHT, PREMULTIPLIED, MATTE = alpha_ref.STRAIGHT, alpha_ref.PREMULTIPLIED, alpha_ref.MATTE
TRIANGLE = view_ref.TRIANGLE
ONE, ZERO = [1.0] * 4, [0.0] * 4
FAKE = 0x10000000  # (never dereferenced on the host: every call below is refused before a device is looked for)
NEW_SYMBOLS = ("hm_decode_item_to_device_alpha", "hm_pipeline_submit_to_device_alpha", "hm_alpha_to_tensor", "hm_alpha_dest_format")


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def L(capi):
    return capi.image_lib()


def alpha_of(capi, mode, background=(0, 0, 0, 0), reserved=(0, 0, 0)):
    return capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*background), (C.c_int32 * 3)(*reserved))


def cut_out(w, h, seed):
    """colour 200 where alpha > 0, colour 0 where alpha == 0: a disc with a soft rim on a transparent ground"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.hypot(xx - w / 2.0, yy - h / 2.0)
    a = np.clip((min(w, h) * 0.4 - d) * 40.0, 0, 255).astype(np.uint8)
    a[(a > 0) & (rng.random((h, w)) < 0.2)] = 1  # (the smallest alpha that still counts)
    px = np.zeros((h, w, 4), np.uint8)
    px[..., 3] = a
    px[..., :3][a > 0] = 200
    return px


@pytest.mark.parametrize("size", [(23, 17), (64, 48), (1, 1)])
def test_premultiplied_sums_leave_no_fringe(size):
    """STRAIGHT under the triangle filter: exactly 200 wherever S_a > 0 - the quotient of sums of at most 514 x 514 products errs by far
    less than 0.01 code -, and 0 where no weight meets a pixel with alpha.  The plain resample of the same picture darkens the rim."""
    px = cut_out(97, 61, 5)
    assert (px[..., 3] == 0).any() and (px[..., 3] == 255).any() and (px[..., 3] == 1).any()
    view = (None, size, TRIANGLE)
    got, S, Sa = alpha_ref.render(px, 8, STRAIGHT, None, view, view_ref.taps, np.uint8, ONE, ZERO)
    assert got.shape == (size[1], size[0], 4)
    assert (Sa > 0).any()
    assert (got[..., :3][Sa > 0] == 200).all()
    assert (got[..., :3][~(Sa > 0)] == 0).all()
    r = S[Sa > 0] / Sa[Sa > 0][:, None]
    assert np.abs(r - 200.0).max() < 0.01
    plain = view_ref.to_integer(view_ref.resample(px, None, size, TRIANGLE), 255)
    assert np.array_equal(plain[..., 3], got[..., 3])  # the alpha element is what it is without the step
    assert (plain[..., :3][Sa > 0] < 200).any(), "the picture has no rim that plain sums darken"


def test_a_matte_of_an_opaque_picture_is_the_plain_resample():
    rng = np.random.default_rng(11)
    px = rng.integers(0, 256, (23, 37, 4), dtype=np.uint8)
    px[..., 3] = 255
    for filt in (TRIANGLE, view_filters_ref.CUBIC, view_filters_ref.LANCZOS3):
        view = ((1, 2, 35, 20), (11, 7), filt)
        got, _, Sa = alpha_ref.render(px, 8, MATTE, (255, 255, 255), view, view_filters_ref.taps, np.uint8, ONE, ZERO)
        plain = view_filters_ref.to_integer(view_filters_ref.resample(px[..., :3], view[0], view[1], filt), 255)
        assert got.shape == (7, 11, 3) and np.array_equal(got, plain), filt
    got, _, _ = alpha_ref.render(px, 8, MATTE, (255, 255, 255), None, view_filters_ref.taps, np.uint8, ONE, ZERO)
    assert np.array_equal(got, px[..., :3])


def test_a_matte_of_a_transparent_picture_is_the_background():
    rng = np.random.default_rng(12)
    px = rng.integers(0, 256, (23, 37, 4), dtype=np.uint8)
    px[..., 3] = 0
    bg = (255, 17, 0)
    for view in (None, (None, (11, 7), TRIANGLE), (None, (11, 7), view_filters_ref.LANCZOS3), (None, (50, 9), view_ref.NEAREST), ((3, 4, 9, 8), None, TRIANGLE)):
        got, _, _ = alpha_ref.render(px, 8, MATTE, bg, view, view_filters_ref.taps, np.uint8, ONE, ZERO)
        assert (got == np.array(bg, np.uint8)).all(), view
    px16 = rng.integers(0, 4096, (9, 13, 4), dtype=np.uint16)
    px16[..., 3] = 0
    got, _, _ = alpha_ref.render(px16, 12, MATTE, (4095, 1, 2048), (None, (5, 4), TRIANGLE), view_filters_ref.taps, np.float32, [2.0, 0.5, 1.0, 1.0], [1.0, 0.0, -3.0, 0.0])
    assert (got == np.array([8191.0, 0.5, 2045.0], np.float32)).all()


def test_straight_without_sums_is_the_picture():
    rng = np.random.default_rng(13)
    px = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    for view in (None, (None, (30, 4), view_ref.NEAREST), ((3, 4, 9, 5), None, TRIANGLE)):
        got, _, _ = alpha_ref.render(px, 8, STRAIGHT, None, view, view_ref.taps, np.uint8, ONE, ZERO)
        assert np.array_equal(got, view_ref.resample(px, view[0] if view else None, view[1] if view else None, view_ref.NEAREST))


def test_dest_format_over_all_targets_modes_and_out_bits(capi, L):
    def tone(out_bits):
        return capi.DeviceTone(1, out_bits, 1000.0, 203.0, 10000.0, 0.0, (C.c_int32 * 2)(0, 0))
    for fmt in (0, 0x101, 0x102, 0x103, 0x301, 3, RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE, 99):
        for mode in (STRAIGHT, PREMULTIPLIED, MATTE):
            for out_bits in (None, 0, 8):
                tn = tone(out_bits) if out_bits is not None else None
                got = L.hm_alpha_dest_format(fmt, C.byref(alpha_of(capi, mode)), C.byref(tn) if tn is not None else None)
                what = (fmt, mode, out_bits, L.hm_last_error().decode())
                if fmt not in (RGBA, RRGGBBAA_LE):
                    assert got < 0, what
                    assert got == (HM_ERR_INVALID_ARG if fmt in (RGB, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE) else HM_ERR_UNSUPPORTED), what
                elif mode == PREMULTIPLIED and tn is not None:
                    assert got == HM_ERR_INVALID_ARG, what
                elif mode != MATTE:
                    assert got == fmt, what
                elif out_bits == 8:
                    assert got == RGB, what
                else:
                    assert got == (RGB if fmt == RGBA else RRGGBB_LE), what
    assert L.hm_alpha_dest_format(RGBA, None, None) == HM_ERR_INVALID_ARG
    for a in (alpha_of(capi, 0), alpha_of(capi, 4), alpha_of(capi, MATTE, reserved=(0, 0, 1)), alpha_of(capi, STRAIGHT, (0, 1, 0, 0)), alpha_of(capi, PREMULTIPLIED, (9, 0, 0, 0)),
              alpha_of(capi, MATTE, (0, 0, 0, 1)), alpha_of(capi, MATTE, (0, 256, 0, 0))):
        assert L.hm_alpha_dest_format(RGBA, C.byref(a), None) == HM_ERR_INVALID_ARG, L.hm_last_error().decode()
    assert L.hm_alpha_dest_format(RRGGBBAA_LE, C.byref(alpha_of(capi, MATTE, (0, 65535, 0, 0))), None) == RRGGBB_LE  # (judged against the image's depth later)


def test_refusals_decided_on_the_host(capi, L):
    """hm_alpha_to_tensor refuses these before it looks for a device"""
    def call(fmt, bits, a, dtype=F32, layout=CHW, lt=None, tn=None, view=None, w=16, h=8):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = FAKE, 1 << 30, layout, dtype
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        rc = L.hm_alpha_to_tensor(fmt, bits, w, h, FAKE, w * 8, C.byref(view) if view is not None else None, C.byref(lt) if lt is not None else None,
                                  C.byref(tn) if tn is not None else None, C.byref(a) if a is not None else None, C.byref(d), None)
        return rc, L.hm_last_error().decode()

    def light(to_transfer=8, from_transfer=13, from_primaries=1):
        return capi.DeviceLight(from_transfer, from_primaries, to_transfer, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))

    def tone(out_bits=0):
        return capi.DeviceTone(1, out_bits, 1000.0, 203.0, 10000.0, 0.0, (C.c_int32 * 2)(0, 0))
    cases = [
        (call(RGBA, 8, None), -1, "null"),
        (call(RGBA, 8, alpha_of(capi, 7)), -1, "mode"),
        (call(RGBA, 8, alpha_of(capi, STRAIGHT, reserved=(1, 0, 0))), -1, "reserved"),
        (call(RGBA, 8, alpha_of(capi, STRAIGHT, (1, 0, 0, 0))), -1, "background"),
        (call(RGBA, 8, alpha_of(capi, MATTE, (0, 0, 0, 5))), -1, "background[3]"),
        (call(RGBA, 8, alpha_of(capi, MATTE, (0, 0, 300, 0))), -1, "peak"),
        (call(RRGGBBAA_LE, 10, alpha_of(capi, MATTE, (0, 0, 1024, 0))), -1, "peak"),
        (call(RGB, 8, alpha_of(capi, STRAIGHT)), -1, "three-channel"),
        (call(RRGGBB_LE, 10, alpha_of(capi, MATTE)), -1, "three-channel"),
        (call(RRGGBBAA_BE, 10, alpha_of(capi, STRAIGHT), dtype=U16, layout=HWC), -1, "_LE"),
        (call(0x101, 8, alpha_of(capi, STRAIGHT)), -2, "planar"),
        (call(0, 8, alpha_of(capi, MATTE)), -2, "planar"),
        (call(RGBA, 8, alpha_of(capi, PREMULTIPLIED), lt=light(16), tn=tone()), -1, "tone"),
        (call(RGBA, 8, alpha_of(capi, PREMULTIPLIED), lt=light(13)), -1, "re-encodes"),
        (call(RGBA, 8, alpha_of(capi, MATTE), tn=tone()), -1, "null light step"),
        (call(RRGGBBAA_LE, 10, alpha_of(capi, STRAIGHT), lt=light(13, 16, 9), tn=tone(8), dtype=U8), -2, "four-channel"),
        (call(RRGGBBAA_LE, 10, alpha_of(capi, MATTE), lt=light(13, 16, 9), tn=tone(8), dtype=U16), -1, "HM_DEV_U16"),
        (call(RRGGBBAA_LE, 13, alpha_of(capi, MATTE), lt=light(8, 16, 9)), -2, "bits"),
        (call(RRGGBBAA_LE, 8, alpha_of(capi, MATTE)), -2, "bits"),
        (call(RGBA, 8, alpha_of(capi, MATTE), dtype=U16), -1, "dtype"),  # the sibling's own integer type
        (call(RGBA, 8, alpha_of(capi, MATTE), lt=light(8), dtype=U8), -1, "float dtype"),
        (call(RGBA, 8, alpha_of(capi, STRAIGHT), lt=light(8, 0, 0)), -1, "from_transfer"),
        (call(RGBA, 8, alpha_of(capi, STRAIGHT), view=capi.DeviceView(0, 0, 0, 0, 0, 4, 0)), -1, "view"),
    ]
    for (rc, msg), status, word in cases:
        assert rc == status and word in msg, (rc, msg, status, word)
    # a matte's destination is sized as the three-channel sibling's: one byte less than that is refused, by that name
    d = capi.DeviceDest()
    d.layout, d.dtype = HWC, U8
    need = L.hm_device_dest_bytes(RGB, 16, 8, C.byref(d))
    assert need == 16 * 8 * 3
    d.ptr, d.len = FAKE, need - 1
    a = alpha_of(capi, MATTE, (255, 255, 255, 0))
    assert L.hm_alpha_to_tensor(RGBA, 8, 16, 8, FAKE, 64, None, None, None, C.byref(a), C.byref(d), None) == -1 and "len" in L.hm_last_error().decode()


def test_abi_and_python_argument(pkg, capi, L):
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(capi.DeviceAlpha) == 24
    decode = pkg.decode
    assert decode._alpha_of(None, RGBA) == (None, 4) and decode._alpha_of(False, RGB) == (None, 3)
    for name, mode in (("straight", STRAIGHT), ("premultiplied", PREMULTIPLIED), ("Straight", STRAIGHT)):
        d, c = decode._alpha_of(name, RGBA)
        assert (d.mode, tuple(d.background), tuple(d.reserved), c) == (mode, (0, 0, 0, 0), (0, 0, 0), 4)
    d, c = decode._alpha_of(dict(mode="matte", background=(255, 128, 0)), RGBA)
    assert (d.mode, tuple(d.background), tuple(d.reserved), c) == (MATTE, (255, 128, 0, 0), (0, 0, 0), 3)
    assert decode._alpha_of(dict(mode="matte", background=(1023, 0, 0)), RRGGBBAA_LE)[1] == 3
    assert decode._alpha_of(dict(mode="premultiplied"), RRGGBBAA_LE)[1] == 4
    for bad in ("matte", "over", 3, True, dict(mode="matte"), dict(mode="matte", background=(1, 2)), dict(mode="matte", background=(1, 2, -1)),
                dict(mode="matte", background=(1, 2, 0.5)), dict(mode="straight", background=(1, 2, 3)), dict(mode="matte", background=(0, 0, 0), colour=1),
                dict(background=(0, 0, 0)), dict(mode=3)):
        with pytest.raises(ValueError):
            decode._alpha_of(bad, RGBA)
    for fmt in (RGB, RRGGBB_LE, RRGGBB_BE):  # a three-channel out_format carries no alpha
        with pytest.raises(ValueError, match="four-channel"):
            decode._alpha_of("straight", fmt)
    for fn in (decode.decode_to_tensor, decode.decode_batch_to_tensor):
        assert inspect.signature(fn).parameters["alpha"].default is None
    with pytest.raises(ValueError, match="four-channel"):
        decode.decode_to_tensor(b"", out_format="rgb", alpha="straight")
