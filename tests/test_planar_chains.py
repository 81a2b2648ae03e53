"""Planar YCbCr targets (HM_OUT_YCBCR_*), CPU side: the product's pipeline search (colour_search.cpp through hm_colour_chain)
against oracle/pipeline_search.py for every request of the matrix, which of them the planar executor accepts, and the numpy
restatement of Op_YCbCr_to_RGB (tests/planar_ref.py) against the oracle's fingerprint-pinned C restatement."""
import ctypes as C
import itertools

import numpy as np
import pytest

import orc
import planar_ref as pr

ps = pr.ps

PROFILES = [None, (2, 2, 2, 0), (1, 1, 1, 1), (0, 1, 13, 1)]  # no nclx, limited BT.601 default, full BT.709, matrix 0 (GBR)
HM_PIPE_PLANAR = 10
HM_ERR_UNSUPPORTED = -2
HM_DETAIL_NO_COLOUR_CHAIN = 2


def desc(capi, chroma, bits, alpha, nclx, target, forced, hdr8, w=64, h=64):
    return capi.ColourDesc(w, h, bits, chroma, 1 if nclx else 0, nclx[0] if nclx else 0, nclx[1] if nclx else 0, nclx[3] if nclx else 0,
                           pr.HM_OUT_YCBCR[target] | (pr.HM_OUT_YCBCR_8BIT if hdr8 else 0), 0, 0, 0, 0, 2 if forced else 0, alpha)


def requests():
    return itertools.product((0, 1, 2, 3), (8, 10, 12), (0, 1), PROFILES, (1, 2, 3), (False, True), (False, True))


def test_product_search_equals_oracle_search_for_planar_targets(pkg):
    """hm_colour_chain() == pipeline_search.chain() op for op, "no chain" included, over {4:0:0, 4:2:0, 4:2:2, 4:4:4} x {8, 10,
    12 bit} x {alpha, none} x 4 profiles x 3 targets x {default, forced bilinear} x {convert_hdr_to_8bit 0 / 1}"""
    capi, L = pkg.capi, pkg.lib()
    names = [n for n, _ in ps.OPS]
    seen = 0
    for chroma, bits, alpha, nclx, target, forced, hdr8 in requests():
        exp = pr.chain_for(chroma, alpha, bits, nclx, target, hdr8, forced)
        d = desc(capi, chroma, bits, alpha, nclx, target, forced, hdr8)
        ops = (C.c_int * 8)()
        cnt = L.hm_colour_chain(C.byref(d), ops, 8)
        key = (chroma, bits, alpha, nclx, target, forced, hdr8)
        if exp is None:
            assert cnt == -1, key
        else:
            assert cnt >= 0 and [names[ops[i]] for i in range(cnt)] == exp, (key, exp)
        seen += 1
    assert seen == 4 * 3 * 2 * 4 * 3 * 2 * 2


def test_known_planar_chains():
    """the chains the issue's table names, from the oracle module"""
    lim = (2, 2, 2, 0)
    assert pr.chain_for(2, 0, 10, lim, 3) == ["Op_YCbCr422_bilinear_to_YCbCr444<uint16_t>"]
    assert pr.chain_for(3, 1, 8, lim, 1) == ["Op_YCbCr444_to_YCbCr420_average<uint8_t>"]
    assert pr.chain_for(2, 0, 10, lim, 1) == ["Op_YCbCr_to_RGB<uint16_t>", "Op_RGB_to_YCbCr<uint16_t>"]  # the float round trip wins the tie
    assert pr.chain_for(2, 0, 10, lim, 1, forced_bilinear=True) == ["Op_YCbCr422_bilinear_to_YCbCr444<uint16_t>", "Op_YCbCr444_to_YCbCr420_average<uint16_t>"]
    assert pr.chain_for(1, 0, 8, (0, 1, 13, 1), 3) == ["Op_YCbCr_to_RGB<uint8_t>", "Op_RGB_to_YCbCr<uint8_t>"]
    assert pr.chain_for(1, 0, 8, (0, 1, 13, 1), 3, forced_bilinear=True) is None
    assert pr.chain_for(0, 0, 8, None, 1) == ["Op_mono_to_YCbCr420"]
    assert pr.chain_for(0, 0, 8, None, 3) == ["Op_mono_to_YCbCr420", "Op_YCbCr420_bilinear_to_YCbCr444<uint8_t>"]
    assert "Op_mono_to_RGB24_32" in pr.chain_for(0, 0, 8, lim, 1)
    assert pr.chain_for(0, 0, 8, None, 1, target_colorspace=ps.CS_MONO) is None  # a monochrome target with a colour chroma


def classify():
    """the requests that must convert (source and target chroma differ): no chain / a chain outside the planar set / inside"""
    none, outside, inside = [], [], []
    for chroma, bits, alpha, nclx, target, forced, hdr8 in requests():
        if chroma == target:
            continue
        chain = pr.chain_for(chroma, alpha, bits, nclx, target, hdr8, forced)
        key = (chroma, bits, alpha, nclx, target, forced, hdr8)
        (none if chain is None else inside if set(chain) <= pr.INSIDE else outside).append((key, chain))
    return none, outside, inside


def test_which_requests_convert(pkg):
    """864 requests: 96 without a chain (all matrix 0 with forced bilinear), 120 whose chain leaves the planar set (all 4:0:0
    sources), 648 inside it - and the product's own answer (hm_colour_pipeline needs no device) for each of them"""
    capi, L = pkg.capi, pkg.lib()
    L.hm_last_error_detail.restype = C.c_int
    none, outside, inside = classify()
    assert (len(none), len(outside), len(inside)) == (96, 120, 648)
    assert all(k[3] and k[3][0] == 0 and k[5] for k, _ in none)
    assert all(k[0] == 0 for k, _ in outside)
    for key, chain in inside:
        assert L.hm_colour_pipeline(C.byref(desc(capi, *key))) == HM_PIPE_PLANAR, (key, L.hm_last_error())
    for key, chain in outside:
        assert L.hm_colour_pipeline(C.byref(desc(capi, *key))) == HM_ERR_UNSUPPORTED, key
        msg = L.hm_last_error().decode()
        assert L.hm_last_error_detail() != HM_DETAIL_NO_COLOUR_CHAIN and all(name in msg for name in chain), (key, msg)
    for key, chain in none:
        assert L.hm_colour_pipeline(C.byref(desc(capi, *key))) == HM_ERR_UNSUPPORTED, key
        assert L.hm_last_error_detail() == HM_DETAIL_NO_COLOUR_CHAIN and "no colour conversion" in L.hm_last_error().decode(), key


def test_planar_codes_are_not_interleaved_formats(pkg):
    L = pkg.lib()
    for code in (0x101, 0x102, 0x103, 0x301, 0x303):
        assert L.hm_out_bytes_per_pixel(code) < 0


@pytest.mark.parametrize("bits", [8, 10, 12])
@pytest.mark.parametrize("chroma", [1, 2, 3])
@pytest.mark.parametrize("nclx", [None, (2, 2, 2, 0), (1, 1, 1, 1), (1, 1, 1, 0), (6, 1, 13, 1), (0, 1, 13, 1), (0, 1, 13, 0), (9, 9, 16, 0)])
def test_numpy_ycbcr_to_rgb_equals_oracle(oracle, bits, chroma, nclx):
    """the numpy Op_YCbCr_to_RGB of planar_ref against orc_ycbcr_to_rgb_float (oracle_colour.c, pinned by the reference
    fingerprints of BASELINE.md), de-interleaved: ties the new restatement to the pinned one"""
    rng = np.random.default_rng(bits * 100 + chroma * 10 + (nclx[0] if nclx else 7))
    w, h = 37, 21
    cw, ch = pr.chroma_size(chroma, w, h)
    bps = 2 if bits > 8 else 1
    maxv = (1 << bits) - 1
    y, cb, cr = orc.alloc_plane(w, h, bps, rng=rng, maxval=maxv), orc.alloc_plane(cw, ch, bps, rng=rng, maxval=maxv), orc.alloc_plane(cw, ch, bps, rng=rng, maxval=maxv)
    fmt = 10 if bits == 8 else 14  # RGB24 for 8 bits, RRGGBB_LE (no depth change) above
    has, m, p, full = (1, nclx[0], nclx[1], nclx[3]) if nclx else (0, 0, 0, 0)
    out, os_ = orc.colour_float(y, cb, cr, w, h, bits, chroma, has, m, p, full, fmt)
    inter = np.ascontiguousarray(out[:h, :w * 3 * bps]).view(pr.dtype_of(bits)).reshape(h, w, 3)
    un = lambda pl, ww, hh: pr._unpadded(pl, ww, hh, bits)  # noqa: E731
    r, g, b = pr.op_ycbcr_to_rgb(un(y, w, h), un(cb, cw, ch), un(cr, cw, ch), bits, chroma, (has, m, p, full))
    assert np.array_equal(inter[:, :, 0], r) and np.array_equal(inter[:, :, 1], g) and np.array_equal(inter[:, :, 2], b)


def test_numpy_average_rules():
    """the odd-edge rules of the averaging ops on a hand-checked plane (chroma_sampling.cc:172-221, 396-420)"""
    p = np.array([[10, 20, 31], [40, 50, 61], [70, 81, 93]], np.uint8)
    assert pr.op_average_420(p).tolist() == [[(10 + 20 + 40 + 50 + 2) // 4, (31 + 61 + 1) // 2], [(70 + 81 + 1) // 2, 93]]
    out, undefined = pr.op_average_422(p)
    assert out.tolist() == [[15, 31], [45, 61], [76, 93]] and undefined == (2, 1)
    assert pr.op_average_422(p[:, :2])[1] is None


def test_no_chain_detail_also_for_interleaved_targets(pkg):
    """"no chain" carries HM_DETAIL_NO_COLOUR_CHAIN for every target, the interleaved RGB ones included (matrix 11: every
    YCbCr -> RGB op refuses): the facade turns it into heif_suberror_Unsupported_color_conversion, where the interleaved
    targets used to report Unsupported_codec.  Status and message are what they were."""
    capi, L = pkg.capi, pkg.lib()
    L.hm_last_error_detail.restype = C.c_int
    d = capi.ColourDesc(64, 64, 8, 3, 1, 11, 1, 1, capi.HM_OUT_RGB, 0, 0, 0, 0, 0, 0)
    assert L.hm_colour_pipeline(C.byref(d)) == HM_ERR_UNSUPPORTED
    assert L.hm_last_error_detail() == HM_DETAIL_NO_COLOUR_CHAIN and L.hm_last_error().decode().startswith("no colour conversion")
