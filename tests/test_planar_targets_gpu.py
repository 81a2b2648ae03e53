"""GPU parity of the planar YCbCr targets (HM_OUT_YCBCR_*): hm_colour_convert_planar and the decode entry points against the
numpy restatement of the reference's chain (tests/planar_ref.py; the chain from oracle/pipeline_search.py).  Bit-exact, every
sample, except the one chroma sample per plane Op_YCbCr444_to_YCbCr422_average leaves unwritten for an odd width."""
import ctypes as C

import numpy as np
import pytest

import orc
import planar_ref as pr
from test_planar_chains import PROFILES, classify

pytestmark = pytest.mark.gpu

HM_ERR_UNSUPPORTED = -2


def _to_device(arr, L):
    import torch
    h, w = arr.shape
    bps = arr.dtype.itemsize
    stride = L.hm_plane_stride(w, bps)
    buf = np.zeros((max(64, (h + 1) & ~1), stride), np.uint8)
    buf[:h, :w * bps] = np.ascontiguousarray(arr).view(np.uint8).reshape(h, w * bps)
    return torch.from_numpy(buf).to("cuda:0"), stride


def _from_device(t, w, h, bits):
    bps = 2 if bits > 8 else 1
    return np.ascontiguousarray(t.cpu().numpy()[:h, :w * bps]).view(pr.dtype_of(bits)).reshape(h, w)


def random_planes(rng, w, h, bits, chroma, alpha):
    cw, ch = pr.chroma_size(chroma, w, h)
    dt, hi = pr.dtype_of(bits), 1 << bits
    P = {"y": rng.integers(0, hi, (h, w), dtype=dt)}
    if chroma:
        P["cb"], P["cr"] = rng.integers(0, hi, (ch, cw), dtype=dt), rng.integers(0, hi, (ch, cw), dtype=dt)
    if alpha:
        P["a"] = rng.integers(0, hi, (h, w), dtype=dt)
    return P


def convert_gpu(pkg, P, bits, chroma, nclx, target, forced=False, hdr8=False, flags=0):
    """hm_colour_convert_planar on the planes of P -> {"y", "cb", "cr"[, "a"]} of the target's size; raises capi.HmError"""
    import torch
    capi, L = pkg.capi, pkg.lib()
    h, w = P["y"].shape
    alpha = "a" in P
    out_bits = 8 if hdr8 else bits
    tcw, tch = pr.chroma_size(target, w, h)
    obps = 2 if out_bits > 8 else 1
    src, dst = capi.Planes(), capi.Planes()
    keep = []
    for c, k in enumerate(("y", "cb", "cr", "a")):
        if k in P:
            t, s = _to_device(P[k], L)
            keep.append(t)
            src.plane[c], src.stride[c] = t.data_ptr(), s
    outs = {}
    for c, k in enumerate(("y", "cb", "cr", "a")):
        if k == "a" and not alpha:
            continue
        pw, ph = (w, h) if k in ("y", "a") else (tcw, tch)
        s = L.hm_plane_stride(pw, obps)
        t = torch.full((max(64, (ph + 1) & ~1), s), 0xA5, dtype=torch.uint8, device="cuda:0")
        outs[k] = (t, pw, ph)
        dst.plane[c], dst.stride[c] = t.data_ptr(), s
    d = capi.ColourDesc(w, h, bits, chroma, 1 if nclx else 0, nclx[0] if nclx else 0, nclx[1] if nclx else 0, nclx[3] if nclx else 0,
                        pr.HM_OUT_YCBCR[target] | (pr.HM_OUT_YCBCR_8BIT if hdr8 else 0),
                        src.stride[0], src.stride[1], src.stride[2], 0, 2 if forced else 0, 1 if alpha else 0)
    stream = torch.cuda.current_stream().cuda_stream
    capi.check(L.hm_colour_convert_planar(C.byref(d), C.byref(src), 0, C.byref(dst), flags, stream))
    torch.cuda.synchronize()
    return {k: _from_device(t, pw, ph, out_bits) for k, (t, pw, ph) in outs.items()}


def expect(P, bits, chroma, nclx, target, forced=False, hdr8=False):
    chain = pr.chain_for(chroma, "a" in P, bits, nclx, target, hdr8, forced)
    assert chain is not None
    out, obits, ochroma, undefined = pr.run_chain(chain, P, bits, chroma, nclx, target, 8 if hdr8 else bits, forced)
    assert ochroma == target and obits == (8 if hdr8 else bits)
    return out, undefined, chain


def assert_same(got, exp, undefined, key):
    assert set(got) == set(exp), key
    assert len(undefined) <= 2, key
    for k in exp:
        g, e = got[k].copy(), exp[k].copy()
        assert g.shape == e.shape and g.dtype == e.dtype, (key, k, g.shape, e.shape)
        for name, row, col in undefined:
            if name == k:
                g[row, col] = e[row, col] = 0
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)
            raise AssertionError(f"{key} plane {k}: {len(bad)} samples differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]} expected {e[tuple(bad[0])]}")


def test_every_request_of_the_matrix(pkg):
    """864 requests (4 profiles x 3 depths x alpha x 9 source / target pairs x convert_hdr_to_8bit x options) at 65 x 33: the three
    sets come from oracle/pipeline_search.py at run time.  Inside the planar set: bit-exact, no refusal; outside: HM_ERR_UNSUPPORTED
    naming the chain; no chain: the conversion error."""
    capi, L = pkg.capi, pkg.lib()
    L.hm_last_error_detail.restype = C.c_int
    none, outside, inside = classify()
    assert len(none) + len(outside) + len(inside) == 864 and len(outside) <= 120
    rng = np.random.default_rng(20261016)
    w, h = 65, 33
    for key, chain in inside:
        chroma, bits, alpha, nclx, target, forced, hdr8 = key
        P = random_planes(rng, w, h, bits, chroma, alpha)
        exp, undefined, _ = expect(P, bits, chroma, nclx, target, forced, hdr8)
        got = convert_gpu(pkg, P, bits, chroma, nclx, target, forced, hdr8)  # (a refusal raises)
        assert not undefined or (target == 2 and any("422_average" in n for n in chain)), key
        assert_same(got, exp, undefined, key)
    for key, chain in outside:
        chroma, bits, alpha, nclx, target, forced, hdr8 = key
        with pytest.raises(capi.HmError) as e:
            convert_gpu(pkg, random_planes(rng, 16, 16, bits, chroma, alpha), bits, chroma, nclx, target, forced, hdr8)
        assert e.value.status == HM_ERR_UNSUPPORTED and all(n in str(e.value) for n in chain), (key, str(e.value))
        assert L.hm_last_error_detail() != capi.HM_DETAIL_NO_COLOUR_CHAIN
    for key, chain in none:
        chroma, bits, alpha, nclx, target, forced, hdr8 = key
        with pytest.raises(capi.HmError) as e:
            convert_gpu(pkg, random_planes(rng, 16, 16, bits, chroma, alpha), bits, chroma, nclx, target, forced, hdr8)
        assert e.value.status == HM_ERR_UNSUPPORTED and "no colour conversion" in str(e.value), key
        assert L.hm_last_error_detail() == capi.HM_DETAIL_NO_COLOUR_CHAIN, key


# one request per kernel and edge rule: (chroma, bits, alpha, nclx, target, forced, hdr8)
SIZE_CASES = [
    (3, 8, 1, (2, 2, 2, 0), 1, False, False),   # average 4:2:0, alpha passed through
    (3, 10, 0, (1, 1, 1, 1), 2, False, False),  # average 4:2:2, 16-bit samples
    (3, 8, 0, None, 2, False, False),           # average 4:2:2, 8 bit
    (2, 10, 0, (2, 2, 2, 0), 1, False, False),  # the float round trip 4:2:2 -> 4:2:0, limited range
    (1, 8, 0, (1, 1, 1, 1), 2, False, False),   # the float round trip 4:2:0 -> 4:2:2
    (1, 8, 0, (0, 1, 13, 1), 3, False, False),  # GBR round trip
    (1, 8, 0, (2, 2, 2, 0), 3, False, False),   # bilinear up
    (2, 12, 1, (2, 2, 2, 0), 1, True, True),    # bilinear up, average down, 8-bit output, alpha through the depth change
    (0, 8, 0, None, 3, False, False),           # neutral chroma, bilinear up
    (0, 10, 1, None, 1, False, False),          # neutral chroma, 16-bit samples
]


@pytest.mark.parametrize("w,h", [(37, 21), (1, 1), (2, 3), (65, 33), (4032, 3024)])
@pytest.mark.parametrize("case", SIZE_CASES)
def test_sizes(pkg, case, w, h):
    chroma, bits, alpha, nclx, target, forced, hdr8 = case
    rng = np.random.default_rng(w * 131 + h + bits)
    P = random_planes(rng, w, h, bits, chroma, alpha)
    exp, undefined, chain = expect(P, bits, chroma, nclx, target, forced, hdr8)
    got = convert_gpu(pkg, P, bits, chroma, nclx, target, forced, hdr8)
    assert_same(got, exp, undefined, (case, w, h, chain))


@pytest.mark.parametrize("w,h", [(37, 21), (1, 1), (640, 481), (4032, 3024)])
@pytest.mark.parametrize("case", [(2, 10, 1, (2, 2, 2, 0), 1), (1, 8, 0, (1, 1, 1, 1), 2), (2, 8, 0, None, 1), (1, 12, 0, (2, 2, 2, 0), 2),
                                  (3, 8, 0, (0, 1, 13, 1), 1), (1, 10, 0, (0, 1, 13, 0), 3), (2, 8, 1, (0, 1, 13, 1), 1)])
def test_fused_round_trip_equals_op_by_op(pkg, case, w, h):
    """Op_YCbCr_to_RGB -> Op_RGB_to_YCbCr as one kernel == the two kernels over planar RGB (HM_PLANAR_UNFUSED), on the GPU"""
    chroma, bits, alpha, nclx, target = case
    assert [n.split("<")[0] for n in pr.chain_for(chroma, alpha, bits, nclx, target)] == ["Op_YCbCr_to_RGB", "Op_RGB_to_YCbCr"]
    rng = np.random.default_rng(w + 7 * h + bits + target)
    P = random_planes(rng, w, h, bits, chroma, alpha)
    fused = convert_gpu(pkg, P, bits, chroma, nclx, target)
    unfused = convert_gpu(pkg, P, bits, chroma, nclx, target, flags=pkg.capi.HM_PLANAR_UNFUSED)
    for k in fused:
        assert np.array_equal(fused[k], unfused[k]), (case, w, h, k)
    if w * h < 1 << 20:
        exp, undefined, _ = expect(P, bits, chroma, nclx, target)
        assert_same(unfused, exp, undefined, (case, w, h))


def test_alpha_of_another_depth_is_refused(pkg):
    """Op_RGB_to_YCbCr returns no image for an alpha plane of another depth (rgb2yuv.cc:111-113): the conversion error"""
    import torch
    capi, L = pkg.capi, pkg.lib()
    L.hm_last_error_detail.restype = C.c_int
    rng = np.random.default_rng(5)
    P = random_planes(rng, 32, 16, 10, 2, 0)
    src, dst = capi.Planes(), capi.Planes()
    keep = []
    for c, k in enumerate(("y", "cb", "cr")):
        t, s = _to_device(P[k], L)
        keep.append(t)
        src.plane[c], src.stride[c] = t.data_ptr(), s
    a, s = _to_device(rng.integers(0, 256, (16, 32), dtype=np.uint8), L)
    src.plane[3], src.stride[3] = a.data_ptr(), s
    outs = [torch.zeros((64, 256), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    for c in range(4):
        dst.plane[c], dst.stride[c] = outs[c].data_ptr(), 256
    d = capi.ColourDesc(32, 16, 10, 2, 1, 2, 2, 0, capi.HM_OUT_YCBCR_420, src.stride[0], src.stride[1], src.stride[2], 0, 0, 1)
    rc = L.hm_colour_convert_planar(C.byref(d), C.byref(src), 8, C.byref(dst), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == HM_ERR_UNSUPPORTED and L.hm_last_error_detail() == capi.HM_DETAIL_NO_COLOUR_CHAIN


# ---- end to end ------------------------------------------------------------------------------------------------------
# Expected = the ORACLE's decode of the native planes (scalar executors on the parser's command stream, pasted by the oracle's
# paste as the existing native-planar tests obtain them: pipeline.cpu_decode) and the profile the oracle reads off the stream,
# pushed through the numpy chain the oracle's pipeline search names.  Nothing of the expectation comes from the product's decode.
import os

import hevcutil
import heifwriter
import pipeline
import synthutil
from test_facade_gpu import _decode as facade_decode
from test_facade_gpu import Err, api  # noqa: F401  (api: the facade fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA_URN = "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"
CS_YCBCR, CS_RGB, CS_UNDEFINED = 0, 1, 99
CH_Y, CH_CB, CH_CR, CH_ALPHA = 0, 1, 2, 6
SUBERROR_UNSUPPORTED_COLOR_CONVERSION = 3003


def oracle_native(hm, tiles, tile_w, tile_h, w, h, cols, is_grid, alpha_pic=None):
    """-> (planes of the decoded image, bits, chroma, nclx or None) by the oracle alone"""
    _, info = orc.oracle_decode(hevcutil.parse(hm, tiles[0]), 3)
    bits, cf = info["bit_depth"], info["chroma"]
    if cf == 0:  # (cpu_decode pastes three planes: a monochrome canvas is pasted here; full-range tiles, no rescale)
        y = np.zeros((h, w), pr.dtype_of(bits))
        for i, t in enumerate(tiles):
            ty = orc.oracle_decode(hevcutil.parse(hm, t), 3)[0][0][:tile_h, :tile_w]
            x0, y0 = (i % cols) * tile_w, (i // cols) * tile_h
            y[y0:y0 + tile_h, x0:x0 + tile_w] = ty[:h - y0, :w - x0]
        P = {"y": y}
    else:
        _, _, canv = pipeline.cpu_decode(hm, tiles, tile_w, tile_h, w, h, cols, is_grid, 10, has_alpha=alpha_pic is not None)
        cw, ch = pr.chroma_size(cf, w, h)
        P = {"y": pr._unpadded(canv[0], w, h, bits), "cb": pr._unpadded(canv[1], cw, ch, bits), "cr": pr._unpadded(canv[2], cw, ch, bits)}
    if alpha_pic is not None:
        P["a"] = orc.oracle_decode(hevcutil.parse(hm, alpha_pic), 3)[0][0][:h, :w].astype(pr.dtype_of(bits))
    nclx = None if is_grid else (info["matrix"], info["primaries"], 2, info["full_range"])
    return P, bits, cf, nclx


def oracle_expect(hm, tiles, tile_w, tile_h, w, h, cols, is_grid, target, forced=False, hdr8=False, alpha_pic=None):
    P, bits, cf, nclx = oracle_native(hm, tiles, tile_w, tile_h, w, h, cols, is_grid, alpha_pic)
    chain = pr.chain_for(cf, "a" in P, bits, nclx, target, hdr8, forced)
    assert chain, chain
    exp, obits, ochroma, undefined = pr.run_chain(chain, P, bits, cf, nclx, target, 8 if hdr8 else bits, forced)
    assert ochroma == target
    m, p, t = (nclx[0], nclx[1], nclx[2]) if nclx else (2, 2, 2)
    profile = dict(matrix=6 if m == 2 else m, primaries=1 if p == 2 else p, transfer=13 if t == 2 else t, full_range=nclx[3] if nclx else 1)
    return exp, obits, undefined, chain, profile


def take(hm, d):
    """an hm_decoded -> ({"y", "cb", "cr"[, "a"]}, meta, raw padded planes); strides are checked against hm_plane_stride"""
    bits = d.bit_depth
    bps = 2 if bits > 8 else 1
    raw, P = {}, {}
    for c, k in enumerate(("y", "cb", "cr")):
        if d.plane[c]:
            assert d.stride[c] == hm.hm_plane_stride(d.plane_width[c], bps)
            raw[k] = np.ctypeslib.as_array(d.plane[c], shape=(d.plane_height[c], d.stride[c])).copy()
            P[k] = np.ascontiguousarray(raw[k][:, :d.plane_width[c] * bps]).view(pr.dtype_of(bits)).reshape(d.plane_height[c], d.plane_width[c])
    if d.alpha:
        assert d.alpha_stride == hm.hm_plane_stride(d.width, bps)
        raw["a"] = np.ctypeslib.as_array(d.alpha, shape=(d.height, d.alpha_stride)).copy()
        P["a"] = np.ascontiguousarray(raw["a"][:, :d.width * bps]).view(pr.dtype_of(bits)).reshape(d.height, d.width)
    meta = {k: getattr(d, k) for k in "width height bit_depth chroma out_format has_nclx primaries transfer matrix full_range has_alpha".split()}
    return P, meta, raw


def decode_item(hm, data, out_format, upsampling=0, hdr8=0, item=0):
    f = pipeline.HeifFile(hm, data)
    prm = pipeline.DecodeParams(out_format, 2, 0, upsampling, None, None, 0, 0, 0, hdr8)
    d = pipeline.Decoded()
    rc = f.hm.hm_decode_item(f.h, item or f.primary(), C.byref(prm), C.byref(d))
    assert rc == 0, f.hm.hm_last_error().decode()
    res = take(f.hm, d)
    f.hm.hm_decoded_free(C.byref(d))
    f.close()
    return res


def check(got, meta, exp, obits, undefined, chain, profile, target, w, h):
    assert meta["chroma"] == target and meta["bit_depth"] == obits and (meta["width"], meta["height"]) == (w, h), meta
    assert meta["has_nclx"] == 1 and {k: meta[k] for k in profile} == profile, (meta, profile)
    assert_same(got, exp, undefined, (target, chain))


def pic_422():
    return synthutil.picture(4220777, width=200, height=120, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30, full_range=0, matrix=1)


def test_decode_422_10bit_to_420(hm):
    pic = pic_422()
    data = heifwriter.write_heic([pic], (200, 120), chroma_format=2, bit_depth=10)
    exp = oracle_expect(hm, [pic], 200, 120, 200, 120, 1, False, 1)
    assert [n.split("<")[0] for n in exp[3]] == ["Op_YCbCr_to_RGB", "Op_RGB_to_YCbCr"]
    got, meta, _ = decode_item(hm, data, pr.HM_OUT_YCBCR[1])
    check(got, meta, *exp, 1, 200, 120)
    exp8 = oracle_expect(hm, [pic], 200, 120, 200, 120, 1, False, 1, hdr8=True)  # convert_hdr_to_8bit: Op_to_sdr_planes joins the chain
    assert "Op_to_sdr_planes" in exp8[3] and exp8[1] == 8
    got, meta, _ = decode_item(hm, data, pr.HM_OUT_YCBCR[1], hdr8=1)
    check(got, meta, *exp8, 1, 200, 120)
    expb = oracle_expect(hm, [pic], 200, 120, 200, 120, 1, False, 1, forced=True)
    assert len(expb[3]) == 2 and "bilinear" in expb[3][0] and "average" in expb[3][1]
    got, meta, _ = decode_item(hm, data, pr.HM_OUT_YCBCR[1], upsampling=2)
    check(got, meta, *expb, 1, 200, 120)


def test_decode_444_with_alpha_to_420(hm):
    """the alpha plane travels through unchanged (as a fourth plane of the planar result)"""
    main = synthutil.picture(4440001, width=128, height=72, chroma_format=3, qp=28)
    alpha = synthutil.picture(4440002, width=128, height=72, chroma_format=0)
    data = heifwriter.write_heic([main], (128, 72), chroma_format=3, aux=[(alpha, (128, 72), ALPHA_URN)])
    exp = oracle_expect(hm, [main], 128, 72, 128, 72, 1, False, 1, alpha_pic=alpha)
    assert exp[3] == ["Op_YCbCr444_to_YCbCr420_average<uint8_t>"] and "a" in exp[0]
    got, meta, _ = decode_item(hm, data, pr.HM_OUT_YCBCR[1])
    assert meta["has_alpha"] == 1 and "a" in got
    check(got, meta, *exp, 1, 128, 72)


def grid_420():
    tiles = [synthutil.picture(4200100 + i, width=64, height=64) for i in range(4)]
    return tiles, heifwriter.write_heic(tiles, (64, 64), grid=(2, 2, 128, 128))


def test_decode_grids(hm):
    tiles, grid = grid_420()
    for target, first in ((3, "Op_YCbCr420_bilinear_to_YCbCr444<uint8_t>"), (2, "Op_YCbCr_to_RGB<uint8_t>")):
        exp = oracle_expect(hm, tiles, 64, 64, 128, 128, 2, True, target)
        assert exp[3][0] == first
        got, meta, _ = decode_item(hm, grid, pr.HM_OUT_YCBCR[target])
        check(got, meta, *exp, target, 128, 128)
    mono = [synthutil.picture(4000100 + i, width=64, height=64, chroma_format=0) for i in range(4)]
    exp = oracle_expect(hm, mono, 64, 64, 128, 128, 2, True, 1)
    assert exp[3] == ["Op_mono_to_YCbCr420"]
    got, meta, _ = decode_item(hm, heifwriter.write_heic(mono, (64, 64), grid=(2, 2, 128, 128), chroma_format=0), pr.HM_OUT_YCBCR[1])
    check(got, meta, *exp, 1, 128, 128)


def test_decode_example_heic_to_444(hm):
    from test_golden_heic import GOLD, _hevc_of, _load
    case = GOLD["cases"][0]
    assert case["file"] == "example.heic"
    w, h = case["w"], case["h"]
    exp = oracle_expect(hm, [_hevc_of(hm, case)], w, h, w, h, 1, False, 3)
    assert exp[3] == ["Op_YCbCr420_bilinear_to_YCbCr444<uint8_t>"]
    got, meta, _ = decode_item(hm, _load(case["file"]), pr.HM_OUT_YCBCR[3], item=case["item"] or 0)
    check(got, meta, *exp, 3, w, h)


def test_target_equal_to_the_native_format_converts_nothing(hm):
    pic = synthutil.picture(4220778, width=96, height=64, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30)
    data = heifwriter.write_heic([pic], (96, 64), chroma_format=2, bit_depth=10)
    _, m0, raw0 = decode_item(hm, data, 0)
    _, m1, raw1 = decode_item(hm, data, pr.HM_OUT_YCBCR[2], hdr8=1)  # (the depth alone converts nothing: context.cc:1547-1552)
    assert {k: v for k, v in m0.items() if k != "out_format"} == {k: v for k, v in m1.items() if k != "out_format"}
    assert all(np.array_equal(raw0[k], raw1[k]) for k in raw0) and set(raw0) == set(raw1)


def test_through_the_pipeline(hm):
    """hm_pipeline_*: the config's out_format carries the planar code, and HM_OUT_YCBCR_8BIT in place of convert_hdr_to_8bit;
    hm_decoded.out_format reports the code without the flag"""
    pic = pic_422()
    data = heifwriter.write_heic([pic], (200, 120), chroma_format=2, bit_depth=10)
    for hdr8 in (False, True):
        exp = oracle_expect(hm, [pic], 200, 120, 200, 120, 1, False, 1, hdr8=hdr8)
        p = pipeline.Pipeline(hm, pr.HM_OUT_YCBCR[1] | (pr.HM_OUT_YCBCR_8BIT if hdr8 else 0), host_threads=2, max_in_flight=2)
        assert p.submit(data, 7)
        r = pipeline.PipelineResult()
        assert hm.hm_pipeline_next(p.h, C.byref(r)) == 0 and r.status == 0 and r.tag == 7
        got, meta, _ = take(hm, r.image)
        hm.hm_pipeline_release(p.h, C.byref(r))
        p.close()
        assert meta["out_format"] == pr.HM_OUT_YCBCR[1]
        check(got, meta, *exp, 1, 200, 120)


def test_through_decode_sequence(hm):
    import moovwriter
    from test_sequence_gpu import bind_sequence
    bind_sequence(hm)
    pics = [synthutil.picture(4220900 + i, width=128, height=64, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30) for i in range(3)]
    f = pipeline.HeifFile(hm, moovwriter.write_movie(pics, (128, 64), chroma_format=2, bit_depth=10))
    prm = pipeline.DecodeParams(pr.HM_OUT_YCBCR[1], 2, 0, 0, None, None, 0, 0, 0, 0)
    out = (pipeline.Decoded * 3)()
    failed = C.c_int32(-2)
    rc = hm.hm_decode_sequence(f.h, 1, 3, C.byref(prm), None, out, C.byref(failed))
    assert rc == 0, hm.hm_last_error().decode()
    for k in range(3):
        got, meta, _ = take(hm, out[k])
        hm.hm_decoded_free(C.byref(out[k]))
        check(got, meta, *oracle_expect(hm, [pics[k]], 128, 64, 128, 64, 1, False, 1), 1, 128, 64)
    f.close()


class Nclx(C.Structure):
    _fields_ = [("version", C.c_uint8), ("color_primaries", C.c_int), ("transfer_characteristics", C.c_int), ("matrix_coefficients", C.c_int),
                ("full_range_flag", C.c_uint8), ("xy", C.c_float * 8)]


def facade_planes(api, hm, img, bits_expected):
    api.heif_image_get_nclx_color_profile.restype = Err
    api.heif_image_get_nclx_color_profile.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Nclx))]
    api.heif_nclx_color_profile_free.argtypes = [C.c_void_p]
    P = {}
    for k, ch in (("y", CH_Y), ("cb", CH_CB), ("cr", CH_CR), ("a", CH_ALPHA)):
        if not api.heif_image_has_channel(img, ch):
            continue
        w, h, bits = api.heif_image_get_width(img, ch), api.heif_image_get_height(img, ch), api.heif_image_get_bits_per_pixel_range(img, ch)
        assert bits == bits_expected
        stride = C.c_int()
        p = api.heif_image_get_plane_readonly(img, ch, C.byref(stride))
        bps = 2 if bits > 8 else 1
        assert stride.value == hm.hm_plane_stride(w, bps)
        a = np.ctypeslib.as_array(p, shape=(h, stride.value)).copy()
        P[k] = np.ascontiguousarray(a[:, :w * bps]).view(pr.dtype_of(bits)).reshape(h, w)
    n = C.POINTER(Nclx)()
    e = api.heif_image_get_nclx_color_profile(img, C.byref(n))
    assert e.code == 0
    prof = dict(matrix=n.contents.matrix_coefficients, primaries=n.contents.color_primaries, transfer=n.contents.transfer_characteristics,
                full_range=n.contents.full_range_flag)
    api.heif_nclx_color_profile_free(n)
    return P, prof


def test_heif_decode_image_ycbcr_targets(api, hm):  # noqa: F811
    """what heif-dec asks for when it writes Y4M: (heif_colorspace_YCbCr, heif_chroma_420), read back through the accessors"""
    pic = pic_422()
    data = heifwriter.write_heic([pic], (200, 120), chroma_format=2, bit_depth=10)
    for cs, target in ((CS_YCBCR, 1), (CS_UNDEFINED, 3), (CS_YCBCR, 2)):
        ctx, h, img, e = facade_decode(api, data, 0, cs, target)
        assert e.code == 0, e.message
        assert api.heif_image_get_colorspace(img) == CS_YCBCR and api.heif_image_get_chroma_format(img) == target
        got, prof = facade_planes(api, hm, img, 10)
        if target == 2:  # the image's own format: the native planes
            native, _, _ = decode_item(hm, data, 0)
            assert all(np.array_equal(got[k], native[k]) for k in native)
        else:
            exp, obits, undefined, chain, profile = oracle_expect(hm, [pic], 200, 120, 200, 120, 1, False, target)
            cw, ch = pr.chroma_size(target, 200, 120)
            assert got["cb"].shape == (ch, cw) and got["y"].shape == (120, 200) and prof == profile
            assert_same(got, exp, undefined, (target, chain))
        api.heif_image_release(img)
        api.heif_image_handle_release(h)
        api.heif_context_free(ctx)
    # a 4:4:4 image with alpha -> 4:2:0: heif_channel_Alpha present and unchanged
    main = synthutil.picture(4440001, width=128, height=72, chroma_format=3, qp=28)
    alpha = synthutil.picture(4440002, width=128, height=72, chroma_format=0)
    ctx, h, img, e = facade_decode(api, heifwriter.write_heic([main], (128, 72), chroma_format=3, aux=[(alpha, (128, 72), ALPHA_URN)]), 0, CS_YCBCR, 1)
    assert e.code == 0, e.message
    got, _ = facade_planes(api, hm, img, 8)
    exp, _, undefined, chain, _ = oracle_expect(hm, [main], 128, 72, 128, 72, 1, False, 1, alpha_pic=alpha)
    assert_same(got, exp, undefined, chain)
    api.heif_image_release(img)
    api.heif_image_handle_release(h)
    api.heif_context_free(ctx)


def test_heif_decode_image_refusals(api, hm):  # noqa: F811
    """(RGB, 4:4:4) stays refused; a monochrome image with its own colourspace and a colour chroma has no chain; a 4:0:0 image with an
    nclx goes through the interleaved ops in the reference: refused naming the chain; "no chain" is Unsupported_color_conversion -
    also for the interleaved RGB targets, whose no-chain refusal used to come back as Unsupported_codec"""
    pic = pic_422()
    data = heifwriter.write_heic([pic], (200, 120), chroma_format=2, bit_depth=10)
    ctx, h, img, e = facade_decode(api, data, 0, CS_RGB, 3)
    assert e.code == 4 and not img
    mono = synthutil.picture(4000200, width=64, height=64, chroma_format=0)
    mdata = heifwriter.write_heic([mono], (64, 64), chroma_format=0)
    ctx, h, img, e = facade_decode(api, mdata, 0, CS_UNDEFINED, 1)
    assert e.code == 4 and e.subcode == SUBERROR_UNSUPPORTED_COLOR_CONVERSION and not img
    lim = synthutil.picture(4000201, width=64, height=64, chroma_format=0, full_range=0, matrix=1)  # an nclx other than the sRGB default
    ctx, h, img, e = facade_decode(api, heifwriter.write_heic([lim], (64, 64), chroma_format=0), 0, CS_YCBCR, 1)
    assert e.code == 4 and e.subcode != SUBERROR_UNSUPPORTED_COLOR_CONVERSION and b"Op_mono_to_RGB24_32" in e.message and not img
    m11 = synthutil.picture(4200300, width=64, height=64, matrix=11)
    for cs, chroma in ((CS_RGB, 10), (CS_YCBCR, 3)):  # every YCbCr -> RGB op refuses matrix 11; bilinear up-sampling does not
        ctx, h, img, e = facade_decode(api, heifwriter.write_heic([m11], (64, 64)), 0, cs, chroma)
        if chroma == 10:
            assert e.code == 4 and e.subcode == SUBERROR_UNSUPPORTED_COLOR_CONVERSION and not img
        else:
            assert e.code == 0 and api.heif_image_get_chroma_format(img) == 3
