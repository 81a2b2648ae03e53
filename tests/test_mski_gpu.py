"""GPU: an 8-bit mask item ('mski' + mskC) through hm_decode_item and its device forms: a monochrome 8-bit image whose samples are the
payload's bytes, on the path of a monochrome 8-bit 'unci' item - the same bytes in such an item give the same tensor from the same
call -, a short payload refused with the destination untouched, and the pipeline's refusal."""
import ctypes as C

import numpy as np
import pytest

from regionwriter import Writer

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, BITSTREAM = 0, -2, -3
W, H = 37, 21


@pytest.fixture(scope="module")
def samples():
    s = np.random.default_rng(4711).integers(0, 256, (H, W)).astype(np.uint8)
    s[0, 0], s[0, 1], s[H - 1, W - 1] = 0, 255, 128
    s.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def files(samples):
    """the mask item, the same bytes as a monochrome 8-bit 'unci' item, and the mask item one byte short"""
    out = {}
    for name, add in (("mski", lambda w: w.mski(samples.tobytes(), (W, H), hidden=False)), ("unci", lambda w: w.unci_mono8(samples.tobytes(), (W, H))),
                      ("short", lambda w: w.mski(samples.tobytes()[:-1], (W, H), hidden=False))):
        w = Writer()
        iid = add(w)
        w.mski(bytes(4), (2, 2))  # (a second item behind it: the payload does not end with the file)
        out[name] = w.finish(primary=iid)
    return out


def decode_host(capi, L, data, fmt=0):
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    try:
        prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
        d = capi.Decoded()
        rc = L.hm_decode_item(fh, L.hm_file_primary_item(fh), C.byref(prm), C.byref(d))
        res = None
        if rc == OK:
            res = dict(size=(d.width, d.height), bit_depth=d.bit_depth, chroma=d.chroma, has_alpha=d.has_alpha,
                       planes=[np.ctypeslib.as_array(d.plane[c], shape=(d.plane_height[c], d.stride[c])).copy() for c in range(3) if d.plane[c]])
            L.hm_decoded_free(C.byref(d))
        return rc, res, L.hm_last_error().decode()
    finally:
        L.hm_file_close(fh)


def test_decode_item_planes_are_the_payload_bytes(pkg, files, samples):
    capi = pkg.capi
    L = capi.image_lib()
    rc, res, msg = decode_host(capi, L, files["mski"])
    assert rc == OK, msg
    assert res["size"] == (W, H) and (res["bit_depth"], res["chroma"], res["has_alpha"]) == (8, 0, 0) and len(res["planes"]) == 1
    assert np.array_equal(res["planes"][0][:H, :W], samples)
    rc, res, msg = decode_host(capi, L, files["mski"], 10)  # HM_OUT_RGB: the chain of a monochrome image, as for the 'unci' item
    rc2, res2, msg2 = decode_host(capi, L, files["unci"], 10)
    assert rc == OK and rc2 == OK, (msg, msg2)
    assert res["size"] == res2["size"] and np.array_equal(res["planes"][0][:H, :3 * W], res2["planes"][0][:H, :3 * W])  # (the pixels, not the stride's padding)


def test_planes_view_and_tensor_equal_the_unci_item(pkg, files, samples):
    import torch
    (y,) = pkg.decode_to_planes(files["mski"])
    assert y.dtype == torch.uint8 and np.array_equal(y.cpu().numpy(), samples)
    (v,) = pkg.decode_to_planes(files["mski"], crop=(3, 5, 20, 11))
    assert np.array_equal(v.cpu().numpy(), samples[5:16, 3:23])
    (r,) = pkg.decode_to_planes(files["mski"], crop=(3, 5, 20, 11), size=(9, 7), dtype=torch.float32)
    (u,) = pkg.decode_to_planes(files["unci"], crop=(3, 5, 20, 11), size=(9, 7), dtype=torch.float32)
    assert torch.equal(r, u)
    for kw in (dict(out_format="rgb"), dict(out_format="rgb", dtype=torch.uint8, layout="hwc"), dict(out_format="rgb", crop=(1, 2, 30, 15), size=(17, 9))):
        a, b = pkg.decode_to_tensor(files["mski"], **kw), pkg.decode_to_tensor(files["unci"], **kw)
        assert torch.equal(a, b), kw


def test_short_payload_is_refused_with_the_destination_untouched(pkg, files):
    import torch
    capi = pkg.capi
    L = capi.image_lib()
    rc, _, msg = decode_host(capi, L, files["short"])
    assert rc == BITSTREAM and "776" in msg, msg
    out = torch.full((3, H, W), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.HmError) as e:
        pkg.decode_to_tensor(files["short"], out_format="rgb", out=out)
    assert e.value.status == BITSTREAM
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_pipeline_refuses_mask_items(pkg, files):
    capi = pkg.capi
    L = capi.image_lib()
    cfg = capi.PipelineConfig(2, 2, 10, 0, 0, 0, -1, 0, 0)
    pipe = C.c_void_p()
    assert L.hm_pipeline_create(C.byref(cfg), C.byref(pipe)) == 0, L.hm_last_error().decode()
    try:
        assert L.hm_pipeline_submit(pipe, files["mski"], len(files["mski"]), 0, 7) == UNSUPPORTED
        assert b"mski" in L.hm_last_error()
        assert L.hm_pipeline_pending(pipe) == 0
    finally:
        L.hm_pipeline_destroy(pipe)
