"""The matrix behind tests/test_emit_fields_gpu.py: pictures x out_format x destination kind, and of every decode the fields of
hm_decoded (no pixels) - or, where the interface refuses the combination, its status and message.  Shared with
tools/record_target_goldens.py, which writes tests/golden/emit_fields.json."""
import ctypes as C

import heifwriter
import moovwriter
import overlaywriter
import synthutil

RGB, RGBA, RRGGBBAA_BE, RRGGBB_LE = 10, 11, 13, 14
HWC, U8, U16, F32 = 0, 0, 1, 3
ALPHA_URN = "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha"
W, H = 24, 16
VIEW = (3, 2, 20, 12, 10, 6, 0)        # crop 3, 2 20 x 12 to 10 x 6, HM_VIEW_TRIANGLE
VIEW_EVEN = (4, 2, 20, 12, 10, 6, 0)   # the same on an even column: what a 4:2:0 / 4:2:2 planar view takes
KINDS = ("host", "dest", "view", "planes", "planes_view", "planes_view_even", "light")
SLOT = 1 << 18                         # bytes of device memory per plane / destination
FIELDS = "width height bit_depth chroma out_format has_nclx primaries transfer matrix full_range has_alpha used_ext_dst alpha_stride warnings".split()


def pictures():
    """name -> (file bytes, 'item' | 'seq', chroma format of the coded picture, has alpha)"""
    def pic(seed, w=W, h=H, **kw):
        return synthutil.picture(62000 + seed, width=w, height=h, **kw)
    out = {
        "p420_8": (heifwriter.write_heic([pic(1)], (W, H)), "item", 1, False),
        "p420_10": (heifwriter.write_heic([pic(2, bit_depth=10)], (W, H), bit_depth=10), "item", 1, False),
        "p444_8": (heifwriter.write_heic([pic(3, chroma_format=3)], (W, H), chroma_format=3), "item", 3, False),
        "mono": (heifwriter.write_heic([pic(4, chroma_format=0)], (W, H), chroma_format=0), "item", 0, False),
        "alpha": (heifwriter.write_heic([pic(5)], (W, H), aux=[(pic(6), (W, H), ALPHA_URN)]), "item", 1, True),
        "grid": (heifwriter.write_heic([pic(10 + t, 16, 16) for t in range(4)], (16, 16), grid=(2, 2, 32, 32)), "item", 1, False),
        "movie": (moovwriter.write_movie([pic(20 + k) for k in range(3)], (W, H)), "seq", 1, False),
    }
    wr = overlaywriter.Writer()
    out["iden"] = (wr.finish(wr.iden([wr.hvc1(pic(7), (W, H))], (W, H))), "item", 1, False)
    wr = overlaywriter.Writer()
    a, b = wr.hvc1(pic(8), (W, H)), wr.hvc1(pic(9, 16, 16), (16, 16))
    out["iovl"] = (wr.finish(wr.iovl([(a, 0, 0), (b, 12, 6)], (32, 24), background=(0x4000, 0x8000, 0xC000, 0xFFFF))), "item", 1, False)
    return out


def formats(chroma):
    """(out_format, convert_hdr_to_8bit): as decoded, a planar target of the picture's own chroma format and one of another, the
    interleaved ones"""
    same = [0x100 + chroma] if chroma else []
    other = 0x101 if chroma == 3 else 0x103
    planar = [(f, to8) for f in same + [other] for to8 in (0, 1)]
    return [(0, 0)] + planar + [(RGB, 0), (RGBA, 0), (RRGGBB_LE, 0), (RRGGBBAA_BE, 0)]


def fields(d):
    r = {n: int(getattr(d, n)) for n in FIELDS}
    for n in ("stride", "plane_width", "plane_height"):
        r[n] = [int(getattr(d, n)[c]) for c in range(3)]
    return r


class Device:
    """five slots of device memory: a destination, or the planes Y, Cb, Cr, alpha"""

    def __init__(self):
        import torch
        self.t = torch.zeros(5 * SLOT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.base = self.t.data_ptr()

    def dest(self, capi, fmt, light, k=0, dtype=None):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout = self.base + (k % 4) * SLOT, SLOT, HWC
        d.dtype = dtype if dtype is not None else F32 if light else (U16 if fmt >= 12 else U8)
        for c in range(4):
            d.scale[c], d.bias[c] = 1.0, 0.0
        return d

    def planes(self, capi, alpha, y_only):
        d = capi.DevicePlanes()
        d.layout, d.dtype = 0, F32
        for c in (0,) if y_only else range(4 if alpha else 3):
            d.plane[c].ptr, d.plane[c].len = self.base + c * SLOT, SLOT
            d.scale[c], d.bias[c] = 1.0, 0.0
        return d


def bind(L, capi):
    L.hm_decode_sequence.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(capi.DecodeParams), C.c_void_p, C.POINTER(capi.Decoded), C.POINTER(C.c_int32)]


def one(capi, L, dev, blob, call, chroma, alpha, fmt, to8, kind):
    """one decode: {"status", "message"[, "failed_frame"], "images": [fields]}"""
    fh = C.c_void_p()
    assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
    n = 3 if call == "seq" else 1
    prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, to8)
    out = (capi.Decoded * n)()
    failed = C.c_int32(7)
    view = capi.DeviceView(*(VIEW_EVEN if kind == "planes_view_even" else VIEW))
    light = capi.DeviceLight(0, 0, 8, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    dests = (capi.DeviceDest * n)(*[dev.dest(capi, fmt, kind == "light", k) for k in range(n)])
    # (a sequence: every frame into the same planes - the fields are what is looked at)
    planes = (capi.DevicePlanes * n)(*[dev.planes(capi, alpha, chroma == 0 and fmt == 0) for _ in range(n)])  # (4:0:0 as coded: Y only)
    try:
        if call == "item":
            item = L.hm_file_primary_item(fh)
            rc = {"host": lambda: L.hm_decode_item(fh, item, C.byref(prm), out),
                  "dest": lambda: L.hm_decode_item_to_device(fh, item, C.byref(prm), dests, out),
                  "view": lambda: L.hm_decode_item_to_device_view(fh, item, C.byref(prm), C.byref(view), dests, out),
                  "light": lambda: L.hm_decode_item_to_device_light(fh, item, C.byref(prm), None, C.byref(light), dests, out),
                  "planes": lambda: L.hm_decode_item_to_device_planes(fh, item, C.byref(prm), planes, out),
                  "planes_view": lambda: L.hm_decode_item_to_device_planes_view(fh, item, C.byref(prm), C.byref(view), planes, out),
                  "planes_view_even": lambda: L.hm_decode_item_to_device_planes_view(fh, item, C.byref(prm), C.byref(view), planes, out)}[kind]()
        else:
            ids = (C.c_uint32 * n)(3, 1, 2)
            f = C.byref(failed)
            rc = {"host": lambda: L.hm_decode_sequence(fh, 1, n, C.byref(prm), None, out, f),
                  "dest": lambda: L.hm_decode_sequence_to_device(fh, 1, n, C.byref(prm), dests, out, f),
                  "view": lambda: L.hm_decode_frames_to_device_view(fh, ids, n, C.byref(prm), C.byref(view), dests, out, f),
                  "light": lambda: L.hm_decode_frames_to_device_light(fh, ids, n, C.byref(prm), C.byref(view), C.byref(light), dests, out, f),
                  "planes": lambda: L.hm_decode_frames_to_device_planes(fh, ids, n, C.byref(prm), planes, out, f),
                  "planes_view": lambda: L.hm_decode_frames_to_device_planes_view(fh, ids, n, C.byref(prm), C.byref(view), planes, out, f),
                  "planes_view_even": lambda: L.hm_decode_frames_to_device_planes_view(fh, ids, n, C.byref(prm), C.byref(view), planes, out, f)}[kind]()
        got = {"status": rc, "message": L.hm_last_error().decode() if rc else ""}
        if call == "seq":
            got["failed_frame"] = failed.value
        if rc == 0:
            got["images"] = [fields(out[k]) for k in range(n)]
            if kind != "host":
                assert not any(out[k].plane[c] for k in range(n) for c in range(3)) and not any(out[k].alpha for k in range(n))
        for k in range(n):
            L.hm_decoded_free(C.byref(out[k]))
        return got
    finally:
        L.hm_file_close(fh)


def walk(capi, L):
    """{"picture | out_format[+8] | kind": result}"""
    bind(L, capi)
    dev = Device()
    got = {}
    for name, (blob, call, chroma, alpha) in pictures().items():
        for fmt, to8 in formats(chroma):
            for kind in KINDS:
                got[f"{name} | {fmt:#x}{'+8' if to8 else ''} | {kind}"] = one(capi, L, dev, blob, call, chroma, alpha, fmt, to8, kind)
    return got


# ---- the tone and alpha steps (tests/golden/emit_fields_steps.json): the same fields through hm_decode_*_to_device_tone / _alpha ----
RRGGBBAA_LE = 15
STEP_KINDS = ("tone", "alpha", "alpha_view", "alpha_light", "alpha_matte_tone8")
STEP_PICTURES = ("p420_8", "p420_10", "alpha", "grid", "movie", "iovl")  # (movie: a sequence takes no alpha step - tone only)
STEP_FORMATS = (RGB, RGBA, RRGGBB_LE, RRGGBBAA_LE)


def one_step(capi, L, dev, blob, call, fmt, kind):
    """one decode through the tone or the alpha entry: {"status", "message"[, "failed_frame"], "images": [fields]}"""
    fh = C.c_void_p()
    assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
    n = 3 if call == "seq" else 1
    prm = capi.DecodeParams(fmt, 2, 0, 0, None, None, 0, 0, 0, 0)
    out = (capi.Decoded * n)()
    failed = C.c_int32(7)
    view = C.byref(capi.DeviceView(*VIEW)) if kind == "alpha_view" else None
    matte8 = kind == "alpha_matte_tone8"
    # the image's own codes to linear light - re-encoded as sRGB under the 8-bit finish
    light = C.byref(capi.DeviceLight(0, 0, 13 if matte8 else 8, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))) if kind in ("tone", "alpha_light") or matte8 else None
    tone = C.byref(capi.DeviceTone(1, 8 if matte8 else 0, 0.0, 100.0, 100.0, 0.0, (C.c_int32 * 2)(0, 0))) if kind == "tone" or matte8 else None
    mode = {"alpha": 2, "alpha_view": 1, "alpha_light": 2, "alpha_matte_tone8": 3}.get(kind, 0)
    alpha = capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*((10, 20, 30, 0) if matte8 else (0, 0, 0, 0))), (C.c_int32 * 3)(0, 0, 0))
    dests = (capi.DeviceDest * n)(*[dev.dest(capi, fmt, light is not None, k, U8 if matte8 else None) for k in range(n)])
    try:
        if kind != "tone":
            rc = L.hm_decode_item_to_device_alpha(fh, L.hm_file_primary_item(fh), C.byref(prm), view, light, tone, C.byref(alpha), dests, out)
        elif call == "item":
            rc = L.hm_decode_item_to_device_tone(fh, L.hm_file_primary_item(fh), C.byref(prm), view, light, tone, dests, out)
        else:
            rc = L.hm_decode_frames_to_device_tone(fh, (C.c_uint32 * n)(3, 1, 2), n, C.byref(prm), view, light, tone, dests, out, C.byref(failed))
        got = {"status": rc, "message": L.hm_last_error().decode() if rc else ""}
        if call == "seq":
            got["failed_frame"] = failed.value
        if rc == 0:
            got["images"] = [fields(out[k]) for k in range(n)]
        for k in range(n):
            L.hm_decoded_free(C.byref(out[k]))
        return got
    finally:
        L.hm_file_close(fh)


def walk_steps(capi, L):
    """{"picture | out_format | kind": result}"""
    dev = Device()
    pics = pictures()
    got = {}
    for name in STEP_PICTURES:
        blob, call = pics[name][:2]
        for fmt in STEP_FORMATS:
            for kind in STEP_KINDS if call == "item" else ("tone",):
                got[f"{name} | {fmt:#x} | {kind}"] = one_step(capi, L, dev, blob, call, fmt, kind)
    return got
