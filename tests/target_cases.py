"""The table of wrong output-target requests behind tests/test_target_refusals.py (and, for the pipeline, which needs a device to
exist, behind tests/test_emit_fields_gpu.py) - shared with tools/record_target_goldens.py, which writes the golden files.

Every request is wrong in a way the library decides on the host, before it asks for a device: no pointer below is ever dereferenced.
A case names the entry-point families it is sent through; a family fills in everything the case leaves alone with values that are in
order.  What comes back is (status, hm_last_error(), failed_frame) - failed_frame None for the calls that have none."""
import ctypes as C

import heifwriter
import moovwriter
import synthutil

FAKE = 0x10000000
HM_ERR_NO_DEVICE = -4
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE, RRGGBBAA_LE = 10, 11, 12, 13, 14, 15
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
STRAIGHT, PREMULTIPLIED, MATTE = 1, 2, 3
N_FRAMES = 3
SENTINEL = 7  # what failed_frame holds before a call

# families: the picture they decode ("tensor": none - the stand-alone entries, on a source pointer that is never read), whether the
# destination is planes, whether they take a view / a light step / a tone step / an alpha step / frame IDs.  An alpha family hands
# on the light and tone steps a case names, and none otherwise.
FAMILIES = {
    "item_dest":          dict(call="item"),
    "item_view":          dict(call="item", view=True),
    "item_light":         dict(call="item", view=True, light=True),
    "item_planes":        dict(call="item", planes=True),
    "item_planes_view":   dict(call="item", planes=True, view=True),
    "seq_dest":           dict(call="seq"),
    "frames_view":        dict(call="seq", view=True, frames=True),
    "frames_light":       dict(call="seq", view=True, light=True, frames=True),
    "frames_planes":      dict(call="seq", planes=True, frames=True),
    "frames_planes_view": dict(call="seq", planes=True, view=True, frames=True),
    "pipe_dest":          dict(call="pipe"),
    "pipe_view":          dict(call="pipe", view=True),
    "pipe_light":         dict(call="pipe", view=True, light=True),
    "pipe_planes":        dict(call="pipe", planes=True),
    "pipe_planes_view":   dict(call="pipe", planes=True, view=True),
    "item_tone":          dict(call="item", view=True, light=True, tone=True),
    "item_alpha":         dict(call="item", view=True, alpha=True),
    "frames_tone":        dict(call="seq", view=True, light=True, tone=True, frames=True),
    "pipe_tone":          dict(call="pipe", view=True, light=True, tone=True),
    "pipe_alpha":         dict(call="pipe", view=True, alpha=True),
    "tensor_dest":        dict(call="tensor"),
    "tensor_view":        dict(call="tensor", view=True),
    "tensor_light":       dict(call="tensor", view=True, light=True),
    "tensor_tone":        dict(call="tensor", view=True, light=True, tone=True),
    "tensor_alpha":       dict(call="tensor", view=True, alpha=True),
}


def _fam(**want):
    return [n for n, f in FAMILIES.items() if all((f.get(k) if k == "call" else bool(f.get(k))) == v for k, v in want.items())]


EVERY = list(FAMILIES)
DEST, PLANES, VIEW, LIGHT = _fam(planes=False), _fam(planes=True), _fam(view=True), _fam(light=True)
DEST_VIEW = [n for n in DEST if n in VIEW]
TONE, ALPHA, TENSOR = _fam(tone=True), _fam(alpha=True), _fam(call="tensor")
WITH_PARAMS = [n for n in EVERY if not n.startswith("pipe_") and n not in TENSOR]  # the entry points that take hm_decode_params
GOOD_VIEW = ((4, 2, 10, 8), (5, 4), TRIANGLE)  # crop, output size, filter
GOOD_LIGHT = (0, 0, 8, 0, 1.0)                # the image's own codes to linear light
LINEAR, ENCODED = (13, 1, 8, 0, 1.0), (13, 1, 13, 0, 1.0)  # sRGB codes, named (the stand-alone entries take no others), to linear light / re-encoded
GOOD_TONE = (1, 0, 1000.0, 100.0, 100.0, 0.0)  # curve, out_bits, src_peak, dst_peak, unit_nits, out_unit_nits
BAD_VIEW = ((10, 10, 10, 10), (5, 5), TRIANGLE)


def tone(curve=1, out_bits=0, src_peak=1000.0, dst_peak=100.0, unit_nits=100.0):
    return (curve, out_bits, src_peak, dst_peak, unit_nits, 0.0)


def alpha(mode, background=(0, 0, 0, 0), reserved=(0, 0, 0)):
    return (mode, background, reserved)

# name, families, overrides: fmt (dest families) / pfmt (planes families), dest={} (every_dest={}: of every frame), planes={}, view=, light=, ext_dst, frames=, first=,
# picture="wide" (176 x 16, the one case a 16 x 16 picture cannot express); tone=, alpha=; fmt16 (the family's 16-bit _LE target), dest_fmt (the target the
# destination is sized as, where that is not fmt), and for the stand-alone entries bits= and src_stride= (bytes added to the tight stride)
CASES = [
    ("ext_dst set", WITH_PARAMS, dict(ext_dst=True)),
    ("unknown layout", DEST, dict(dest=dict(layout=5))),
    ("unknown dtype", DEST, dict(dest=dict(dtype=9))),
    ("planes: unknown layout", PLANES, dict(planes=dict(layout=5))),
    ("planes: unknown dtype", PLANES, dict(planes=dict(dtype=9))),
    ("big-endian target with a float dtype", DEST, dict(fmt=RRGGBB_BE, dest=dict(dtype=F32))),
    ("null ptr", DEST, dict(dest=dict(ptr=None))),
    ("len one byte short", DEST, dict(dest=dict(short=1))),
    ("row pitch too small", DEST, dict(dest=dict(row_pitch=-1))),
    ("view: the crop leaves the picture", VIEW, dict(view=((10, 10, 10, 10), (5, 5), TRIANGLE))),
    ("view: output of 0", VIEW, dict(view=((0, 0, 16, 16), (0, 4), TRIANGLE))),
    ("view: reduction beyond the filter's limit", VIEW, dict(view=((0, 0, 176, 16), (2, 16), LANCZOS3), picture="wide")),
    ("planes with an interleaved out_format", PLANES, dict(pfmt=RGB)),
    ("planes with an unknown out_format", PLANES, dict(pfmt=9)),
    ("planes: null plane[0].ptr", PLANES, dict(planes=dict(null=0))),
    ("planes: plane 0 one byte short", PLANES, dict(planes=dict(short=0))),
    ("planes: plane 1 one byte short", PLANES, dict(planes=dict(short=1))),
    ("light: unknown transfer", LIGHT, dict(light=(0, 0, 99, 0, 1.0))),
    ("light: big-endian target, float dtype", LIGHT, dict(fmt=RRGGBB_BE)),
    ("light: big-endian target, raw words, re-encoded", LIGHT, dict(fmt=RRGGBB_BE, every_dest=dict(dtype=U16), light=(0, 0, 13, 0, 1.0), view=None)),
    ("frame ID 0", _fam(call="seq"), dict(frames=[1, 0, 2], first=0)),
    ("frame ID frame_count + 1", _fam(call="seq"), dict(frames=[1, 2, N_FRAMES + 1], first=2)),
    ("two faults: short len and a bad view", DEST_VIEW, dict(dest=dict(short=1), view=((10, 10, 10, 10), (5, 5), TRIANGLE))),
    ("two faults: short plane and a bad view", [n for n in PLANES if n in VIEW], dict(planes=dict(short=0), view=((10, 10, 10, 10), (5, 5), TRIANGLE))),
    ("two faults: null ptr and an unknown layout", DEST, dict(dest=dict(ptr=None, layout=5))),
    ("two faults: ext_dst and an unknown dtype", [n for n in DEST if n in WITH_PARAMS], dict(ext_dst=True, dest=dict(dtype=9))),
    # the stand-alone entries' own: the source
    ("source: stride below the bytes of a row", TENSOR, dict(src_stride=-1)),
    ("source: 16-bit samples at an odd stride", TENSOR, dict(fmt16=True, src_stride=+1)),
    # the tone step's own
    ("tone: unknown curve", TONE, dict(tone=tone(curve=2))),
    ("tone: dst_peak 0", TONE, dict(tone=tone(dst_peak=0.0))),
    ("tone: the knee lies below black", TONE, dict(tone=tone(src_peak=10000.0, dst_peak=1.0))),
    ("tone: out_bits 8 with HM_DEV_U16", TONE, dict(fmt=RRGGBB_LE, light=ENCODED, tone=tone(out_bits=8), dest=dict(dtype=U16))),
    ("tone: out_bits 8 on a four-channel target", TONE, dict(fmt=RGBA, light=ENCODED, tone=tone(out_bits=8))),
    ("alpha: out_bits 8 without a matte", ALPHA, dict(light=ENCODED, tone=tone(out_bits=8), alpha=alpha(STRAIGHT))),
    ("tone without a light step", TONE + ALPHA, dict(light=None, tone=GOOD_TONE)),
    ("tone: unit_nits 0 beside a transfer that is not PQ", ["tensor_tone", "tensor_alpha"], dict(light=LINEAR, tone=tone(unit_nits=0.0))),
    ("tone: src_peak 0", ["tensor_tone", "tensor_alpha"], dict(light=LINEAR, tone=tone(src_peak=0.0))),
    # the alpha step's own
    ("alpha: unknown mode", ALPHA, dict(alpha=alpha(9))),
    ("alpha: reserved not 0", ALPHA, dict(alpha=alpha(STRAIGHT, reserved=(0, 1, 0)))),
    ("alpha: a background outside MATTE", ALPHA, dict(alpha=alpha(PREMULTIPLIED, (0, 1, 0, 0)))),
    ("alpha: background[3]", ALPHA, dict(alpha=alpha(MATTE, (0, 0, 0, 1)), dest_fmt=RGB)),
    ("alpha: a three-channel target", ALPHA, dict(fmt=RGB)),
    ("alpha: a big-endian target", ALPHA, dict(fmt=RRGGBBAA_BE)),
    ("alpha: background above 255 on RGBA", ALPHA, dict(alpha=alpha(MATTE, (0, 0, 256, 0)), dest_fmt=RGB)),
    ("alpha: PREMULTIPLIED beside a tone step", ALPHA, dict(light=LINEAR, tone=GOOD_TONE, alpha=alpha(PREMULTIPLIED))),
    ("alpha: PREMULTIPLIED beside a light step that re-encodes", ALPHA, dict(light=ENCODED, alpha=alpha(PREMULTIPLIED))),
    ("alpha: a matte one byte short of the three-channel sibling", ALPHA, dict(alpha=alpha(MATTE, (1, 2, 3, 0)), dest_fmt=RGB, dest=dict(short=1))),
    ("alpha: a 16-bit background above the peak of a 10-bit image", ["tensor_alpha"], dict(fmt16=True, bits=10, alpha=alpha(MATTE, (1024, 0, 0, 0)), dest_fmt=RRGGBB_LE)),
    ("two faults: a bad alpha mode and an unknown dtype", ALPHA, dict(alpha=alpha(9), dest=dict(dtype=9))),
    ("two faults: a bad tone curve and an unknown light transfer", TONE, dict(tone=tone(curve=2), light=(13, 1, 99, 0, 1.0))),
    ("two faults: a bad view and a matte one byte short", ALPHA, dict(view=BAD_VIEW, alpha=alpha(MATTE, (1, 2, 3, 0)), dest_fmt=RGB, dest=dict(short=1))),
    ("two faults: null ptr and a bad alpha mode", ALPHA, dict(alpha=alpha(9), dest=dict(ptr=None))),
    ("two faults: ext_dst and a bad tone", [n for n in TONE if n in WITH_PARAMS], dict(ext_dst=True, tone=tone(curve=2))),
    ("two faults: an odd source stride with 16-bit samples and a short len", TENSOR, dict(fmt16=True, src_stride=+1, dest=dict(short=1))),
    # (the stand-alone entries judge the image's depth before the destination's len, the decode entries behind it)
    ("two faults: samples of 16 bits under a light step and a short len", ["tensor_light", "tensor_tone", "tensor_alpha"], dict(fmt16=True, bits=16, light=LINEAR, dest=dict(short=1))),
]
# Sent through a family, these reach the device probe (no declared-size check stands in front of it there), so what they answer
# depends on the machine: they stay with the *_gpu tests of that family.
BEHIND_THE_PROBE = {("len one byte short", "seq_dest"), ("row pitch too small", "seq_dest")}


def files():
    """name -> bytes: a 16 x 16 picture and a 3-frame movie of such pictures, and the same at 176 x 16"""
    out = {}
    for name, w in (("", 16), ("wide", 176)):
        pics = [synthutil.picture(61000 + w + k, width=w, height=16) for k in range(N_FRAMES)]
        out[name + "item"] = heifwriter.write_heic(pics[:1], (w, 16))
        out[name + "seq"] = moovwriter.write_movie(pics, (w, 16))
        out[name + "pipe"] = out[name + "item"]
    return out


def make_view(capi, view):
    (x, y, w, h), (ow, oh), filt = view
    return capi.DeviceView(x, y, w, h, ow, oh, filt)


def make_light(capi, light):
    return capi.DeviceLight(light[0], light[1], light[2], light[3], light[4], (C.c_int32 * 3)(0, 0, 0))


def make_dest(capi, L, fmt, w, h, layout=HWC, dtype=U8, ptr=FAKE, short=0, row_pitch=0):
    d = capi.DeviceDest()
    d.layout, d.dtype = layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    need = L.hm_device_dest_bytes(fmt, w, h, C.byref(d))
    tight = L.hm_device_dest_bytes(fmt, w, 1, C.byref(d))
    d.ptr, d.len = ptr, (need if need > 0 else 1 << 20) - short
    if row_pitch < 0 and tight > 0:  # (one element below the tight pitch)
        d.row_pitch, d.len = tight - {U8: 1, U16: 2, F16: 2, F32: 4}[dtype], 1 << 20
    return d


def make_planes(capi, L, w, h, layout=0, dtype=U8, null=None, short=None):
    d = capi.DevicePlanes()
    d.layout, d.dtype = layout, dtype
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    need = (C.c_int64 * 4)()
    if L.hm_device_planes_bytes(1, 8, w, h, C.byref(d), C.byref(need)) < 0:
        need = [1 << 16] * 3 + [0]
    for c in range(3):
        if need[c]:
            d.plane[c].ptr, d.plane[c].len = FAKE + c * (1 << 20), need[c] - (1 if short == c else 0)
    if null is not None:
        d.plane[null].ptr = None
    return d


def make_tone(capi, t):
    return capi.DeviceTone(t[0], t[1], t[2], t[3], t[4], t[5], (C.c_int32 * 2)(0, 0))


def make_alpha(capi, a):
    return capi.DeviceAlpha(a[0], (C.c_uint16 * 4)(*a[1]), (C.c_int32 * 3)(*a[2]))


def run(capi, L, data, family, over, pipelines=None, tensor_call=None):
    """one request through one family: [status, message, failed_frame | None]"""
    fam = FAMILIES[family]
    call, planes, with_alpha, tensor = fam["call"], bool(fam.get("planes")), bool(fam.get("alpha")), fam["call"] == "tensor"
    wide = over.get("picture") == "wide"
    fmt = over.get("pfmt", 0) if planes else over.get("fmt", RGBA if with_alpha else RGB)
    if over.get("fmt16"):
        fmt = RRGGBBAA_LE if with_alpha else RRGGBB_LE
    view = over.get("view", GOOD_VIEW) if fam.get("view") else None
    src_w = 176 if wide else 16
    w, h = view[1] if view and view[1] != (0, 0) and min(view[1]) > 0 else (src_w, 16)
    # the steps this family's entry point takes, in the order of its arguments (an alpha family: light and tone where the case names them)
    light = over.get("light", LINEAR if tensor else GOOD_LIGHT) if fam.get("light") else over.get("light") if with_alpha else None
    tone_ = over.get("tone", GOOD_TONE) if fam.get("tone") else over.get("tone") if with_alpha else None
    steps = []
    if fam.get("view"):
        steps.append(C.byref(make_view(capi, view)) if view else None)
    if fam.get("light") or with_alpha:
        steps.append(C.byref(make_light(capi, light)) if light else None)
    if fam.get("tone") or with_alpha:
        steps.append(C.byref(make_tone(capi, tone_)) if tone_ else None)
    if with_alpha:
        steps.append(C.byref(make_alpha(capi, over.get("alpha", alpha(STRAIGHT)))))
    host = (C.c_uint8 * 4096)()
    n = N_FRAMES if call == "seq" else 1
    bad = 1 if n > 1 else 0  # (a sequence: the wrong destination is that of the second frame)
    if planes:
        arr = (capi.DevicePlanes * n)(*[make_planes(capi, L, w, h, **(over.get("planes", {}) if k == bad else {})) for k in range(n)])
    else:
        dest_fmt = over.get("dest_fmt", fmt)
        good = dict(dtype=(U16 if dest_fmt >= RRGGBB_BE else U8) if not light else F32)
        good.update(over.get("every_dest", {}))
        kw = dict(good)
        kw.update(over.get("dest", {}))
        arr = (capi.DeviceDest * n)(*[make_dest(capi, L, dest_fmt, w, h, **(kw if k == bad else good)) for k in range(n)])
    if tensor:  # no file: a source of src_w x 16 pixels at FAKE
        bpp = {RGB: 3, RGBA: 4, RRGGBB_BE: 6, RRGGBBAA_BE: 8, RRGGBB_LE: 6, RRGGBBAA_LE: 8}[fmt]
        bits = () if family in ("tensor_dest", "tensor_view") else (over.get("bits", 8 if bpp < 6 else 10),)
        if tensor_call:  # (tools/asan/target_walk.py: the same request as plain values, for a program that makes the call itself)
            return tensor_call(family, fmt, bits[0] if bits else 0, src_w, 16, src_w * bpp + over.get("src_stride", 0), view, light, tone_,
                               over.get("alpha", alpha(STRAIGHT)) if with_alpha else None, arr[0])
        fn = {"tensor_dest": L.hm_to_tensor, "tensor_view": L.hm_resample_to_tensor}.get(family) or getattr(L, "hm_" + family[len("tensor_"):] + "_to_tensor")
        rc = fn(fmt, *bits, src_w, 16, FAKE, src_w * bpp + over.get("src_stride", 0), *steps, arr, None)
        return [rc, L.hm_last_error().decode(), None]
    blob = data[("wide" if wide else "") + call]
    prm = capi.DecodeParams(fmt, 1, 0, 0, None, C.cast(host, C.c_void_p) if over.get("ext_dst") else None, 4096 if over.get("ext_dst") else 0,
                            64 if over.get("ext_dst") else 0, 0, 0)
    out = (capi.Decoded * n)()
    failed = C.c_int32(SENTINEL)
    kind = family.split("_", 1)[1]  # dest, view, light, tone, alpha, planes, planes_view
    if call == "item":
        fh = C.c_void_p()
        assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
        try:
            item = L.hm_file_primary_item(fh)
            fn = getattr(L, "hm_decode_item_to_device" + ("" if kind == "dest" else "_" + kind))
            rc = fn(fh, item, C.byref(prm), *steps, arr, out)
            msg = L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
        return [rc, msg, None]
    if call == "seq":
        fh = C.c_void_p()
        assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
        try:
            ids = (C.c_uint32 * n)(*over.get("frames", [1, 2, 3]))
            if family == "seq_dest":
                rc = L.hm_decode_sequence_to_device(fh, over.get("first", 1), n, C.byref(prm), arr, out, C.byref(failed))
            else:
                rc = getattr(L, "hm_decode_frames_to_device_" + kind)(fh, ids, n, C.byref(prm), *steps, arr, out, C.byref(failed))
            msg = L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
        return [rc, msg, failed.value]
    p = pipelines(fmt)
    if not p:  # (the pipeline itself refuses this out_format)
        return [pipelines.refused[fmt][0], pipelines.refused[fmt][1], None]
    rc = getattr(L, "hm_pipeline_submit_to_device" + ("" if kind == "dest" else "_" + kind))(p, blob, len(blob), 0, 1, *steps, arr)
    return [rc, L.hm_last_error().decode(), None]


def walk(capi, L, call_kinds, pipelines=None):
    """{"case | family": [status, message, failed_frame]} for every case x family whose call is one of call_kinds"""
    data = files()
    got = {}
    for name, families, over in CASES:
        for family in families:
            if FAMILIES[family]["call"] in call_kinds and (name, family) not in BEHIND_THE_PROBE:
                got[f"{name} | {family}"] = run(capi, L, data, family, over, pipelines)
    return got


class Pipelines:
    """one pipeline per out_format, created when first asked for (a device must exist)"""

    def __init__(self, capi, L):
        self.capi, self.L, self.made, self.refused = capi, L, {}, {}

    def __call__(self, fmt):
        if fmt not in self.made:
            p = C.c_void_p()
            cfg = self.capi.PipelineConfig(1, 2, fmt, 0, 0, 0, -1, 0, 0)
            rc = self.L.hm_pipeline_create(C.byref(cfg), C.byref(p))
            if rc:
                self.refused[fmt] = (rc, self.L.hm_last_error().decode())
            self.made[fmt] = p if rc == 0 else None
        return self.made[fmt]

    def close(self):
        for p in self.made.values():
            if p:
                self.L.hm_pipeline_destroy(p)
        self.made = {}
