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
RGB, RGBA, RRGGBB_BE, RRGGBBAA_BE, RRGGBB_LE = 10, 11, 12, 13, 14
HWC, CHW = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
TRIANGLE, NEAREST, CUBIC, LANCZOS3 = 0, 1, 16, 17
N_FRAMES = 3
SENTINEL = 7  # what failed_frame holds before a call

# families: the picture they decode, whether the destination is planes, whether they take a view / a light step / frame IDs
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
}


def _fam(**want):
    return [n for n, f in FAMILIES.items() if all((f.get(k) if k == "call" else bool(f.get(k))) == v for k, v in want.items())]


EVERY = list(FAMILIES)
DEST, PLANES, VIEW, LIGHT = _fam(planes=False), _fam(planes=True), _fam(view=True), _fam(light=True)
DEST_VIEW = [n for n in DEST if n in VIEW]
GOOD_VIEW = ((4, 2, 10, 8), (5, 4), TRIANGLE)  # crop, output size, filter
GOOD_LIGHT = (0, 0, 8, 0, 1.0)                # the image's own codes to linear light

# name, families, overrides: fmt (dest families) / pfmt (planes families), dest={} (every_dest={}: of every frame), planes={}, view=, light=, ext_dst, frames=, first=,
# picture="wide" (176 x 16, the one case a 16 x 16 picture cannot express)
CASES = [
    ("ext_dst set", [n for n in EVERY if not n.startswith("pipe_")], dict(ext_dst=True)),
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
    ("two faults: ext_dst and an unknown dtype", [n for n in DEST if not n.startswith("pipe_")], dict(ext_dst=True, dest=dict(dtype=9))),
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


def run(capi, L, data, family, over, pipelines=None):
    """one request through one family: [status, message, failed_frame | None]"""
    fam = FAMILIES[family]
    planes, lit = bool(fam.get("planes")), bool(fam.get("light"))
    wide = over.get("picture") == "wide"
    blob = data[("wide" if wide else "") + fam["call"]]
    fmt = over.get("pfmt", 0) if planes else over.get("fmt", RGB)
    view = over.get("view", GOOD_VIEW) if fam.get("view") else None
    w, h = view[1] if view and view[1] != (0, 0) and min(view[1]) > 0 else (176 if wide else 16, 16)
    pv = C.byref(make_view(capi, view)) if view else None
    plight = C.byref(make_light(capi, over.get("light", GOOD_LIGHT))) if lit else None
    host = (C.c_uint8 * 4096)()
    n = N_FRAMES if fam["call"] == "seq" else 1
    bad = 1 if n > 1 else 0  # (a sequence: the wrong destination is that of the second frame)
    if planes:
        arr = (capi.DevicePlanes * n)(*[make_planes(capi, L, w, h, **(over.get("planes", {}) if k == bad else {})) for k in range(n)])
    else:
        good = dict(dtype=(U16 if fmt >= RRGGBB_BE else U8) if not lit else F32)
        good.update(over.get("every_dest", {}))
        kw = dict(good)
        kw.update(over.get("dest", {}))
        arr = (capi.DeviceDest * n)(*[make_dest(capi, L, fmt, w, h, **(kw if k == bad else good)) for k in range(n)])
    prm = capi.DecodeParams(fmt, 1, 0, 0, None, C.cast(host, C.c_void_p) if over.get("ext_dst") else None, 4096 if over.get("ext_dst") else 0,
                            64 if over.get("ext_dst") else 0, 0, 0)
    out = (capi.Decoded * n)()
    failed = C.c_int32(SENTINEL)
    if fam["call"] == "item":
        fh = C.c_void_p()
        assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
        try:
            item = L.hm_file_primary_item(fh)
            args = {"item_dest": (arr,), "item_view": (pv, arr), "item_light": (pv, plight, arr), "item_planes": (arr,), "item_planes_view": (pv, arr)}[family]
            fn = getattr(L, "hm_decode_item_to_device" + ("" if family == "item_dest" else "_" + family[len("item_"):]))
            rc = fn(fh, item, C.byref(prm), *args, out)
            msg = L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
        return [rc, msg, None]
    if fam["call"] == "seq":
        fh = C.c_void_p()
        assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
        try:
            ids = (C.c_uint32 * n)(*over.get("frames", [1, 2, 3]))
            if family == "seq_dest":
                rc = L.hm_decode_sequence_to_device(fh, over.get("first", 1), n, C.byref(prm), arr, out, C.byref(failed))
            else:
                args = {"frames_view": (pv, arr), "frames_light": (pv, plight, arr), "frames_planes": (arr,), "frames_planes_view": (pv, arr)}[family]
                rc = getattr(L, "hm_decode_frames_to_device_" + family[len("frames_"):])(fh, ids, n, C.byref(prm), *args, out, C.byref(failed))
            msg = L.hm_last_error().decode()
        finally:
            L.hm_file_close(fh)
        return [rc, msg, failed.value]
    p = pipelines(fmt)
    if not p:  # (the pipeline itself refuses this out_format)
        return [pipelines.refused[fmt][0], pipelines.refused[fmt][1], None]
    args = {"pipe_dest": (arr,), "pipe_view": (pv, arr), "pipe_light": (pv, plight, arr), "pipe_planes": (arr,), "pipe_planes_view": (pv, arr)}[family]
    rc = getattr(L, "hm_pipeline_submit_to_device" + ("" if family == "pipe_dest" else "_" + family[len("pipe_"):]))(p, blob, len(blob), 0, 1, *args)
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
