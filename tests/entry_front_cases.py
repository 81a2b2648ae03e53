"""The matrix behind tests/test_entry_front.py - shared with tools/record_entry_front.py, which writes tests/golden/entry_front.json:
every device entry of the item, frames, stand-alone tensor and pipeline families, and for each one every subset of its step pointers
(view, light, ootf, tone, alpha, gain, as far as the entry has them) passed as NULL, the rest valid structs.

What an entry does with the pointers is decided before it asks for a device: the record holds "null argument", the exact
"<step>: null light step" message, or "passed the front" for any other outcome (the destinations are the fake device pointer of
target_cases: a request that passes the front is refused by the gain step's own rules, for want of a device, or by the pointer check -
nothing is ever queued).  For a call refused at the front it also holds whether *out was left alone ("untouched") or zeroed and, for
the frames family, what the call left in failed_frame (target_cases.SENTINEL before it)."""
import ctypes as C
import itertools

import target_cases as T

PASSED = "passed the front"
FILL = 0xA5  # what *out holds before a call

# suffix of the entry's name -> its step arguments in order
ITEM_ENTRIES = {"": (), "_view": ("view",), "_light": ("view", "light"), "_tone": ("view", "light", "tone"), "_alpha": ("view", "light", "tone", "alpha"),
                "_ootf": ("view", "light", "ootf", "tone", "alpha"), "_gain": ("view", "light", "tone", "gain"), "_planes": (), "_planes_view": ("view",)}
FRAMES_ENTRIES = {"_view": ("view",), "_light": ("view", "light"), "_tone": ("view", "light", "tone"), "_ootf": ("view", "light", "ootf", "tone"), "_planes": (),
                  "_planes_view": ("view",)}
TENSOR_ENTRIES = {"hm_to_tensor": (), "hm_resample_to_tensor": ("view",), "hm_light_to_tensor": ("view", "light"), "hm_tone_to_tensor": ("view", "light", "tone"),
                  "hm_alpha_to_tensor": ("view", "light", "tone", "alpha"), "hm_ootf_to_tensor": ("view", "light", "ootf", "tone", "alpha"),
                  "hm_gain_to_tensor": ("view", "light", "tone", "gain")}


def rows(call):
    """[(entry, its step arguments, the steps passed as NULL)] of one family: "item", "seq", "tensor" or "pipe" """
    if call == "tensor":
        entries = dict(TENSOR_ENTRIES)
    else:
        prefix = {"item": "hm_decode_item_to_device", "seq": "hm_decode_frames_to_device", "pipe": "hm_pipeline_submit_to_device"}[call]
        entries = {prefix + s: a for s, a in (FRAMES_ENTRIES if call == "seq" else ITEM_ENTRIES).items()}
        if call == "seq":
            entries["hm_decode_sequence_to_device"] = ()
    return [(e, a, null) for e, a in entries.items() for n in range(len(a) + 1) for null in itertools.combinations(a, n)]


def case_id(entry, null):
    return f"{entry} | null: {' '.join(null) or '-'}"


def make_step(capi, name):
    if name == "view":
        return T.make_view(capi, T.GOOD_VIEW)
    if name == "light":
        return T.make_light(capi, T.LINEAR)
    if name == "tone":
        return T.make_tone(capi, T.GOOD_TONE)
    if name == "alpha":
        return T.make_alpha(capi, T.alpha(T.STRAIGHT))
    if name == "ootf":
        return capi.DeviceOotf(capi.HM_OOTF_HLG, 1000.0, 0.0, (C.c_int32 * 5)())
    g = capi.DeviceGain()  # map_item 0: the decoded item's own map (the fixtures have no 'tmap' item: refused behind the front)
    g.headroom = 1.0
    g.params.alternate_headroom = 2.0
    for c in range(3):
        g.params.map_max[c], g.params.gamma[c] = 1.0, 1.0
        g.params.base_offset[c] = g.params.alternate_offset[c] = 1.0 / 64.0
    g.params.use_base_primaries = 1
    return g


def classify(rc, msg):
    if rc < 0 and (msg == "null argument" or msg.endswith(": null light step")):
        return msg
    return PASSED


def out_state(buf):
    raw = bytes(buf)
    return "untouched" if raw == bytes([FILL]) * len(raw) else "zeroed" if not any(raw) else "changed"


def run(capi, L, data, call, entry, args, null, pipelines=None):
    """one call: {"front": ...} and, refused at the front, "out": ... (where the entry has an *out) and "failed_frame": ... (frames)"""
    planes, with_alpha = "_planes" in entry, "alpha" in args and "alpha" not in null
    fmt = 0 if planes else T.RGBA if with_alpha else T.RGB
    structs = [None if a in null else make_step(capi, a) for a in args]
    steps = [None if s is None else C.byref(s) for s in structs]
    w, h = T.GOOD_VIEW[1] if "view" in args and "view" not in null else (16, 16)
    n = T.N_FRAMES if call == "seq" else 1
    if planes:
        arr = (capi.DevicePlanes * n)(*[T.make_planes(capi, L, w, h) for _ in range(n)])
    else:
        arr = (capi.DeviceDest * n)(*[T.make_dest(capi, L, fmt, w, h, dtype=T.F32 if "light" in args and "light" not in null else T.U8) for _ in range(n)])
    got = {}
    if call == "tensor":
        bits = () if entry in ("hm_to_tensor", "hm_resample_to_tensor") else (8,)
        gain_map = (T.FAKE + (1 << 24), 16, 16, 16, 8) if entry == "hm_gain_to_tensor" else ()  # d_map, map_stride, map_w, map_h, map_bits
        rc = getattr(L, entry)(fmt, *bits, 16, 16, T.FAKE, 16 * (4 if fmt == T.RGBA else 3), *gain_map, *steps, arr, None)
        return {"front": classify(rc, L.hm_last_error().decode())}
    prm = capi.DecodeParams(fmt, 1, 0, 0, None, None, 0, 0, 0, 0)
    out = (capi.Decoded * n)()
    C.memset(out, FILL, C.sizeof(out))
    blob = data[call]
    if call == "pipe":
        rc = getattr(L, entry)(pipelines(fmt), blob, len(blob), 0, 1, *steps, arr)
        return {"front": classify(rc, L.hm_last_error().decode())}
    fh = C.c_void_p()
    assert L.hm_file_open(blob, len(blob), C.byref(fh)) == 0
    try:
        if call == "item":
            rc = getattr(L, entry)(fh, L.hm_file_primary_item(fh), C.byref(prm), *steps, arr, out)
        else:
            failed = C.c_int32(T.SENTINEL)
            first = (1,) if entry == "hm_decode_sequence_to_device" else ((C.c_uint32 * n)(1, 2, 3),)
            rc = getattr(L, entry)(fh, *first, n, C.byref(prm), *steps, arr, out, C.byref(failed))
        got["front"] = classify(rc, L.hm_last_error().decode())
    finally:
        L.hm_file_close(fh)
    if got["front"] != PASSED:  # (behind the front the answer, and with it the frame it names, depends on whether there is a device)
        got["out"] = out_state(out)
        if call == "seq":
            got["failed_frame"] = failed.value
    return got


def walk(capi, L, calls, pipelines=None):
    """{case id: what run() saw} for every row of the families `calls`"""
    data = T.files()
    return {case_id(e, null): run(capi, L, data, call, e, a, null, pipelines) for call in calls for e, a, null in rows(call)}
