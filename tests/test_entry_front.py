"""The front of the device entry points: which step pointers an entry requires, which "<step>: null light step" it answers, what a
call refused there leaves in failed_frame and in *out - for every entry of the item, frames and stand-alone tensor families and every
subset of its step pointers passed as NULL (tests/entry_front_cases.py), against tests/golden/entry_front.json
(tools/record_entry_front.py, recorded from the entries as each family wrote them out by hand).  All of it is decided before the
library asks for a device.  The pipeline family needs a device to exist: its part of the record was taken on a machine with one and is
walked by the test marked gpu - every submission is refused before anything is queued.

And the table the Python layer picks an entry by (capi.ENTRY_KINDS): for every family and every combination of steps that goes
together, the entry and the order of its step arguments are those of the if / elif ladders decode.py had, written out here arm by arm."""
import itertools
import json
import os

import pytest

import entry_front_cases as cases
import target_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_front.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def compare(got, recorded, calls):
    wanted = [cases.case_id(e, null) for call in calls for e, _, null in cases.rows(call)]
    assert len(set(wanted)) == len(wanted)
    assert sorted(recorded) == sorted(wanted), "the record and the matrix name different calls"
    assert sorted(got) == sorted(wanted), "a row of the matrix was not run"
    wrong = {k: (got[k], recorded[k]) for k in wanted if got[k] != recorded[k]}
    assert not wrong, "\n".join(f"{k}: got {g}, recorded {r}" for k, (g, r) in wrong.items())


def test_the_matrix_is_every_subset_of_every_entry():
    n = {call: len(cases.rows(call)) for call in ("item", "seq", "tensor", "pipe")}
    # 2 ** (number of step arguments), summed over the entries: item and pipeline 1 + 2 + 4 + 8 + 16 + 32 + 16 + 1 + 2; frames
    # 2 + 4 + 8 + 16 + 1 + 2 and hm_decode_sequence_to_device; tensor 1 + 2 + 4 + 8 + 16 + 32 + 16
    assert n == {"item": 82, "seq": 34, "tensor": 79, "pipe": 82}


def test_item_frames_and_tensor_entries_answer_as_recorded(pkg, recorded):
    got = cases.walk(pkg.capi, pkg.capi.image_lib(), ("item", "seq", "tensor"))
    compare(got, recorded["host"], ("item", "seq", "tensor"))


def test_the_record_sees_every_kind_of_answer(recorded):
    host = recorded["host"]
    fronts = {v["front"] for v in host.values()}
    assert fronts == {"null argument", "tone: null light step", "ootf: null light step", "gain: null light step", cases.PASSED}
    assert all(("out" in v) == (v["front"] != cases.PASSED) for k, v in host.items() if "_to_device" in k)
    frames = {k: v for k, v in host.items() if "hm_decode_frames" in k or "hm_decode_sequence" in k}
    assert all(("failed_frame" in v) == (k in frames and v["front"] != cases.PASSED) for k, v in host.items())
    assert {v["failed_frame"] for v in frames.values() if "failed_frame" in v} == {-1}  # (set before any check, whatever the refusal)


@pytest.mark.gpu
def test_pipeline_entries_answer_as_recorded(pkg, recorded):
    capi, L = pkg.capi, pkg.capi.image_lib()
    pipes = target_cases.Pipelines(capi, L)
    try:
        got = cases.walk(capi, L, ("pipe",), pipes)
        assert all(L.hm_pipeline_pending(p) == 0 for p in pipes.made.values() if p)  # nothing was queued
    finally:
        pipes.close()
    compare(got, recorded["pipeline"], ("pipe",))


# ---- the Python table ---------------------------------------------------------------------------------------------------------------
# (steps present, suffix of the entry, its step arguments in order): decode_to_tensor's and decode_batch_to_tensor's ladders, which were
# the same arm by arm - gain, ootf, alpha, tone, light, then the plain entry without a view and _view with one
ITEM_AND_PIPELINE = [
    ("", "", ""),
    ("view", "_view", "view"),
    ("alpha", "_alpha", "view light tone alpha"),
    ("view alpha", "_alpha", "view light tone alpha"),
    ("light", "_light", "view light"),
    ("view light", "_light", "view light"),
    ("light alpha", "_alpha", "view light tone alpha"),
    ("view light alpha", "_alpha", "view light tone alpha"),
    ("light ootf", "_ootf", "view light ootf tone alpha"),
    ("view light ootf", "_ootf", "view light ootf tone alpha"),
    ("light alpha ootf", "_ootf", "view light ootf tone alpha"),
    ("view light alpha ootf", "_ootf", "view light ootf tone alpha"),
    ("light gain", "_gain", "view light tone gain"),
    ("view light gain", "_gain", "view light tone gain"),
    ("light tone", "_tone", "view light tone"),
    ("view light tone", "_tone", "view light tone"),
    ("light tone alpha", "_alpha", "view light tone alpha"),
    ("view light tone alpha", "_alpha", "view light tone alpha"),
    ("light tone ootf", "_ootf", "view light ootf tone alpha"),
    ("view light tone ootf", "_ootf", "view light ootf tone alpha"),
    ("light tone alpha ootf", "_ootf", "view light ootf tone alpha"),
    ("view light tone alpha ootf", "_ootf", "view light ootf tone alpha"),
    ("light tone gain", "_gain", "view light tone gain"),
    ("view light tone gain", "_gain", "view light tone gain"),
]
# decode_sequence_to_tensor's ladder: ootf, tone, light, else _view - with the view or with NULL (the family has no plain entry, and no
# alpha or gain step)
FRAMES = [
    ("", "_view", "view"),
    ("view", "_view", "view"),
    ("light", "_light", "view light"),
    ("view light", "_light", "view light"),
    ("light tone", "_tone", "view light tone"),
    ("view light tone", "_tone", "view light tone"),
    ("light ootf", "_ootf", "view light ootf tone"),
    ("view light ootf", "_ootf", "view light ootf tone"),
    ("light tone ootf", "_ootf", "view light ootf tone"),
    ("view light tone ootf", "_ootf", "view light ootf tone"),
]
PLANES = [("", "_planes", ""), ("view", "_planes_view", "view")]  # the three planes functions: _planes without a view, else _planes_view
LADDERS = {"hm_decode_item_to_device": ITEM_AND_PIPELINE, "hm_pipeline_submit_to_device": ITEM_AND_PIPELINE, "hm_decode_frames_to_device": FRAMES}


def allowed(names):
    """every combination of the steps `names` that goes together: tone, gain and ootf need light; gain excludes alpha and ootf"""
    for n in range(len(names) + 1):
        for combo in itertools.combinations(names, n):
            s = set(combo)
            if (s & {"tone", "gain", "ootf"} and "light" not in s) or ("gain" in s and s & {"alpha", "ootf"}):
                continue
            yield frozenset(s)


@pytest.mark.parametrize("family", sorted(LADDERS))
def test_the_table_picks_the_entries_the_ladders_picked(pkg, family):
    capi, ladder = pkg.capi, LADDERS[family]
    names = ("view", "light", "tone", "ootf") if family == "hm_decode_frames_to_device" else ("view", "light", "tone", "alpha", "gain", "ootf")
    assert sorted(map(sorted, (frozenset(p.split()) for p, _, _ in ladder))) == sorted(map(sorted, allowed(names)))
    for present, suffix, args in ladder:
        assert capi.entry_of(family, set(present.split())) == (family + suffix, args.split()), present
    for present, suffix, args in PLANES:
        assert capi.entry_of(family, set(present.split()), planes=True) == (family + suffix, args.split()), present


# the argument types bind_image gave every entry when each was declared on a line of its own: the family's head, the step pointers of the
# kind (names of capi's structures), the family's tail
HEADS = {"hm_decode_item_to_device": "c_void_p c_uint32 *DecodeParams", "hm_decode_frames_to_device": "c_void_p *c_uint32 c_int32 *DecodeParams",
         "hm_pipeline_submit_to_device": "c_void_p c_char_p c_size_t c_uint32 c_uint64"}
TAILS = {"hm_decode_item_to_device": "*{dest} *Decoded", "hm_decode_frames_to_device": "*{dest} *Decoded *c_int32", "hm_pipeline_submit_to_device": "*{dest}"}
STEPS = {"": "", "_view": "*DeviceView", "_light": "*DeviceView *DeviceLight", "_tone": "*DeviceView *DeviceLight *DeviceTone",
         "_alpha": "*DeviceView *DeviceLight *DeviceTone *DeviceAlpha", "_ootf": "*DeviceView *DeviceLight *DeviceOotf *DeviceTone *DeviceAlpha",
         "_gain": "*DeviceView *DeviceLight *DeviceTone *DeviceGain", "_planes": "", "_planes_view": "*DeviceView"}
FRAMES_STEPS = dict(STEPS, _ootf="*DeviceView *DeviceLight *DeviceOotf *DeviceTone")  # (the frames family has no alpha step)
FRAMES_LACKS = ("", "_alpha", "_gain")


def test_every_entry_is_exported_and_bound_to_its_own_types(pkg):
    import ctypes as C
    capi = pkg.capi
    L = capi.image_lib()

    def types(text):
        return [C.POINTER(getattr(capi, t[1:], None) or getattr(C, t[1:])) if t.startswith("*") else getattr(C, t) for t in text.split()]
    bound = 0
    for family in HEADS:
        frames = family == "hm_decode_frames_to_device"
        for suffix, steps in (FRAMES_STEPS if frames else STEPS).items():
            if frames and suffix in FRAMES_LACKS:
                assert not hasattr(L, family + suffix)
                continue
            dest = "DevicePlanes" if "_planes" in suffix else "DeviceDest"
            want = types(HEADS[family]) + types(steps) + types(TAILS[family].format(dest=dest))
            assert getattr(L, family + suffix).argtypes == want, family + suffix  # (AttributeError: no such export)
            bound += 1
    assert bound == 9 + 6 + 9
