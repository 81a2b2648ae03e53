"""GPU: the fields of hm_decoded (no pixels) for every picture x out_format x destination kind of tests/emit_cases.py - width,
height, bit_depth, chroma, out_format, the nclx values, has_alpha, used_ext_dst, the strides, the plane sizes, warnings - and
the status and message where the interface refuses the combination, against tests/golden/emit_fields.json
(tools/record_target_goldens.py --gpu) - and the same fields through the tone and alpha steps (emit_cases.walk_steps) against
tests/golden/emit_fields_steps.json.  With them, the refusal table of tests/target_cases.py through the pipeline's submit
calls, which need a device to exist."""
import json
import os

import pytest

import emit_cases
import target_cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emit_fields.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def differences(got, recorded):
    assert sorted(got) == sorted(recorded)
    return "\n".join(f"{k}: got {got[k]}, recorded {recorded[k]}" for k in recorded if got[k] != recorded[k])


def test_the_matrix_is_the_one_the_issue_names(recorded):
    keys = [k.split(" | ") for k in recorded["decodes"]]
    assert {k[0] for k in keys} == {"p420_8", "p420_10", "p444_8", "mono", "alpha", "grid", "iden", "iovl", "movie"}
    assert {k[2] for k in keys} == set(emit_cases.KINDS)
    assert {"0x0", "0x101", "0x103", "0x101+8", "0x103+8", "0xa", "0xb", "0xe", "0xd"} <= {k[1] for k in keys}
    assert any(v["status"] == 0 for v in recorded["decodes"].values()) and any(v["status"] < 0 for v in recorded["decodes"].values())


def test_fields_of_every_decode(pkg, recorded):
    got = json.loads(json.dumps(emit_cases.walk(pkg.capi, pkg.capi.image_lib())))
    assert not differences(got, recorded["decodes"])


def test_fields_of_every_decode_through_the_tone_and_alpha_steps(pkg):
    with open(os.path.join(os.path.dirname(GOLDEN), "emit_fields_steps.json")) as f:
        steps = json.load(f)
    keys = [k.split(" | ") for k in steps]
    assert {k[0] for k in keys} == set(emit_cases.STEP_PICTURES) and {k[2] for k in keys} == set(emit_cases.STEP_KINDS)
    assert {k[1] for k in keys} == {"0xa", "0xb", "0xe", "0xf"}
    assert all(any(v["status"] == 0 for k, v in steps.items() if k.endswith(kind)) for kind in emit_cases.STEP_KINDS)
    got = json.loads(json.dumps(emit_cases.walk_steps(pkg.capi, pkg.capi.image_lib())))
    assert not differences(got, steps)


def test_pipeline_refusals(pkg, recorded):
    L = pkg.capi.image_lib()
    pipes = target_cases.Pipelines(pkg.capi, L)
    try:
        got = json.loads(json.dumps(target_cases.walk(pkg.capi, L, ("pipe",), pipes)))
    finally:
        pipes.close()
    assert all(v[0] < 0 and v[0] != target_cases.HM_ERR_NO_DEVICE for v in recorded["pipeline_refusals"].values())
    assert not differences(got, recorded["pipeline_refusals"])
