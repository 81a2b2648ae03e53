"""Every wrong output-target request of tests/target_cases.py, through every item and sequence entry point that takes it: status,
hm_last_error() and failed_frame are those recorded in tests/golden/target_refusals.json (tools/record_target_goldens.py).  This
pins which refusal wins when a request is wrong in two ways, the text of each, and which of the sequence forms name a frame.
All of it is decided before the library asks for a device, so the file is the same with and without a GPU; the pipeline's
submit calls need a device to exist and are walked by tests/test_emit_fields_gpu.py."""
import json
import os

import pytest

import target_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_refusals.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(pkg):
    return target_cases.walk(pkg.capi, pkg.capi.image_lib(), ("item", "seq", "tensor"))


def test_every_case_is_decided_before_the_device_probe(recorded):
    assert recorded and all(v[0] < 0 and v[0] != target_cases.HM_ERR_NO_DEVICE for v in recorded.values())


def test_the_table_and_the_file_name_the_same_requests(recorded, got):
    assert sorted(got) == sorted(recorded)
    wanted = {name for name, _, _ in target_cases.CASES}
    assert {k.split(" | ")[0] for k in recorded} == wanted


def test_refusals_are_the_recorded_ones(recorded, got):
    wrong = {k: (got[k], recorded[k]) for k in recorded if got.get(k) != recorded[k]}
    assert not wrong, "\n".join(f"{k}: got {g}, recorded {r}" for k, (g, r) in wrong.items())
