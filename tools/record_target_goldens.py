"""Writes the characterisation files of the output-target plumbing from the library as it is built now:
    tests/golden/target_refusals.json   (tests/test_target_refusals.py; needs no GPU)
    tests/golden/emit_fields.json       (tests/test_emit_fields_gpu.py; --gpu, on a machine with one)
    tests/golden/emit_fields_steps.json (the same test file and switch: the tone and alpha steps)
Run it on a commit whose behaviour is the one to keep, then commit the files: a refactor must reproduce them byte for byte.

    python tools/record_target_goldens.py --record [--gpu] [--out-dir DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--gpu", action="store_true", help="record emit_fields.json (and the pipeline's refusals in it) instead")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import __graft_entry__ as g
    import emit_cases
    import target_cases
    capi = g.load_package().capi
    L = capi.image_lib()
    if not args.gpu:
        dump(os.path.join(args.out_dir, "target_refusals.json"), target_cases.walk(capi, L, ("item", "seq", "tensor")))
        return
    pipes = target_cases.Pipelines(capi, L)
    try:
        refusals = target_cases.walk(capi, L, ("pipe",), pipes)
    finally:
        pipes.close()
    dump(os.path.join(args.out_dir, "emit_fields.json"), {"decodes": emit_cases.walk(capi, L), "pipeline_refusals": refusals})
    dump(os.path.join(args.out_dir, "emit_fields_steps.json"), emit_cases.walk_steps(capi, L))


if __name__ == "__main__":
    main()
