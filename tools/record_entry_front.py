"""Writes tests/golden/entry_front.json (tests/test_entry_front.py) from the library as it is built now: what every device entry does
with every subset of its step pointers passed as NULL (tests/entry_front_cases.py).  Run it on a commit whose behaviour is the one to
keep, then commit the file: a change to the entry front must reproduce it case by case.

    python tools/record_entry_front.py --record [--gpu] [--out-dir DIR]

Without --gpu the item, frames and tensor families are recorded (no device is needed) and the file's "pipeline" part is kept as it
is; with --gpu, on a machine with a device, the pipeline family is recorded and the rest is kept."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--gpu", action="store_true", help="record the pipeline family (needs a device)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import __graft_entry__ as g
    import entry_front_cases
    import target_cases
    capi = g.load_package().capi
    L = capi.image_lib()
    path = os.path.join(args.out_dir, "entry_front.json")
    record = {"host": {}, "pipeline": {}}
    if os.path.exists(path):
        with open(path) as f:
            record.update(json.load(f))
    if args.gpu:
        pipes = target_cases.Pipelines(capi, L)
        try:
            record["pipeline"] = entry_front_cases.walk(capi, L, ("pipe",), pipes)
        finally:
            pipes.close()
    else:
        record["host"] = entry_front_cases.walk(capi, L, ("item", "seq", "tensor"))
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
