#!/usr/bin/env python3
"""The light step with an ICC profile as its source, timed kernel by kernel against the step as it was (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_icc.py --run [--icc] [--tree TREE] --manifest DIR/manifest.json
    python3 tools/bench_device_icc.py --summarise LABEL=DIR [LABEL=DIR ...] --out profiles/icc_light_step.txt

--run queues, on one 4032 x 3024 RGB24 image in device memory (random samples, and a smooth image), behind two warm-up launches each:
  pointwise to CHW float32 (k_light_tensor) and the 12 MP -> 224 x 224 HM_VIEW_TRIANGLE view (k_light_h + k_light_v), sRGB codes as
  the source - one table, the path every build has; with --icc also a writer-made Display P3 profile (one curve: one table, the
  same path) and one with three distinct curves (three tables), through hm_icc_to_tensor.
--tree: the checkout whose library is loaded (default: this one) - a build of the parent commit, to time the one-table path in both.
Two runs of each tree in one session, alternating, give the run-to-run spread the difference is judged by.
It times nothing itself: the kernel times are the profiler's.  Nothing here is a pass / fail check."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 4032, 3024
RGB, CHW, F32 = 10, 1, 3
REPEATS, WARM = 10, 2
KERNELS = ("k_light_tensor", "k_light_h", "k_light_v")


def run(manifest_path, tree, icc):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    st = torch.cuda.current_stream().cuda_stream
    stride = capi.lib().hm_plane_stride(W, 3)
    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.randint(0, 256, (H, stride), dtype=torch.uint8, device="cuda", generator=gen)
    yy = torch.arange(H, device="cuda").view(H, 1).float()
    xx = (torch.arange(stride, device="cuda") // 3).view(1, stride).float()
    smooth = ((yy * (255.0 / H) + xx * (255.0 / W)) / 2).to(torch.uint8).contiguous()
    manifest = []

    def dest_of(t):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        return d
    full = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    small = torch.empty((3, 224, 224), dtype=torch.float32, device="cuda")
    d_full, d_small = dest_of(full), dest_of(small)
    codes = capi.DeviceLight(13, 1, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    view = capi.DeviceView(0, 0, 0, 0, 224, 224, 0)
    calls = [("codes, one table", None)]
    if icc:
        import icc_cases
        from_icc = capi.DeviceLight(-1, -1, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
        calls += [("profile, one curve: one table", icc_cases.display_p3()), ("profile, three curves: three tables", icc_cases.three_curves())]

    def light(src, what, prof, v, d, kernels, label):
        if prof is None:
            capi.check_image(L.hm_light_to_tensor(RGB, 8, W, H, src.data_ptr(), stride, C.byref(v) if v is not None else None, C.byref(codes), C.byref(d), st))
        else:
            capi.check_image(L.hm_icc_to_tensor(RGB, 8, W, H, src.data_ptr(), stride, C.byref(v) if v is not None else None, prof, len(prof), C.byref(from_icc), None, None,
                                                C.byref(d), st))
        manifest.append((label, kernels))
    shapes = [(None, d_full, ["k_light_tensor"], "pointwise k_light_tensor"), (view, d_small, ["k_light_h", "k_light_v"], "view k_light_h + k_light_v")]
    for _ in range(WARM):
        for what, prof in calls:
            for v, d, kernels, _ in shapes:
                light(noise, what, prof, v, d, kernels, "warm-up")
    torch.cuda.synchronize()
    for v, d, kernels, shape in shapes:
        for _ in range(REPEATS):
            for what, prof in calls:
                for src, sname in ((noise, "random samples"), (smooth, "smooth image")):
                    light(src, what, prof, v, d, kernels, f"{shape}, {sname}, {what}")
            torch.cuda.synchronize()
    with open(manifest_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "launches": manifest}, f)
    print(f"{len(manifest)} calls queued; manifest in {manifest_path}")


def short_name(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k + "<" in name or k + "(" in name or name.endswith(k):
            return k
    return None


def read_run(folder):
    """label -> kernel -> [us]"""
    with open(os.path.join(folder, "manifest.json")) as f:
        manifest = json.load(f)
    rows = []
    for base, _, files in os.walk(folder):
        for name in files:
            if name.endswith("kernel_trace.csv"):
                with open(os.path.join(base, name), newline="") as f:
                    for r in csv.DictReader(f):
                        k = short_name(r["Kernel_Name"])
                        if k:
                            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    rows.sort()
    want = [(label, k) for label, kernels in manifest["launches"] for k in kernels]
    if [k for _, k in want] != [r[2] for r in rows]:
        sys.exit(f"{folder}: the trace has {len(rows)} dispatches of the kernels, the manifest {len(want)}: they do not match")
    times = {}
    for (label, k), (t0, t1, _) in zip(want, rows):
        if label != "warm-up":
            times.setdefault(label, {}).setdefault(k, []).append((t1 - t0) / 1e3)
    return manifest["device"], times


def summarise(runs, out):
    med = lambda v: sorted(v)[len(v) // 2]
    data, device = [], ""
    for spec in runs:
        name, folder = spec.split("=", 1)
        device, times = read_run(folder)
        data.append((name, times))
    lines = [f"device: {device or 'MI355X'}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches per process, in us: median (min .. max)",
             f"source: one {W} x {H} RGB24 image in device memory; pointwise to CHW float32, and the 224 x 224 HM_VIEW_TRIANGLE view of it",
             "runs: processes of one session in this order, the parent commit's build and this one alternating: " + ", ".join(n for n, _ in data), ""]
    labels = []
    for _, times in data:
        for label in times:
            if label not in labels:
                labels.append(label)
    for label in labels:
        lines.append(label)
        for name, times in data:
            if label in times:
                for k, v in times[label].items():
                    if k != "k_light_v":  # (the vertical pass holds no lin)
                        lines.append(f"    {name:14s} {k:15s} {med(v):8.1f} ({min(v):.1f} .. {max(v):.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--icc", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--manifest", default="manifest.json")
    ap.add_argument("--summarise", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        run(args.manifest, os.path.abspath(args.tree), args.icc)
    if args.summarise:
        summarise(args.summarise, args.out)


if __name__ == "__main__":
    main()
