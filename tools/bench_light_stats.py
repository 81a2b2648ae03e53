#!/usr/bin/env python3
"""The light statistics (hm_light_stats_of_tensor), timed kernel by kernel beside the pointwise light step (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_light_stats.py --run --manifest DIR/manifest.json
    rocprofv3 --kernel-trace --stats -d DIR0 --output-format csv -- python3 tools/bench_light_stats.py --run --lib PARENT.so --manifest DIR0/manifest.json
    python3 tools/bench_light_stats.py --summarise DIR [--baseline DIR0] --out profiles/light_stats.txt

--run queues, on one 4032 x 3024 RRGGBB_LE image of 10-bit PQ BT.2020 samples in device memory, for each of three contents - flat (one
code everywhere: all 64 lanes of every wave count into one bin), uniform noise (every lane another bin, and another table entry), a
decoded photograph of the fixtures (tests/data/example.heic) tiled up to that size - five repeats, alternating, behind two warm-up
launches of each:
  1. hm_light_stats_of_tensor (k_light_stats<2, 3, true>);
  2. hm_light_to_tensor to HWC float16, linear light (k_light_tensor<2, 3, __half, false, true>): the yardstick - the pointwise pass that
     reads the same bytes through the same table.
--lib PATH runs the yardstick alone on another build of the library (the parent commit's).
It times nothing itself: the kernel times are the profiler's.  --summarise reads the trace, matches the dispatches to the manifest in
launch order and prints the table and the three ratios; nothing here is a pass / fail check."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, BITS = 4032, 3024, 10
RRGGBB_LE, HWC, F16 = 14, 0, 2
REPEATS, WARM = 5, 2
KERNELS = ("k_light_stats", "k_light_tensor")
CONTENTS = ("flat", "noise", "photograph")


def contents(pkg, torch, stride):
    """name -> H x stride / 2 int16 tensor of 10-bit codes"""
    out = {}
    out["flat"] = torch.full((H, stride // 2), 517, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    out["noise"] = torch.randint(0, 1 << BITS, (H, stride // 2), dtype=torch.int16, device="cuda", generator=gen)
    with open(os.path.join(ROOT, "tests", "data", "example.heic"), "rb") as f:
        photo = pkg.decode_to_tensor(f.read(), out_format="rrggbb_le", layout="hwc", dtype=torch.uint16).view(torch.int16)  # (8-bit pictures come as 10-bit codes)
    ph, pw, _ = photo.shape
    tiled = photo.repeat((H + ph - 1) // ph, (W + pw - 1) // pw, 1)[:H, :W].reshape(H, W * 3)
    t = torch.zeros((H, stride // 2), dtype=torch.int16, device="cuda")
    t[:, :W * 3] = tiled
    out["photograph"] = t
    return out


def run(manifest_path, other_lib):
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    stride = capi.lib().hm_plane_stride(W, 6)
    src = contents(pkg, torch, stride)
    if other_lib:  # the yardstick on another build: only what both builds have is bound
        L = C.CDLL(other_lib)
        L.hm_light_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.DeviceView), C.POINTER(capi.DeviceLight),
                                         C.POINTER(capi.DeviceDest), C.c_void_p]
        L.hm_last_error.restype = C.c_char_p
    st = torch.cuda.current_stream().cuda_stream
    manifest = []
    half = torch.empty((H, W, 3), dtype=torch.float16, device="cuda")
    d = capi.DeviceDest()
    d.ptr, d.len, d.layout, d.dtype = half.data_ptr(), half.numel() * 2, HWC, F16
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    linear = capi.DeviceLight(16, 9, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    seen = {}

    def check(rc):
        if rc:
            sys.exit(f"status {rc}: {L.hm_last_error().decode()}")

    def stats(name, label):
        s = capi.LightStatsC()
        check(L.hm_light_stats_of_tensor(RRGGBB_LE, BITS, W, H, src[name].data_ptr(), stride, None, C.byref(linear), None, 0.0, C.byref(s), st))
        seen[name] = (int(s.pixels), sum(1 for v in s.hist if v), int(s.max_code), float(s.max_nits), float(s.average_nits))
        manifest.append((label, ["k_light_stats"]))

    def light(name, label):
        check(L.hm_light_to_tensor(RRGGBB_LE, BITS, W, H, src[name].data_ptr(), stride, None, C.byref(linear), C.byref(d), st))
        manifest.append((label, ["k_light_tensor"]))
    cases = []
    for name in CONTENTS:
        if not other_lib:
            cases.append((lambda lab, n=name: stats(n, lab), f"{name}: statistics"))
        cases.append((lambda lab, n=name: light(n, lab), f"{name}: light step to f16"))
    for _ in range(WARM):
        for fn, _label in cases:
            fn("warm-up")
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for fn, label in cases:
            fn(label)
        torch.cuda.synchronize()
    with open(manifest_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "launches": manifest, "seen": seen}, f)
    print(f"{len(manifest)} calls queued; manifest in {manifest_path}")


def short_name(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k + "<" in name or k + "(" in name or name.endswith(k):
            return k
    return None


def read(folder):
    """(device, label -> [us], kernel instance names, what the statistics saw) of one profiled run"""
    with open(os.path.join(folder, "manifest.json")) as f:
        manifest = json.load(f)
    rows, device = [], manifest["device"]
    for base, _, files in os.walk(folder):
        for name in files:
            if name.endswith("agent_info.csv") and not device:  # (torch may not know the product's name: the profiler's agent table does)
                with open(os.path.join(base, name), newline="") as f:
                    gpus = [r for r in csv.DictReader(f) if r.get("Agent_Type") == "GPU"]
                if gpus:
                    device = f"{gpus[0].get('Name', '')}, {gpus[0].get('Cu_Count', '?')} CUs"
            if name.endswith("kernel_trace.csv"):
                with open(os.path.join(base, name), newline="") as f:
                    for r in csv.DictReader(f):
                        k = short_name(r["Kernel_Name"])
                        if k:
                            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, r["Kernel_Name"]))
    rows.sort()
    want = [(label, k) for label, kernels in manifest["launches"] for k in kernels]
    rows = rows[len(rows) - len(want):]  # (in front of them: the decode of the photograph, whose write is a k_light-free path, or not)
    if [k for _, k in want] != [r[2] for r in rows]:
        sys.exit(f"{folder}: the trace has {len(rows)} dispatches of the kernels, the manifest {len(want)}: they do not match")
    times, names = {}, set()
    for (label, k), (t0, t1, _, full) in zip(want, rows):
        if label != "warm-up":
            times.setdefault(label, []).append((t1 - t0) / 1e3)
            m = re.search(r"k_\w+<[^>]*>", full)
            names.add(m.group(0) if m else k)
    return device, times, names, manifest.get("seen", {})


def med(v):
    return sorted(v)[len(v) // 2]


def table(times, tag):
    return [f"  {tag + label:48s} {med(v):8.1f} ({min(v):.1f} .. {max(v):.1f})" for label, v in times.items()]


def summarise(folder, baseline, out):
    device, times, names, seen = read(folder)
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} RRGGBB_LE image of {BITS}-bit PQ samples in device memory (6 bytes per pixel, {W * H * 6 / 1e6:.1f} MB)"]
    for name, (pixels, bins, max_code, max_nits, avg) in seen.items():
        lines.append(f"  {name}: {pixels} pixels in {bins} bins, max_code {max_code}, max_nits {max_nits:.6g}, average_nits {avg:.6g}")
    lines += table(times, "")
    t0 = None
    if baseline:
        _, t0, _, _ = read(baseline)
        lines.append("the yardstick on the parent commit's build (its margin is the spread of its repeats):")
        lines += table(t0, "parent: ")
    lines.append("ratios, statistics / yardstick" + (" of the parent commit's build" if t0 else "") + " (medians):")
    for name in CONTENTS:
        y = (t0 or times)[f"{name}: light step to f16"]
        s = times[f"{name}: statistics"]
        lines.append(f"  {name:12s} {med(s) / med(y):.2f}   ({W * H * 6 / med(s) / 1e3:.0f} GB/s of source bytes against {W * H * 6 / med(y) / 1e3:.0f})")
    lines.append("instances: " + "; ".join(sorted(names)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--manifest", default="manifest.json")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        run(args.manifest, args.lib)
    if args.summarise:
        summarise(args.summarise, args.baseline, args.out)


if __name__ == "__main__":
    main()
