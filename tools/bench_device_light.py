#!/usr/bin/env python3
"""The light step (hm_device_light), timed kernel by kernel (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_light.py --run --manifest DIR/manifest.json
    python3 tools/bench_device_light.py --summarise DIR --out profiles/device_light.txt

--run queues, on one 4032 x 3024 RGB24 image in device memory:
  1. pointwise, to CHW float32: hm_to_tensor (k_to_tensor) and hm_light_to_tensor (k_light_tensor, sRGB -> linear light), five
     repeats each, alternating, behind two warm-up launches of each; the light kernel on a source of random samples (every lookup of a
     wave meets another table entry: the worst case for LDS bank conflicts) and on a smooth one (a photograph's neighbours mostly share
     entries);
  2. the 12 MP -> 224 x 224 HM_VIEW_TRIANGLE view: hm_resample_to_tensor (k_resample_h + k_resample_v) and hm_light_to_tensor under
     the same view (k_light_h + k_light_v), five repeats each, alternating.
It times nothing itself: the kernel times are the profiler's.  --summarise reads the trace, matches the dispatches to the manifest in
launch order and prints both tables; nothing here is a pass / fail check."""
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

W, H = 4032, 3024
RGB, CHW, F32 = 10, 1, 3
REPEATS, WARM = 5, 2
KERNELS = ("k_to_tensor", "k_light_tensor", "k_resample_h", "k_resample_v", "k_light_h", "k_light_v")


def run(manifest_path):
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
    lt = capi.DeviceLight(13, 1, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    view = capi.DeviceView(0, 0, 0, 0, 224, 224, 0)

    def plain(src, label):
        capi.check_image(L.hm_to_tensor(RGB, W, H, src.data_ptr(), stride, C.byref(d_full), st))
        manifest.append((label, ["k_to_tensor"]))

    def light(src, label):
        capi.check_image(L.hm_light_to_tensor(RGB, 8, W, H, src.data_ptr(), stride, None, C.byref(lt), C.byref(d_full), st))
        manifest.append((label, ["k_light_tensor"]))

    def plain_view(src, label):
        capi.check_image(L.hm_resample_to_tensor(RGB, W, H, src.data_ptr(), stride, C.byref(view), C.byref(d_small), st))
        manifest.append((label, ["k_resample_h", "k_resample_v"]))

    def light_view(src, label):
        capi.check_image(L.hm_light_to_tensor(RGB, 8, W, H, src.data_ptr(), stride, C.byref(view), C.byref(lt), C.byref(d_small), st))
        manifest.append((label, ["k_light_h", "k_light_v"]))
    for _ in range(WARM):
        for fn in (plain, light, plain_view, light_view):
            fn(noise, "warm-up")
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        plain(noise, "pointwise k_to_tensor")
        light(noise, "pointwise k_light_tensor, random samples")
        light(smooth, "pointwise k_light_tensor, smooth image")
        torch.cuda.synchronize()
    for _ in range(REPEATS):
        plain_view(noise, "view k_resample_h + k_resample_v")
        light_view(noise, "view k_light_h + k_light_v, random samples")
        light_view(smooth, "view k_light_h + k_light_v, smooth image")
        torch.cuda.synchronize()
    with open(manifest_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "launches": manifest}, f)
    print(f"{len(manifest)} calls queued; manifest in {manifest_path}")


def short_name(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k + "<" in name or k + "(" in name or name.endswith(k):
            return k
    return None


def summarise(folder, out):
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
    if [k for _, k in want] != [r[2] for r in rows]:
        sys.exit(f"the trace has {len(rows)} dispatches of the kernels, the manifest {len(want)}: they do not match")
    times, full_names = {}, {}
    for (label, k), (t0, t1, _, full) in zip(want, rows):
        if label != "warm-up":
            times.setdefault(label, {}).setdefault(k, []).append((t1 - t0) / 1e3)
            m = re.search(r"k_\w+<[^>]*>", full)
            full_names[k] = m.group(0) if m else k
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} RGB24 image in device memory, destination CHW float32 (3 + 12 bytes per pixel pointwise)"]

    def med(v):
        return sorted(v)[len(v) // 2]
    for label in times:
        total = [sum(v) for v in zip(*times[label].values())]
        parts = ", ".join(f"{k} {med(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times[label].items())
        lines.append(f"  {label:48s} {med(total):8.1f} ({min(total):.1f} .. {max(total):.1f})" + (f"   [{parts}]" if len(times[label]) > 1 else ""))
    lines.append("instances: " + "; ".join(sorted(full_names.values())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--manifest", default="manifest.json")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        run(args.manifest)
    if args.summarise:
        summarise(args.summarise, args.out)


if __name__ == "__main__":
    main()
