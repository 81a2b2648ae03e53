#!/usr/bin/env python3
"""The alpha step (hm_device_alpha), timed kernel by kernel against the write of the same image without the step (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_alpha.py --run --manifest DIR/manifest.json
    python3 tools/bench_device_alpha.py --summarise DIR --out profiles/device_alpha.txt

--run queues, on one 4032 x 3024 RGBA32 image in device memory (random colour samples - every table lookup of a wave meets another
entry, the light step's worst case - under the alpha of a soft-rimmed disc), five repeats of each behind two warm-up launches, the
counterpart and its cases alternating:
  1. pointwise, to CHW float32: hm_to_tensor (k_to_tensor, four channels) and the HM_ALPHA_MATTE write (k_alpha_tensor, three);
  2. the 12 MP -> 512 x 384 HM_VIEW_TRIANGLE view: hm_resample_to_tensor (k_resample_h + k_resample_v) and the alpha step under the
     same view in each mode (k_alpha_h + k_alpha_v);
  3. the same view beside the light step (sRGB -> linear light): hm_light_to_tensor (k_light_h + k_light_v) and the alpha step beside
     it in each mode.
The counterparts are the kernels as they were before the step existed: it changes none of them.  The script times nothing itself: the
kernel times are the profiler's.  --summarise reads the trace, matches the dispatches to the manifest in launch order and prints each
case with its ratio to its counterpart; nothing here is a pass / fail check."""
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
OW, OH = 512, 384
RGBA, CHW, F32 = 11, 1, 3
REPEATS, WARM = 5, 2
MODES = (("straight", 1), ("premultiplied", 2), ("matte", 3))
KERNELS = ("k_to_tensor", "k_alpha_tensor", "k_resample_h", "k_resample_v", "k_light_h", "k_light_v", "k_alpha_h", "k_alpha_v")
POINT, VIEW, LIT = "pointwise hm_to_tensor (RGBA)", "view hm_resample_to_tensor (RGBA)", "view hm_light_to_tensor (RGBA)"


def run(manifest_path):
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    st = torch.cuda.current_stream().cuda_stream
    stride = W * 4
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda", generator=gen)
    yy = torch.arange(H, device="cuda").view(H, 1).float() - H / 2
    xx = torch.arange(W, device="cuda").view(1, W).float() - W / 2
    src[..., 3] = ((H * 0.45 - torch.sqrt(xx * xx + yy * yy)) * 2.0).clamp(0, 255).to(torch.uint8)
    src = src.contiguous()
    manifest = []

    def dest_of(t):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        return d
    full = torch.empty((4, H, W), dtype=torch.float32, device="cuda")
    small = torch.empty((4, OH, OW), dtype=torch.float32, device="cuda")
    d_full, d_small = dest_of(full), dest_of(small)
    lt = capi.DeviceLight(13, 1, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    view = capi.DeviceView(0, 0, 0, 0, OW, OH, 0)

    def alpha(mode):
        bg = (255, 255, 255, 0) if mode == capi.HM_ALPHA_MATTE else (0, 0, 0, 0)
        return capi.DeviceAlpha(mode, (C.c_uint16 * 4)(*bg), (C.c_int32 * 3)(0, 0, 0))

    def plain(label):
        capi.check_image(L.hm_to_tensor(RGBA, W, H, src.data_ptr(), stride, C.byref(d_full), st))
        manifest.append((label, ["k_to_tensor"]))

    def matte(label):
        al = alpha(capi.HM_ALPHA_MATTE)
        capi.check_image(L.hm_alpha_to_tensor(RGBA, 8, W, H, src.data_ptr(), stride, None, None, None, C.byref(al), C.byref(d_full), st))
        manifest.append((label, ["k_alpha_tensor"]))

    def plain_view(label):
        capi.check_image(L.hm_resample_to_tensor(RGBA, W, H, src.data_ptr(), stride, C.byref(view), C.byref(d_small), st))
        manifest.append((label, ["k_resample_h", "k_resample_v"]))

    def light_view(label):
        capi.check_image(L.hm_light_to_tensor(RGBA, 8, W, H, src.data_ptr(), stride, C.byref(view), C.byref(lt), C.byref(d_small), st))
        manifest.append((label, ["k_light_h", "k_light_v"]))

    def alpha_view(mode, lit, label):
        al = alpha(mode)
        capi.check_image(L.hm_alpha_to_tensor(RGBA, 8, W, H, src.data_ptr(), stride, C.byref(view), C.byref(lt) if lit else None, None, C.byref(al), C.byref(d_small), st))
        manifest.append((label, ["k_alpha_h", "k_alpha_v"]))

    def everything(warm):
        def name(s):
            return "warm-up" if warm else s
        plain(name(POINT))
        matte(name("pointwise alpha matte"))
        torch.cuda.synchronize()
        plain_view(name(VIEW))
        for mode_name, mode in MODES:
            alpha_view(mode, False, name(f"view alpha {mode_name}"))
        torch.cuda.synchronize()
        light_view(name(LIT))
        for mode_name, mode in MODES:
            alpha_view(mode, True, name(f"view light + alpha {mode_name}"))
        torch.cuda.synchronize()
    for _ in range(WARM):
        everything(True)
    for _ in range(REPEATS):
        everything(False)
    with open(manifest_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "launches": manifest}, f)
    print(f"{len(manifest)} calls queued; manifest in {manifest_path}")


def short_name(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k + "<" in name or k + "(" in name or name.endswith(k):
            return k
    return None


def counterpart(label):
    return POINT if label.startswith("pointwise") else LIT if "light" in label else VIEW


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
            full_names.setdefault(m.group(0) if m else k, None)
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} RGBA32 image in device memory (random colour, a disc's alpha), destination CHW float32; the view: {OW} x {OH}, HM_VIEW_TRIANGLE",
             "ratio: the case's median over the median of its counterpart, the same write without the alpha step"]

    def med(v):
        return sorted(v)[len(v) // 2]
    totals = {label: [sum(v) for v in zip(*times[label].values())] for label in times}
    for label in times:
        total = totals[label]
        parts = ", ".join(f"{k} {med(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times[label].items())
        ratio = "" if label == counterpart(label) else f"  x {med(total) / med(totals[counterpart(label)]):.2f}"
        lines.append(f"  {label:38s} {med(total):8.1f} ({min(total):.1f} .. {max(total):.1f}){ratio:9s}" + (f"   [{parts}]" if len(times[label]) > 1 else ""))
    lines.append("instances: " + "; ".join(sorted(full_names)))
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
