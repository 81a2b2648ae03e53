#!/usr/bin/env python3
"""The tone step (hm_device_tone), timed kernel by kernel (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_tone.py --run --manifest DIR/manifest.json
    python3 tools/bench_device_tone.py --summarise DIR [--baseline DIR0] --out profiles/device_tone.txt

--run queues, on one 4032 x 3024 RRGGBB_LE image of 10-bit PQ BT.2020 samples in device memory, each launch with and without a tone
step (1000 -> 203 cd/m2), five repeats each, alternating, behind two warm-up launches of each:
  1. pointwise to CHW float32, linear light (k_light_tensor<2, 3, float>);
  2. pointwise to HWC integers, 2020 -> 709 and sRGB: uint8 through the 8-bit finish with the tone step (k_light_tensor<2, 3, uint8_t>) -
     the launch without one is the light step's own integer form of this target, HWC uint16 (k_light_tensor<2, 3, uint16_t>);
  3. the 12 MP -> 224 x 224 HM_VIEW_TRIANGLE view to CHW float32 (k_light_h + k_light_v).
The source is random samples: every lookup of a wave meets another table entry, the worst case for LDS bank conflicts.
--lib PATH runs the launches WITHOUT a tone step on another build of the library (the parent commit's: the yardstick).
It times nothing itself: the kernel times are the profiler's.  --summarise reads the trace, matches the dispatches to the manifest in
launch order and prints the table (with --baseline: the other build's beside it); nothing here is a pass / fail check."""
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
RGB, RRGGBB_LE, HWC, CHW, U8, U16, F32 = 10, 14, 0, 1, 0, 1, 3
REPEATS, WARM = 5, 2
KERNELS = ("k_light_tensor", "k_light_h", "k_light_v")


def run(manifest_path, other_lib):
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    if other_lib:  # the launches without a tone step, on another build: only what both builds have is bound
        L = C.CDLL(other_lib)
        L.hm_light_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.DeviceView), C.POINTER(capi.DeviceLight),
                                         C.POINTER(capi.DeviceDest), C.c_void_p]
        L.hm_last_error.restype = C.c_char_p
    st = torch.cuda.current_stream().cuda_stream
    stride = capi.lib().hm_plane_stride(W, 6)
    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.randint(0, 1 << BITS, (H, stride // 2), dtype=torch.int16, device="cuda", generator=gen)
    manifest = []

    def dest_of(t, layout, dtype):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), layout, dtype
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        return d
    full = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    bytes8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    words = torch.empty((H, W, 3), dtype=torch.int16, device="cuda")
    small = torch.empty((3, 224, 224), dtype=torch.float32, device="cuda")
    d_full, d_u8, d_u16, d_small = dest_of(full, CHW, F32), dest_of(bytes8, HWC, U8), dest_of(words, HWC, U16), dest_of(small, CHW, F32)
    zero3 = (C.c_int32 * 3)(0, 0, 0)
    linear = capi.DeviceLight(16, 9, capi.HM_LIGHT_LINEAR, 0, 1.0, zero3)
    srgb = capi.DeviceLight(16, 9, 13, 1, 1.0, zero3)
    view = capi.DeviceView(0, 0, 0, 0, 224, 224, 0)

    def check(rc):
        if rc:
            sys.exit(f"status {rc}: {L.hm_last_error().decode()}")

    def light(lt, v, d, kernels, label):
        check(L.hm_light_to_tensor(RRGGBB_LE, BITS, W, H, noise.data_ptr(), stride, C.byref(v) if v is not None else None, C.byref(lt), C.byref(d), st))
        manifest.append((label, kernels))

    def tone(lt, v, d, out_bits, kernels, label):
        tn = capi.DeviceTone(capi.HM_TONE_BT2390, out_bits, 1000.0, 203.0, 10000.0, 203.0, (C.c_int32 * 2)(0, 0))
        check(L.hm_tone_to_tensor(RRGGBB_LE, BITS, W, H, noise.data_ptr(), stride, C.byref(v) if v is not None else None, C.byref(lt), C.byref(tn), C.byref(d), st))
        manifest.append((label, kernels))
    point, two = ["k_light_tensor"], ["k_light_h", "k_light_v"]
    cases = [(lambda lab: light(linear, None, d_full, point, lab), "pointwise CHW f32, light"),
             (lambda lab: tone(linear, None, d_full, 0, point, lab), "pointwise CHW f32, light + tone"),
             (lambda lab: light(srgb, None, d_u16, point, lab), "pointwise HWC u16 sRGB 709, light"),
             (lambda lab: tone(srgb, None, d_u8, 8, point, lab), "pointwise HWC u8 sRGB 709, light + tone, out_bits 8"),
             (lambda lab: light(linear, view, d_small, two, lab), "view 224 x 224 CHW f32, light"),
             (lambda lab: tone(linear, view, d_small, 0, two, lab), "view 224 x 224 CHW f32, light + tone")]
    if other_lib:
        cases = [c for c in cases if "tone" not in c[1]]
    for _ in range(WARM):
        for fn, _label in cases:
            fn("warm-up")
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for fn, label in cases:
            fn(label)
        torch.cuda.synchronize()
    with open(manifest_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "launches": manifest}, f)
    print(f"{len(manifest)} calls queued; manifest in {manifest_path}")


def short_name(name):
    for k in sorted(KERNELS, key=len, reverse=True):
        if k + "<" in name or k + "(" in name or name.endswith(k):
            return k
    return None


def read(folder):
    """(device, label -> kernel -> [us], kernel instance names) of one profiled run"""
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
        sys.exit(f"{folder}: the trace has {len(rows)} dispatches of the kernels, the manifest {len(want)}: they do not match")
    times, names = {}, set()
    for (label, k), (t0, t1, _, full) in zip(want, rows):
        if label != "warm-up":
            times.setdefault(label, {}).setdefault(k, []).append((t1 - t0) / 1e3)
            m = re.search(r"k_\w+<[^>]*>", full)
            names.add(m.group(0) if m else k)
    return device, times, names


def table(times, tag):
    def med(v):
        return sorted(v)[len(v) // 2]
    lines = []
    for label in times:
        total = [sum(v) for v in zip(*times[label].values())]
        parts = ", ".join(f"{k} {med(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times[label].items())
        lines.append(f"  {tag + label:62s} {med(total):8.1f} ({min(total):.1f} .. {max(total):.1f})" + (f"   [{parts}]" if len(times[label]) > 1 else ""))
    return lines


def summarise(folder, baseline, out):
    device, times, names = read(folder)
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} RRGGBB_LE image of random {BITS}-bit samples in device memory (6 bytes per pixel); tone step 1000 -> 203 cd/m2"]
    lines += table(times, "")
    if baseline:
        _, t0, _ = read(baseline)
        lines.append("the launches without a tone step on the parent commit's build (the yardstick; its margin is the spread of its repeats):")
        lines += table(t0, "parent: ")
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
