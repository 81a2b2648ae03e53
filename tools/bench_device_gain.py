#!/usr/bin/env python3
"""The gain step (hm_device_gain), timed kernel by kernel against the light write of the same image without the step (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_gain.py --run --manifest DIR/manifest.json
    rocprofv3 --kernel-trace --stats -d PDIR --output-format csv -- python3 tools/bench_device_gain.py --run --manifest PDIR/manifest.json --parent-lib PARENT.so
    python3 tools/bench_device_gain.py --summarise DIR --parent PDIR --out profiles/device_gain.txt

--run queues, on one 4032 x 3024 RGB24 image and a 2016 x 1512 8-bit gain map in device memory (random samples - every table lookup of a
wave meets another entry, the worst case of the tables), five repeats of each behind two warm-up launches, the counterparts and the gain
cases alternating:
  1. pointwise, to CHW float32: hm_light_to_tensor (k_light_tensor) and the light + gain write (k_gain_tensor: ONE kernel - M is formed
     from the map's tap tables inside it, no full-size intermediate);
  2. the 12 MP -> 512 x 384 HM_VIEW_TRIANGLE view: hm_resample_to_tensor (k_resample_h + k_resample_v), hm_light_to_tensor (k_light_h +
     k_light_v) and the light + gain write (k_gain_map_h + k_gain_map_v, k_light_h, k_gain_v).
--parent-lib: the counterpart rows alone, through another build of the library (the parent commit's, which has no gain step): their
kernels are untouched by the step, so the two builds must agree within the spread of the repeats; --summarise --parent prints them
side by side and says so where they do not.  The script times nothing itself: the kernel times are the profiler's.  --summarise
reads the trace, matches the dispatches to the manifest in launch order, and prints each case with its ratio to its counterpart and
the bytes the form moves (computed from the shapes, below); nothing here is a pass / fail check."""
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
MW, MH = 2016, 1512
OW, OH = 512, 384
RGB, CHW, F32 = 10, 1, 3
REPEATS, WARM = 5, 2
KERNELS = ("k_light_tensor", "k_gain_tensor", "k_resample_h", "k_resample_v", "k_light_h", "k_light_v", "k_gain_map_h", "k_gain_map_v", "k_gain_v")
POINT, VIEW, LIT = "pointwise hm_light_to_tensor", "view hm_resample_to_tensor", "view hm_light_to_tensor"
POINT_GAIN, LIT_GAIN = "pointwise light + gain", "view light + gain"
MB = 1e6


def moved_bytes():
    """the bytes each form moves, from the shapes: samples read + elements written (+ the float32 intermediates written and read back);
    tables and tap tables (kilobytes) are left out"""
    px, mp, out, small = W * H * 3, MW * MH, W * H * 3 * 4, OW * OH * 3 * 4
    base_tmp, map_tmp, m_plane = OW * H * 3 * 4, OW * MH * 4, OW * OH * 4
    return {POINT: px + out, POINT_GAIN: px + mp + out,
            VIEW: px + 2 * base_tmp + small, LIT: px + 2 * base_tmp + small,
            LIT_GAIN: px + 2 * base_tmp + small + mp + 2 * map_tmp + 2 * m_plane,
            "unfused": px + mp + out + 2 * W * H * 4}  # (what a full-size float32 M plane would add to the pointwise form: written, then read)


class DeviceDest(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_uint64), ("layout", C.c_int32), ("dtype", C.c_int32), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64),
                ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class DeviceView(C.Structure):
    _fields_ = [(n, C.c_int32) for n in "crop_x crop_y crop_w crop_h out_w out_h filter".split()]


class DeviceLight(C.Structure):
    _fields_ = [("from_transfer", C.c_int32), ("from_primaries", C.c_int32), ("to_transfer", C.c_int32), ("to_primaries", C.c_int32), ("gain", C.c_float),
                ("reserved", C.c_int32 * 3)]


def run(manifest_path, parent_lib):
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    Dest, View, Light = DeviceDest, DeviceView, DeviceLight
    if parent_lib:  # (a build without the gain step: the entry points of the counterparts alone, bound here to the structures above)
        L = C.CDLL(os.path.abspath(parent_lib))
        L.hm_last_error.restype = C.c_char_p
        L.hm_light_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(View), C.POINTER(Light), C.POINTER(Dest), C.c_void_p]
        L.hm_resample_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(View), C.POINTER(Dest), C.c_void_p]
        gain_of = None
    else:
        import __graft_entry__ as g
        capi = g.load_package().capi
        L = capi.image_lib()
        Dest, View, Light = capi.DeviceDest, capi.DeviceView, capi.DeviceLight

        def gain_of():
            p = capi.GainParams()
            p.base_headroom, p.alternate_headroom, p.use_base_primaries = 0.0, 2.0, 1
            for c in range(3):
                p.map_min[c], p.map_max[c], p.gamma[c], p.base_offset[c], p.alternate_offset[c] = -0.5, 2.0, 2.2, 1.0 / 64, 1.0 / 64
            return capi.DeviceGain(0, 1.5, p, (C.c_int32 * 4)(0, 0, 0, 0))

    def check(rc):
        if rc < 0:
            sys.exit(f"status {rc}: {L.hm_last_error().decode()}")
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen).contiguous()
    gmap = torch.randint(0, 256, (MH, MW), dtype=torch.uint8, device="cuda", generator=gen).contiguous()
    manifest = []

    def dest_of(t):
        d = Dest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        return d
    full = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    small = torch.empty((3, OH, OW), dtype=torch.float32, device="cuda")
    d_full, d_small = dest_of(full), dest_of(small)
    lt = Light(13, 1, 8, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    view = View(0, 0, 0, 0, OW, OH, 0)

    def light(v, d, label, kernels):
        check(L.hm_light_to_tensor(RGB, 8, W, H, src.data_ptr(), W * 3, C.byref(view) if v else None, C.byref(lt), C.byref(d), st))
        manifest.append((label, kernels))

    def resample(label):
        check(L.hm_resample_to_tensor(RGB, W, H, src.data_ptr(), W * 3, C.byref(view), C.byref(d_small), st))
        manifest.append((label, ["k_resample_h", "k_resample_v"]))

    def gain(v, d, label, kernels):
        gn = gain_of()
        check(L.hm_gain_to_tensor(RGB, 8, W, H, src.data_ptr(), W * 3, gmap.data_ptr(), MW, MW, MH, 8, C.byref(view) if v else None, C.byref(lt), None, C.byref(gn),
                                  C.byref(d), st))
        manifest.append((label, kernels))

    def everything(warm):
        def name(s):
            return "warm-up" if warm else s
        light(False, d_full, name(POINT), ["k_light_tensor"])
        if gain_of:
            gain(False, d_full, name(POINT_GAIN), ["k_gain_tensor"])
        torch.cuda.synchronize()
        resample(name(VIEW))
        light(True, d_small, name(LIT), ["k_light_h", "k_light_v"])
        if gain_of:
            gain(True, d_small, name(LIT_GAIN), ["k_gain_map_h", "k_gain_map_v", "k_light_h", "k_gain_v"])
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


def read_trace(folder):
    """label -> kernel -> [us per repeat], the device's name, the instances' names"""
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
    times, full_names = {}, {}
    for (label, k), (t0, t1, _, full) in zip(want, rows):
        if label != "warm-up":
            times.setdefault(label, {}).setdefault(k, []).append((t1 - t0) / 1e3)
            m = re.search(r"k_\w+<[^>]*>", full)
            full_names.setdefault(m.group(0) if m else k, None)
    return times, device, full_names


def med(v):
    return sorted(v)[len(v) // 2]


def summarise(folder, parent, out):
    times, device, full_names = read_trace(folder)
    nbytes = moved_bytes()
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} RGB24 image and a {MW} x {MH} 8-bit gain map in device memory (random samples), destination CHW float32; the view: {OW} x {OH}, HM_VIEW_TRIANGLE",
             "ratio: the case's median over the median of its counterpart, the same light write without the gain step; MB: samples read + elements written + float32",
             "intermediates written and read back, from the shapes (tables and tap tables left out)"]
    totals = {label: [sum(v) for v in zip(*times[label].values())] for label in times}
    counterpart = {POINT_GAIN: POINT, LIT_GAIN: LIT}
    for label in times:
        total = totals[label]
        parts = ", ".join(f"{k} {med(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times[label].items())
        ratio = f"  x {med(total) / med(totals[counterpart[label]]):.2f}" if label in counterpart else ""
        lines.append(f"  {label:30s} {med(total):8.1f} ({min(total):.1f} .. {max(total):.1f}){ratio:9s} {nbytes[label] / MB:7.1f} MB   {nbytes[label] / med(total) / 1e6:5.2f} TB/s"
                     + (f"   [{parts}]" if len(times[label]) > 1 else ""))
    lines.append(f"the pointwise path is fused: k_gain_tensor forms M from the map's tap tables (at most two taps per axis), ONE dispatch per call and no intermediate; a full-size")
    lines.append(f"float32 M plane written and read back would move {nbytes['unfused'] / MB:.1f} MB instead of {nbytes[POINT_GAIN] / MB:.1f} MB (x {nbytes['unfused'] / nbytes[POINT_GAIN]:.2f})")
    if parent:
        ptimes, _, _ = read_trace(parent)
        lines.append("the counterpart rows through the parent commit's build of the library (its kernels are untouched by the step), beside this commit's:")
        for label in (POINT, VIEW, LIT):
            a, b = [sum(v) for v in zip(*ptimes[label].values())], totals[label]
            overlap = min(a) <= max(b) and min(b) <= max(a)
            lines.append(f"  {label:30s} parent {med(a):8.1f} ({min(a):.1f} .. {max(a):.1f})   this commit {med(b):8.1f} ({min(b):.1f} .. {max(b):.1f})   "
                         + ("the ranges overlap" if overlap else "THE RANGES DO NOT OVERLAP"))
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        run(args.manifest, args.parent_lib)
    if args.summarise:
        summarise(args.summarise, args.parent, args.out)


if __name__ == "__main__":
    main()
