#!/usr/bin/env python3
"""The OOTF step (hm_device_ootf), timed kernel by kernel under tools/bench_device_tone.py's protocol (GPU box, repo root):

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/bench_device_ootf.py --run --manifest DIR/manifest.json
    rocprofv3 --kernel-trace --stats -d DIR0 --output-format csv -- python3 tools/bench_device_ootf.py --run --lib PARENT.so --manifest DIR0/manifest.json
    python3 tools/bench_device_ootf.py --summarise DIR [--baseline DIR0] --out profiles/device_ootf.txt

--run queues, on one 4032 x 3024 image of random HLG BT.2020 samples in device memory - RGB24, and RRGGBB_LE of 10 bits -, to CHW
float32 linear light, pointwise and under a 4 x HM_VIEW_TRIANGLE reduction (1008 x 756): the light step alone, light + tone
(1000 -> 203 cd/m2) and light + OOTF (display peak 1000), five repeats each, alternating, behind two warm-up launches of each.
--lib PATH runs the launches WITHOUT the OOTF step on another build of the library (the parent commit's: the yardstick).
It times nothing itself: the kernel times are the profiler's; nothing here is a pass / fail check."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_device_tone as bt  # noqa: E402  (the trace reader and the table)

W, H = 4032, 3024
OW, OH = W // 4, H // 4
RGB, RRGGBB_LE, CHW, F32 = 10, 14, 1, 3
REPEATS, WARM = bt.REPEATS, bt.WARM


def run(manifest_path, other_lib):
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    if other_lib:  # the launches without the step, on another build: only what both builds have is bound
        L = C.CDLL(other_lib)
        L.hm_light_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.DeviceView), C.POINTER(capi.DeviceLight),
                                         C.POINTER(capi.DeviceDest), C.c_void_p]
        L.hm_tone_to_tensor.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(capi.DeviceView), C.POINTER(capi.DeviceLight),
                                        C.POINTER(capi.DeviceTone), C.POINTER(capi.DeviceDest), C.c_void_p]
        L.hm_last_error.restype = C.c_char_p
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(1)
    stride8, stride16 = capi.lib().hm_plane_stride(W, 3), capi.lib().hm_plane_stride(W, 6)
    src8 = torch.randint(0, 256, (H, stride8), dtype=torch.uint8, device="cuda", generator=gen)
    src16 = torch.randint(0, 1024, (H, stride16 // 2), dtype=torch.int16, device="cuda", generator=gen)
    manifest = []

    def dest_of(t):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0, 0.0
        return d
    full = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    small = torch.empty((3, OH, OW), dtype=torch.float32, device="cuda")
    d_full, d_small = dest_of(full), dest_of(small)
    lt = capi.DeviceLight(18, 9, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    tn = capi.DeviceTone(capi.HM_TONE_BT2390, 0, 1000.0, 203.0, 1000.0, 203.0, (C.c_int32 * 2)(0, 0))
    view = capi.DeviceView(0, 0, 0, 0, OW, OH, 0)

    def check(rc):
        if rc:
            sys.exit(f"status {rc}: {L.hm_last_error().decode()}")

    def call(step, fmt, bits, src, stride, v, d, kernels, label):
        vp = C.byref(v) if v is not None else None
        if step == "light":
            check(L.hm_light_to_tensor(fmt, bits, W, H, src.data_ptr(), stride, vp, C.byref(lt), C.byref(d), st))
        elif step == "tone":
            check(L.hm_tone_to_tensor(fmt, bits, W, H, src.data_ptr(), stride, vp, C.byref(lt), C.byref(tn), C.byref(d), st))
        else:
            oo = capi.DeviceOotf(capi.HM_OOTF_HLG, 1000.0, 0.0, (C.c_int32 * 5)(0, 0, 0, 0, 0))
            check(L.hm_ootf_to_tensor(fmt, bits, W, H, src.data_ptr(), stride, vp, C.byref(lt), C.byref(oo), None, None, C.byref(d), st))
        manifest.append((label, kernels))
    point, two = ["k_light_tensor"], ["k_light_h", "k_light_v"]
    cases = []
    for name, fmt, bits, src, stride in (("RGB24", RGB, 8, src8, stride8), ("10-bit", RRGGBB_LE, 10, src16, stride16)):
        for shape, v, d, kernels in (("pointwise", None, d_full, point), (f"view {OW} x {OH}", view, d_small, two)):
            for step, text in (("light", "light"), ("tone", "light + tone"), ("ootf", "light + OOTF")):
                if other_lib and step == "ootf":
                    continue
                cases.append((lambda lab, a=(step, fmt, bits, src, stride, v, d, kernels): call(*a, lab), f"{name} {shape} CHW f32, {text}"))
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


def summarise(folder, baseline, out):
    device, times, names = bt.read(folder)
    lines = [f"device: {device}; kernel times of rocprofv3 --kernel-trace, {REPEATS} repeats behind {WARM} warm-up launches, in us: median (min .. max)",
             f"source: one {W} x {H} image of random HLG BT.2020 samples in device memory, RGB24 and RRGGBB_LE of 10 bits; tone step 1000 -> 203 cd/m2, OOTF for 1000 cd/m2"]
    lines += bt.table(times, "")
    if baseline:
        _, t0, _ = bt.read(baseline)
        lines.append("the launches without the OOTF step on the parent commit's build (the yardstick; its margin is the spread of its repeats):")
        lines += bt.table(t0, "parent: ")
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
