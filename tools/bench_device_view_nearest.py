#!/usr/bin/env python3
"""HM_VIEW_NEAREST views, measured (GPU box, repo root):  python3 tools/bench_device_view_nearest.py [--root CHECKOUT] [--out FILE]

hm_resample_to_tensor (k_view_nearest) and hm_light_to_tensor (k_light_nearest, sRGB -> linear light) under a nearest view of one
4032 x 3024 RGB24 / RGBA32 image in device memory, to 1024 x 768 and 4000 x 3000, CHW float32 and HWC float16, timed like
tools/bench_device_view_filters.py: device events around blocks of launches, medians of the rounds.  --root measures the build of
another checkout (the parent commit's: the yardstick).  Nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys

W, H = 4032, 3024
RGB, RGBA, CHW, HWC, U8, F16, F32 = 10, 11, 1, 0, 0, 2, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=40)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    L = capi.image_lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; library under {root}; {args.rounds} rounds of {args.launches} launches, medians (min .. max)")
    st = torch.cuda.current_stream().cuda_stream
    lt = capi.DeviceLight(13, 1, capi.HM_LIGHT_LINEAR, 0, 1.0, (C.c_int32 * 3)(0, 0, 0))
    for fmt, ch, label in ((RGB, 3, "RGB24"), (RGBA, 4, "RGBA32")):
        stride = pkg.lib().hm_plane_stride(W, ch)
        src = torch.randint(0, 256, (H, stride), dtype=torch.uint8, device="cuda")
        for ow, oh in ((1024, 768), (4000, 3000)):
            for layout, dtype, tdt, lname in ((CHW, F32, torch.float32, "CHW f32"), (HWC, F16, torch.float16, "HWC f16")):
                shape = (ch, oh, ow) if layout == CHW else (oh, ow, ch)
                dst = torch.empty(shape, dtype=tdt, device="cuda")
                d = capi.DeviceDest()
                d.ptr, d.len, d.layout, d.dtype = dst.data_ptr(), dst.numel() * dst.element_size(), layout, dtype
                for k in range(4):
                    d.scale[k], d.bias[k] = 1.0 / 255, 0.0
                v = capi.DeviceView(0, 0, 0, 0, ow, oh, capi.HM_VIEW_NEAREST)

                def plain():
                    capi.check_image(L.hm_resample_to_tensor(fmt, W, H, src.data_ptr(), stride, C.byref(v), C.byref(d), st))

                def light():
                    capi.check_image(L.hm_light_to_tensor(fmt, 8, W, H, src.data_ptr(), stride, C.byref(v), C.byref(lt), C.byref(d), st))

                def block(fn):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / args.launches
                paths = [("k_view_nearest", plain), ("k_light_nearest", light)]
                for _, fn in paths:
                    block(fn)
                times = {n: [] for n, _ in paths}
                for _ in range(args.rounds):
                    for n, fn in paths:
                        times[n].append(block(fn))
                for n, _ in paths:
                    t = times[n]
                    say(f"  {label} {W} x {H} -> {ow} x {oh} {lname}: {n:16s} {median(t) * 1e3:8.1f} us ({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
