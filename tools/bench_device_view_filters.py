#!/usr/bin/env python3
"""The filters of a view, measured (GPU box, repo root):  python3 tools/bench_device_view_filters.py [--out FILE]

The view step alone (hm_resample_to_tensor) on one 4032 x 3024 RGB24 image to 224 x 224 and to 1024 x 768 CHW float32: HM_VIEW_TRIANGLE
on its per-lane horizontal kernel (k_resample_h), HM_VIEW_CUBIC and HM_VIEW_LANCZOS3 on the staged one (k_resample_h_staged),
HM_VIEW_CUBIC forced through the per-lane kernel (test hook view_h_staged = 0 of libheif_mi355x_test.so, which is the library
measured throughout: the shipping library's objects), and a device-to-device copy by the runtime of the source rectangle's byte
count - device events around blocks of launches, all paths in the same run in alternating blocks, medians of the rounds.
Prints (and writes to --out); nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB, CHW, F32 = 10, 1, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=40)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    pkg.lib()  # (torch's HIP runtime first)
    L = C.CDLL(capi.TEST_LIB_PATH)
    L.hm_last_error.restype = C.c_char_p
    L.hm_debug_set.argtypes = [C.c_char_p, C.c_int]
    capi.bind_image(L)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds of {args.launches} launches per path, medians (min .. max of the rounds)")
    st = torch.cuda.current_stream().cuda_stream
    stride = pkg.lib().hm_plane_stride(W, 3)
    src = torch.randint(0, 256, (H, stride), dtype=torch.uint8, device="cuda")
    rect = W * H * 3
    a = torch.empty(rect, dtype=torch.uint8, device="cuda")
    b = torch.empty(rect, dtype=torch.uint8, device="cuda")
    say(f"hm_resample_to_tensor, {W} x {H} RGB24 (source rows {stride} bytes apart, {rect / 1e6:.1f} MB) -> CHW float32")
    for ow, oh in ((224, 224), (1024, 768)):
        dst = torch.empty((3, oh, ow), dtype=torch.float32, device="cuda")
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = dst.data_ptr(), dst.numel() * 4, CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0 / 255, 0.0

        def view_step(filt, staged):
            v = capi.DeviceView(0, 0, 0, 0, ow, oh, filt)

            def run():
                rc = L.hm_resample_to_tensor(RGB, W, H, src.data_ptr(), stride, C.byref(v), C.byref(d), st)
                assert rc == 0, L.hm_last_error().decode()

            def block():
                assert L.hm_debug_set(b"view_h_staged", staged) == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    run()
                e1.record()
                e1.synchronize()
                L.hm_debug_set(b"view_h_staged", 1)
                return e0.elapsed_time(e1) / args.launches  # ms per launch
            return block

        def copy_block():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                b.copy_(a)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.launches
        paths = [("triangle, per-lane k_resample_h", view_step(capi.HM_VIEW_TRIANGLE, 1)),
                 ("cubic, k_resample_h_staged", view_step(capi.HM_VIEW_CUBIC, 1)),
                 ("lanczos3, k_resample_h_staged", view_step(capi.HM_VIEW_LANCZOS3, 1)),
                 ("cubic, per-lane k_resample_h (hook)", view_step(capi.HM_VIEW_CUBIC, 0)),
                 ("runtime D2D copy of the rectangle", copy_block)]
        for _, fn in paths:
            fn()  # warm-up: code object load, pool
        times = {n: [] for n, _ in paths}
        for _ in range(args.rounds):
            for n, fn in paths:
                times[n].append(fn())
        copy = median(times[paths[-1][0]])
        say(f"  whole image -> {ow} x {oh}:")
        for n, _ in paths:
            t = times[n]
            say(f"     {n:38s} {median(t) * 1e3:8.1f} us ({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f})  {median(t) / copy:6.2f} x the copy")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
