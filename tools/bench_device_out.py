#!/usr/bin/env python3
"""Device-resident output, measured (GPU box, repo root):  python3 tools/bench_device_out.py [--out FILE]

1. k_to_tensor alone on one 4032 x 3024 RGB24 image -> CHW float32 and CHW float16 (hm_to_tensor), timed with device events
   around blocks of launches, against a device-to-device copy by the runtime (torch's same-dtype contiguous copy_ is one
   hipMemcpyAsync) that moves the same total number of bytes (read + written), timed in the same run in alternating blocks.
2. One 12 MP grid (the 48 tiles of bench.py) end to end, 16 entropy-decode threads: hm_decode_item to pinned host memory against
   hm_decode_item_to_device (HWC uint8, CHW float32), host clock around calls that return with the pixels in place, alternating.
Prints (and writes to --out) medians with their spread; nothing here is a pass / fail check.
--device-only leaves the kernel-alone part and the host-destination path out: what is left under
`rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3 tools/bench_device_out.py --device-only --calls 7` is the
device-destination path alone (k_to_tensor among the kernels, no image-sized device-to-host copy among the copies)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB, HWC, CHW, U8, F16, F32 = 10, 0, 1, 0, 2, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import heifwriter
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds, medians (min .. max of the rounds)")
    # ---- 1. the kernel alone ----
    stride = capi.lib().hm_plane_stride(W, 3)
    src = torch.randint(0, 256, (H, stride), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if not args.device_only:
        say(f"1. k_to_tensor, {W} x {H} RGB24 (source rows {stride} bytes apart), {args.launches} launches per block")
    for name, dtype, tdt, elem in (("CHW float32", F32, torch.float32, 4), ("CHW float16", F16, torch.float16, 2)) if not args.device_only else ():
        dst = torch.empty((3, H, W), dtype=tdt, device="cuda")
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = dst.data_ptr(), dst.numel() * elem, CHW, dtype
        for k in range(3):
            d.scale[k], d.bias[k] = 1.0 / (255 * (0.229, 0.224, 0.225)[k]), -(0.485, 0.456, 0.406)[k] / (0.229, 0.224, 0.225)[k]
        total = W * H * 3 + W * H * 3 * elem  # bytes read + written
        a = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(total // 2, dtype=torch.uint8, device="cuda")

        def kernel():
            capi.check_image(L.hm_to_tensor(RGB, W, H, src.data_ptr(), stride, C.byref(d), st))

        def copy():
            b.copy_(a)

        def block(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.launches  # ms per launch
        for fn in (kernel, copy):
            block(fn)  # warm-up: code object load, pool
        tk, tc = [], []
        for _ in range(args.rounds):
            tk.append(block(kernel))
            tc.append(block(copy))
        mk, mc = median(tk), median(tc)
        say(f"   {name}: {total / 1e6:.1f} MB read + written")
        say(f"     k_to_tensor        {mk * 1e3:8.1f} us ({min(tk) * 1e3:.1f} .. {max(tk) * 1e3:.1f})  {total / mk / 1e9:7.2f} TB/s")
        say(f"     runtime D2D copy   {mc * 1e3:8.1f} us ({min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f})  {total / mc / 1e9:7.2f} TB/s  (copy of {total // 2} bytes)")
        say(f"     kernel rate / copy rate = {mc / mk:.2f}")
    # ---- 2. one 12 MP grid end to end ----
    tiles = [bench.tile_stream(9100 + i) for i in range(48)]
    data = heifwriter.write_heic(tiles, (bench.TILE, bench.TILE), grid=(bench.GRID_ROWS, bench.GRID_COLS, bench.OUT_W, bench.OUT_H))
    fh = C.c_void_p()
    capi.check_image(L.hm_file_open(data, len(data), C.byref(fh)))
    iid = L.hm_file_primary_item(fh)
    w, h = bench.OUT_W, bench.OUT_H
    prm = capi.DecodeParams(RGB, 16, 0, 0, None, None, 0, 0, 0, 0)
    t_u8 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    t_f32 = torch.empty((3, h, w), dtype=torch.float32, device="cuda")

    def dest_of(t, layout, dtype):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), layout, dtype
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0 / 255, 0.0
        return d
    d_u8, d_f32 = dest_of(t_u8, HWC, U8), dest_of(t_f32, CHW, F32)

    def host():
        out = capi.Decoded()
        capi.check_image(L.hm_decode_item(fh, iid, C.byref(prm), C.byref(out)))
        L.hm_decoded_free(C.byref(out))

    def device(d):
        out = capi.Decoded()
        capi.check_image(L.hm_decode_item_to_device(fh, iid, C.byref(prm), C.byref(d), C.byref(out)))
    paths = (("hm_decode_item -> pinned host", host), ("to_device HWC uint8", lambda: device(d_u8)), ("to_device CHW float32", lambda: device(d_f32)))
    if args.device_only:
        paths = paths[1:]
    for _, fn in paths:
        for _ in range(5):
            fn()
    times = {n: [] for n, _ in paths}
    per_round = max(1, args.calls // args.rounds)
    for _ in range(args.rounds):
        for n, fn in paths:
            for _ in range(per_round):
                t0 = time.perf_counter()
                fn()
                times[n].append((time.perf_counter() - t0) * 1e3)
    say(f"2. one {w} x {h} grid of 48 tiles end to end, 16 threads, {per_round * args.rounds} calls per path in {args.rounds} alternating rounds (ms per call)")
    for n, _ in paths:
        v = sorted(times[n])
        say(f"     {n:32s} median {median(v):.3f}  best {v[0]:.3f}  mean {sum(v) / len(v):.3f}  worst {v[-1]:.3f}")
    L.hm_file_close(fh)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
