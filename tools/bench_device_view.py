#!/usr/bin/env python3
"""Views (hm_device_view), measured (GPU box, repo root):  python3 tools/bench_device_view.py [--out FILE] [--parent-lib FILE]

1. The resampling kernels alone (hm_resample_to_tensor) on one 4032 x 3024 RGB24 image: to 224 x 224 and to 1024 x 768 CHW float32,
   and the crop alone, 1024 x 1024, to CHW float32 - device events around blocks of launches, each beside a device-to-device copy
   by the runtime of the source rectangle's byte count, in the same run in alternating blocks.
2. One 12 MP grid (the 48 tiles of bench.py) end to end through hm_decode_item_to_device_view to 224 x 224 CHW float32, 16
   entropy-decode threads, for crops that cover 1, 4 and 12 tiles and for the whole image, beside hm_decode_item_to_device of the
   whole image to CHW float32 (this build's, and - with --parent-lib - that of a library built from the parent commit, loaded
   beside it): host clock around calls that return with the pixels in place, alternating rounds, medians.
Prints (and writes to --out); nothing here is a pass / fail check.  --view-only CROP runs one view decode path alone (for
`rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3 tools/bench_device_view.py --view-only 1 --calls 7`)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB, CHW, F32 = 10, 1, 3
# crop -> tiles of 512 x 512 it touches
CROPS = {1: (520, 520, 448, 448), 4: (300, 300, 448, 448), 12: (300, 300, 1500, 1000), 48: (0, 0, 0, 0)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--calls", type=int, default=42)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--view-only", type=int, default=0, choices=[0] + sorted(CROPS))
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

    def dest_of(t):
        d = capi.DeviceDest()
        d.ptr, d.len, d.layout, d.dtype = t.data_ptr(), t.numel() * t.element_size(), CHW, F32
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0 / 255, 0.0
        return d

    say(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds, medians (min .. max of the rounds)")
    st = torch.cuda.current_stream().cuda_stream
    if not args.view_only:
        stride = capi.lib().hm_plane_stride(W, 3)
        src = torch.randint(0, 256, (H, stride), dtype=torch.uint8, device="cuda")
        say(f"1. hm_resample_to_tensor, {W} x {H} RGB24 (source rows {stride} bytes apart) -> CHW float32, {args.launches} launches per block")
        for name, crop, size in (("whole image -> 224 x 224", (0, 0, 0, 0), (224, 224)), ("whole image -> 1024 x 768", (0, 0, 0, 0), (1024, 768)),
                                 ("crop 1024 x 1024 alone", (1500, 1000, 1024, 1024), (0, 0))):
            ow, oh = size if size[0] else crop[2:]
            cw, ch = crop[2:] if crop[2] else (W, H)
            dst = torch.empty((3, oh, ow), dtype=torch.float32, device="cuda")
            d = dest_of(dst)
            v = capi.DeviceView(*crop, *size, 0)
            rect = cw * ch * 3  # the source rectangle's bytes
            a = torch.empty(rect, dtype=torch.uint8, device="cuda")
            b = torch.empty(rect, dtype=torch.uint8, device="cuda")

            def kernel():
                capi.check_image(L.hm_resample_to_tensor(RGB, W, H, src.data_ptr(), stride, C.byref(v), C.byref(d), st))

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
            written = ow * oh * 12
            say(f"   {name}: {rect / 1e6:.1f} MB of source rectangle, {written / 1e6:.2f} MB written")
            say(f"     resampling step     {mk * 1e3:8.1f} us ({min(tk) * 1e3:.1f} .. {max(tk) * 1e3:.1f})  {rect / mk / 1e9:7.3f} TB/s of source")
            say(f"     runtime D2D copy    {mc * 1e3:8.1f} us ({min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f})  {rect / mc / 1e9:7.3f} TB/s  (copy of {rect} bytes)")
            say(f"     step time / copy time = {mk / mc:.2f}")
    # ---- 2. one 12 MP grid end to end ----
    tiles = [bench.tile_stream(9100 + i) for i in range(48)]
    data = heifwriter.write_heic(tiles, (bench.TILE, bench.TILE), grid=(bench.GRID_ROWS, bench.GRID_COLS, bench.OUT_W, bench.OUT_H))
    w, h = bench.OUT_W, bench.OUT_H
    prm = capi.DecodeParams(RGB, 16, 0, 0, None, None, 0, 0, 0, 0)
    t_full = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    t_view = torch.empty((3, 224, 224), dtype=torch.float32, device="cuda")
    d_full, d_view = dest_of(t_full), dest_of(t_view)

    def opened(lib):
        fh = C.c_void_p()
        assert lib.hm_file_open(data, len(data), C.byref(fh)) == 0
        return fh, lib.hm_file_primary_item(fh)
    fh, iid = opened(L)

    def whole(lib, handle, item):
        out = capi.Decoded()
        assert lib.hm_decode_item_to_device(handle, item, C.byref(prm), C.byref(d_full), C.byref(out)) == 0

    def view_of(tiles_touched):
        v = capi.DeviceView(*CROPS[tiles_touched], 224, 224, 0)
        plan = (C.c_int32 * 4)()
        capi.check_image(L.hm_plan_view(fh, iid, C.byref(prm), C.byref(v), C.byref(plan)))
        assert plan[1] * plan[3] == tiles_touched, tuple(plan)

        def run():
            out = capi.Decoded()
            capi.check_image(L.hm_decode_item_to_device_view(fh, iid, C.byref(prm), C.byref(v), C.byref(d_view), C.byref(out)))
        return run
    paths = [(f"view -> 224 x 224, crop on {n:2d} tiles", view_of(n)) for n in sorted(CROPS) if args.view_only in (0, n)]
    if not args.view_only:
        paths.append(("to_device, whole image, this build", lambda: whole(L, fh, iid)))
        if args.parent_lib:
            P = C.CDLL(os.path.abspath(args.parent_lib))
            P.hm_file_open.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
            P.hm_file_primary_item.argtypes = [C.c_void_p]
            P.hm_file_primary_item.restype = C.c_uint32
            P.hm_decode_item_to_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(capi.DecodeParams), C.POINTER(capi.DeviceDest), C.POINTER(capi.Decoded)]
            ph, pid = opened(P)
            paths.append(("to_device, whole image, parent build", lambda: whole(P, ph, pid)))
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
        say(f"     {n:40s} median {median(v):.3f}  best {v[0]:.3f}  mean {sum(v) / len(v):.3f}  worst {v[-1]:.3f}")
    L.hm_file_close(fh)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
