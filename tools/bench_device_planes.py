#!/usr/bin/env python3
"""Device-resident planar YCbCr, measured (GPU box, repo root):  python3 tools/bench_device_planes.py [--out FILE] [--parent-lib SO]

1. k_planes_to_tensor alone (hm_planes_to_tensor) on the planes of one 4032 x 3024 4:2:0 image: 8-bit to NV12 uint8, I420 uint8 and
   NV12 float16, 10-bit to P010 (uint16, msb_aligned), timed with device events around blocks of launches, each against a
   device-to-device copy by the runtime that moves the same total number of bytes (read + written), in alternating blocks.
2. One 12 MP grid (the 48 tiles of bench.py) end to end with out_format 0, 16 entropy-decode threads: hm_decode_item to pinned host
   memory against hm_decode_item_to_device_planes (NV12 uint8, I420 uint8), host clock around calls that return with the planes in
   place, alternating.  --parent-lib: a libheif_mi355x.so built from the parent commit; its hm_decode_item is timed beside them.
Prints medians with their spread and writes them to --out (default: profiles/device_planes.txt); nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
SEPARATE, SEMI, U8, U16, F16 = 0, 1, 0, 1, 2


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_planes.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--calls", type=int, default=42)
    ap.add_argument("--parent-lib", default=None)
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
    st = torch.cuda.current_stream().cuda_stream
    cw, ch = W // 2, H // 2

    def planes_of(tensors, layout, dtype, msb=0):
        d = capi.DevicePlanes()
        d.layout, d.dtype, d.msb_aligned = layout, dtype, msb
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0 / 255, 0.0
        for t, slot in zip(tensors, (0, 1, 2)):
            d.plane[slot].ptr, d.plane[slot].len = t.data_ptr(), t.numel() * t.element_size()
        return d

    # ---- 1. the kernel alone ----
    say(f"1. k_planes_to_tensor, {W} x {H} 4:2:0, {args.launches} launches per block")
    for name, bits, layout, dtype, tdt, elem, msb in (("8 bit -> NV12 uint8", 8, SEMI, U8, torch.uint8, 1, 0), ("8 bit -> I420 uint8", 8, SEPARATE, U8, torch.uint8, 1, 0),
                                                      ("8 bit -> NV12 float16", 8, SEMI, F16, torch.float16, 2, 0),
                                                      ("10 bit -> P010 (uint16, msb_aligned)", 10, SEMI, U16, torch.uint16, 2, 1)):
        sb = 2 if bits > 8 else 1
        ys, cs = capi.lib().hm_plane_stride(W, sb), capi.lib().hm_plane_stride(cw, sb)
        src = [torch.randint(0, 256, (H, ys), dtype=torch.uint8, device="cuda"), torch.randint(0, 256, (ch, cs), dtype=torch.uint8, device="cuda"),
               torch.randint(0, 256, (ch, cs), dtype=torch.uint8, device="cuda")]
        if bits > 8:  # samples below 1 << bits: the high byte of every word
            for t in src:
                t[:, 1::2] &= (1 << (bits - 8)) - 1
        srcs = (C.c_void_p * 4)(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), None)
        strides = (C.c_int32 * 4)(ys, cs, cs, 0)
        if layout == SEMI:
            dst = [torch.empty((H, W), dtype=tdt, device="cuda"), torch.empty((ch, cw, 2), dtype=tdt, device="cuda")]
        else:
            dst = [torch.empty((H, W), dtype=tdt, device="cuda"), torch.empty((ch, cw), dtype=tdt, device="cuda"), torch.empty((ch, cw), dtype=tdt, device="cuda")]
        d = planes_of(dst, layout, dtype, msb)
        samples = W * H + 2 * cw * ch
        total = samples * sb + samples * elem  # bytes read + written
        a = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(total // 2, dtype=torch.uint8, device="cuda")

        def kernel():
            capi.check_image(L.hm_planes_to_tensor(1, bits, W, H, 0, C.byref(srcs), C.byref(strides), C.byref(d), st))

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
        say(f"     k_planes_to_tensor {mk * 1e3:8.1f} us ({min(tk) * 1e3:.1f} .. {max(tk) * 1e3:.1f})  {total / mk / 1e9:7.2f} TB/s")
        say(f"     runtime D2D copy   {mc * 1e3:8.1f} us ({min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f})  {total / mc / 1e9:7.2f} TB/s  (copy of {total // 2} bytes)")
        say(f"     kernel rate / copy rate = {mc / mk:.2f}")
    # ---- 2. one 12 MP grid end to end, as coded ----
    tiles = [bench.tile_stream(9100 + i) for i in range(48)]
    data = heifwriter.write_heic(tiles, (bench.TILE, bench.TILE), grid=(bench.GRID_ROWS, bench.GRID_COLS, bench.OUT_W, bench.OUT_H))
    w, h = bench.OUT_W, bench.OUT_H
    prm = capi.DecodeParams(0, 16, 0, 0, None, None, 0, 0, 0, 0)

    def opened(lib):
        fh = C.c_void_p()
        capi.check_image(lib.hm_file_open(data, len(data), C.byref(fh)))
        return fh, lib.hm_file_primary_item(fh)
    fh, iid = opened(L)
    gw, gh = (w + 1) // 2, (h + 1) // 2
    nv12 = [torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((gh, gw, 2), dtype=torch.uint8, device="cuda")]
    i420 = [torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((gh, gw), dtype=torch.uint8, device="cuda"), torch.empty((gh, gw), dtype=torch.uint8, device="cuda")]
    d_nv12, d_i420 = planes_of(nv12, SEMI, U8), planes_of(i420, SEPARATE, U8)

    def host(lib=L, handle=fh):
        out = capi.Decoded()
        capi.check_image(lib.hm_decode_item(handle, iid, C.byref(prm), C.byref(out)))
        lib.hm_decoded_free(C.byref(out))

    def device(d):
        out = capi.Decoded()
        capi.check_image(L.hm_decode_item_to_device_planes(fh, iid, C.byref(prm), C.byref(d), C.byref(out)))
    paths = [("hm_decode_item -> pinned host", host), ("to_device_planes NV12 uint8", lambda: device(d_nv12)), ("to_device_planes I420 uint8", lambda: device(d_i420))]
    if args.parent_lib:
        P = C.CDLL(os.path.abspath(args.parent_lib))
        P.hm_file_open.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        P.hm_file_close.argtypes = [C.c_void_p]
        P.hm_file_primary_item.argtypes = [C.c_void_p]
        P.hm_file_primary_item.restype = C.c_uint32
        P.hm_decode_item.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(capi.DecodeParams), C.POINTER(capi.Decoded)]
        P.hm_decoded_free.argtypes = [C.POINTER(capi.Decoded)]
        P.hm_decoded_free.restype = None
        pfh, _ = opened(P)
        paths.insert(0, ("parent build: hm_decode_item", lambda: host(P, pfh)))
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
    say(f"2. one {w} x {h} grid of 48 tiles end to end, out_format 0, 16 threads, {per_round * args.rounds} calls per path in {args.rounds} alternating rounds (ms per call)")
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
