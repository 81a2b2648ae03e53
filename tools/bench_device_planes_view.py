#!/usr/bin/env python3
"""Planar views (a view into hm_device_planes), measured (GPU box, repo root):  python3 tools/bench_device_planes_view.py [--out FILE]

1. The step alone (hm_resample_planes_to_tensor) on the planes of one 4032 x 3024 4:2:0 picture: 8 bit -> 1920 x 1080 NV12 uint8 and
   -> 224 x 224 I420 float32, triangle and bicubic; 10 bit -> 1920 x 1080 P010 (uint16, msb_aligned), triangle - device events around
   blocks of launches, each beside a device-to-device copy by the runtime of the source rectangles' byte count and beside the RGB
   view step (hm_resample_to_tensor on 4032 x 3024 RGB24 -> the same size, CHW of the same dtype) in the same run, alternating blocks.
2. One 12 MP grid (the 48 tiles of bench.py) as coded, end to end through hm_decode_item_to_device_planes_view to 224 x 224 NV12, 16
   entropy-decode threads, for crops on 1, 4 and 12 tiles and for the whole image, beside hm_decode_item_to_device_planes of the
   whole image (what the parent commit offers): host clock around calls that return with the planes in place, alternating rounds.
Prints and writes profiles/device_planes_view.txt (--out); nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB, RRGGBB_LE, CHW = 10, 14, 1
SEPARATE, SEMI = 0, 1
U8, U16, F16, F32 = 0, 1, 2, 3
TRIANGLE, CUBIC = 0, 16
# crop -> tiles of 512 x 512 it touches
CROPS = {1: (520, 520, 448, 448), 4: (300, 300, 448, 448), 12: (300, 300, 1500, 1000), 48: (0, 0, 0, 0)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_planes_view.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=42)
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

    tdt = {U8: torch.uint8, U16: torch.uint16, F16: torch.float16, F32: torch.float32}

    def planes_of(layout, dtype, ow, oh, msb, peak):
        cw, ch = (ow + 1) // 2, (oh + 1) // 2
        shapes = [(oh, ow), (ch, 2 * cw)] if layout == SEMI else [(oh, ow), (ch, cw), (ch, cw)]
        ts = [torch.empty(s, dtype=tdt[dtype], device="cuda") for s in shapes]
        d = capi.DevicePlanes()
        d.layout, d.dtype, d.msb_aligned = layout, dtype, msb
        for k in range(4):
            d.scale[k], d.bias[k] = 1.0 / peak, 0.0
        for t, slot in zip(ts, (0, 1, 2)):
            d.plane[slot].ptr, d.plane[slot].len = t.data_ptr(), t.numel() * t.element_size()
        return d, ts

    say(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds, medians (min .. max of the rounds)")
    st = torch.cuda.current_stream().cuda_stream

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.launches  # ms per launch

    say(f"1. hm_resample_planes_to_tensor on the planes of a {W} x {H} 4:2:0 picture, {args.launches} launches per block")
    hl = capi.lib()
    for bits, layout, dtype, msb, size, filt, name in ((8, SEMI, U8, 0, (1920, 1080), TRIANGLE, "8 bit -> 1920 x 1080 NV12 uint8, triangle"),
                                                       (8, SEMI, U8, 0, (1920, 1080), CUBIC, "8 bit -> 1920 x 1080 NV12 uint8, bicubic"),
                                                       (8, SEPARATE, F32, 0, (224, 224), TRIANGLE, "8 bit -> 224 x 224 I420 float32, triangle"),
                                                       (8, SEPARATE, F32, 0, (224, 224), CUBIC, "8 bit -> 224 x 224 I420 float32, bicubic"),
                                                       (10, SEMI, U16, 1, (1920, 1080), TRIANGLE, "10 bit -> 1920 x 1080 P010 (msb_aligned), triangle")):
        sb = 2 if bits > 8 else 1
        peak = float((1 << bits) - 1)
        cw, ch = (W + 1) // 2, (H + 1) // 2
        srcs, strides, keep = (C.c_void_p * 4)(), (C.c_int32 * 4)(), []
        for c, (pw, ph) in enumerate(((W, H), (cw, ch), (cw, ch))):
            stride = hl.hm_plane_stride(pw, sb)
            if sb == 1:
                t = torch.randint(0, 256, (ph, stride), dtype=torch.uint8, device="cuda")
            else:
                t = torch.randint(0, 1 << bits, (ph, stride // 2), dtype=torch.int16, device="cuda")
            keep.append(t)
            srcs[c], strides[c] = t.data_ptr(), stride
        ow, oh = size
        d, outs = planes_of(layout, dtype, ow, oh, msb, peak)
        v = capi.DeviceView(0, 0, 0, 0, ow, oh, filt)
        rect = (W * H + 2 * cw * ch) * sb  # the source rectangles' bytes
        a = torch.empty(rect, dtype=torch.uint8, device="cuda")
        b = torch.empty(rect, dtype=torch.uint8, device="cuda")
        # the RGB view step of tools/bench_device_view.py on the same picture size, the same output size, filter and dtype
        obpp, fmt = (3, RGB) if bits == 8 else (6, RRGGBB_LE)
        rstride = hl.hm_plane_stride(W, obpp)
        rsrc = torch.randint(0, 256, (H, rstride), dtype=torch.uint8, device="cuda")
        if bits > 8:
            rsrc = torch.randint(0, 1 << bits, (H, rstride // 2), dtype=torch.int16, device="cuda")
        rdst = torch.empty((3, oh, ow), dtype=tdt[dtype], device="cuda")
        rd = capi.DeviceDest()
        rd.ptr, rd.len, rd.layout, rd.dtype = rdst.data_ptr(), rdst.numel() * rdst.element_size(), CHW, dtype
        for k in range(4):
            rd.scale[k], rd.bias[k] = 1.0 / peak, 0.0

        def planar():
            capi.check_image(L.hm_resample_planes_to_tensor(1, bits, W, H, 0, C.byref(srcs), C.byref(strides), C.byref(v), C.byref(d), st))

        def rgb():
            capi.check_image(L.hm_resample_to_tensor(fmt, W, H, rsrc.data_ptr(), rstride, C.byref(v), C.byref(rd), st))

        def copy():
            b.copy_(a)
        for fn in (planar, rgb, copy):
            block(fn)  # warm-up: code object load, pool
        tp, tr, tc = [], [], []
        for _ in range(args.rounds):
            tp.append(block(planar))
            tr.append(block(rgb))
            tc.append(block(copy))
        mp, mr, mc = median(tp), median(tr), median(tc)
        say(f"   {name}: {rect / 1e6:.1f} MB of source planes")
        say(f"     planar view step    {mp * 1e3:8.1f} us ({min(tp) * 1e3:.1f} .. {max(tp) * 1e3:.1f})  {rect / mp / 1e9:7.3f} TB/s of source")
        say(f"     RGB view step       {mr * 1e3:8.1f} us ({min(tr) * 1e3:.1f} .. {max(tr) * 1e3:.1f})  ({W * H * obpp / 1e6:.1f} MB of source pixels)")
        say(f"     runtime D2D copy    {mc * 1e3:8.1f} us ({min(tc) * 1e3:.1f} .. {max(tc) * 1e3:.1f})  {rect / mc / 1e9:7.3f} TB/s  (copy of {rect} bytes)")
        say(f"     planar / RGB = {mp / mr:.2f}   planar / copy = {mp / mc:.2f}")
        del keep, outs, a, b, rsrc, rdst
    # ---- 2. one 12 MP grid as coded, end to end ----
    tiles = [bench.tile_stream(9100 + i) for i in range(48)]
    data = heifwriter.write_heic(tiles, (bench.TILE, bench.TILE), grid=(bench.GRID_ROWS, bench.GRID_COLS, bench.OUT_W, bench.OUT_H))
    w, h = bench.OUT_W, bench.OUT_H
    prm = capi.DecodeParams(0, 16, 0, 0, None, None, 0, 0, 0, 0)
    d_full, keep_full = planes_of(SEMI, U8, w, h, 0, 255.0)
    d_view, keep_view = planes_of(SEMI, U8, 224, 224, 0, 255.0)
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    iid = L.hm_file_primary_item(fh)

    def whole():
        out = capi.Decoded()
        capi.check_image(L.hm_decode_item_to_device_planes(fh, iid, C.byref(prm), C.byref(d_full), C.byref(out)))

    def view_of(tiles_touched):
        v = capi.DeviceView(*CROPS[tiles_touched], 224, 224, TRIANGLE)
        plan = (C.c_int32 * 4)()
        capi.check_image(L.hm_plan_planes_view(fh, iid, C.byref(prm), C.byref(v), C.byref(plan)))
        assert plan[1] * plan[3] == tiles_touched, tuple(plan)

        def run():
            out = capi.Decoded()
            capi.check_image(L.hm_decode_item_to_device_planes_view(fh, iid, C.byref(prm), C.byref(v), C.byref(d_view), C.byref(out)))
        return run
    paths = [(f"planes view -> 224 x 224 NV12, crop on {n:2d} tiles", view_of(n)) for n in sorted(CROPS)]
    paths.append(("to_device_planes, whole image (NV12)", whole))
    for _, fn in paths:
        for _ in range(3):
            fn()
    times = {n: [] for n, _ in paths}
    per_round = max(1, args.calls // args.rounds)
    for _ in range(args.rounds):
        for n, fn in paths:
            for _ in range(per_round):
                t0 = time.perf_counter()
                fn()
                times[n].append((time.perf_counter() - t0) * 1e3)
    say(f"2. one {w} x {h} grid of 48 tiles as coded, end to end, 16 threads, {per_round * args.rounds} calls per path in {args.rounds} alternating rounds (ms per call)")
    for n, _ in paths:
        v = sorted(times[n])
        say(f"     {n:48s} median {median(v):.3f}  best {v[0]:.3f}  mean {sum(v) / len(v):.3f}  worst {v[-1]:.3f}")
    L.hm_file_close(fh)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
