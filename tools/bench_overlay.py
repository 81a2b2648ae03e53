#!/usr/bin/env python3
"""Overlay composition ('iovl' items, k_overlay), measured (GPU box, repo root):  python3 tools/bench_overlay.py [--out FILE]

On a 4032 x 3024 canvas, three cases: (a) one opaque 12 MP grid child (the 48 tiles of bench.py), (b) the same plus a 512 x 128 alpha
watermark, (c) four 2016 x 1512 alpha layers.
1. k_overlay alone (test hook hm_debug_overlay_launch on planes filled with random bytes, RGB24 out): device events around blocks of
   launches, beside a device-to-device copy by the runtime of the output's byte count in the same run, alternating blocks.
2. End to end: hm_decode_item_to_device of the overlay item (HWC uint8), 16 entropy-decode threads, host clock around calls that return
   with the pixels in place; for (a) beside the same call on the grid item itself.
Prints and writes profiles/overlay.txt (--out); nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB = 10


class Rect(C.Structure):
    _fields_ = [(n, C.c_int32) for n in "x0 y0 x1 y1 sx sy opaque".split()]


class Layer(C.Structure):
    """hm_overlay_layer (csrc/hm_overlay.h)"""
    _fields_ = [("rect", Rect), ("plane", C.c_void_p * 4), ("pitch", C.c_int32 * 4), ("plane_w", C.c_int32 * 4), ("plane_h", C.c_int32 * 4),
                ("width", C.c_int32), ("height", C.c_int32), ("chroma", C.c_int32), ("has_nclx", C.c_int32), ("matrix", C.c_int32),
                ("primaries", C.c_int32), ("full_range", C.c_int32)]


class Job(C.Structure):
    """hm_overlay_job"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("background", C.c_uint8 * 3), ("out_kind", C.c_int32), ("out", C.c_void_p * 3),
                ("out_pitch", C.c_int32)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch
    import bench
    import synthutil
    from overlaywriter import Writer
    import __graft_entry__ as g
    pkg = g.load_package(test_knobs="always")
    capi = pkg.capi
    hooks = pkg.lib()
    L = capi.image_lib()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds, medians (min .. max of the rounds)")
    st = torch.cuda.current_stream().cuda_stream
    hooks.hm_debug_overlay_launch.argtypes = [C.POINTER(Job), C.POINTER(Layer), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
    hooks.hm_debug_overlay_release.argtypes = [C.c_void_p, C.c_void_p]
    hooks.hm_debug_overlay_release.restype = None

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.launches

    def plane(w, h):
        pitch = (w + 63) // 64 * 64
        return torch.randint(0, 256, (max(h, 64), pitch), dtype=torch.uint8, device="cuda"), pitch

    def layer(w, h, dx, dy, chroma, alpha, keep):
        cw, ch = (w if chroma == 3 else (w + 1) // 2), ((h + 1) // 2 if chroma == 1 else h)
        ly = Layer()
        x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + w, W), min(dy + h, H)
        ly.rect = Rect(x0, y0, x1, y1, x0 - dx, y0 - dy, 0 if alpha else 1)
        for c, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch), (w, h))):
            if c == 3 and not alpha:
                continue
            t, pitch = plane(pw, ph)
            keep.append(t)
            ly.plane[c], ly.pitch[c], ly.plane_w[c], ly.plane_h[c] = t.data_ptr(), pitch, pw, ph
        ly.width, ly.height, ly.chroma, ly.has_nclx, ly.matrix, ly.primaries, ly.full_range = w, h, chroma, 0, 2, 2, 1
        return ly

    cases = {
        "one opaque 12 MP 4:2:0 layer": lambda keep: [layer(W, H, 0, 0, 1, False, keep)],
        "... plus a 512 x 128 alpha watermark": lambda keep: [layer(W, H, 0, 0, 1, False, keep), layer(512, 128, W - 560, H - 170, 3, True, keep)],
        "four 2016 x 1512 alpha layers": lambda keep: [layer(2016, 1512, x, y, 1, True, keep) for x, y in ((0, 0), (2016, 0), (0, 1512), (1000, 700))],
    }
    out_pitch = (W * 3 + 63) // 64 * 64
    out = torch.empty((H, out_pitch), dtype=torch.uint8, device="cuda")
    src = torch.randint(0, 256, (H, out_pitch), dtype=torch.uint8, device="cuda")
    out_bytes = W * H * 3
    say(f"1. k_overlay alone, {W} x {H} canvas -> RGB24 ({out_bytes / 1e6:.1f} MB written); copy = hipMemcpy2DAsync device to device of the same bytes")
    for name, make in cases.items():
        keep = []
        lys = make(keep)
        arr = (Layer * len(lys))(*lys)
        job = Job(W, H, (C.c_uint8 * 3)(16, 128, 235), 0, (C.c_void_p * 3)(out.data_ptr(), None, None), out_pitch)
        held = []

        def launch():
            p, d = C.c_void_p(), C.c_void_p()
            rc = hooks.hm_debug_overlay_launch(C.byref(job), arr, len(lys), C.byref(p), C.byref(d), st)
            assert rc == 0, rc
            held.append((p, d))

        def copy():
            out.copy_(src)

        launch(); copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(args.rounds):
            tk.append(block(launch))
            tc.append(block(copy))
        torch.cuda.synchronize()
        for p, d in held:
            hooks.hm_debug_overlay_release(p, d)
        k, c = median(tk), median(tc)
        say(f"   {name:42s} k_overlay {k:7.3f} ms ({min(tk):.3f} .. {max(tk):.3f})   copy {c:7.3f} ms ({min(tc):.3f} .. {max(tc):.3f})   "
            f"copy / k_overlay = {c / k:.2f}   {out_bytes / k / 1e6:.0f} GB/s of output bytes")

    say(f"2. end to end: hm_decode_item_to_device (HWC uint8), 16 threads, {args.calls} calls per round")
    w = Writer()
    tiles = [w.hvc1(bench.tile_stream(9100 + i), (bench.TILE, bench.TILE)) for i in range(48)]
    grid = w.grid(tiles, bench.GRID_ROWS, bench.GRID_COLS, bench.OUT_W, bench.OUT_H)
    mark = w.hvc1(synthutil.picture(9301, width=512, height=128, chroma_format=3), (512, 128), chroma_format=3)
    w.alpha(synthutil.picture(9302, width=512, height=128, chroma_format=0, level_span=1000, density=100, qp=40), (512, 128), mark)
    quarters = []
    for i in range(4):
        q = w.hvc1(synthutil.picture(9310 + i, width=2016, height=1512), (2016, 1512))
        w.alpha(synthutil.picture(9320 + i, width=2016, height=1512, chroma_format=0, level_span=1000, density=100, qp=40), (2016, 1512), q)
        quarters.append(q)
    items = {
        "the grid item itself (no overlay)": grid,
        "one opaque 12 MP grid child": w.iovl([(grid, 0, 0)], (W, H)),
        "... plus a 512 x 128 alpha watermark": w.iovl([(grid, 0, 0), (mark, W - 560, H - 170)], (W, H)),
        "four 2016 x 1512 alpha layers": w.iovl([(q, x, y) for q, (x, y) in zip(quarters, ((0, 0), (2016, 0), (0, 1512), (1000, 700)))], (W, H)),
    }
    data = w.finish(primary=grid)
    f = C.c_void_p()
    capi.check_image(L.hm_file_open(data, len(data), C.byref(f)))
    dst = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    dest = capi.DeviceDest(dst.data_ptr(), dst.numel(), capi.HM_DEV_LAYOUT_HWC, capi.HM_DEV_U8, 0, 0, one, zero)
    prm = capi.DecodeParams(RGB, 16, 0, 0, None, None, 0, 0, 0, 0)
    d = capi.Decoded()
    times = {k: [] for k in items}
    for r in range(args.rounds + 1):
        for name, iid in items.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                capi.check_image(L.hm_decode_item_to_device(f, iid, C.byref(prm), C.byref(dest), C.byref(d)))
            if r:  # (the first round warms pools and streams)
                times[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
    L.hm_file_close(f)
    for name, v in times.items():
        say(f"   {name:42s} {median(v):7.3f} ms per call ({min(v):.3f} .. {max(v):.3f})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
