#!/usr/bin/env python3
"""The region rasteriser (hm_rasterise_regions, csrc/regions.hip), timed on the GPU box from the repo root:

    python3 tools/bench_regions.py --out profiles/regions_raster.txt

A 4032 x 3024 canvas with 16 polygons of 64 points each - one per cell of a 4 x 4 grid, a wobbling star that fills most of its cell -
in HM_REGIONS_STACK mode to HM_DEV_U8: 16 planes, 195 MB written.  The call (staging, one upload, ONE launch) is timed with device
events, REPEATS times behind WARM warm-up calls, alternating with a hipMemsetAsync of the same number of bytes timed the same way: the
write-only floor the kernel is judged against.  ms: median (min .. max); ratio = rasteriser time / memset time.  Nothing here is a
pass / fail check."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, POINTS = 4032, 3024, 16, 64
REPEATS, WARM = 20, 3


def polygons():
    out = []
    cw, ch = W // 4, H // 4
    for k in range(N):
        cx, cy = (k % 4) * cw + cw // 2, (k // 4) * ch + ch // 2
        out.append([(cx + int((0.30 + 0.18 * math.sin(5 * t + k)) * cw * math.cos(t)), cy + int((0.30 + 0.18 * math.sin(5 * t + k)) * ch * math.sin(t)))
                    for t in (2 * math.pi * i / POINTS for i in range(POINTS))])
    return out


def hip_runtime():
    """the HIP runtime this process has loaded already (torch's): the same library object, by its path"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    capi = pkg.capi
    L = capi.image_lib()
    polys = [np.ascontiguousarray(np.array(p, dtype=np.int32)) for p in polygons()]
    regions, data = (capi.Region * N)(), (C.c_void_p * N)()
    for i, p in enumerate(polys):
        regions[i].type, regions[i].n_points, data[i] = capi.HM_REGION_POLYGON, POINTS, p.ctypes.data
    dest = capi.RegionsDest(0, 0, capi.HM_DEV_U8, 0, 0, 0, 1.0, 0.0)
    total = L.hm_regions_dest_bytes(capi.HM_REGIONS_STACK, N, W, H, C.byref(dest))
    print(f"{N} planes of {W} x {H}: {total} bytes")
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing to measure")
    out = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    dest.ptr, dest.len = out.data_ptr(), total
    st = torch.cuda.current_stream().cuda_stream
    hip = hip_runtime()
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    floor = torch.empty((total,), dtype=torch.uint8, device="cuda")

    def raster():
        capi.check_image(L.hm_rasterise_regions(regions, data, N, W, H, None, capi.HM_REGIONS_STACK, C.byref(dest), st))

    def memset():
        assert hip.hipMemsetAsync(floor.data_ptr(), 0, total, st) == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(WARM):
        raster()
        memset()
    torch.cuda.synchronize()
    covered = float((out != 0).float().mean())
    tr, tm = [], []
    for _ in range(REPEATS):
        tr.append(timed(raster))
        tm.append(timed(memset))
    mr, mm = statistics.median(tr), statistics.median(tm)
    lines = [f"device: {torch.cuda.get_device_name(0)}; canvas {W} x {H}, {N} polygons of {POINTS} points, HM_REGIONS_STACK to HM_DEV_U8: {total} bytes written, "
             f"{100 * covered:.1f} % of the pixels set; device events around one call, {REPEATS} repeats behind {WARM} warm-up calls, rasteriser and memset alternating; "
             "ms: median (min .. max); GB/s = bytes written / median",
             f"hm_rasterise_regions {mr:7.3f} ({min(tr):.3f} .. {max(tr):.3f}) ms {total / mr / 1e6:7.0f} GB/s | hipMemsetAsync {mm:7.3f} ({min(tm):.3f} .. {max(tm):.3f}) ms "
             f"{total / mm / 1e6:7.0f} GB/s | ratio {mr / mm:.2f} (measured once, one box)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
