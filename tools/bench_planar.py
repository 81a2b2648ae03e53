"""Micro-benchmark of the planar-target colour operations (hm_colour_convert_planar, device-resident in / out) against the
yardstick of their class, the standalone float kernel k_ycbcr_float (hm_colour_convert on a limited-range 4:2:2 image).

  python tools/bench_planar.py                          every size and depth, HIP events over ITERS calls after warm-up
  python tools/bench_planar.py --size 4032x3024 --bits 8   one size / depth: the form to run under
                                                        `rocprofv3 --kernel-trace --stats -- python ...` for per-kernel times
  python tools/bench_planar.py --decode                 wall time of one 12 MP 10-bit 4:2:2 decode, out_format 0 against 4:2:0

Times are per call (all kernels and plane copies of the operation); bytes are the algorithmic ones: every plane the operation
reads plus every plane it writes, once.  One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
L = pkg.lib()
capi = pkg.capi
ITERS = 20
LIMITED = (1, 2, 2, 0)  # nclx present, unspecified matrix, limited range: the float matrix path with the range scaling


def plane(w, h, bps):
    stride = L.hm_plane_stride(w, bps)
    return torch.randint(0, 256 if bps == 1 else 4, (max(64, (h + 1) & ~1), stride), dtype=torch.uint8, device="cuda:0"), stride


def timed(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def report(name, w, h, bits, ms, alg):
    print(json.dumps({"op": name, "w": w, "h": h, "bits": bits, "us": round(ms * 1e3, 1), "alg_MB": round(alg / 1e6, 1),
                      "GBps": round(alg / ms / 1e6, 1), "frac_of_8TBps": round(alg / ms / 1e6 / 8000, 4)}), flush=True)


def yardstick(w, h, bits):
    bps = 2 if bits > 8 else 1
    fmt = 10 if bits == 8 else 14  # RGB24 / RRGGBB_LE: no depth change behind the float op
    cw = (w + 1) // 2
    (y, ys), (cb, cs), (cr, _) = plane(w, h, bps), plane(cw, h, bps), plane(cw, h, bps)
    obpp = L.hm_out_bytes_per_pixel(fmt)
    out, os_ = plane(w, h, obpp)
    d = capi.ColourDesc(w, h, bits, 2, *LIMITED, fmt, ys, cs, cs, os_)
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: capi.check(L.hm_colour_convert(C.byref(d), y.data_ptr(), cb.data_ptr(), cr.data_ptr(), out.data_ptr(), st)))
    report("k_ycbcr_float 4:2:2 -> interleaved (yardstick)", w, h, bits, ms, (w * h + 2 * cw * h) * bps + w * h * obpp)


def planar(name, w, h, bits, chroma, target, flags=0):
    bps = 2 if bits > 8 else 1
    size = lambda c: ((w if c == 3 else (w + 1) // 2), ((h + 1) // 2 if c == 1 else h))  # noqa: E731
    (cw, ch), (tw, th) = size(chroma), size(target)
    src, dst = capi.Planes(), capi.Planes()
    keep = []
    for c, (pw, ph) in enumerate(((w, h), (cw, ch), (cw, ch))):
        t, s = plane(pw, ph, bps)
        keep.append(t)
        src.plane[c], src.stride[c] = t.data_ptr(), s
    for c, (pw, ph) in enumerate(((w, h), (tw, th), (tw, th))):
        t, s = plane(pw, ph, bps)
        keep.append(t)
        dst.plane[c], dst.stride[c] = t.data_ptr(), s
    d = capi.ColourDesc(w, h, bits, chroma, *LIMITED, 0x100 | target, src.stride[0], src.stride[1], src.stride[2], 0, 0, 0)
    st = torch.cuda.current_stream().cuda_stream
    ms = timed(lambda: capi.check(L.hm_colour_convert_planar(C.byref(d), C.byref(src), 0, C.byref(dst), flags, st)))
    report(name, w, h, bits, ms, (2 * w * h + 2 * cw * ch + 2 * tw * th) * bps)


def decode():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import heifwriter
    import pipeline
    import synthutil
    w, h = 4032, 3024
    pic = synthutil.picture(4221200, width=w, height=h, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30)
    f = pipeline.HeifFile(L, heifwriter.write_heic([pic], (w, h), chroma_format=2, bit_depth=10))
    for fmt in (0, 0x101, 0, 0x101):
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            f.decode(f.primary(), fmt, threads=16, copy=False)
            ts.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"op": "hm_decode_item 12 MP 10-bit 4:2:2", "out_format": hex(fmt), "ms_median_of_7": round(sorted(ts)[3], 2), "ms_min": round(min(ts), 2)}), flush=True)
    f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size")
    ap.add_argument("--bits", type=int)
    ap.add_argument("--decode", action="store_true")
    a = ap.parse_args()
    if a.decode:
        decode()
        sys.exit(0)
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else [(4032, 3024), (16384, 16384)]
    for w, h in sizes:
        for bits in ([a.bits] if a.bits else [8, 10]):
            yardstick(w, h, bits)
            planar("average down 4:4:4 -> 4:2:0 (k_average_down + luma copy)", w, h, bits, 3, 1)
            planar("round trip 4:2:2 -> 4:2:0 fused (k_to_ycbcr from YCbCr)", w, h, bits, 2, 1)
            planar("round trip 4:2:2 -> 4:2:0 op by op (k_to_rgb_planes + k_to_ycbcr)", w, h, bits, 2, 1, capi.HM_PLANAR_UNFUSED)
