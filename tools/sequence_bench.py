"""Image sequences: frames per second and kernel milliseconds of hm_decode_sequence (all frames in one device batch) against a
loop of hm_decode_item over the same frames (one picture per batch - how the fork decodes a movie, context.cc:1603-1727).

The frames are the three real 1080p pictures of tests/data (basketball_1080p_qp{1,25,32}) repeated, written as a fork-style movie
(tests/moovwriter.py), decoded to RGBA with 16 host threads.

  python tools/sequence_bench.py                  wall clock of both modes at 32 and 128 frames (one JSON line per measurement)
  python tools/sequence_bench.py --kernel-trace   the same, each measurement also run under rocprofv3 --kernel-trace --stats in a
                                                  child process: the sum of the kernel times per call
  --out FILE                                      also write the lines to FILE (e.g. profiles/sequence_bench.txt)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def movie(n):
    import moovwriter
    pics = [open(os.path.join(ROOT, "tests", "data", f"basketball_1080p_qp{q}.hevc"), "rb").read() for q in (1, 25, 32)]
    return moovwriter.write_movie([pics[k % 3] for k in range(n)], (1920, 1080))


def run(mode, n, iters, warmup, threads, fmt):
    import __graft_entry__ as g
    import pipeline
    hm = g.load_package().lib()
    pipeline.bind(hm)

    class FrameDest(C.Structure):
        _fields_ = [("ext_dst", C.c_void_p), ("ext_dst_len", C.c_uint32), ("ext_dst_stride", C.c_uint32)]
    hm.hm_decode_sequence.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(pipeline.DecodeParams), C.POINTER(FrameDest),
                                      C.POINTER(pipeline.Decoded), C.POINTER(C.c_int32)]
    f = pipeline.HeifFile(hm, movie(n))
    prm = pipeline.DecodeParams(fmt, threads, 0, 0, None, None, 0, 0, 0, 0)
    out = (pipeline.Decoded * n)()
    failed = C.c_int32()

    def once():
        if mode == "sequence":
            rc = hm.hm_decode_sequence(f.h, 1, n, C.byref(prm), None, out, C.byref(failed))
            if rc:
                raise RuntimeError(hm.hm_last_error().decode())
            for k in range(n):
                hm.hm_decoded_free(C.byref(out[k]))
        else:
            for k in range(n):
                rc = hm.hm_decode_item(f.h, k + 1, C.byref(prm), C.byref(out[k]))
                if rc:
                    raise RuntimeError(hm.hm_last_error().decode())
                hm.hm_decoded_free(C.byref(out[k]))
    for _ in range(warmup):
        once()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        once()
        times.append((time.perf_counter() - t0) * 1e3)
    f.close()
    times.sort()
    med = times[len(times) // 2]
    return dict(mode=mode, frames=n, iters=iters, host_threads=threads, out_format=fmt, median_ms=round(med, 3),
                min_ms=round(times[0], 3), fps=round(n / med * 1e3, 1))


def kernel_ms(mode, n, iters, warmup, threads, fmt):
    """kernel time per call: the child's rocprofv3 kernel stats summed, divided by its calls"""
    d = tempfile.mkdtemp(prefix="seqbench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--child", mode, "--frames", str(n), "--iters", str(iters), "--warmup", str(warmup), "--threads", str(threads), "--format", str(fmt)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        total_ns, launches = 0, 0
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                total_ns += float(row["TotalDurationNs"])
                launches += int(row["Calls"])
        calls = iters + warmup
        return dict(kernel_ms=round(total_ns / 1e6 / calls, 3), launches_per_call=round(launches / calls, 1))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--format", type=int, default=11)  # HM_OUT_RGBA
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--child", choices=["sequence", "items"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run(a.child, a.frames[0], a.iters, a.warmup, a.threads, a.format)))
        return
    lines = []
    for n in a.frames:
        for mode in ("sequence", "items"):
            r = run(mode, n, a.iters, a.warmup, a.threads, a.format)
            if a.kernel_trace:
                r.update(kernel_ms(mode, n, a.iters, a.warmup, a.threads, a.format) or {})
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
