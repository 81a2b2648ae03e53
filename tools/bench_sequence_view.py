#!/usr/bin/env python3
"""A clip under a view, measured (GPU box, repo root):  python3 tools/bench_sequence_view.py [--out profiles/sequence_view.txt]

32 and 128 frames of 1920 x 1080 (the three basketball_1080p_qp{1,25,32} pictures repeated, as tools/sequence_bench.py) -> RGB24 ->
224 x 224 CHW float32 slices of one T x 3 x 224 x 224 allocation, HM_VIEW_TRIANGLE and HM_VIEW_CUBIC, three ways in the same run in
alternating rounds:
  batched     hm_decode_frames_to_device_view (one launch per resampling pass and chunk for all frames)
  per-frame   the same call with the test hook view_batch = 0 (hm_out_write once per frame behind the one decode batch)
  items       `count` calls of hm_decode_item_to_device_view (a batch of one picture each)
Wall clock of the call(s), and the span between two HIP events recorded on the stream in front of and behind them (the calls are
synchronous: the span holds the host's entropy decode too).  libheif_mi355x_test.so is the library measured throughout: the
shipping library's objects plus the hook.  Prints (and writes to --out); nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, OW, OH = 1920, 1080, 224, 224
RGB, CHW, F32 = 10, 1, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--frames", type=int, nargs="*", default=[32, 128])
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import moovwriter
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

    pics = [open(os.path.join(ROOT, "tests", "data", f"basketball_1080p_qp{q}.hevc"), "rb").read() for q in (1, 25, 32)]
    say(f"device: {torch.cuda.get_device_name(0)}; {args.threads} host threads; {args.rounds} alternating rounds per path, medians (min .. max)")
    say(f"{W} x {H} 8-bit 4:2:0 frames -> RGB24 -> whole frame at {OW} x {OH}, CHW float32, slices of one T x 3 x {OH} x {OW} tensor")
    for n in args.frames:
        data = moovwriter.write_movie([pics[k % 3] for k in range(n)], (W, H))
        fh = C.c_void_p()
        assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
        dst = torch.empty((n, 3, OH, OW), dtype=torch.float32, device="cuda")
        per = 3 * OH * OW * 4
        dests = (capi.DeviceDest * n)()
        for k in range(n):
            dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = dst.data_ptr() + k * per, per, CHW, F32
            for c in range(4):
                dests[k].scale[c], dests[k].bias[c] = 1.0 / 255, 0.0
        ids = (C.c_uint32 * n)(*range(1, n + 1))
        prm = capi.DecodeParams(RGB, args.threads, 0, 0, torch.cuda.current_stream().cuda_stream or None, None, 0, 0, 0, 0)
        out = (capi.Decoded * n)()
        for fname, filt in (("triangle", capi.HM_VIEW_TRIANGLE), ("bicubic", capi.HM_VIEW_CUBIC)):
            view = capi.DeviceView(0, 0, 0, 0, OW, OH, filt)

            def frames_call(batch):
                assert L.hm_debug_set(b"view_batch", batch) == 0
                rc = L.hm_decode_frames_to_device_view(fh, ids, n, C.byref(prm), C.byref(view), dests, out, None)
                assert rc == 0, L.hm_last_error().decode()
                L.hm_debug_set(b"view_batch", 1)

            def items_call():
                one = capi.Decoded()
                for k in range(n):
                    rc = L.hm_decode_item_to_device_view(fh, k + 1, C.byref(prm), C.byref(view), C.byref(dests[k]), C.byref(one))
                    assert rc == 0, L.hm_last_error().decode()

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
            paths = [("batched (hm_decode_frames_to_device_view)", lambda: frames_call(1)), ("per-frame hm_out_write (view_batch = 0)", lambda: frames_call(0)),
                     (f"{n} x hm_decode_item_to_device_view", items_call)]
            results = {}
            for name, fn in paths:
                fn()  # warm-up: code object load, pools
                results[name] = dst.clone()
            assert all(torch.equal(r, results[paths[0][0]]) for r in results.values()), "the three paths do not give the same bytes"
            times = {name: [] for name, _ in paths}
            for _ in range(args.rounds):
                for name, fn in paths:
                    times[name].append(timed(fn))
            say(f"  {n} frames, {fname}: (the three paths' tensors are identical)")
            for name, _ in paths:
                wall, ev = [t[0] for t in times[name]], [t[1] for t in times[name]]
                say(f"     {name:46s} wall {median(wall):8.2f} ms ({min(wall):.2f} .. {max(wall):.2f})   events {median(ev):8.2f} ms ({min(ev):.2f} .. {max(ev):.2f})")
        L.hm_file_close(fh)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
