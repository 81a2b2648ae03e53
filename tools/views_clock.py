#!/usr/bin/env python3
"""Many views of one picture, measured (GPU box, repo root):  python3 tools/views_clock.py [--out profiles/device_views.txt]

The picture is ONE 12 MP 8-bit grid (4032 x 3024, 8 x 6 tiles of 512 x 512, 4:2:0), built as bench.py's config 2 builds it.  View sets,
all HM_VIEW_TRIANGLE into CHW float32:
  multi-crop   2 x 224^2 from crops of 40 .. 100 % of the area and 8 x 96^2 from 5 .. 40 %, aspect 3:4 .. 4:3, fixed seed
  pyramid      four thumbnail levels of the whole image: 1008 x 756, 504 x 378, 252 x 189, 126 x 95
  one view     224^2 of one crop: the control
For each set, three ways in the same process in alternating rounds:
  (a) K calls of hm_decode_item_to_device_view                    what a caller had before
  (b) hm_decode_item_to_device_views with the hook view_multi = 0  one decode, hm_out_write per view
  (c) hm_decode_item_to_device_views                               one decode, one launch per pass and group
The calls are synchronous (they return with the stream drained): the time is the host's wall clock around them, warm-up first, median
of the rounds with min .. max - sections 4 and 5 ("Steady state and noise") of the measuring guide this project follows: warm every shape
up, compare versions in one call, alternating, and look at the spread before trusting a difference.  libheif_mi355x_test.so is the
library measured throughout: the shipping library's objects plus the hook.  Every view set runs in a child process of its own under a
time limit; after a child that fails or runs out of time nothing more is started.  Nothing here is a pass / fail check."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 4032, 3024
RGB, CHW, F32, TRIANGLE = 10, 1, 3, 0
SETS = ("multi-crop", "pyramid", "one view")


def view_set(name):
    """[(crop or None, (ow, oh))]"""
    import random
    if name == "pyramid":
        return [(None, (1008, 756)), (None, (504, 378)), (None, (252, 189)), (None, (126, 95))]
    rng = random.Random(20241)

    def crop(lo, hi):
        area = rng.uniform(lo, hi) * W * H
        aspect = rng.uniform(3 / 4, 4 / 3)
        cw, ch = min(W, int((area * aspect) ** 0.5)), min(H, int((area / aspect) ** 0.5))
        return rng.randrange(0, W - cw + 1), rng.randrange(0, H - ch + 1), cw, ch
    crops = [(crop(0.40, 1.00), (224, 224)) for _ in range(2)] + [(crop(0.05, 0.40), (96, 96)) for _ in range(8)]
    return crops if name == "multi-crop" else [(crops[2][0], (224, 224))]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def build_file(path):
    import bench
    import heifwriter
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        tiles = list(pool.map(bench.tile_stream, range(8300000, 8300000 + bench.GRID_COLS * bench.GRID_ROWS)))
    with open(path, "wb") as f:
        f.write(heifwriter.write_heic(tiles, (bench.TILE, bench.TILE), grid=(bench.GRID_ROWS, bench.GRID_COLS, W, H)))


def measure(name, path, rounds, threads):
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
    data = open(path, "rb").read()
    fh = C.c_void_p()
    assert L.hm_file_open(data, len(data), C.byref(fh)) == 0
    iid = L.hm_file_primary_item(fh)
    specs = view_set(name)
    n = len(specs)
    views, dests, tensors = (capi.DeviceView * n)(), (capi.DeviceDest * n)(), []
    for k, (crop, (ow, oh)) in enumerate(specs):
        views[k] = capi.DeviceView(*(crop or (0, 0, 0, 0)), ow, oh, TRIANGLE)
        t = torch.empty((3, oh, ow), dtype=torch.float32, device="cuda")
        tensors.append(t)
        dests[k].ptr, dests[k].len, dests[k].layout, dests[k].dtype = t.data_ptr(), t.numel() * 4, CHW, F32
        for c in range(4):
            dests[k].scale[c], dests[k].bias[c] = 1.0 / 255, 0.0
    prm = capi.DecodeParams(RGB, threads, 0, 0, None, None, 0, 0, 0, 0)
    out = (capi.Decoded * n)()
    tiles = (C.c_int32 * 4)()
    assert L.hm_plan_views(fh, iid, C.byref(prm), views, n, C.byref(tiles)) == 0

    def singles():
        one = capi.Decoded()
        for k in range(n):
            rc = L.hm_decode_item_to_device_view(fh, iid, C.byref(prm), C.byref(views[k]), C.byref(dests[k]), C.byref(one))
            assert rc == 0, L.hm_last_error().decode()

    def many(multi):
        assert L.hm_debug_set(b"view_multi", multi) == 0
        rc = L.hm_decode_item_to_device_views(fh, iid, C.byref(prm), views, dests, n, None, None, None, None, out, None)
        assert rc == 0, L.hm_last_error().decode()
        L.hm_debug_set(b"view_multi", 1)
    paths = [(f"(a) {n} x hm_decode_item_to_device_view", singles), ("(b) hm_decode_item_to_device_views, view_multi = 0", lambda: many(0)),
             ("(c) hm_decode_item_to_device_views", lambda: many(1))]
    results = []
    for _, fn in paths:  # warm-up: code objects, pools, worker threads - and the three paths' bytes
        fn()
        fn()
        torch.cuda.synchronize()
        results.append([t.clone() for t in tensors])
    same = all(torch.equal(a, b) for r in results[1:] for a, b in zip(r, results[0]))
    times = {label: [] for label, _ in paths}
    for _ in range(rounds):
        for label, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) * 1e3)
    mp = sum(ow * oh for _, (ow, oh) in specs) / 1e6
    print(f"{name}: {n} views, {mp:.3f} MP written; tiles decoded by (b) and (c): rows {tiles[0]} .. {tiles[0] + tiles[1] - 1}, columns {tiles[2]} .. {tiles[2] + tiles[3] - 1} "
          f"({tiles[1] * tiles[3]} of 48); the three paths' tensors are {'identical' if same else 'NOT identical'}")
    for label, _ in paths:
        v = times[label]
        print(f"     {label:52s} {median(v):8.2f} ms ({min(v):.2f} .. {max(v):.2f})")
    a, c = median(times[paths[0][0]]), median(times[paths[2][0]])
    print(f"     (a) / (c) = {a / c:.2f}")
    L.hm_file_close(fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=240, help="seconds a view set's child process may take")
    ap.add_argument("--set", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--file", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.set:
        return measure(args.set, args.file, args.rounds, args.threads)
    lines = ["$ python3 tools/views_clock.py " + " ".join(sys.argv[1:]),
             f"one 12 MP grid ({W} x {H}, 8 x 6 tiles of 512 x 512, 8-bit 4:2:0) -> RGB24 -> HM_VIEW_TRIANGLE views, CHW float32; {args.threads} host threads; "
             f"{args.rounds} alternating rounds per path behind two warm-up calls each, wall clock of the synchronous calls: median (min .. max)"]
    print("\n".join(lines), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "grid12mp.heic")
        build_file(path)
        for name in SETS:
            cmd = [sys.executable, os.path.abspath(__file__), "--set", name, "--file", path, "--rounds", str(args.rounds), "--threads", str(args.threads)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
            except subprocess.TimeoutExpired:
                lines.append(f"{name}: no result within {args.limit} s; nothing more was started")
                print(lines[-1], flush=True)
                break
            print(r.stdout, end="", flush=True)
            lines += r.stdout.splitlines()
            if r.returncode != 0:
                lines.append(f"{name}: the child process ended with status {r.returncode}; nothing more was started\n{r.stderr[-2000:]}")
                print(lines[-1], flush=True)
                break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
