"""The schedules of hm_batch_execute's overlapped groups (csrc/hm_overlap_plan.h) on bench.py's batch, in one process: ms per
step (host clock around a synchronise, 3 x 8 steps) on one stream, with the default schedule, and with the cut forced through the
test library's knobs overlap_min_pics / overlap_cut; the outputs of a sample of images are compared with the single stream's in
every variant.  profiles/batch_overlap.txt holds the runs.

usage: python tools/overlap_sweep.py [IMAGES[,IMAGES...]] [OUTPUT.txt]      the variants at 384 images, halves and the plan's cut at the others
       SWEEP=1 python tools/overlap_sweep.py IMAGES[,...] [OUTPUT.txt]      every whole-round cut and the halves at every count"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


import torch
import __graft_entry__ as g
import bench

pkg = g.load_package(test_knobs="always")
L = pkg.lib()
L.hm_debug_batch_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
capi = pkg.capi
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
st = torch.cuda.current_stream().cuda_stream
NT = bench.GRID_COLS * bench.GRID_ROWS
COUNTS = [int(x) for x in (sys.argv[1].split(",") if len(sys.argv) > 1 else "384,256,192,128,96,48".split(","))]
BMAX = max(COUNTS)
t0 = time.time()
seeds = (1200000 + 48 * (k // NT) + k % NT for k in range(BMAX * NT))
blobs = [b for _, b in bench.make_streams(capi, seeds, keep_data=False)]
say(f"# {BMAX} images synthesised and parsed in {time.time() - t0:.1f} s")


def knob(**kw):
    for k, v in kw.items():
        assert L.hm_debug_set(k.encode(), v) == 0


def groups(gb):
    cut = C.c_int(-1)
    return L.hm_debug_batch_groups(gb.batch.h, C.byref(cut)), cut.value


def clock(gb, reps=3, steps=8):
    for _ in range(2):
        gb.step(st)
    torch.cuda.synchronize()
    v = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(steps):
            gb.step(st)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t) / steps * 1e3)
    return v


def fmt(v):
    return f"median {statistics.median(v):7.3f}  range {min(v):7.3f} .. {max(v):7.3f}"


for B in COUNTS:
    gb = bench.GridBatch(pkg, dev, bench.GRID_COLS, bench.GRID_ROWS, bench.TILE, bench.OUT_W, bench.OUT_H)
    for j in range(B):
        gb.add_image(blobs[j * NT:(j + 1) * NT])
    gb.finish(st, 0)
    knob(overlap_min_pics=0, overlap_cut=0)
    gb.batch.set_concurrency(1)
    gb.step(st)
    torch.cuda.synchronize()
    gb.batch.check()
    sample = list(range(0, B, max(1, B // 24)))
    want = {i: gb.images[i]["rgb"].clone() for i in sample}
    say(f"\n## {B} images = {B * NT} pictures")
    variants = [("single stream (set_concurrency 1)", 1, {}),
                ("default (set_concurrency 0, no knobs)", 0, {})]
    if B >= 2:
        variants += [("auto forced on, plan's cut", 0, dict(overlap_min_pics=1)),
                     ("auto forced on, equal halves", 0, dict(overlap_min_pics=1, overlap_cut=B // 2))]
    if os.environ.get("SWEEP"):
        variants = variants[:2]
        for k in range(1, 6):
            cut = k * 5120 // NT
            if cut < B - 1:
                variants.append((f"cut behind {k} round(s): image {cut}, {B * NT / 5120 - k:.2f} rounds second", 0, dict(overlap_min_pics=1, overlap_cut=cut)))
        variants.append(("equal halves", 0, dict(overlap_min_pics=1, overlap_cut=B // 2)))
    elif B == 384:
        for cut in (106, 160, 213, 214, 240, 266, 320):
            variants.append((f"cut at image {cut} ({cut * NT} pictures first)", 0, dict(overlap_min_pics=1, overlap_cut=cut)))
        variants += [("3 equal groups (set_concurrency 3)", 3, {}), ("4 equal groups (set_concurrency 4)", 4, {})]
    variants.append(("single stream again", 1, {}))
    for name, conc, kn in variants:
        knob(overlap_min_pics=0, overlap_cut=0)
        knob(**kn)
        gb.batch.set_concurrency(conc)
        for i in sample:
            gb.images[i]["rgb"].zero_()
        v = clock(gb)
        same = all(torch.equal(gb.images[i]["rgb"], want[i]) for i in sample)
        gb.batch.check()
        say(f"{name:52s} groups {groups(gb)}  {fmt(v)}  pixels {'equal' if same else 'DIFFER'}")
        if not same:
            say("STOP: pixels differ")
            sys.exit(2)
    # what the timing slots say on the default
    knob(overlap_min_pics=0, overlap_cut=0)
    for conc in (1, 0):
        gb.batch.set_concurrency(conc)
        elapsed, avg = bench.timed_steps(torch, gb, st, 5)
        say(f"timings5 (chain, -, tail, -, residual) set_concurrency({conc}): {[round(x, 3) for x in avg]}  step {elapsed / 5 * 1e3:.3f} ms")
    gb.batch.set_concurrency(0)
    gb.batch.close()
    del gb, want
    torch.cuda.empty_cache()
say("done")
