"""Helper of test_residual_fixed_costs_gpu.py (run as a script, once for all its cases: the cut knobs are test hooks of the test
library, which a process must load in place of the shipping one).  Every case is a batch of a few synthetic pictures decoded on
the GPU at stages 0 (reconstruction: k_residual's residuals and micro-ops under k_chain) and 1 (+ deblocking through the separate
k_deblock, which reads k_residual's block map) - and 3 where SAO is comparable - and held against the oracle, bit for bit, once
per knob setting of the case.  "[case] <name> <settings>" goes to stderr before every setting's decodes, so that the launchers'
chain_debug lines behind it can be told apart; the last line of stdout is a JSON object {case: "ok" | first difference}."""
import json
import sys

import numpy as np

import __graft_entry__ as g
import gpudecode
import knobs
import orc
import synthutil

CUT_DEFAULTS = {"chain_pairs": -1, "chain_share": 0, "chain_ring": -1, "chain_alt": 1, "chain_np": 0, "resid_segs": 0, "chain_early": 1}
TWO_ROWS_COPIES = 912  # of each of three sizes, the tallest 3 CTB rows: 2736 x 2 x 3 = 16416 (row, kind) units, over the launcher's 16384

# every cut of k_chain that chain_mode_check.py's callers force: a wave per picture / row pair / row / chain with and without the
# early CTU start, row pairs taken in turn (hand-over through HBM), rings of bands (hand-over through LDS), alternating and not
FORCED_CUTS = ([{"chain_pairs": p, "chain_early": e} for p in (0, 1, 2, 3) for e in (1, 0)] + [{"chain_share": w} for w in (2, 3)] +
               [{"chain_ring": w, "chain_pairs": p} for p in (1, 2, 3) for w in (2, 3)] + [{"chain_ring": w, "chain_pairs": 3, "chain_alt": 0} for w in (2, 4)])


def pictures(first_seed, n, **kw):
    return [synthutil.picture(first_seed + k, **kw) for k in range(n)]


def cases():
    """name -> (streams, stages, knob settings)"""
    base = dict(log2_ctb=5, bit_depth=8, chroma_format=1)
    one, three, wide = dict(base, width=32, height=32), dict(base, width=96, height=96), dict(base, width=128, height=64)
    mixed = pictures(810, 2, **one) + pictures(820, 2, **three) + pictures(830, 2, **wide)
    c = {
        "one_ctb": (pictures(810, 3, **one), (0, 1, 3), [{}]),
        "three_rows": (pictures(820, 3, **three), (0, 1, 3), [{}, {"resid_segs": 1}, {"resid_segs": 2}, {"resid_segs": 3}]),
        "two_rows_wide": (pictures(830, 3, **wide), (0, 1, 3), [{}]),
        "mixed_few": (mixed, (0, 1, 3), [{}]),
        "mixed_two_rows_per_wave": ([mixed[0], mixed[2], mixed[4]] * TWO_ROWS_COPIES, (1,), [{}]),  # (one decode: stage 1 holds residuals and block map)
        # width and height no multiples of the CTB; CTB 16 at 8 bit: no SAO stage (the reference's 8-sample chroma quirk)
        "ragged_ctb16": (pictures(840, 3, width=72, height=40, log2_ctb=4), (0, 1), [{}]),
        "ragged_ctb32": (pictures(843, 3, width=72, height=40, log2_ctb=5), (0, 1, 3), [{}]),
        "ctb64": (pictures(850, 3, width=128, height=128, log2_ctb=6), (0, 1, 3), [{}]),
        "ten_bit_420": (pictures(860, 3, width=64, height=64, bit_depth=10), (0, 1, 3), [{}]),
        "ten_bit_422": (pictures(863, 3, width=64, height=64, bit_depth=10, chroma_format=2), (0, 1, 3), [{}]),
        "eight_bit_422": (pictures(866, 3, width=64, height=64, chroma_format=2), (0, 1, 3), [{}]),
        "mono": (pictures(870, 3, width=64, height=64, chroma_format=0), (0, 1, 3), [{}]),
        # whole 32x32 / 16x16 transform blocks in the last columns and rows of pictures that end inside a CTB (the wave-wide block-map path
        # next to the map's right and bottom edge; a transform block never crosses the edge itself)
        "big_blocks_at_the_edges": (pictures(880, 3, width=72, height=40, no_split=1, log2_max_tb=5, density=90) +
                                    pictures(883, 3, width=104, height=56, no_split=1, log2_max_tb=4, density=90), (0, 1, 3), [{}]),
        "slices_deblock_per_slice": (pictures(890, 3, width=128, height=96, slices=60, slice_lf_random=1, deblock_override=1) +
                                     pictures(893, 2, width=128, height=96, slices=80, pps_lf_across_slices_off=1, slice_lf_random=1), (0, 1, 3), [{}]),
        # k_chain (and its flush of finished CTUs) in every forced cut: 4 x 3 CTUs (a row pair plus a single row); and where a
        # chroma CTU has 64 rows (4:2:2, CTB 64)
        "forced_cuts": (pictures(900, 2, width=128, height=96), (0, 3), FORCED_CUTS),
        "forced_cuts_422_ctb64": (pictures(905, 2, width=128, height=128, log2_ctb=6, bit_depth=10, chroma_format=2), (0,), FORCED_CUTS),
    }
    return c


def fused_tail_case(pkg):
    """the block map under the FUSED tail (k_tail420) and under the separate kernels, both against the CPU flow (oracle tiles,
    paste, integer matrix): a 2 x 1 grid of 128 x 128 tiles cropped to 250 x 120"""
    import bench
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    cols, rows, tile, w, h = 2, 1, 128, 250, 120
    made = list(bench.make_streams(pkg.capi, (920 + k for k in range(cols * rows)), width=tile, height=tile))
    out = []
    for group in (0, -1):  # 0: fused where possible, -1: never
        gb = bench.GridBatch(pkg, dev, cols, rows, tile, w, h)
        gb.add_image([b for _, b in made])
        gb.finish(st, group)
        gb.batch.execute(3, st)
        torch.cuda.synchronize()
        gb.batch.check()
        if gb.batch.tail_fused() != (group == 0):
            return f"group {group}: tail_fused() is {gb.batch.tail_fused()}"
        out.append(gb.images[0]["rgb"].cpu().numpy()[:h, :w * 3].copy())
        strides = (gb.ys, gb.cs, gb.os)
        gb.batch.close()
    exp = bench.cpu_grid_image([d for d, _ in made], [b for _, b in made], cols, rows, tile, w, h, strides, False)[:h, :w * 3]
    for name, got in zip(("fused tail", "separate kernels"), out):
        if not np.array_equal(got, exp):
            return f"{name}: {int((got != exp).sum())} bytes differ from the CPU flow"
    return "ok"


def run_case(pkg, hm, streams, stages_list, settings):
    """-> "ok", or the first difference"""
    parsed = {}  # (a stream repeated in the batch is parsed once)
    for s in streams:
        if s not in parsed:
            parsed[s] = pkg.capi.parse_hevc(s)
    blobs = [parsed[s] for s in streams]
    expected = {}  # (id of a blob, stages) -> the oracle's planes: once per picture for all settings
    for cut in settings:
        for k, v in {**CUT_DEFAULTS, **cut}.items():
            knobs.set_knob(hm, k, v)
        print(f"[case] {CASE[0]} {json.dumps(cut, sort_keys=True)}", file=sys.stderr, flush=True)
        for stages in stages_list:
            got = gpudecode.decode_pictures(pkg, blobs, stages)
            for i, pic in enumerate(got):
                key = (id(blobs[i]), stages)
                if key not in expected:
                    expected[key] = orc.oracle_decode(blobs[i], stages, crop=True)[0]
                exp = expected[key]
                if len(pic) != len(exp):
                    return f"{json.dumps(cut, sort_keys=True)}: stages {stages}, picture {i}: {len(pic)} planes, the oracle {len(exp)}"
                for c in range(len(exp)):
                    if not np.array_equal(pic[c], exp[c]):
                        bad = np.argwhere(pic[c] != exp[c])
                        return f"{json.dumps(cut, sort_keys=True)}: stages {stages}, picture {i} plane {c}: {len(bad)} samples differ, first (y, x) = {bad[0].tolist()}"
    return "ok"


CASE = [""]  # the case that runs (for the "[case]" lines)


def main():
    pkg = g.load_package(test_knobs="always")
    hm = pkg.lib()
    knobs.set_knob(hm, "quad_class", 1)  # every class that can take the split chains does: k_residual runs for all cases
    knobs.set_knob(hm, "chain_debug", 1)
    wanted = sys.argv[1:]
    results = {}
    for name, (streams, stages_list, settings) in cases().items():
        if wanted and name not in wanted:
            continue
        CASE[0] = name
        try:  # (a case that raises - a refused stream, a wave that gave up - is that case's verdict, not the end of the others)
            results[name] = run_case(pkg, hm, streams, stages_list, settings)
        except Exception as e:  # noqa: BLE001
            results[name] = f"{type(e).__name__}: {e}"
        for k, v in CUT_DEFAULTS.items():
            knobs.set_knob(hm, k, v)
    if not wanted or "fused_tail" in wanted:
        print("[case] fused_tail {}", file=sys.stderr, flush=True)
        try:
            results["fused_tail"] = fused_tail_case(pkg)
        except Exception as e:  # noqa: BLE001
            results["fused_tail"] = f"{type(e).__name__}: {e}"
    print(json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
