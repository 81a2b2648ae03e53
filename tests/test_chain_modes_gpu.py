"""GPU: the cuts of the prediction-chain kernel (chain.hip) - a wave per picture, per pair of CTU rows, per row, per
chain - must all give the oracle's pictures, for every picture class that can take the split-chain path
(HM_QUAD_CLASS=1 sends all of them there); and the waits between waves are bounded: with the first band's progress
withheld (fault injection) the launch is flagged, hm_batch_check reports HM_ERR_INTERNAL, nothing hangs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(env_extra, *names, timeout=300):
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE, env.get("PYTHONPATH", "")])
    return subprocess.run([sys.executable, os.path.join(HERE, "chain_mode_check.py"), *names], env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("cut", [0, 1, 2, 3])
def test_every_cut_gives_the_same_pictures(cut):
    r = _run({"HM_CHAIN_PAIRS": str(cut), "HM_QUAD_CLASS": "1"})
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("share", [2, 3, 4])
def test_waves_that_take_the_row_pairs_of_a_picture_in_turn(share):
    """mid-size batches: W waves per picture, wave b works on the pairs of CTU rows b, b + W, ... (hand-over in both
    directions, the wave's line of the row above refilled from the hand-over lines for every pair)"""
    r = _run({"HM_CHAIN_SHARE": str(share), "HM_QUAD_CLASS": "1", "HM_CHAIN_DEBUG": "1"})
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "in turn" in r.stderr, r.stderr


@pytest.mark.parametrize("cut", [1, 2, 3])
@pytest.mark.parametrize("waves", [2, 3, 8])
def test_waves_of_a_picture_in_one_workgroup_hand_over_in_a_ring(waves, cut):
    """mid-size batches: the W waves that take a picture's bands (pairs of rows, rows, chains of a row) in turn lie in one workgroup,
    every hand-over - also from the last wave back to the first - goes through its LDS (chain.hip: wg_ring)"""
    r = _run({"HM_CHAIN_RING": str(waves), "HM_CHAIN_PAIRS": str(cut), "HM_QUAD_CLASS": "1", "HM_CHAIN_DEBUG": "1"})
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "in a ring" in r.stderr, r.stderr
    r = _run({"HM_CHAIN_RING": str(waves), "HM_CHAIN_PAIRS": str(cut)}, "mixed")
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    if cut == 3:  # a wave per chain: by default the waves swap the luma and the chroma chain from band to band; also with fixed kinds
        r = _run({"HM_CHAIN_RING": str(waves), "HM_CHAIN_PAIRS": "3", "HM_CHAIN_ALT": "0", "HM_QUAD_CLASS": "1"})
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_large_pictures_keep_their_wavefront():
    """32 pictures of 48 x 64 CTUs (BASELINE config 4): a wave per chain of every row still fits the device, and a ring of 8 rows in
    flight would cost the picture its wavefront (measured 8.3 instead of 27.7 GP/s) - the launcher's estimate must say no; with 128 of
    them the cuts without the ring are the slower ones (18.6 against 11.4 ms)"""
    r = _run({"HM_CHECK_COPIES": "32", "HM_CHAIN_DEBUG": "1"}, "big422", timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "in a ring" not in r.stderr and "one per chain of a CTU row" in r.stderr, r.stderr
    r = _run({"HM_CHECK_COPIES": "128", "HM_CHAIN_DEBUG": "1"}, "big422", timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "in a ring" in r.stderr, r.stderr


@pytest.mark.parametrize("name, copies, waves", [("tile512_a", 300, 8), ("tile512_a", 1000, 4), ("tile512_a", 1100, 4), ("tile512_a", 1500, 4), ("tile512_a", 2048, 2),
                                                 ("hi422_10", 3000, 4), ("mono10_wide", 2500, 2)])
def test_the_ring_the_launcher_chooses(name, copies, waves):
    """512x512 tiles: the finest cut whose waves are all resident (r05: twenty one-chain waves per CU, sixteen of row pairs - 1100 tiles
    take rings of two one-chain waves per kind, where three row-pair waves fitted before; r06: 1500 tiles take rings of two one-chain bands per kind in two rounds - measured
    against the resident ring of two row-pair waves, which 2048 tiles keep); 10-bit 4:2:2 pictures, whose wave per picture is so short of LDS that
    a CU holds ten: rings of 2 bands x 2 kinds even when they do not all fit the device (profiles/r04_ring_sweep.txt) - and the
    oracle's pictures"""
    r = _run({"HM_CHECK_COPIES": str(copies), "HM_CHAIN_DEBUG": "1"}, name, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert f"a picture's {waves} waves in one workgroup" in r.stderr, r.stderr


@pytest.mark.parametrize("segs", [2, 5, 16])
def test_residual_prepass_in_segments_of_a_row(segs):
    """few pictures: k_residual cuts every CTU row into runs of CTUs (the levels of a run start where the CTU header says,
    its residuals at the CTU's own place in the row's slab); forced here for every class, also more segments than CTUs"""
    r = _run({"HM_RESID_SEGS": str(segs), "HM_QUAD_CLASS": "1"})
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_widest_pictures_fall_back_to_a_finer_cut():
    """16384 columns of 16-bit 4:2:2 samples with 64x64 CTBs: the sample lines of a wave per picture (forced here) do not
    fit a wave's share of LDS; the launcher then cuts the pictures into a wave per CTU row (or chain) instead of refusing"""
    r = _run({"HM_CHAIN_PAIRS": "0", "HM_CHAIN_DEBUG": "1"}, "wide16k")
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "one per CTU row" in r.stderr or "one per chain" in r.stderr, r.stderr


@pytest.mark.parametrize("cut", [1, 2, 3])
def test_bounded_waits_flag_the_launch(cut):
    r = _run({"HM_CHAIN_PAIRS": str(cut), "HM_CHAIN_TEST_STALL": "1", "HM_CHAIN_SPIN_LIMIT": "2000"}, "tile512_a", timeout=120)
    assert r.returncode == 3 and "gave up waiting" in r.stdout, r.stdout + r.stderr


def test_bounded_waits_in_the_ring():
    r = _run({"HM_CHAIN_RING": "4", "HM_CHAIN_PAIRS": "2", "HM_CHAIN_TEST_STALL": "1", "HM_CHAIN_SPIN_LIMIT": "2000"}, "tile512_a", timeout=120)
    assert r.returncode == 3 and "gave up waiting" in r.stdout, r.stdout + r.stderr


def test_bounded_waits_with_several_waves_per_picture():
    """the same fault injection when three waves take a picture's pairs of rows in turn: the wave that owns pair 0 keeps
    its progress to itself, the others give up, the launch is flagged, nothing hangs"""
    r = _run({"HM_CHAIN_SHARE": "3", "HM_CHAIN_TEST_STALL": "1", "HM_CHAIN_SPIN_LIMIT": "2000"}, "tile512_a", timeout=120)
    assert r.returncode == 3 and "gave up waiting" in r.stdout, r.stdout + r.stderr


def test_partial_last_round_goes_to_a_launch_of_its_own():
    """r05: 5632 pictures = one full round of the 5120 wave-per-picture chains the device holds + 512.  The 512 go to a launch of
    their own on a second stream, in the cut the launcher takes for 512 pictures (rings), beside the full round (9.9 -> 7.9 ms);
    every picture equals the oracle's (the knob chain_split = 0 keeps r04's one launch: tools/r05_staircase.sh)."""
    r = _run({"HM_CHECK_COPIES": "5632", "HM_CHAIN_DEBUG": "1"}, "tile512_a", timeout=1200)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "[k_chain] 512 pictures" in r.stderr and "in a ring" in r.stderr and "[k_chain] 5120 pictures, 5120 waves (one per picture)" in r.stderr, r.stderr


def test_two_mid_size_batches_side_by_side_never_starve_each_other():
    """1300 tiles is where the launcher lets several waves per picture take its row pairs in turn through HBM -
    a cut whose waves must all be resident together.  Two such launches side by side (two batches on two streams of one process, as
    the plugin worker's executors and hm_batch_set_concurrency produce them) must not hold half of the device each and wait for the
    other half: the waves are reserved per device for the launch's lifetime, the launch that does not get them takes a wave per
    picture (chain.hip: share_reserve).  50 rounds: no HM_ERR_INTERNAL, every picture the oracle's."""
    code = r'''
import sys, numpy as np, torch
import __graft_entry__ as g, corpus, orc
pkg = g.load_package(test_knobs=True)
capi, L = pkg.capi, pkg.lib()
dev = torch.device("cuda:0")
blob = capi.parse_hevc(corpus.stream("tile512_a"))
exp = orc.oracle_decode(blob, 3, crop=True)[0]
ys, cs = L.hm_plane_stride(512, 1), L.hm_plane_stride(256, 1)
streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
batches, planes = [], []
for k in range(2):
    p = [torch.zeros((512, ys), dtype=torch.uint8, device=dev), torch.zeros((256, cs), dtype=torch.uint8, device=dev), torch.zeros((256, cs), dtype=torch.uint8, device=dev)]
    b = capi.Batch()
    for i in range(1300):
        d = capi.TileDest()
        d.plane[0], d.plane[1], d.plane[2] = p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr()
        d.pitch[0], d.pitch[1], d.pitch[2] = ys, cs, cs
        d.canvas_width, d.canvas_height, d.x0, d.y0 = 512, 512, 0, 0
        b.add(blob, d)
    b.upload(streams[k].cuda_stream)
    batches.append(b); planes.append(p)
torch.cuda.synchronize()
for rnd in range(50):
    for k in range(2):
        for t in planes[k]:
            t.zero_()
    torch.cuda.synchronize()
    for k in range(2):
        batches[k].execute(3, streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        batches[k].check()  # raises on HM_ERR_INTERNAL
        for c, (w, h) in enumerate(((512, 512), (256, 256), (256, 256))):
            if not np.array_equal(planes[k][c].cpu().numpy()[:h, :w], exp[c].astype(np.uint8)):
                print(f"round {rnd}, batch {k}, plane {c} differs"); sys.exit(1)
print("OK")
'''
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE, env.get("PYTHONPATH", "")])
    env["HM_CHAIN_DEBUG"] = "1"
    env["HM_CHAIN_SHARE"] = "3"  # (the cut under test, whatever the launcher's own choice for 1300 tiles is on this device)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "taking its pairs of CTU rows in turn" in r.stderr, r.stderr[-2000:]  # (the cut under test ran ...)
    assert "1300 waves (one per picture)" in r.stderr, r.stderr[-2000:]          # (... and a launch beside it stepped aside)


def test_hot_path_kernels_hold_their_registers_without_a_spill():
    """A spilled register comes back with a LOAD, and loads and stores share one in-order counter: a reload inside a loop waits for every
    store in flight ("One counter" - k_residual lost 10 % to three spilled values).  The kernels of the hot path as the
    loaded code object has them (test hook hm_debug_kernel_regs): no scratch, and the register counts their waves per SIMD need -
    k_residual seven (72), the wave per picture of the 8-bit classes and every cut with one chain per wave five (96), k_tail420 eight (64)."""
    import ctypes as C
    import __graft_entry__ as g
    pkg = g.load_package()
    pkg.lib()  # (torch's HIP runtime first)
    L = C.CDLL(pkg.capi.TEST_LIB_PATH)  # (the shipping library's objects + the probe: csrc/test_hooks.cpp)
    L.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()

    def regs(which, a=0, b=0, c=0):
        assert L.hm_debug_kernel_regs(which, a, b, c, C.byref(out)) == 0
        return out[0], out[1]
    r, scratch = regs(0)
    assert scratch == 0 and r <= 72, ("k_residual", r, scratch)
    r, scratch = regs(1)
    assert scratch == 0 and r <= 64, ("k_tail420", r, scratch)
    r, scratch = regs(3)  # (r06: its 16-bit instantiation, the class of HDR photographs - four workgroups per CU by LDS, 128 registers would do)
    assert scratch == 0 and r <= 96, ("k_tail420<16-bit>", r, scratch)
    for l2 in (4, 5):  # (CTBs of 64: the wave per picture stays at four waves per SIMD - its LDS allows ten waves per CU)
        r, scratch = regs(2, l2, 1, 0)
        assert scratch == 0 and r <= 96, ("k_chain, a wave per picture", l2, r, scratch)
    for l2 in (4, 5, 6):
        for bps in (1, 2):
            for mode in (0, 1, 2, 3, 4, 5, 6):  # (5 / 6: 3 / 4 with the early CTU start, the kernels of launches the device holds at once)
                r, scratch = regs(2, l2, bps, mode)
                assert scratch == 0, ("k_chain", l2, bps, mode, r, scratch)
                if mode >= 3 and not (bps == 2 and l2 == 6):
                    assert r <= 96, ("k_chain, one chain per wave", l2, bps, mode, r)


@pytest.mark.parametrize("cls", ["8bit_420_ctb32", "8bit_420_ctb16", "10bit_420_ctb32"])
def test_the_launcher_stays_near_the_best_cut(cls):
    """tools/check_launcher.py on three tile counts between the regimes: the launcher's own cut within 15 % of the best of the 27 cuts
    it can be forced into (profiles/r05_launcher_check.txt: within 4 % at 118 of 126 points).  A kernel change that makes some cut
    faster than the launcher's calibration knows - r05: five waves per SIMD for the one-chain cuts - shows up here."""
    import json
    env = dict(os.environ, HM_CLASS_ONLY=cls)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_launcher.py"), "768", "1280", "2560"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = json.loads(r.stdout.strip().splitlines()[-1])["rows"]
    for row in rows:
        assert row["ratio"] < 1.15, (cls, row["tiles"], row["ratio"], row["best_forced"], row["auto_ms"], row["best_ms"])


# ---- every cut on pictures with structure: several slices (ending in the middle of a CTU row: no OP_FAR block behind the CTUs below
# the end), dependent segments, HEVC tiles, WPP with slices (chain_mode_check.py: the set `structure`), reconstruction only and in full,
# against the oracle and the reference decoder's fingerprints.  One process per group of cuts; the stderr of every decode says which
# cut ran (HM_CHAIN_DEBUG).

# the 8-bit 4:2:0 512 x 512 tiles of CTB 32 with slices: 16 CTU rows, a ring of 4 or 8 bands with one chain each fits one workgroup
SLICED512 = ["tile512_slices", "tile512_slices_dependent_nolf", "tile512_tiles_uniform_slices", "tile512_tiles_explicit_slices", "tile512_wpp_slices"]
EARLY = "a CTU starts when the CTU above it is done"


def _run_cuts(cuts, *names, env_extra=None, timeout=600):
    """chain_mode_check.py once per entry of `cuts` (in one process) -> {(entry, picture name): that decode's stderr}"""
    env = {"HM_CHECK_CUTS": json.dumps(cuts), "HM_CHECK_STAGES": "0,3", "HM_CHAIN_DEBUG": "1", "HM_QUAD_CLASS": "1"}
    env.update(env_extra or {})
    r = _run(env, *names, timeout=timeout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr[-4000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[check] cut "):
            cut, key = int(line.split()[2]), None
        elif line.startswith("[check] "):
            key = (cut, line.split()[1])
            out.setdefault(key, "")
        elif key is not None:
            out[key] += line + "\n"
    assert {c for c, _ in out} == set(range(len(cuts))), sorted(out)
    return out


def _launches(text, kernel="k_chain"):
    return [ln for ln in text.splitlines() if ln.startswith(f"[{kernel}] ") and " pictures" in ln]


def test_every_cut_on_pictures_with_structure():
    """a wave per picture / per pair of CTU rows / per row / per chain of a row, the last with and without the early CTU start (MODE 5 and 3)"""
    want = {0: "(one per picture)", 1: "(one per pair of CTU rows)", 2: "(one per CTU row)", 3: "(one per chain of a CTU row)"}
    cuts = [{"chain_pairs": p, "chain_early": e} for p in (0, 1, 2, 3) for e in (1, 0)]
    out = _run_cuts(cuts, "structure")
    for (n, name), text in out.items():
        p, e = cuts[n]["chain_pairs"], cuts[n]["chain_early"]
        launches = _launches(text)
        assert launches, (cuts[n], name, text)
        mono = "mono" in name
        for ln in launches:
            assert want[2 if p == 3 and mono else p] in ln, (cuts[n], name, ln)  # (4:0:0: one chain per row already)
        # (the early start: the kernels of one chain per wave - a wave per chain, or per row of a 4:0:0 picture)
        assert (EARLY in text) == (e == 1 and (p == 3 or (p == 2 and mono))), (cuts[n], name, text)


def test_waves_that_take_row_pairs_in_turn_on_pictures_with_structure():
    cuts = [{"chain_share": w} for w in (2, 3, 4)]
    out = _run_cuts(cuts, "structure")
    for (n, name), text in out.items():
        launches = _launches(text)
        assert launches and not any("(one per picture)" in ln for ln in launches), (cuts[n], name, text)
        if name.startswith("tile512") and "ctb64" not in name:  # (8 or 32 CTU rows: more pairs than waves)
            assert all("taking its pairs of CTU rows in turn" in ln for ln in launches), (cuts[n], name, text)


def test_rings_on_pictures_with_structure():
    """rings of 2, 3, 4, 8 bands of row pairs / rows / chains, the one-chain rings also with fixed kinds of chain (chain_alt 0)"""
    cuts = [{"chain_ring": w, "chain_pairs": p} for p in (1, 2, 3) for w in (2, 3, 4, 8)]
    cuts += [{"chain_ring": w, "chain_pairs": 3, "chain_alt": 0} for w in (2, 3, 4, 8)]
    out = _run_cuts(cuts, "structure")
    for (n, name), text in out.items():
        c = cuts[n]
        if name in SLICED512 and c["chain_pairs"] == 3 and "in a ring" in text:  # the early start: alternating rings, rings of at least 4 bands
            assert (EARLY in text) == (c.get("chain_alt", 1) == 1 or c["chain_ring"] >= 4), (c, name, text)
    for n in range(len(cuts)):  # (a ring whose waves do not fit one workgroup's LDS falls back to a wave per picture: not every class takes every ring)
        assert any("in a ring" in text for (k, _), text in out.items() if k == n), cuts[n]


def test_early_start_in_non_alternating_rings_on_sliced_tiles():
    """The configuration the launcher allows by argument only (chain.hip: EARLY): rings of 4 and 8 bands with one chain each and fixed
    kinds, the early CTU start (MODE 5: a few pictures), on 512 x 512 tiles whose slices end in the middle of CTU rows - where a band may
    finish CTU j one CTU behind the band above instead of two.  One uploaded batch, 20 executes, every output compared each time."""
    cuts = [{"chain_ring": w, "chain_pairs": 3, "chain_alt": 0} for w in (4, 8)]
    out = _run_cuts(cuts, *SLICED512, env_extra={"HM_CHECK_EXECUTES": "20"}, timeout=900)
    for (n, name), text in out.items():
        w = cuts[n]["chain_ring"]
        assert f"a picture's {2 * w} waves in one workgroup" in text and EARLY in text, (cuts[n], name, text)


def test_pictures_per_workgroup_on_pictures_with_structure():
    cuts = [{"chain_np": k} for k in (2, 6, 16)] + [{"chain_np": k, "chain_pairs": p} for p in (1, 3) for k in (2, 6, 16)]
    out = _run_cuts(cuts, "structure")
    for n, c in enumerate(cuts):
        assert any(f", {c['chain_np']} waves per workgroup" in ln for (k, _), text in out.items() if k == n for ln in _launches(text)), c


def test_residual_segments_on_pictures_with_structure():
    cuts = [{"resid_segs": s} for s in (2, 5, 16)]
    out = _run_cuts(cuts, "structure")
    for (n, name), text in out.items():
        launches = _launches(text, "k_residual")
        assert launches and all(f"in {cuts[n]['resid_segs']} segments" in ln for ln in launches), (cuts[n], name, text)


def test_sliced_and_tiled_pictures_of_different_sizes_in_one_launch():
    cuts = [{}, {"chain_pairs": 1}, {"chain_pairs": 3}, {"chain_share": 3}, {"chain_ring": 4, "chain_pairs": 2},
            {"chain_ring": 8, "chain_pairs": 3, "chain_alt": 0}, {"chain_ring": 3, "chain_pairs": 3}]
    out = _run_cuts(cuts, "mixed_structure")
    for (n, name), text in out.items():
        assert len(_launches(text)) == 2, (cuts[n], text)  # (one class: one launch per decode - stages 0 and 3)
        if "chain_ring" in cuts[n]:
            assert "in a ring" in text, (cuts[n], text)


@pytest.mark.parametrize("copies, waves", [(300, 8), (1100, 4), (2048, 2)])
def test_the_ring_the_launcher_chooses_for_a_sliced_tile(copies, waves):
    """test_the_ring_the_launcher_chooses on a tile whose slices end in the middle of CTU rows: the resident rings and the rings in rounds"""
    r = _run({"HM_CHECK_COPIES": str(copies), "HM_CHECK_STAGES": "0,3", "HM_CHAIN_DEBUG": "1"}, "tile512_slices", timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr[-3000:]
    assert f"a picture's {waves} waves in one workgroup" in r.stderr, r.stderr[-3000:]
