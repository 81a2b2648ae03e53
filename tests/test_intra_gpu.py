"""GPU: the HIP intra prediction, branch by branch (corpus.intra_sweep ...).  tests/test_intra.py shows on the CPU which branches
these streams reach and holds tests/intra_ref.py - the prediction from the standard, in numpy - against the reference decoder.
Here intra_ref runs on the product's OWN reconstruction-stage planes: every observable block must equal its prediction from
the product's neighbours (plus residual_ref's residual), which names the first wrong block instead of a picture that differs."""
import json
import os
import re

import numpy as np
import pytest

import corpus
import gpudecode
import intrautil as iu
import orc
import residual_ref as rr
import synthutil
from test_decode_gpu import _check, _fp

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intra.json")))
N_SWEEP = len(GOLD["cases"])


def _sweep(pkg, order):
    """the sweep in one batch with the given record order: stages 0 / 1 / 3 == the oracle and the fingerprints of the reference's
    scalar build; stage 0 block by block against intra_ref.  Returns the set of (split chains, CTB size, bytes per sample)."""
    cases = corpus.intra_sweep(N_SWEEP)
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d, record_order=order) for d in streams]
    seen = set()
    for stage, bits in (("recon", 0), ("deblock", 1), ("full", 3)):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), data, blob, g in zip(cases, streams, blobs, got):
            if bits == 0:
                h = pkg.capi.stream_header(blob)
                seen.add((bool(h["flags"] & rr.PIC_SPLIT_CHAINS), 1 << h["log2_ctb"], 2 if h["bit_depth"] > 8 else 1))
                P = rr.Picture(blob if order == iu.DECODE_ORDER else pkg.capi.parse_hevc(data, record_order=iu.DECODE_ORDER))
                bad = iu.first_mismatch(seed, P, g)
                assert bad is None, f"{kw}: not intra_ref's prediction from the product's own neighbours: {bad}"
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"
            assert _fp(g) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}: not the reference's fingerprint"
    return seen


def test_intra_sweep_as_parsed(pkg):
    """split chains (k_residual + k_chain) wherever the class allows, k_recon for the rest"""
    seen = _sweep(pkg, 0)
    assert {s for s in seen if s[0]} == {(True, 1 << l, b) for l in (4, 5, 6) for b in (1, 2)}, seen
    assert any(not s[0] for s in seen)


def test_intra_sweep_in_decode_order(pkg):
    """the same pictures forced into decode order: k_recon on all of them, the ordinary ones included (its plain instantiations)"""
    seen = _sweep(pkg, iu.DECODE_ORDER)
    assert seen == {(False, 1 << l, b) for l in (4, 5, 6) for b in (1, 2)}, seen


def test_single_ctb_pictures_block_by_block(pkg):
    """288 pictures of one CTB (CTB 16 / 32 / 64, every depth and chroma format, whole and split blocks, mostly calm units) in one batch, in
    both record orders: every observable block against intra_ref"""
    cases = corpus.intra_single_ctb_cases(288)
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    pics = [rr.Picture(pkg.capi.parse_hevc(d, record_order=iu.DECODE_ORDER)) for d in streams]
    for order in (iu.DECODE_ORDER, 0):
        blobs = [pkg.capi.parse_hevc(d, record_order=order) for d in streams]
        split = sum(bool(pkg.capi.stream_header(b)["flags"] & rr.PIC_SPLIT_CHAINS) for b in blobs)
        assert (split == 0) if order == iu.DECODE_ORDER else (split > 100), split
        got = gpudecode.decode_pictures(pkg, blobs, 0)
        for (seed, kw), P, g in zip(cases, pics, got):
            bad = iu.first_mismatch(seed, P, g)
            assert bad is None, f"{kw} record order {order}: {bad}"


def test_intra_tiles_in_forced_cuts():
    """corpus.intra_tiles through chain_mode_check.py in the cuts of test_chain_modes_gpu.py: a wave per picture (32 pictures in the batch: phase C with
    four groups busy), a wave per chain pair count 1-3 with and without the early start, rings of 2 / 4 / 8 bands, shared chains"""
    cuts = [{"chain_pairs": 0}] + [{"chain_pairs": p, "chain_early": e} for p in (1, 2, 3) for e in (0, 1)] + \
           [{"chain_ring": r, "chain_pairs": 2} for r in (2, 4, 8)] + [{"chain_share": 2}]
    err = _check({"HM_CHECK_CUTS": json.dumps(cuts), "HM_CHECK_STAGES": "0,3", "HM_CHECK_COPIES": "8", "HM_CHAIN_DEBUG": "1", "HM_QUAD_CLASS": "1"},
                 "intra512", timeout=900)
    parts = err.split("[check] cut ")[1:]
    assert len(parts) == len(cuts)
    assert all(re.search(r"^\[k_chain\] ", p, re.M) for p in parts), err[-3000:]
    assert "(one per picture)" in parts[0] and all("in a ring" in p for p in parts[7:10]), err[-3000:]
