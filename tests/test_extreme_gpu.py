"""GPU: the HIP residual path at the edges of its arithmetic - levels over the whole int16 range, QpY from -QpBdOffset to 51,
scaling factors pinned at 1 and 255 (corpus.extreme_sweep ...).  tests/test_extreme.py shows on the CPU that these streams
reach the edges (wrapping flat products, dequantised coefficients and stage-1 values at the int16 rails, second stages beyond
int16, DC-only blocks with clipped coefficients) and holds the oracle against the reference decoder's scalar build on them."""
import json
import os
import re

import numpy as np
import pytest

import corpus
import extremeutil as eu
import gpudecode
import orc
import synthutil
from test_decode_gpu import _check, _fp, _recon_launches

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extreme.json")))
N_SWEEP = len(GOLD["cases"])


def test_extreme_sweep(pkg):
    """all classes in one batch (k_residual + k_chain next to every k_recon variant): HIP == oracle plane for plane at stages
    0 / 1 / 3, and the fingerprints of the reference decoder's scalar build.  Behind them in the same batch the nine 8-bit cases with
    transquant bypass / unfiltered PCM as drawn (corpus.extreme_sweep(pcmf_8bit=True): no fingerprints - the reference's builds disagree
    on their deblocking; the oracle's reconstruction of them is held against the scalar build on the CPU)"""
    cases = corpus.extreme_sweep(N_SWEEP) + corpus.extreme_sweep(N_SWEEP, pcmf_8bit=True)
    blobs = [pkg.capi.parse_hevc(synthutil.picture(seed, **kw)) for seed, kw in cases]
    split = sum(bool(pkg.capi.stream_header(b)["flags"] & 0x1000) for b in blobs)
    assert len(cases) == N_SWEEP + 9 and 40 < split < N_SWEEP - 40  # both record orders
    for stage, bits in (("recon", 0), ("deblock", 1), ("full", 3)):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for k, ((seed, kw), blob, g) in enumerate(zip(cases, blobs, got)):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, (f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()} "
                                       f"got {g[c][tuple(bad[0])]} expected {exp[c][tuple(bad[0])]}")
            assert k >= N_SWEEP or _fp(g) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}: not the reference's fingerprint"


def test_extreme_sweep_in_decode_order():
    """the same pictures forced into decode order (HM_RECORDS_DECODE_ORDER): k_recon<..., false> on the ordinary ones, in all six
    instantiations, and neither k_residual nor k_chain; chain_mode_check.py holds every picture against the oracle on the same
    records AND against the fingerprints of the reference's scalar build"""
    err = _check({"HM_CHECK_ORDER": "2", "HM_CHECK_STAGES": "0,1,3", "HM_CHECK_COPIES": "1", "HM_CHAIN_DEBUG": "1"}, "extreme_sweep")
    assert "[k_chain]" not in err and "[k_residual]" not in err, err[-3000:]
    plain = {(ctb, bps) for _, ctb, bps, _, rare in _recon_launches(err) if not rare}
    assert plain == {(ctb, bps) for ctb in (16, 32, 64) for bps in (1, 2)}, plain


def test_single_ctb_pictures_equal_residual_ref(pkg):
    """3300 pictures of one CTB in one batch, stage 0, in both record orders: the first block of every component ==
    clip(1 << (bit_depth - 1) + residual_ref) - int64 numpy written from the standard (tests/residual_ref.py)"""
    pics, _ = eu.single_ctb_pictures(pkg.capi)
    for order in (eu.DECODE_ORDER, 0):  # decode order for all; the parser's own choice: split chains wherever the class allows
        blobs = [pkg.capi.parse_hevc(data, record_order=order) for _, _, data, _ in pics]
        split = sum(bool(pkg.capi.stream_header(b)["flags"] & 0x1000) for b in blobs)
        assert (split == 0) if order == eu.DECODE_ORDER else (split > 500), split
        got = gpudecode.decode_pictures(pkg, blobs, 0)
        for (seed, kw, _, firsts), g in zip(pics, got):
            bad = eu.first_mismatch(g, firsts)
            assert bad is None, f"seed {seed} {kw} record order {order}: {bad}"


def test_extreme_tiles_and_large_pictures_in_forced_cuts():
    """512 x 512 tiles and one large picture per class with the same knobs through chain_mode_check.py: a wave per picture, a ring
    of four bands of row pairs, a wave per chain with the early CTU start - the int16 residual slab and the hand-over lines
    carry rail values from wave to wave"""
    cuts = [{"chain_pairs": 0}, {"chain_ring": 4, "chain_pairs": 2}, {"chain_pairs": 3, "chain_early": 1}]
    err = _check({"HM_CHECK_CUTS": json.dumps(cuts), "HM_CHECK_STAGES": "0,3", "HM_CHECK_COPIES": "2", "HM_CHAIN_DEBUG": "1", "HM_QUAD_CLASS": "1"},
                 "extreme512", "extreme_large", timeout=900)
    parts = err.split("[check] cut ")[1:]
    assert len(parts) == len(cuts)
    assert all(re.search(r"^\[k_chain\] ", p, re.M) and re.search(r"^\[k_residual\] ", p, re.M) for p in parts), err[-3000:]
    assert "(one per picture)" in parts[0] and "in a ring" in parts[1] and "(one per chain of a CTU row)" in parts[2], err[-3000:]
