"""GPU: the range-extension residual tools of k_recon's rare-syntax instances, block by block (corpus.rext_residual_sweep ...): implicit RDPCM,
transform-skip rotation, cross-component prediction, PCM, and the workgroup's one 32x32 staging area that the waves take in turn.
tests/test_rext_residual.py shows on the CPU which branches these streams reach and holds the model - tests/residual_ref.py +
tests/intra_ref.py - against the reference decoder.  Here the model runs on the product's OWN reconstruction-stage planes: every block must be
what the model computes from the product's neighbours, which names the first wrong block; the three stages are held against the oracle and the
reference's recorded fingerprints (tests/golden/rext_residual.json).

The lock pictures come FIRST in this file and in a batch of their own: theirs is the one test here whose failure could be a hang."""
import json
import os

import numpy as np
import pytest

import corpus
import gpudecode
import intrautil as iu
import orc
import residual_ref as rr
import rextutil as xu
import synthutil

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rext_residual.json")))
STAGES = (("recon", 0), ("deblock", 1), ("full", 3))


def _against_oracle_and_fingerprint(seed, kw, blob, g, stage, bits):
    exp, _ = orc.oracle_decode(blob, bits, crop=True)
    assert len(g) == len(exp)
    for c in range(len(exp)):
        bad = np.argwhere(g[c] != exp[c])
        assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"
    assert xu.fingerprint(g) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}: not the reference's fingerprint"


def test_lock_pictures_eight_copies_each(pkg):
    """pictures whose CTB rows are full of whole 32x32 blocks with residuals, eight copies of each in one batch: the waves of a workgroup take the
    32x32 staging area in turn.  Every block of every copy against the model, from the copy's own neighbours."""
    cases = corpus.rext_residual_lock_pictures()
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d) for d in streams]
    pics = [rr.Picture(pkg.capi.parse_hevc(d, record_order=xu.DECODE_ORDER)) for d in streams]
    for blob, P in zip(blobs, pics):
        assert not pkg.capi.stream_header(blob)["flags"] & rr.PIC_SPLIT_CHAINS
        # every CTB row - a wave of the picture's workgroup each - holds 32x32 blocks with residuals of their own, the blocks that take the staging area
        rows = [0] * P.ctb_h
        for rec in P.records():
            if rec["log2"] == 5 and rec["cbf"] and not rec["pcm"]:
                rows[(rec["y"] << (0 if rec["cidx"] == 0 or P.chroma_format != 1 else 1)) >> P.log2_ctb] += 1
        assert P.ctb_h >= 3 and min(rows) >= 2, rows
    got = gpudecode.decode_pictures(pkg, [b for b in blobs for _ in range(8)], 0)
    for i, g in enumerate(got):
        (seed, kw), P = cases[i // 8], pics[i // 8]
        bad = iu.first_mismatch(seed, P, g)
        assert bad is None, f"{kw} copy {i % 8}: {bad}"
        assert xu.fingerprint(g) == GOLD["cases"][str(seed)]["recon"], f"seed {seed} {kw} copy {i % 8}"


@pytest.fixture(scope="module")
def sweep(pkg):
    """the sweep in ONE batch per stage: (cases, blobs as parsed, Pictures in decode order, {stage bits: planes of every picture})"""
    cases = corpus.rext_residual_sweep(xu.N_SWEEP)
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d) for d in streams]
    pics = [rr.Picture(pkg.capi.parse_hevc(d, record_order=xu.DECODE_ORDER)) for d in streams]
    return cases, blobs, pics, {bits: gpudecode.decode_pictures(pkg, blobs, bits) for _, bits in STAGES}


@pytest.mark.parametrize("cls", xu.CLASSES)
def test_sweep_block_by_block(sweep, cls):
    """stage 0 of the pictures of one kernel class: every block - RDPCM, rotated, with a cross-component term, PCM - against the model computed from the
    product's own planes"""
    cases, blobs, pics, got = sweep
    n = 0
    for (seed, kw), P, g in zip(cases, pics, got[0]):
        if xu.kernel_class(P) != cls:
            continue
        bad = iu.first_mismatch(seed, P, g, pcm_bits=xu.pcm_bits(kw))
        assert bad is None, f"{kw}: not the model's block from the product's own neighbours: {bad}"
        n += 1
    assert n >= 100, n


def test_sweep_stages_oracle_fingerprints_and_instances(pkg, sweep):
    """stages 0 / 1 / 3 == the oracle and the reference's fingerprints; no picture goes out as split chains, and the six rare-syntax instances of
    k_recon (CTB size x bytes per sample) are all there"""
    cases, blobs, pics, got = sweep
    seen = set()
    for blob in blobs:
        h = pkg.capi.stream_header(blob)
        assert not h["flags"] & rr.PIC_SPLIT_CHAINS
        seen.add((1 << h["log2_ctb"], 2 if h["bit_depth"] > 8 else 1))
    assert seen == {(1 << l, b) for l in (4, 5, 6) for b in (1, 2)}, seen
    for stage, bits in STAGES:
        for (seed, kw), blob, g in zip(cases, blobs, got[bits]):
            _against_oracle_and_fingerprint(seed, kw, blob, g, stage, bits)


def test_single_ctb_pictures_block_by_block(pkg):
    """180 pictures of one CTB in one batch: the first block of every component is clip(1 << (bit_depth - 1) + residual), the tools' arithmetic alone;
    every block against the model, the three stages against the oracle and the fingerprints"""
    cases = corpus.rext_residual_single_ctb_cases()
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d) for d in streams]
    pics = [rr.Picture(pkg.capi.parse_hevc(d, record_order=xu.DECODE_ORDER)) for d in streams]
    assert all(P.n_ctbs == 1 for P in pics)
    for stage, bits in STAGES:
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), blob, P, g in zip(cases, blobs, pics, got):
            assert not pkg.capi.stream_header(blob)["flags"] & rr.PIC_SPLIT_CHAINS
            if bits == 0:
                bad = iu.first_mismatch(seed, P, g, pcm_bits=xu.pcm_bits(kw))
                assert bad is None, f"{kw}: {bad}"
            _against_oracle_and_fingerprint(seed, kw, blob, g, stage, bits)


def test_tiles_through_the_full_path(pkg):
    """four 192 x 144 tiles with the tools at stages 0 and 3: the oracle, the fingerprints, and at stage 0 every block against the model"""
    cases = corpus.rext_residual_tiles()
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d) for d in streams]
    for stage, bits in (STAGES[0], STAGES[2]):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), data, blob, g in zip(cases, streams, blobs, got):
            if bits == 0:
                bad = iu.first_mismatch(seed, rr.Picture(pkg.capi.parse_hevc(data, record_order=xu.DECODE_ORDER)), g, pcm_bits=xu.pcm_bits(kw))
                assert bad is None, f"{kw}: {bad}"
            _against_oracle_and_fingerprint(seed, kw, blob, g, stage, bits)
