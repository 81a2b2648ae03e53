"""CPU: the range-extension residual tools, block by block (corpus.rext_residual_sweep, rext_residual_single_ctb_cases,
rext_residual_lock_pictures): implicit RDPCM, transform-skip rotation, cross-component prediction, PCM.

  * tests/residual_ref.py + tests/intra_ref.py - the tools in numpy, written from the standard and the reference's scalar code -
    reproduce the reference decoder's reconstruction stage on EVERY block: live on a seeded slice of the pictures, and through the
    recorded fingerprints (tests/golden/rext_residual.json) on the rest - a set of planes that carries the reference's fingerprint
    is the reference's set of planes;
  * the oracle against the model on the oracle's own planes, and against the fingerprints at the three stages;
  * the census: which branches of the tools these streams reach, counted with the model alone from the records and those planes;
  * the switches of residual_ref.Quirks.  The GPU tests (test_rext_residual_gpu.py) run the same streams."""
import json
import os

import numpy as np
import pytest

import corpus
import intrautil as iu
import orc
import residual_ref as rr
import rextutil as xu
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "rext_residual.json")))
LIVE_EVERY = 6  # the live slice of the reference decoder: every sixth picture of each corpus (a seeded choice: the seeds are consecutive)


@pytest.fixture(scope="module")
def pictures(pkg):
    """{corpus: [(seed, kw, stream, Picture in decode order)]}"""
    out = {}
    for name, cases in xu.corpora().items():
        out[name] = []
        for seed, kw in cases:
            data = synthutil.picture(seed, **kw)
            assert f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}" == GOLD["cases"][str(seed)]["stream_fnv"], f"seed {seed}: not the blessed stream"
            out[name].append((seed, kw, data, rr.Picture(pkg.capi.parse_hevc(data, record_order=xu.DECODE_ORDER))))
    assert GOLD["sweep_cases"] == xu.N_SWEEP == len(out["sweep"])
    return out


@pytest.fixture(scope="module")
def census(pictures):
    """the oracle's reconstruction-stage planes of every picture carry the reference's recorded fingerprint - they ARE the reference's planes -, the
    model reproduces every block of them, and the census is taken on the way"""
    C = xu.Census()
    C.wrap_seeds, C.classes = [], set()
    for name, lst in pictures.items():
        for seed, kw, data, P in lst:
            planes, _ = orc.oracle_decode(P.blob, 0, crop=True)
            assert xu.fingerprint(planes) == GOLD["cases"][str(seed)]["recon"], f"seed {seed} {kw}: the oracle's reconstruction is not the reference's"
            assert not P.flags & rr.PIC_SPLIT_CHAINS
            cls = xu.kernel_class(P)
            C.classes.add(cls)
            C.count_syntax(cls, P)
            before = sum(v for k, v in C.counts.items() if k[3] == ("ccp", "wrap"))
            bad = iu.first_mismatch(seed, P, planes, tools_note=C.noter(cls), pcm_bits=xu.pcm_bits(kw))
            assert bad is None, f"{kw}: the model is not the oracle (== the reference decoder): {bad}"
            if sum(v for k, v in C.counts.items() if k[3] == ("ccp", "wrap")) > before:
                C.wrap_seeds.append(seed)
    return C


def test_the_model_reproduces_the_reference_decoder_live(pictures):
    """every block of the live reference decoder's reconstruction stage (scalar build: Q10) == intra_ref + residual_ref from the reference's own neighbours,
    on every sixth picture; its three stages carry the recorded fingerprints (the default build from the deblocking stage on where the "pcmf" branch acts)"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    n = 0
    for name, lst in pictures.items():
        for seed, kw, data, P in lst[::LIVE_EVERY]:
            for stage, flags, bits in xu.STAGES:
                ref, _ = orc.ref_decode(data, flags | xu.ref_build(name, kw, bits))
                assert xu.fingerprint(ref) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}: not the recorded fingerprint"
                if bits == 0:
                    bad = iu.first_mismatch(seed, P, ref, pcm_bits=xu.pcm_bits(kw))
                    assert bad is None, f"{kw}: the model is not the reference decoder: {bad}"
                    n += P.n_tus
    assert n > 30000


def test_the_oracle_is_the_model_and_carries_the_fingerprints(pkg, census, pictures):
    """oracle == model block by block on the oracle's own reconstruction (the census fixture), and the oracle's deblocking and full stages carry the reference's
    fingerprints; the same for the four tiles of the full path"""
    for name, lst in pictures.items():
        for seed, kw, data, P in lst:
            for stage, _, bits in xu.STAGES[1:]:
                mine, _ = orc.oracle_decode(P.blob, bits, crop=True)
                assert xu.fingerprint(mine) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}"
    assert census.blocks > 200000
    for seed, kw in corpus.rext_residual_tiles():
        P = rr.Picture(pkg.capi.parse_hevc(synthutil.picture(seed, **kw), record_order=xu.DECODE_ORDER))
        for stage, _, bits in xu.STAGES:
            mine, _ = orc.oracle_decode(P.blob, bits, crop=True)
            assert xu.fingerprint(mine) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}"
            if bits == 0:
                bad = iu.first_mismatch(seed, P, mine, pcm_bits=xu.pcm_bits(kw))
                assert bad is None, f"{kw}: {bad}"


def test_where_the_default_build_differs_is_the_known_class():
    """the reference's default build reconstructs some pictures otherwise (recorded beside the fingerprints): every first differing block is an 8-bit 4x4
    transform-skip block (saturating 16-bit arithmetic), and none of them is a picture that is held to the default build"""
    rec = GOLD["simd_vs_scalar"]
    assert rec["cases_that_differ"] > 0 and set(rec["first_blocks_that_differ_by_class"]) == {"8-bit 4x4 transform skip"}
    kws = {seed: (name, kw) for name, lst in xu.corpora().items() for seed, kw in lst}
    assert not any(xu.default_build_holds(*kws[s]) for s in rec["seeds"] if s in kws)


def test_the_branches_are_reached(census):
    """Every (kernel class, luma / chroma, block size) holds blocks in every cell of the census that can occur (rextutil.required); the cells that cannot
    occur (rextutil.impossible, each with its reason) and those that the corpora leave out (rextutil.excluded: none) are zero.  Observability is a
    condition here, not a measurement: every record of these corpora is computed by the model."""
    print(census.table())
    assert census.blocks == census.observable
    assert census.classes == set(xu.CLASSES)
    missing = []
    for cls in xu.CLASSES:
        for kind in xu.KINDS:
            for nT in xu.SIZES:
                imp = xu.impossible(cls, kind, nT)
                if imp is None:
                    assert not any(k[:3] == (cls, kind, nT) for k in census.counts), (cls, kind, nT)
                    continue
                for cell, why in list(imp.items()) + list(xu.excluded(cls, kind, nT).items()):
                    assert census.seen(cls, kind, nT, cell) == 0, (cls, kind, nT, cell, why)
                missing += [(cls, kind, nT) + cell for cell in xu.required(cls, kind, nT) if not census.seen(cls, kind, nT, cell)]
    assert not missing, missing
    committed = os.path.join(HERE, "..", "profiles", "rext_residual_census.txt")
    assert open(committed).read() == census.table(), "profiles/rext_residual_census.txt is stale: tools/make_fixtures.py rext"


def test_quirk_switches(census, pictures):
    """shift_pair_int32 off (the shift pair in unbounded integers) is red on the first picture in which the pair wraps, on a block with a scale;
    res16 off changes nothing: what carries that for ALL pictures is the census cell ("res16", "acts") == 0 - the model with the switch on
    notes every int16 store that changes a value, and where none does the two settings compute the same numbers (rextutil.impossible gives
    the bound) -, asserted here again; the walk with the switch off over the first 40 8-bit pictures with transform skip is a demonstration
    of it, not the proof.  The switch documents the reference's code and no behaviour."""
    assert census.wrap_seeds, "no picture in which the shift pair wraps"
    by_seed = {seed: (kw, P) for lst in pictures.values() for seed, kw, data, P in lst}
    seed = census.wrap_seeds[0]
    kw, P = by_seed[seed]
    planes, _ = orc.oracle_decode(P.blob, 0, crop=True)
    bad = iu.first_mismatch(seed, P, planes, quirks=rr.Quirks(shift_pair_int32=False))
    print("shift_pair_int32 off:", bad)
    assert bad is not None and "scale" in bad and f"seed {seed} " in bad
    arm = 0
    for s, (kw, P) in list(by_seed.items()):
        if P.bit_depth != 8 or not kw.get("transform_skip", 1):
            continue
        planes, _ = orc.oracle_decode(P.blob, 0, crop=True)
        assert iu.first_mismatch(s, P, planes, quirks=rr.Quirks(res16=False)) is None, s
        arm += 1
        if arm == 40:
            break
    assert sum(v for k, v in census.counts.items() if k[3] == ("res16", "arm")) > 1000
    assert sum(v for k, v in census.counts.items() if k[3] == ("res16", "acts")) == 0
