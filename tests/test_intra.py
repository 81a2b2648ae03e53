"""CPU: intra sample prediction, branch by branch (corpus.intra_sweep, corpus.intra_single_ctb_cases).

  * tests/intra_ref.py - 8.4.4.2.1-8.4.4.2.6 in numpy, written from the standard - reproduces the live reference decoder's
    reconstruction stage on every observable block: one without a residual holds its prediction, one with a residual that
    residual_ref restates holds clip(prediction + residual);
  * the oracle against the reference decoder's scalar build plane for plane, and that build against its recorded
    fingerprints (tests/golden/intra.json);
  * the census: which branches of the prediction these streams reach, counted with intra_ref alone from the records and the
    reference decoder's planes.  The GPU tests (test_intra_gpu.py) run the same streams."""
import hashlib
import json
import os

import numpy as np
import pytest

import corpus
import hevcutil
import intra_ref as ir
import intrautil as iu
import orc
import residual_ref as rr
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "intra.json")))
N_SWEEP = len(GOLD["cases"])
STAGES = (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO, 0), ("deblock", orc.REF_F_NO_SAO, 1), ("full", 0, 3))
# sha256 over every stream that existed before the knobs `calm` and `mode_span`: all corpus.CASES, the first 16 cases of each earlier
# sweep, rext_large, extreme_sweep(144), the extreme tiles and the first large extreme picture - the digest of the parent commit's
# synthesiser, and the same with both knobs in place
STREAMS_BEFORE_CALM = "439cd0a6b5f619d907d29857dd1c36d068e00349efc87ed6d3b3b9727b11169a"
STREAMS_BEFORE_SAO_SPAN = "6103057603e7c4743e1536ad593c6fb68dd5085003eef6a937259337a63136f5"  # (taken at the commit before the knob)
STREAMS_BEFORE_LEVEL_SAT = "64663fc9c93d9b0e964b33425235dbfbee0226607bcc5d8ea09a90fcd5fdc6f2"  # (taken with the synthesiser of the commit before the knob)


def _fp(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype(np.uint8)
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


def test_new_knobs_leave_every_existing_stream_alone_and_act():
    h = hashlib.sha256()
    for name in sorted(corpus.CASES):
        h.update(corpus.stream(name))
    for sweep in (corpus.rare_syntax_sweep(16), corpus.structure_sweep(16), corpus.rext_sweep(16), corpus.single_ctb_cases(600)[:16],
                  corpus.rext_large(), corpus.extreme_sweep(144), corpus.extreme_tiles(), corpus.extreme_large()[:1]):
        for seed, kw in sweep:
            h.update(synthutil.picture(seed, **kw))
    assert h.hexdigest() == STREAMS_BEFORE_CALM
    assert synthutil.picture(5, width=64, height=64, calm=500) != synthutil.picture(5, width=64, height=64)
    assert synthutil.picture(5, width=64, height=64, mode_span=800) != synthutil.picture(5, width=64, height=64)
    # the knob sao_span (offsets and band positions at the ends of their ranges) came with the SAO corpora: the streams of the intra and deblocking corpora too
    h = hashlib.sha256()
    for sweep in (corpus.intra_sweep(16), corpus.intra_single_ctb_cases(16), corpus.intra_tiles(), corpus.deblock_sweep(320)[::8], corpus.deblock_single_edge_cases()[::10],
                  corpus.deblock_tiles()):
        for seed, kw in sweep:
            h.update(synthutil.picture(seed, **kw))
    assert h.hexdigest() == STREAMS_BEFORE_SAO_SPAN
    assert synthutil.picture(5, width=64, height=64, sao_span=500) != synthutil.picture(5, width=64, height=64)
    assert synthutil.picture(5, width=64, height=64, sao_span=500, sao=0) == synthutil.picture(5, width=64, height=64, sao=0)
    # the knob level_sat (whole blocks of saturated levels of one sign, for RDPCM run sums) came with the range-extension residual corpora: the streams of the SAO corpora too.
    # This pin covers the corpora that the two pins above do not; the three together are the guarantee that every earlier stream is byte-identical
    h = hashlib.sha256()
    for sweep in (corpus.sao_sweep(660)[::8], corpus.sao_small_cases()[::10], corpus.sao_tiles()):
        for seed, kw in sweep:
            h.update(synthutil.picture(seed, **kw))
    assert h.hexdigest() == STREAMS_BEFORE_LEVEL_SAT
    assert synthutil.picture(5, width=64, height=64, level_span=1000, level_sat=800) != synthutil.picture(5, width=64, height=64, level_span=1000)
    assert synthutil.picture(5, width=64, height=64, level_sat=800) != synthutil.picture(5, width=64, height=64)  # (full blocks without level_span too)


@pytest.fixture(scope="module")
def sweep(pkg):
    """[(seed, kw, stream, kernel class, Picture in decode order)] of the sweep"""
    out = []
    for seed, kw in corpus.intra_sweep(N_SWEEP):
        data = synthutil.picture(seed, **kw)
        split = bool(pkg.capi.stream_header(pkg.capi.parse_hevc(data))["flags"] & rr.PIC_SPLIT_CHAINS)
        P = rr.Picture(pkg.capi.parse_hevc(data, record_order=iu.DECODE_ORDER))
        out.append((seed, kw, data, iu.kernel_class(P.bit_depth, split), P))
    return out


@pytest.fixture(scope="module")
def census(sweep):
    """intra_ref against the live reference decoder on every observable block, and the census taken on the way"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    C = iu.Census()
    for seed, kw, data, cls, P in sweep:
        ref, _ = orc.ref_decode(data, STAGES[0][1] | orc.REF_F_SCALAR)
        bad = iu.first_mismatch(seed, P, ref, C.noter(cls))
        assert bad is None, f"{kw}: intra_ref is not the reference decoder: {bad}"
    return C


def test_intra_ref_reproduces_the_reference_decoder(census):
    """every observable block of every sweep picture; no skip list beyond "not observable\""""
    assert census.observable > 100000


def test_single_ctb_pictures_intra_ref_reproduces_the_reference_decoder(pkg):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    for seed, kw in corpus.intra_single_ctb_cases(288):
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(pkg.capi.parse_hevc(data, record_order=iu.DECODE_ORDER))
        assert P.n_ctbs == 1
        ref, _ = orc.ref_decode(data, STAGES[0][1] | orc.REF_F_SCALAR)
        bad = iu.first_mismatch(seed, P, ref)
        assert bad is None, f"{kw}: {bad}"
        mine, _ = orc.oracle_decode(P.blob, 0, crop=True)
        assert all(np.array_equal(a, b) for a, b in zip(mine, ref)), f"seed {seed} {kw}: the oracle's reconstruction"


def test_intra_tiles_oracle_and_intra_ref_against_the_reference_decoder(hm, pkg):
    """the 512 x 512 tiles of the forced cuts (GPU: against the oracle): the oracle == the reference decoder at the three stages, and
    intra_ref == the reference decoder on every observable block"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    for seed, kw in corpus.intra_tiles():
        data = synthutil.picture(seed, **kw)
        blob = hevcutil.parse(hm, data)
        for stage, rf, bits in STAGES:
            ref, _ = orc.ref_decode(data, rf)
            mine, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(mine) == len(ref) and all(np.array_equal(a, b) for a, b in zip(mine, ref)), f"seed {seed} {kw}: stage {stage}"
            if bits == 0:
                bad = iu.first_mismatch(seed, rr.Picture(pkg.capi.parse_hevc(data, record_order=iu.DECODE_ORDER)), ref)
                assert bad is None, f"{kw}: {bad}"


def test_intra_sweep_oracle_reference_and_fingerprints(hm, sweep):
    """oracle == the reference decoder's scalar build plane for plane at the three stages (live, where oracle/_ref is built), and
    == its recorded fingerprints; the streams are the blessed ones"""
    live = orc.have_ref()
    classes = set()
    for seed, kw, data, cls, _ in sweep:
        gold = GOLD["cases"][str(seed)]
        assert f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}" == gold["stream_fnv"], f"seed {seed}: not the blessed stream"
        blob = hevcutil.parse(hm, data)
        classes.add(cls)
        for stage, rf, bits in STAGES:
            mine, _ = orc.oracle_decode(blob, bits, crop=True)
            assert _fp(mine) == gold[stage], f"seed {seed} {kw}: stage {stage}"
            if live:
                ref, _ = orc.ref_decode(data, rf | orc.REF_F_SCALAR)
                assert len(mine) == len(ref)
                for c in range(len(ref)):
                    bad = np.argwhere(mine[c] != ref[c])
                    assert bad.size == 0, f"seed {seed} {kw}: stage {stage} plane {c}: {len(bad)} samples, first (y,x)={bad[0].tolist()}"
    assert classes == set(iu.CLASSES)


def test_where_the_default_build_differs_is_the_known_class():
    """the reference's SIMD build decodes some level_span pictures otherwise (recorded beside the fingerprints): every first
    differing block is a transform-skip block of a picture with level_span - saturating 16-bit arithmetic, DESIGN.md Q10"""
    rec = GOLD["simd_vs_scalar"]
    kw = dict(corpus.intra_sweep(N_SWEEP))
    assert all(kw[s]["level_span"] for s in rec["seeds"])
    assert all(k.startswith("level_span ") and k.endswith(": transform skip") and not k.startswith("level_span 0") for k in rec["first_blocks_that_differ_by_class"])


def test_the_branches_are_reached(census, sweep):
    """Every (kernel class, luma / chroma, block size) holds OBSERVABLE blocks in every cell of the census that can occur
    (intrautil.required).  The cells that cannot occur (intrautil.impossible, each with its reason) and those that the parser's
    or the sweep's choices exclude (intrautil.excluded) are zero over ALL blocks.  At least a third of all prediction blocks
    are observable.  The corner is never available without the whole left column and top row: the corner as a substitution
    source, and the order of TL and T in the fill of a missing left column, are dead branches.  A sum of the bilinear decision
    exactly at its limit or one below is reported, and required over the sweep as a whole (the `<` of the decision)."""
    print(census.table())
    assert 3 * census.observable >= census.blocks
    for _, _, _, _, P in sweep:
        for rec in P.records():
            nT = 1 << rec["log2"]
            assert not rec["avail_tl"] or (rec["avail_left"] == nT and rec["avail_top"] == nT), (rec["x"], rec["y"])
    missing = []
    for cls in iu.CLASSES:
        for kind in iu.KINDS:
            for nT in iu.SIZES:
                imp = iu.impossible(cls, kind, nT)
                if imp is None:
                    assert not any(k[:3] == (cls, kind, nT) for k in census.counts), (cls, kind, nT)
                    continue
                for cell, why in list(imp.items()) + list(iu.excluded(cls, kind, nT).items()):
                    assert census.counts.get((cls, kind, nT, cell), [0, 0])[0] == 0, (cls, kind, nT, cell, why)
                missing += [(cls, kind, nT) + cell for cell in iu.required(cls, kind, nT) if not census.seen(cls, kind, nT, cell)]
    print("at the limit of the bilinear decision:", {cls: census.seen(cls, "luma", 32, ("strong", "at_limit")) for cls in iu.CLASSES})
    assert sum(census.seen(cls, "luma", 32, ("strong", "at_limit")) for cls in iu.CLASSES) >= 1
    assert not missing, missing
