"""CPU: the arithmetic edges of the residual path - levels over the whole int16 range, QpY from -QpBdOffset to 51 with the
wrap of (8-283), scaling factors pinned at 1 and 255 (corpus.extreme_sweep, corpus.single_ctb_cases).

  * the oracle against the reference decoder's SCALAR build (live where oracle/_ref is built, and always against its
    recorded fingerprints, tests/golden/extreme.json);
  * the oracle against tests/residual_ref.py - int64 numpy written from the standard - on pictures of one CTB, where the
    residual of a block is observable as clip(1 << (bit_depth - 1) + residual);
  * the census: that these streams reach the edges, counted from the records with residual_ref alone.  The GPU tests
    (test_extreme_gpu.py) run the same streams: this is what keeps them from being hollow."""
import json
import os

import numpy as np
import pytest

import corpus
import extremeutil as eu
import hevcutil
import orc
import residual_ref as rr
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "extreme.json")))
N_SWEEP = len(GOLD["cases"])
STAGES = (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO, 0), ("deblock", orc.REF_F_NO_SAO, 1), ("full", 0, 3))


def _fp(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype(np.uint8)
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


def test_each_new_knob_changes_the_stream():
    """level_span / qp_span / scaling_span act.  (That 0 leaves every draw alone is not shown here: the bytes of every corpus stream
    are pinned by stream_fnv in tests/golden/synth.json - test_synth_corpus_matches_reference_fingerprints.)"""
    base = dict(width=64, height=64, scaling_list=2, qp=30)
    plain = synthutil.picture(5, **base)
    for knob in ("level_span", "qp_span", "scaling_span"):
        assert synthutil.picture(5, **{knob: 500 if knob != "qp_span" else 1}, **base) != plain, knob


def test_extreme_sweep_oracle_matches_reference_fingerprints(hm):
    """parser + oracle == the recorded pictures of the reference's scalar build, at the three stages"""
    for seed, kw in corpus.extreme_sweep(N_SWEEP):
        data = synthutil.picture(seed, **kw)
        gold = GOLD["cases"][str(seed)]
        assert f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}" == gold["stream_fnv"], f"seed {seed}: not the blessed stream"
        blob = hevcutil.parse(hm, data)
        for stage, _, bits in STAGES:
            planes, _ = orc.oracle_decode(blob, bits, crop=True)
            assert _fp(planes) == gold[stage], f"seed {seed} {kw}: stage {stage}"


def test_extreme_sweep_oracle_matches_reference_scalar_build_live(hm):
    """... and plane for plane against the decoder itself (needs oracle/_ref)"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    orders = set()
    for seed, kw in corpus.extreme_sweep(N_SWEEP):
        data = synthutil.picture(seed, **kw)
        blob = hevcutil.parse(hm, data)
        orders.add(bool(int.from_bytes(blob[36:40], "little") & 0x1000))
        for stage, rf, bits in STAGES:
            ref, _ = orc.ref_decode(data, rf | orc.REF_F_SCALAR)
            mine, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(mine) == len(ref)
            for c in range(len(ref)):
                bad = np.argwhere(mine[c] != ref[c])
                assert bad.size == 0, f"seed {seed} {kw}: stage {stage} plane {c}: {len(bad)} samples, first (y,x)={bad[0].tolist()}"
    assert orders == {False, True}  # both record orders: k_residual + k_chain and k_recon see such pictures
    # the 8-bit cases whose draws hold transquant bypass / unfiltered PCM, WITH them: at the reconstruction stage, where the
    # "pcmf" deblocking branch (in which the reference's builds disagree) does not enter
    pcmf = corpus.extreme_sweep(N_SWEEP, pcmf_8bit=True)
    assert len(pcmf) == 9
    for seed, kw in pcmf:
        data = synthutil.picture(seed, **kw)
        ref, _ = orc.ref_decode(data, STAGES[0][1] | orc.REF_F_SCALAR)
        mine, _ = orc.oracle_decode(hevcutil.parse(hm, data), 0, crop=True)
        assert len(mine) == len(ref) and all(np.array_equal(a, b) for a, b in zip(mine, ref)), f"seed {seed} {kw}: reconstruction stage"


@pytest.fixture(scope="module")
def single_ctb(pkg):
    return eu.single_ctb_pictures(pkg.capi)


def test_single_ctb_oracle_equals_residual_ref(pkg, single_ctb):
    """the first block of every component of a one-CTB picture: the oracle's stage-0 samples == clip(mid + residual_ref), in
    both record orders"""
    pics, _ = single_ctb
    assert len(pics) == 5 * (eu.N_PER_SHAPE + eu.N_WRAP_PER_SHAPE)
    split = 0
    for seed, kw, data, firsts in pics:
        # decode order for all; and the parser's own choice, which is split chains for every picture without rare syntax
        for order in (eu.DECODE_ORDER, 0):
            blob = pkg.capi.parse_hevc(data, record_order=order)
            is_split = bool(pkg.capi.stream_header(blob)["flags"] & 0x1000)
            assert not (is_split and order == eu.DECODE_ORDER)
            split += is_split
            planes, _ = orc.oracle_decode(blob, 0)
            bad = eu.first_mismatch(planes, firsts)
            assert bad is None, f"seed {seed} {kw} record order {order}: {bad}"
    assert split > 800, split  # (measured: 1036 of the 3300 pictures go out as split chains)


def test_saturation_does_not_hide_the_residual(single_ctb):
    """a residual far beyond the sample range saturates the block and would hide an error: of the samples the single-CTB tests
    compare, at least a quarter lie strictly between 0 and the maximum, and for every bit depth and block size at least one
    unit with a clipped coefficient or a wrapped product still holds such samples.  (Measured with the levels as tuned in
    corpus.single_ctb_cases: 71 % of the samples.)"""
    _, census = single_ctb
    share = census["samples_in_range"] / census["samples"]
    print(f"in range: {census['samples_in_range']} of {census['samples']} samples ({share:.3f})")
    assert share >= 0.25
    for bd in (8, 10, 12):
        for log2 in (2, 3, 4, 5):
            print(bd, log2, census[(bd, log2, "edge_and_in_range")])
            assert census[(bd, log2, "edge_and_in_range")] >= 1, (bd, log2)


def test_the_edges_are_reached(pkg, single_ctb):
    """Every bit depth and block size holds units of each kind - counted from the records with residual_ref alone, over the
    single-CTB pictures (whose residuals are observable) and the sweep:
      a dequantised coefficient clipped at +32767, one at -32768; a clipped stage-1 value; a DC-only block with a clipped
      coefficient; for 16x16 / 32x32 blocks one with levels in the top-left 4x4 only and one with a level in the last group
      of four rows and of four columns; a flat product that wraps int32 - at 12 bit.
    Two kinds cannot exist, by arithmetic, and are asserted so instead:
      * a wrapping flat product at 8 / 10 bit: |level| <= 32768, levelScale << (qP / 6) <= 57 << 8 at qP <= 51 resp. 57 << 10
        at qP <= 63, offset <= 2^9: 32768 * 58368 + 512 < 2^31.  At 12 bit (qP <= 75: 57 << 12) it wraps.
      * a DST block whose stage-2 clip acts (Q4): |stage 2| <= 242 * 32768 >> 8 < 32767 up to 12 bit (residual_ref asserts it
        for every DST unit it computes).  What Q4 leaves observable is the DCT's UNclipped second stage beyond int16: reached
        at 12 bit in 16x16 and 32x32 blocks.
    And over the sweep: QpY = -QpBdOffset, QpY = 51, and the QP derivation wrapping in each direction."""
    _, single = single_ctb
    sweep, qp = eu.sweep_census(pkg.capi, corpus.extreme_sweep(N_SWEEP))
    total = single + sweep
    for bd in (8, 10, 12):
        for log2 in (2, 3, 4, 5):
            row = {k: total[(bd, log2, k)] for k in ("wrap", "clip_hi", "clip_lo", "stage1_clip", "dc_only_clipped", "top_left_only", "last_group",
                                                     "stage2_beyond_int16", "dst", "dct", "tskip", "bypass")}
            print(bd, log2, row, "of them observable (single CTB):", {k: single[(bd, log2, k)] for k in ("wrap", "clip_hi", "clip_lo", "stage1_clip", "dc_only_clipped")})
            for k in ("clip_hi", "clip_lo", "stage1_clip", "dc_only_clipped"):
                assert single[(bd, log2, k)] >= 1, (bd, log2, k)  # (each of them where the residual is observable)
            if log2 >= 4:
                assert row["top_left_only"] >= 1 and row["last_group"] >= 1, (bd, log2)
            assert (row["wrap"] >= 1) == (bd == 12), (bd, log2, row["wrap"])
            if bd == 12:  # ... and where the residual is observable, in a block that still holds samples inside the range
                assert single[(bd, log2, "wrap")] >= 1 and single[(bd, log2, "wrap_and_in_range")] >= 1, (bd, log2)
            assert row["dct"] >= 1 and row["tskip"] >= 1 and (log2 != 2 or row["dst"] >= 1)
        max_scale = max(rr.LEVEL_SCALE[q % 6] << (q // 6) for q in range(52 + 6 * (bd - 8)))
        assert (32768 * max_scale + (1 << 9) < 1 << 31) == (bd < 12)
    assert total[(12, 4, "stage2_beyond_int16")] >= 1 and total[(12, 5, "stage2_beyond_int16")] >= 1
    assert int(np.abs(rr.DST).sum(axis=0).max()) * 32768 + 128 >> 8 < 32767
    assert all(qp.values()), qp
