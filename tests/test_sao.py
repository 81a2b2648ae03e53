"""CPU: sample adaptive offset, sample by sample (corpus.sao_sweep, corpus.sao_small_cases, corpus.sao_tiles).

  * tests/sao_ref.py - 8.7.3 in numpy, written from the standard, every sample reading the input picture - applied to the live reference
    decoder's planes in front of SAO gives its planes behind SAO, every sample of every plane of every picture, at two stage pairs: deblocked
    input (stage 1 -> 3) and SAO alone on the sharper reconstruction (stage 0 -> 2).  The reference's scalar build for the Q9 class (8 bit,
    CTB 16, sub-sampled chroma), its default build for 8-bit pictures of the "pcmf" branch (input and output alike; corpus.SIMD_BUILD_ONLY
    tells why), no picture in both, and everywhere else both builds, which agree.  Pictures with a conformance window: the reference hands
    out the window alone, so its whole planes come from the twin stream without the window (saoutil.reference_whole);
  * the oracle (oracle/oracle_recon.c, which every GPU test trusts) against the same model on its own planes, and against the reference's
    recorded fingerprints (tests/golden/sao.json, written by tools/make_fixtures.py sao);
  * the census: which branches of SAO these streams reach, counted with sao_ref alone on the reference's planes
    (profiles/sao_census.txt).  The GPU tests (test_sao_gpu.py) run the same streams;
  * the model's quirk switches turned off are noticed by these streams."""
import json
import os

import numpy as np
import pytest

import corpus
import orc
import residual_ref as rr
import sao_ref as sr
import saoutil as su
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "sao.json")))
CENSUS_FILE = os.path.join(HERE, "..", "profiles", "sao_census.txt")
STAGE_PAIRS = ((1, 3), (0, 2))


def all_cases():
    """[(corpus name, seed, parameters)] of the three corpora"""
    return [("sweep", s, kw) for s, kw in corpus.sao_sweep(GOLD["sweep_cases"])] + [("small", s, kw) for s, kw in corpus.sao_small_cases()] + \
           [("tiles", s, kw) for s, kw in corpus.sao_tiles()]


@pytest.fixture(scope="module")
def pictures(pkg):
    """[(corpus name, seed, kw, stream, Picture in decode order)]"""
    out = []
    for name, seed, kw in all_cases():
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(pkg.capi.parse_hevc(data, record_order=su.DECODE_ORDER))
        assert P.bit_depth == kw.get("bit_depth", 8) and P.bit_depth_c == P.bit_depth
        assert f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}" == GOLD["cases"][str(seed)]["stream_fnv"], f"seed {seed}: not the blessed stream"
        out.append((name, seed, kw, data, P))
    return out


@pytest.fixture(scope="module")
def census(pictures):
    """sao_ref against the live reference decoder on every sample, and the census taken on the way"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    C = su.Census()
    for name, seed, kw, data, P in pictures:
        fps = su.hold_picture(seed, kw, data, P, C)
        assert all(fps[s] == GOLD["cases"][str(seed)][s] for s in "0123"), f"{name} seed {seed}: not the recorded fingerprints"
    return C


def test_the_corpora_cover_the_shapes_the_issue_names(pictures):
    """bit depth x chroma format x CTB size crossed; pictures of one CTB, of 2 x 2 CTBs, strips one CTB wide and one CTB high; no picture in both classes
    of the reference's builds (Q9: scalar build; 8-bit pcmf: default build); 8-bit pictures carry no transform skip (Q10)"""
    crossed = {(P.bit_depth, P.chroma_format, P.log2_ctb) for name, seed, kw, data, P in pictures if name == "sweep"}
    assert crossed == {(bd, cf, ctb) for bd in (8, 9, 10, 11, 12) for cf in (0, 1, 2, 3) for ctb in (4, 5, 6)}
    small = {(P.log2_ctb, P.ctb_w, P.ctb_h) for name, seed, kw, data, P in pictures if name == "small"}
    assert small == {(4, 1, 1), (4, 2, 2), (4, 1, 4), (4, 4, 1), (5, 1, 1), (5, 2, 2), (5, 1, 4), (5, 4, 1), (6, 1, 1), (6, 2, 2), (6, 1, 2), (6, 2, 1)}
    for name, seed, kw, data, P in pictures:
        assert not (corpus.sao_class_q9(kw) and corpus.sao_class_pcmf8(kw)), (seed, kw)
        assert corpus.sao_class_pcmf8(kw) == (P.bit_depth == 8 and bool(P.flags & rr.PIC_PCMF)), (seed, kw)
        assert P.bit_depth > 8 or kw["transform_skip"] == 0
        assert name != "sweep" or (64 <= P.width <= 128 and 64 <= P.height <= 96), (seed, P.width, P.height)
    windows = {(P.crop[0] % 8 == 0, (P.crop[0] // 2) % 8 == 0) for name, seed, kw, data, P in pictures if P.crop[0]}
    assert windows == {(True, True), (True, False), (False, False)}   # the left offset a multiple of 8 in luma and chroma, in luma alone, in neither


def test_sao_ref_reproduces_the_reference_decoder(census, pictures):
    """100 % of the samples of 100 % of the pictures, both stage pairs"""
    assert sum(census.pictures.values()) == 2 * len(pictures) and census.samples > 20000000
    assert {c for c, p in census.pictures} == set(su.CLASSES)


def test_the_oracle_equals_sao_ref_and_the_fingerprints(pictures):
    """oracle_recon.c behind SAO == sao_ref of its own planes in front of it (whole coded pictures, crop=False), both stage pairs, and the conformance
    window of every stage == the reference's recorded fingerprints"""
    for name, seed, kw, data, P in pictures:
        planes = {s: orc.oracle_decode(P.blob, s)[0] for s in range(4)}
        for s_in, s_out in STAGE_PAIRS:
            bad = su.first_mismatch(seed, P, data, planes[s_in], planes[s_out])
            assert bad is None, f"{name} {kw} stages {s_in} -> {s_out}: the oracle: {bad}"
        for s in range(4):
            assert su.fingerprint(su.crop(planes[s], P)) == GOLD["cases"][str(seed)][str(s)], f"{name} seed {seed} {kw}: stage {s}: not the reference's fingerprint"


def test_the_branches_are_reached(census):
    """Every (kernel class, luma / chroma, stage pair) holds samples in every cell that saoutil.required lists; the cells that cannot occur
    (saoutil.impossible, each with its reason) and those left out by choice (saoutil.excluded: none) are zero.  The table is the committed
    profiles/sao_census.txt."""
    table = census.table()
    print(table)
    missing = []
    for cls in su.CLASSES:
        for kind in su.KINDS:
            for pair in su.PAIRS:
                for cell, why in list(su.impossible(cls, kind, pair).items()) + list(su.excluded(cls, kind, pair).items()):
                    assert census.seen(cls, kind, pair, cell) == 0, (cls, kind, pair, cell, why)
                missing += [(cls, kind, pair) + cell for cell in su.required(cls, kind, pair) if not census.seen(cls, kind, pair, cell)]
    assert not missing, missing
    assert table == open(CENSUS_FILE).read(), "profiles/sao_census.txt is not this census: tools/make_fixtures.py sao writes it"


def _first_red(pictures, quirks, only=lambda P: True):
    for name, seed, kw, data, P in pictures:
        if name == "tiles" or not only(P):
            continue
        before, after = orc.oracle_decode(P.blob, 1)[0], orc.oracle_decode(P.blob, 3)[0]
        got, _ = sr.sao(before, P, data, quirks)
        if any(not np.array_equal(a, b) for a, b in zip(got, after)):
            return seed
    return None


def test_the_quirk_switches_matter(pictures):
    """each of the reference's three departures turned off (the standard's text) turns a picture red: Q13 one with several slices and sub-sampled
    chroma, the fast path one with several slices, the order by slice address one with tiles and slices"""
    sliced = lambda P: P.n_slices > 1
    assert _first_red(pictures, sr.Quirks(chroma_slice_lookup=False), only=lambda P: sliced(P) and P.chroma_format in (1, 2)) is not None
    assert _first_red(pictures, sr.Quirks(pps_fast_path=False), only=sliced) is not None
    assert _first_red(pictures, sr.Quirks(slice_order_by_address=False), only=lambda P: sliced(P) and bool(P.flags & rr.PIC_TILES)) is not None


def test_the_tile_structure_is_read_from_the_pps(pictures):
    """sao_ref's own reading of the PPS - uniform and explicit tile sizes - gives the tiles_enabled and loop_filter_across_tiles flags the parser reports, and
    as many tiles as the parameters ask for"""
    seen = set()
    for name, seed, kw, data, P in pictures:
        pps = sr.read_pps(data)
        assert bool(pps["tiles_enabled"]) == bool(P.flags & rr.PIC_TILES), seed
        if pps["tiles_enabled"]:
            assert bool(pps["lf_across_tiles"]) == bool(P.flags & rr.PIC_LF_ACROSS_TILES), seed
            T = sr.Tiles(pps, P.ctb_w, P.ctb_h)
            assert len(np.unique(T.tile_id)) == min(kw["tile_cols"], P.ctb_w) * min(kw["tile_rows"], P.ctb_h), seed
            seen.add((bool(pps["uniform"]), bool(pps["lf_across_tiles"])))
        assert bool(pps["lf_across_slices"]) == (not kw.get("pps_lf_across_slices_off", 0)), seed
    assert seen == {(u, l) for u in (False, True) for l in (False, True)}
