"""CPU: the deblocking filter, decision by decision (corpus.deblock_sweep, corpus.deblock_single_edge_cases, corpus.deblock_tiles).

  * tests/deblock_ref.py - 8.7.2 in numpy, written from the standard, all vertical edges of a plane and then all horizontal ones -
    applied to the live reference decoder's reconstruction-stage planes gives its deblocking-stage planes, every sample of every
    plane of every picture: the scalar build for pictures outside the "pcmf" branch (and its default build agrees with it there),
    the default build for 8-bit pictures inside it (corpus.SIMD_BUILD_ONLY tells why);
  * the oracle (oracle/oracle_recon.c, which every GPU test trusts) against the same model on its own planes, and against the
    reference's recorded fingerprints (tests/golden/deblock.json, written by tools/make_fixtures.py deblock);
  * the census: which decisions of the filter these streams reach, counted with deblock_ref alone on the reference's planes
    (profiles/deblock_census.txt).  The GPU tests (test_deblock_gpu.py) run the same streams;
  * the model's quirk switches turned off are noticed by these streams."""
import json
import os

import numpy as np
import pytest

import corpus
import deblock_ref as dr
import deblockutil as du
import orc
import residual_ref as rr
import synthutil

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "deblock.json")))
CENSUS_FILE = os.path.join(HERE, "..", "profiles", "deblock_census.txt")
NO_FILTERS, NO_SAO = orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO, orc.REF_F_NO_SAO


def _fp(planes):
    h = 0
    for p in planes:
        a = np.ascontiguousarray(p if p.max() > 255 else p.astype(np.uint8))
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


def all_cases():
    """[(corpus name, seed, parameters)] of the three corpora"""
    return [("sweep", s, kw) for s, kw in corpus.deblock_sweep(GOLD["sweep_cases"])] + [("edge", s, kw) for s, kw in corpus.deblock_single_edge_cases()] + \
           [("tiles", s, kw) for s, kw in corpus.deblock_tiles()]


@pytest.fixture(scope="module")
def pictures(pkg):
    """[(corpus name, seed, kw, stream, kernel class, Picture in decode order, takes the 8-bit "pcmf" branch)]"""
    out = []
    for name, seed, kw in all_cases():
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(pkg.capi.parse_hevc(data, record_order=du.DECODE_ORDER))
        assert P.bit_depth == kw.get("bit_depth", 8) and P.bit_depth_c == P.bit_depth  # (9 and 11 bit: synthesiser and parser take them)
        out.append((name, seed, kw, data, du.kernel_class(P.flags, P.bit_depth), P, P.bit_depth == 8 and bool(P.flags & rr.PIC_PCMF)))
    return out


@pytest.fixture(scope="module")
def census(pictures):
    """deblock_ref against the live reference decoder on every sample, and the census taken on the way"""
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    C = du.Census()
    C.shapes = {}
    C.corner_windows = 0
    for name, seed, kw, data, cls, P, pcmf8 in pictures:
        build = 0 if pcmf8 else orc.REF_F_SCALAR
        before, _ = orc.ref_decode(data, NO_FILTERS | build)
        after, _ = orc.ref_decode(data, NO_SAO | build)
        single = du.Census()
        bad = du.first_mismatch(seed, P, before, after, du.quirks_for(default_build=pcmf8), lambda ev: (C.noter(cls, P)(ev), single.noter(cls, P)(ev)))
        assert bad is None, f"{name} {kw}: deblock_ref is not the reference decoder: {bad}"
        assert _fp(before) == GOLD["cases"][str(seed)]["recon"] and _fp(after) == GOLD["cases"][str(seed)]["deblock"], f"{name} seed {seed}: not the recorded fingerprints"
        # the other build: the same planes outside the pcmf branch; inside it (8 bit) the same reconstruction
        other0, _ = orc.ref_decode(data, NO_FILTERS | (orc.REF_F_SCALAR if pcmf8 else 0))
        assert all(np.array_equal(a, b) for a, b in zip(other0, before)), f"{name} seed {seed} {kw}: the reference's builds reconstruct differently"
        if not pcmf8:
            other1, _ = orc.ref_decode(data, NO_SAO)
            assert all(np.array_equal(a, b) for a, b in zip(other1, after)), f"{name} seed {seed} {kw}: the reference's builds deblock differently"
        if name == "edge":
            C.shapes.setdefault((P.width, P.height), du.Census()).counts.update(single.counts)
            if (P.width, P.height) == (16, 16):
                # the four corner windows of filters.hip (half windows in both directions: 4 x 4 luma samples each) hold no unit: untouched
                for ys in (slice(0, 4), slice(12, 16)):
                    for xs in (slice(0, 4), slice(12, 16)):
                        assert np.array_equal(after[0][ys, xs], before[0][ys, xs]), f"seed {seed} {kw}: the reference changed a corner window"
                        C.corner_windows += 1
    return C


def test_deblock_ref_reproduces_the_reference_decoder(census, pictures):
    """100 % of the samples of 100 % of the pictures; both builds of the reference agree wherever the picture is outside the pcmf branch"""
    assert sum(census.pictures.values()) == len(pictures) and census.units > 500000
    assert set(census.pictures) == set(du.CLASSES)


def test_the_oracle_equals_deblock_ref_and_the_fingerprints(pictures):
    """oracle_recon.c at the deblocking stage == deblock_ref of its own reconstruction-stage planes (the product follows the reference's
    default build: "simd"), and both stages == the reference's recorded fingerprints; the streams are the blessed ones"""
    for name, seed, kw, data, cls, P, pcmf8 in pictures:
        gold = GOLD["cases"][str(seed)]
        assert f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}" == gold["stream_fnv"], f"seed {seed}: not the blessed stream"
        before, _ = orc.oracle_decode(P.blob, 0, crop=True)
        after, _ = orc.oracle_decode(P.blob, 1, crop=True)
        bad = du.first_mismatch(seed, P, before, after, du.quirks_for(default_build=True))
        assert bad is None, f"{name} {kw}: the oracle: {bad}"
        assert _fp(before) == gold["recon"] and _fp(after) == gold["deblock"], f"{name} seed {seed} {kw}: not the reference's fingerprints"


def test_the_decisions_are_reached(census):
    """Every (kernel class, luma / chroma, direction) holds units in every cell that deblockutil.required lists; the cells that cannot occur
    (deblockutil.impossible, each with its reason) and those left out by choice (deblockutil.excluded) are zero.  The table is the committed
    profiles/deblock_census.txt."""
    table = census.table()
    print(table)
    missing = []
    for cls in du.CLASSES:
        for kind in du.KINDS:
            for d in du.DIRS:
                for cell, why in list(du.impossible(cls, kind, d).items()) + list(du.excluded(cls, kind, d).items()):
                    assert census.seen(cls, kind, d, cell) == 0, (cls, kind, d, cell, why)
                missing += [(cls, kind, d) + cell for cell in du.required(cls, kind, d) if not census.seen(cls, kind, d, cell)]
    assert not missing, missing
    assert table == open(CENSUS_FILE).read(), "profiles/deblock_census.txt is not this census: tools/make_fixtures.py deblock writes it"


def test_one_edge_pictures_hold_each_kind_of_window(census):
    """16x8: one vertical luma edge, its two units in a top and in a bottom half window, no horizontal edge.  8x16: the same turned.  16x16:
    the interior window with the crossing, where the horizontal edge reads what the vertical one wrote, all four half windows, and the four
    corner windows (half windows in both directions), which hold no unit - a unit writes three samples on either side of its edge, the corner
    samples lie five and more from it - and come back untouched: the census fixture has looked at each of them, and the GPU tests compare
    whole planes."""
    S = census.shapes
    assert set(S) == {(16, 8), (8, 16), (16, 16)}

    def kinds(shape, d):
        return {cell[1] for (cls, kind, dd, cell), n in S[shape].counts.items() if kind == "luma" and dd == d and cell[0] == "window" and n}

    def units(shape, d, bs):
        return sum(n for (cls, kind, dd, cell), n in S[shape].counts.items() if kind == "luma" and dd == d and cell == ("bS", bs))
    n = len(corpus.deblock_single_edge_cases()) // 3
    assert kinds((16, 8), "V") == {"first_half", "second_half"} and kinds((16, 8), "H") == set()
    assert kinds((8, 16), "H") == {"first_half", "second_half"} and kinds((8, 16), "V") == set()
    assert kinds((16, 16), "V") == kinds((16, 16), "H") == {"first_half", "second_half", "interior"}
    assert units((16, 8), "V", 2) == 2 * n and units((8, 16), "H", 2) == 2 * n      # exactly one edge of two units in every such picture
    assert units((16, 8), "H", 2) == units((8, 16), "V", 2) == 0
    assert any(cell == ("crossing",) and n for (cls, kind, dd, cell), n in S[(16, 16)].counts.items())
    assert census.corner_windows == 4 * n


def _first_red(pictures, quirks, only=lambda P: True):
    for name, seed, kw, data, cls, P, pcmf8 in pictures:
        if name == "tiles" or not only(P):
            continue
        before, _ = orc.oracle_decode(P.blob, 0, crop=True)
        after, _ = orc.oracle_decode(P.blob, 1, crop=True)
        got, _ = dr.deblock(before, P, quirks)
        if any(not np.array_equal(a, b) for a, b in zip(got, after)):
            return seed
    return None


def test_the_quirk_switches_matter(pictures):
    """pcmf_luma and vchroma_p_for_both turned off (the standard's text) go red on pictures with PCM / bypass units; segment_params cannot be
    observed (deblock_ref's text, and the census cell segment_differs)"""
    pcmf = lambda P: bool(P.flags & rr.PIC_PCMF)
    assert _first_red(pictures, dr.Quirks(pcmf_luma="off"), only=pcmf) is not None
    assert _first_red(pictures, dr.Quirks(pcmf_luma="scalar"), only=lambda P: pcmf(P) and P.bit_depth == 8) is not None
    assert _first_red(pictures, dr.Quirks(vchroma_p_for_both=False), only=pcmf) is not None
    assert _first_red(pictures, dr.Quirks(segment_params=False)) is None
