"""GPU parity of the HEVC-intra path: HIP reconstruction / deblocking / SAO (through the C ABI)
vs the oracle's scalar executors on the same command streams, stage by stage, and - where the
real reference decoder (oracle/_ref) is present - vs libde265 itself.  Bit-exact."""
import glob
import os

import numpy as np
import pytest

import gpudecode
import orc

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def _streams():
    return sorted(glob.glob(os.path.join(DATA, "*.hevc")))


@pytest.mark.parametrize("path", _streams(), ids=lambda p: os.path.basename(p))
@pytest.mark.parametrize("stages", [0, 1, 3])
def test_stages_match_oracle(pkg, path, stages):
    data = open(path, "rb").read()
    blob = pkg.capi.parse_hevc(data, annexb=False)
    exp, _ = orc.oracle_decode(blob, stages, crop=True)
    got = gpudecode.decode_pictures(pkg, [blob], stages)[0]
    for c in range(3):
        bad = np.argwhere(got[c] != exp[c])
        assert bad.size == 0, f"plane {c}: {len(bad)} mismatches, first at (y,x)={bad[0].tolist()} got {got[c][tuple(bad[0])]} exp {exp[c][tuple(bad[0])]}"


@pytest.mark.parametrize("path", _streams(), ids=lambda p: os.path.basename(p))
def test_matches_reference_decoder(pkg, path):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (reference sources absent)")
    data = open(path, "rb").read()
    ref, _ = orc.ref_decode(data, 0)
    got = gpudecode.decode_pictures(pkg, [pkg.capi.parse_hevc(data)], 3)[0]
    for c in range(3):
        np.testing.assert_array_equal(got[c], ref[c])


import corpus  # noqa: E402
import json  # noqa: E402

SYNTH = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth.json")))


def _fp(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype(np.uint8)
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


@pytest.mark.parametrize("name", sorted(corpus.CASES))
def test_synth_corpus(pkg, name):
    """every corpus case: HIP == oracle at every stage, and == the reference decoder's fingerprints"""
    blob = pkg.capi.parse_hevc(corpus.stream(name))
    for stage, bits in (("recon", 0), ("deblock", 1), ("full", 3)):
        got = gpudecode.decode_pictures(pkg, [blob], bits)[0]
        exp, _ = orc.oracle_decode(blob, bits, crop=True)
        assert len(got) == len(exp)  # one plane for monochrome pictures
        for c in range(len(exp)):
            bad = np.argwhere(got[c] != exp[c])
            assert bad.size == 0, f"{name} {stage} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"
        assert _fp(got) == SYNTH[name][stage]


def test_whole_corpus_in_one_batch(pkg):
    names = sorted(corpus.CASES)
    blobs = [pkg.capi.parse_hevc(corpus.stream(n)) for n in names]
    got = gpudecode.decode_pictures(pkg, blobs, 3)
    for n, g in zip(names, got):
        assert _fp(g) == SYNTH[n]["full"], n


def test_batch_of_mixed_pictures(pkg):
    """several pictures (different sizes / CTB sizes) in one batch = independent workgroups"""
    paths = _streams()
    if len(paths) < 2:
        pytest.skip("needs at least two fixture streams")
    blobs = [pkg.capi.parse_hevc(open(p, "rb").read()) for p in paths]
    got = gpudecode.decode_pictures(pkg, blobs, 3)
    for blob, g in zip(blobs, got):
        exp, _ = orc.oracle_decode(blob, 3, crop=True)
        for c in range(3):
            np.testing.assert_array_equal(g[c], exp[c])


def test_rare_syntax_sweep(pkg):
    """PCM / transquant-bypass / scaling-list streams in one batch (rare-syntax kernel variants next to the common ones):
    HIP == oracle at every stage"""
    import synthutil
    cases = corpus.rare_syntax_sweep(48) + [(9000 + i, dict(width=64, height=64)) for i in range(4)]  # + ordinary pictures
    blobs = [pkg.capi.parse_hevc(synthutil.picture(seed, **kw)) for seed, kw in cases]
    for bits in (0, 1, 3):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), blob, g in zip(cases, blobs, got):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"


def test_structure_sweep(pkg):
    """several slices, dependent slice segments, tiles, WPP, loop filters stopped at slice / tile borders, conformance
    windows - in one batch next to ordinary pictures: HIP == oracle at every stage"""
    import synthutil
    cases = corpus.structure_sweep(64)
    blobs = [pkg.capi.parse_hevc(synthutil.picture(seed, **kw)) for seed, kw in cases]
    for bits in (0, 1, 3):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), blob, g in zip(cases, blobs, got):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"


def test_range_extension_sweep(pkg):
    """range-extension tools (transform-skip rotation / context / block sizes up to 32x32, implicit RDPCM, intra smoothing
    off, persistent Rice adaptation, CU chroma QP offsets, cross-component prediction, SAO offset scaling) in one batch:
    HIP == oracle at every stage.  The oracle equals the reference decoder on the same sweep (test_oracle_decode.py)."""
    import synthutil
    cases = corpus.rext_sweep(120)
    blobs = [pkg.capi.parse_hevc(synthutil.picture(seed, **kw)) for seed, kw in cases]
    for bits in (0, 1, 3):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), blob, g in zip(cases, blobs, got):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"


def test_range_extension_large_blocks(pkg):
    """the same tools on larger pictures with 32x32 transform-skip / bypass blocks and CTB 64 (RDPCM runs of 32 samples,
    cross-component prediction of 32x32 blocks through the workgroup's shared staging)"""
    import synthutil
    cases = corpus.rext_large()
    blobs = [pkg.capi.parse_hevc(synthutil.picture(seed, **kw)) for seed, kw in cases]
    for bits in (0, 3):
        got = gpudecode.decode_pictures(pkg, blobs, bits)
        for (seed, kw), blob, g in zip(cases, blobs, got):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            for c in range(len(exp)):
                bad = np.argwhere(g[c] != exp[c])
                assert bad.size == 0, f"seed {seed} {kw} stages {bits} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"


@pytest.mark.parametrize("shape", [dict(log2_ctb=5), dict(log2_ctb=6), dict(log2_ctb=5, bit_depth=10), dict(log2_ctb=6, bit_depth=12, chroma_format=2),
                                   dict(log2_ctb=4), dict(log2_ctb=5, chroma_format=0)],
                         ids=["8bit_ctb32", "8bit_ctb64", "10bit_ctb32", "12bit_422_ctb64", "8bit_ctb16", "mono_ctb32"])
@pytest.mark.parametrize("density, qp", [(97, 4), (80, 22), (30, 40)], ids=["dense_qp4", "qp22", "sparse_qp40"])
def test_large_transform_blocks(pkg, shape, density, qp):
    """16x16 / 32x32 transform blocks wherever the quadtree allows them (no_split), from a few levels in the top-left corner to levels
    in every group of four rows and columns: the residual pre-pass's large-block path (k_residual: big_residual - both stages over
    the groups of four inputs that hold a level, fallback-dct.cc:592-733; DC-only blocks; levels beyond the staged ones, read from
    memory inside a pass) at every bit depth's shifts, against the oracle and - where it is there - the real libde265"""
    import synthutil
    data = synthutil.picture(515151 + density, width=320, height=192, qp=qp, density=density, no_split=1, cu_qp_delta=1, transform_skip=0, **shape)
    blob = pkg.capi.parse_hevc(data)
    assert int.from_bytes(blob[36:40], "little") & 0x1000  # split chains: k_residual + k_chain
    got = gpudecode.decode_pictures(pkg, [blob], 3)[0]
    exp, _ = orc.oracle_decode(blob, 3, crop=True)
    for c in range(len(exp)):
        bad = np.argwhere(got[c] != exp[c])
        assert bad.size == 0, f"{shape} density {density} qp {qp} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"
    if orc.have_ref():
        # (8-bit CTB 16: the reference's AVX2 SAO filters 8 columns too many of 8-sample-wide chroma CTBs, its SSE4 and scalar code do
        #  not - quirk Q9, DESIGN.md 3: the scalar build is the one to meet there)
        ref, _ = orc.ref_decode(data, orc.REF_F_SCALAR if shape.get("log2_ctb") == 4 and shape.get("bit_depth", 8) == 8 else 0)
        for c in range(len(ref)):
            assert np.array_equal(got[c], ref[c]), f"{shape} density {density} qp {qp} plane {c} differs from the reference decoder"


@pytest.mark.parametrize("shape", [dict(width=2304, height=1296, log2_ctb=5), dict(width=1920, height=1080, log2_ctb=4),
                                   dict(width=1600, height=1200, log2_ctb=6, bit_depth=10), dict(width=2048, height=1152, log2_ctb=5, chroma_format=2, bit_depth=10),
                                   dict(width=1536, height=1024, log2_ctb=6, chroma_format=0),
                                   # one 16x16 transform block per CTB: 64 CTBs start inside one 64-record chunk of the residual pre-pass
                                   dict(width=2048, height=512, log2_ctb=4, no_split=1)],
                         ids=["8bit_ctb32", "8bit_ctb16", "10bit_ctb64", "10bit_422_ctb32", "mono_ctb64", "8bit_ctb16_one_block_per_ctb"])
def test_large_single_pictures(pkg, shape):
    """large single pictures of every class through the split chains (k_residual + k_chain), with as many waves per picture as the wavefront,
    the LDS and the machine allow - 3, 5, 6, 7 as well as powers of two (sample lines are handed from wave to wave through
    LDS slots row % (rows in flight)): HIP == oracle"""
    import synthutil
    blob = pkg.capi.parse_hevc(synthutil.picture(424242, qp=30, density=40, **shape))
    assert int.from_bytes(blob[36:40], "little") & 0x1000  # split chains
    got = gpudecode.decode_pictures(pkg, [blob, blob], 3)
    exp, _ = orc.oracle_decode(blob, 3, crop=True)
    for g in got:
        for c in range(len(exp)):
            bad = np.argwhere(g[c] != exp[c])
            assert bad.size == 0, f"{shape} plane {c}: {len(bad)} mismatches, first (y,x)={bad[0].tolist()}"


def test_corrupted_but_parsable_streams(pkg, hm):
    """differential check on wild syntax: bit flips in the slice data of streams of every kernel class; whatever the
    parser still accepts (the entropy decoder re-synchronises on other - extreme - modes, levels and QPs) must come out of
    the HIP kernels exactly as out of the oracle, at the reconstruction stage and after the filters.  (tools/fuzz_gpu.py
    runs the same with thousands of streams; tools/fuzz_ref.py compares parser + oracle with the reference decoder.)"""
    import random
    import hevcutil
    rng = random.Random(20260)
    blobs, tags = [], []
    for name in ("ragged", "ctb64_wpp", "hi422_10", "ctb16_nosao", "pcm_bypass_sl_wpp", "yuv444_rare", "rext_cross_444_all", "rext_ts_bypass_422_10",
                 "slices_headers", "tiles_3x2_nolf", "dense_lowqp", "sl_sps_12bit_highqp"):
        data = corpus.stream(name)
        got = tries = 0
        while got < 8 and tries < 600:
            tries += 1
            b = bytearray(data)
            for _ in range(rng.randrange(1, 4)):
                b[rng.randrange(len(b) // 3, len(b))] ^= 1 << rng.randrange(8)
            try:
                blobs.append(hevcutil.parse(hm, bytes(b)))
            except RuntimeError:
                continue
            tags.append((name, tries))
            got += 1
    assert len(blobs) > 60
    for bits in (0, 3):
        out = gpudecode.decode_pictures(pkg, blobs, bits)
        for tag, blob, g in zip(tags, blobs, out):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            for c in range(len(exp)):
                assert np.array_equal(g[c], exp[c]), f"{tag} stages {bits} plane {c}"


# ---- k_recon: the kernel of a picture in decode order (chain_mode_check.py in a process of its own: the launcher's choices on stderr,
# the waves per picture forced through the test library's knobs)

import re  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

RARE_SYNTAX = 0x100 | 0x200 | 0x400 | 0x800 | 0x2000 | 0x4000 | 0x8000 | 0x10000 | 0x20000  # HM_PIC_RARE_SYNTAX (hm_stream.h)
HERE = os.path.dirname(os.path.abspath(__file__))


def _check(env_extra, *names, timeout=600):
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), HERE, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(HERE, "chain_mode_check.py"), *names], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr[-4000:]
    return r.stderr


def _recon_launches(stderr):
    """[k_recon] lines -> [(pictures, CTB size, bytes per sample, waves per picture, rare syntax)]"""
    out = []
    for m in re.finditer(r"^\[k_recon\] (\d+) pictures of CTB (\d+), (\d)-byte samples, (\d+) waves per picture(, rare syntax)?$", stderr, re.M):
        out.append((int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5] is not None))
    return out


def test_decode_order_records_of_ordinary_pictures(pkg):
    """HM_RECORDS_DECODE_ORDER (a public parse option): an ordinary picture parsed so is a class without rare syntax and without split chains
    (batch.cpp) - k_recon<Pix, L2, false>, which nothing else launches.  Every non-rare corpus case and the structure sweep, at stages 0 / 1 / 3:
    the oracle's pictures and the reference decoder's fingerprints; between them all six instantiations ran (8 / 16-bit samples x CTB 16 / 32 / 64),
    and neither k_residual nor k_chain."""
    names = [n for n in sorted(corpus.CASES) if not pkg.capi.stream_header(pkg.capi.parse_hevc(corpus.stream(n)))["flags"] & RARE_SYNTAX]
    assert len(names) > 40
    err = _check({"HM_CHECK_ORDER": "2", "HM_CHECK_STAGES": "0,1,3", "HM_CHECK_COPIES": "1", "HM_CHAIN_DEBUG": "1"}, *names, "structure_sweep")
    assert "[k_chain]" not in err and "[k_residual]" not in err, err[-3000:]
    plain = {(ctb, bps) for _, ctb, bps, _, rare in _recon_launches(err) if not rare}
    assert plain == {(ctb, bps) for ctb in (16, 32, 64) for bps in (1, 2)}, plain


def test_waves_per_picture_of_k_recon():
    """k_recon with 1, 2, 3, 4, 8 waves per picture (forced: knob recon_waves) on the rare-syntax sweep and the rare-syntax 512 x 512 tiles"""
    cuts = [{"recon_waves": w} for w in (1, 2, 3, 4, 8)]
    err = _check({"HM_CHECK_CUTS": json.dumps(cuts), "HM_CHECK_STAGES": "0,3", "HM_CHAIN_DEBUG": "1"}, "rare_sweep", "rare512")
    parts = err.split("[check] cut ")[1:]
    assert len(parts) == len(cuts)
    for c, part in zip(cuts, parts):
        launches = _recon_launches(part)
        assert launches and all(rare for *_, rare in launches), part[-2000:]
        waves = [nw for _, _, _, nw, _ in launches]
        assert max(waves) <= c["recon_waves"], (c, waves)  # (fewer where a picture has fewer useful waves or the LDS holds fewer)
        if c["recon_waves"] <= 4:
            assert c["recon_waves"] in waves, (c, waves)


@pytest.mark.parametrize("copies", [300, 1100])
def test_many_pictures_with_rare_syntax(copies):
    """k_recon's waves per picture for many pictures (recon.hip: above 256 pictures the count that puts the most waves on a CU, above 1024 four
    at most): hundreds of copies of the rare-syntax 512 x 512 tiles, every picture the oracle's"""
    err = _check({"HM_CHECK_COPIES": str(copies), "HM_CHECK_STAGES": "0,3", "HM_CHAIN_DEBUG": "1"}, "rare512", timeout=900)
    launches = _recon_launches(err)
    assert {(n, rare) for n, *_, rare in launches} == {(copies, True)}, launches
    if copies > 1024:
        assert all(nw <= 4 for _, _, _, nw, _ in launches), launches
