"""GPU: the HIP implementations of sample adaptive offset, sample by sample (corpus.sao_sweep ...).  tests/test_sao.py shows on the CPU which
branches these streams reach and holds tests/sao_ref.py - 8.7.3 from the standard, in numpy, every sample reading the input picture - against
the reference decoder.  Here sao_ref runs on the product's OWN planes in front of SAO (the deblocking stage, and the reconstruction stage
for SAO alone): its planes behind SAO must be the model's, which names the first wrong sample with its event record instead of a plane that
differs."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import corpus
import gpudecode
import orc
import residual_ref as rr
import sao_ref as sr
import saoutil as su
import synthutil
from test_deblock_gpu import _hook_batch
from test_decode_gpu import _fp

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sao.json")))
STAGE_PAIRS = ((1, 3), (0, 2))
# sao_ref is a function of the planes it reads, the records and the stream: a second batch that hands it the same planes (the other record order) gets the
# same answer without computing it again; the oracle's planes of a stream likewise
_MODEL, _ORACLE = {}, {}


def _expected(seed, P, data, s_in, before):
    key = (seed, s_in, _fp(before))
    if key not in _MODEL:
        _MODEL[key] = sr.sao(before, P, data, record=False)[0]
    return _MODEL[key]


def _oracle(seed, P):
    if seed not in _ORACLE:
        _ORACLE[seed] = {s: orc.oracle_decode(P.blob, s)[0] for s in range(4)}
    return _ORACLE[seed]


def _hold(seed, kw, P, data, got):
    """got[stage]: the product's planes (the conformance window) of stages 0-3.  Stage 3 == sao_ref(stage 1), stage 2 == sao_ref(stage 0), every stage == the
    oracle's and the reference's fingerprint.  A picture with a conformance window: the product's planes in front of SAO must be the window of the oracle's,
    and the model runs on the oracle's whole planes.  Returns the seconds the model took."""
    whole = _oracle(seed, P)
    model_s = 0.0
    for s in range(4):
        exp = su.crop(whole[s], P)
        assert len(got[s]) == len(exp)
        for c in range(len(exp)):
            diff = np.argwhere(got[s][c] != exp[c])
            if diff.size and s >= 2:  # (a wrong SAO sample: the model tells about it below)
                break
            assert diff.size == 0, f"seed {seed} {kw} stage {s} plane {c}: {len(diff)} samples differ from the oracle, first (y,x)={diff[0].tolist()}"
    for s_in, s_out in STAGE_PAIRS:
        before = whole[s_in] if any(P.crop) else got[s_in]  # (the window of the oracle's planes == the product's: asserted above)
        t = time.perf_counter()
        exp = _expected(seed, P, data, s_in, before)
        model_s += time.perf_counter() - t
        if any(not np.array_equal(g, e) for g, e in zip(got[s_out], su.crop(exp, P))):
            bad = su.first_mismatch(seed, P, data, before, got[s_out], cropped_after=True)
            raise AssertionError(f"{kw} stages {s_in} -> {s_out}: {bad}")
    for s in range(4):
        assert _fp(got[s]) == GOLD["cases"][str(seed)][str(s)], f"seed {seed} {kw}: stage {s}: not the reference's fingerprint"
    return model_s


def _batch(pkg, cases, order):
    """the cases in one batch per stage with the given record order; returns the set of kernel classes met"""
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d, record_order=order) for d in streams]
    t0 = time.perf_counter()
    got = [gpudecode.decode_pictures(pkg, blobs, s) for s in range(4)]
    gpu_s = time.perf_counter() - t0
    classes, model_s = set(), 0.0
    for k, ((seed, kw), data, blob) in enumerate(zip(cases, streams, blobs)):
        P = rr.Picture(blob if order == su.DECODE_ORDER else pkg.capi.parse_hevc(data, record_order=su.DECODE_ORDER))
        classes.add(su.kernel_class(P.flags, P.bit_depth))
        model_s += _hold(seed, kw, P, data, [got[s][k] for s in range(4)])
    print(f"sao_ref on {len(cases)} pictures, two stage pairs: {model_s:.1f} s; the four batches: {gpu_s:.1f} s")
    return classes


def test_sao_sweep_and_small_pictures_as_parsed(pkg):
    """900 pictures in one batch per stage (0, 1, 2, 3), split chains wherever the class allows: k_sao_paste<uint8_t / uint16_t, RARE or not> with its packed
    groups, its per-sample path for each of its three reasons, and the paste of conformance windows.  (Measured on an MI355X host: 6.0 s, of which the model
    3.1 s, the four batches 0.7 s, the rest the oracle's planes and the streams; the deblocking sweep: 7.1 s.)"""
    assert _batch(pkg, corpus.sao_sweep(GOLD["sweep_cases"]) + corpus.sao_small_cases(), 0) == set(su.CLASSES)


def test_sao_sweep_and_small_pictures_in_decode_order(pkg):
    """the same pictures forced into decode order (the model's and the oracle's answers are kept from the first batch where the planes SAO reads are the same: 0.8 s)"""
    assert _batch(pkg, corpus.sao_sweep(GOLD["sweep_cases"]) + corpus.sao_small_cases(), su.DECODE_ORDER) == set(su.CLASSES)


# (bit depth, chroma format, full range, matrix, output format, bytes per pixel) of the canvas each tile of corpus.sao_tiles is converted from, and the fused
# tail it must take: (the batch's kind: 0 the integer 4:2:0 chain, 1 the float chain; the kernel launched: 1 / 2 k_tail420 on 8- / 16-bit samples,
# 3 + 2 * (CF - 1) + (16-bit samples) k_tailf<Pix, CF> - test_hooks.cpp: hm_debug_batch_tail)
TILE_CHAINS = [(8, 1, 1, 6, "HM_OUT_RGB", 3, (0, 1)), (8, 1, 1, 6, "HM_OUT_RGB", 3, (0, 1)), (8, 1, 1, 6, "HM_OUT_RGB", 3, (0, 1)), (10, 1, 1, 9, "HM_OUT_RGB", 3, (1, 2)),
               (8, 1, 0, 1, "HM_OUT_RGBA", 4, (1, 3)), (10, 1, 1, 1, "HM_OUT_RRGGBB_BE", 6, (1, 4)), (8, 2, 1, 6, "HM_OUT_RGB", 3, (1, 5)), (10, 2, 0, 9, "HM_OUT_RRGGBB_LE", 6, (1, 6))]
TILE_IDS = ["8bit_420_ctb16", "8bit_420_one_slice", "8bit_420_40_slices", "10bit_420_tail420", "8bit_420_tailf", "10bit_420_tailf", "8bit_422_tailf", "10bit_422_tailf"]


@pytest.mark.parametrize("tile", range(8), ids=TILE_IDS)
def test_tiles_in_the_fused_tails(pkg, hm_hooks, tile):
    """corpus.sao_tiles, one picture per fused-tail instance the test hook can name: tail_sao of k_tail420 with UNI off (CTB 16), with UNI in one slice
    (all_ok in the CTBs off the picture's border), with UNI in 40 slices whose flags stop the deblocking filter (the batch fuses several slices only while
    no CTB needs the ring test of Q13: the PPS flag is on, SAO takes the reference's fast path, and the neighbour mask differs from 0xFF at the picture's
    border alone), its 16-bit instantiation, and tile_sao of k_tailf<uint8_t / uint16_t, 4:2:0 / 4:2:2>; with deblocking and SAO (stages 3) and with SAO alone
    (stages 2) the fused tail == the separate kernels, pixel for pixel of the converted image; the hook tells that the kernel this tile is here for ran; and
    the separate kernels' planes are held to sao_ref, the oracle and the reference's fingerprints.

    The canvas is 192 x 144, not the 512 x 512 of the deblocking tiles: the batch's fusing condition (decide_tail) asks for a width that is a multiple of 16 and
    a canvas covered by its pictures, no least size, and TAIL_MINW is a launch bound (waves per SIMD), no width.  192 x 144 is one and a half cells of the
    fused kernels wide (128 samples) and more than two high, the last ones cut, with the CTBs of 32 cut at the bottom.

    Known limit: the 10-bit 4:2:0 tile on k_tail420 is converted after its shift to 8 bits, so the comparison of the images sees a SAO change only where it
    changes the upper 8 bits; its offsets are drawn at their largest (sao_span 900), and the share of changed samples that survive the shift is computed from
    the model and printed (measured: 4138 of 4152, 99.7 %) - a figure, no threshold; the planes held to the model sample by sample are those of the
    separate kernels.  (The model's share of the run time: less than 0.1 s per tile.)"""
    import torch
    capi, L = pkg.capi, pkg.lib()
    seed, kw = corpus.sao_tiles()[tile]
    bd, cf, full, matrix, fmt, obpp, fused_tail = TILE_CHAINS[tile]
    assert (kw.get("bit_depth", 8), kw.get("chroma_format", 1), kw["full_range"], kw["matrix"]) == (bd, cf, full, matrix)
    data = synthutil.picture(seed, **kw)
    blob = capi.parse_hevc(data)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    w, h = corpus.SAO_TILE_W, corpus.SAO_TILE_H
    bps = 2 if bd > 8 else 1
    ys, cs, os_ = L.hm_plane_stride(w, bps), L.hm_plane_stride((w + 1) // 2, bps), L.hm_plane_stride(w, obpp)
    ch = h // 2 if cf == 1 else h
    for stages in (3, 2):
        out = []
        for group in (0, -1):  # 0: fused where possible, -1: never
            batch = _hook_batch(pkg, hm_hooks)
            im = dict(y=torch.zeros((h, ys), dtype=torch.uint8, device=dev), cb=torch.zeros((max(64, ch), cs), dtype=torch.uint8, device=dev),
                      cr=torch.zeros((max(64, ch), cs), dtype=torch.uint8, device=dev), rgb=torch.zeros((h, os_), dtype=torch.uint8, device=dev))
            d = capi.TileDest()
            d.plane[0], d.plane[1], d.plane[2] = im["y"].data_ptr(), im["cb"].data_ptr(), im["cr"].data_ptr()
            d.pitch[0], d.pitch[1], d.pitch[2] = ys, cs, cs
            d.canvas_width, d.canvas_height, d.x0, d.y0 = w, h, 0, 0
            if fused_tail[0] == 0:  # bench.GridBatch's description: the tile items carry the profile, the integer 4:2:0 operation converts
                d.tile_has_nclx, d.tile_full_range, d.tile_matrix = 1, full, matrix
                desc = capi.ColourDesc(w, h, 8, 1, 0, 0, 0, 0, capi.HM_OUT_RGB, ys, cs, cs, os_)
            else:                   # the canvas carries the tile's profile, nothing is rescaled
                d.tile_has_nclx = 0
                desc = capi.ColourDesc(w, h, bd, cf, 1, matrix, 1, full, getattr(capi, fmt), ys, cs, cs, os_)
            batch.add(blob, d)
            batch.upload(st)
            batch.tail()  # (forgets what earlier batches launched)
            ptrs = [(C.c_void_p * 1)(im[k].data_ptr()) for k in ("y", "cb", "cr", "rgb")]
            batch.set_colour(desc, 1, *ptrs, group)
            batch.execute(stages, st)
            torch.cuda.synchronize()
            batch.check()
            assert batch.tail_fused() == (group == 0), (tile, stages, group)
            assert batch.tail() == (fused_tail if group == 0 else (-1, 0)), (tile, stages, group)
            out.append(im["rgb"].cpu().numpy()[:h, :w * obpp].copy())
            batch.close()
        assert out[0].any() and np.array_equal(out[0], out[1]), f"tile {tile} stages {stages}: the fused tail differs from the separate kernels"
    got = [gpudecode.decode_pictures(pkg, [blob], s)[0] for s in range(4)]
    P = rr.Picture(capi.parse_hevc(data, record_order=su.DECODE_ORDER))
    model_s = _hold(seed, kw, P, data, got)
    changed = sum(int(np.count_nonzero(a != b)) for a, b in zip(got[3], got[1]))
    assert changed > 0
    print(f"tile {TILE_IDS[tile]}: SAO changes {changed} samples of stage 1; sao_ref: {model_s:.2f} s")
    if tile == 3:
        exp = _expected(seed, P, data, 1, got[1])
        alive = sum(int(np.count_nonzero((np.asarray(a, np.int64) >> 2) != (e >> 2))) for a, e in zip(got[1], exp))
        total = sum(int(np.count_nonzero(np.asarray(a, np.int64) != e)) for a, e in zip(got[1], exp))
        print(f"10-bit tile behind the shift to 8 bits: {alive} of {total} samples that SAO changes still differ ({100.0 * alive / total:.1f} %)")
