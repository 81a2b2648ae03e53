"""GPU: the HIP deblocking filters, decision by decision (corpus.deblock_sweep ...).  tests/test_deblock.py shows on the CPU which
decisions these streams reach and holds tests/deblock_ref.py - 8.7.2 from the standard, in numpy, vertical edges of a whole plane
before horizontal ones - against the reference decoder.  Here deblock_ref runs on the product's OWN reconstruction-stage planes:
its deblocking-stage planes must be the model's, which names the first wrong unit with its event record instead of a plane that
differs."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import corpus
import deblockutil as du
import gpudecode
import orc
import residual_ref as rr
import synthutil
from test_decode_gpu import _fp

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deblock.json")))


def _batch(pkg, cases, order):
    """the cases in one batch per stage with the given record order: stage 1 == deblock_ref of the product's own stage 0, == the oracle, == the
    reference's fingerprints (and stage 0 likewise).  Returns the set of kernel classes met and the seconds the model took."""
    streams = [synthutil.picture(seed, **kw) for seed, kw in cases]
    blobs = [pkg.capi.parse_hevc(d, record_order=order) for d in streams]
    before = gpudecode.decode_pictures(pkg, blobs, 0)
    after = gpudecode.decode_pictures(pkg, blobs, 1)
    classes, model_s = set(), 0.0
    for (seed, kw), data, blob, g0, g1 in zip(cases, streams, blobs, before, after):
        P = rr.Picture(blob if order == du.DECODE_ORDER else pkg.capi.parse_hevc(data, record_order=du.DECODE_ORDER))
        classes.add(du.kernel_class(P.flags, P.bit_depth))
        t = time.perf_counter()
        bad = du.first_mismatch(seed, P, g0, g1, du.quirks_for(default_build=True))
        model_s += time.perf_counter() - t
        assert bad is None, f"{kw} record order {order}: {bad}"
        for stage, bits, g in (("recon", 0, g0), ("deblock", 1, g1)):
            exp, _ = orc.oracle_decode(blob, bits, crop=True)
            assert len(g) == len(exp)
            for c in range(len(exp)):
                diff = np.argwhere(g[c] != exp[c])
                assert diff.size == 0, f"seed {seed} {kw} stage {stage} plane {c}: {len(diff)} samples differ from the oracle, first (y,x)={diff[0].tolist()}"
            assert _fp(g) == GOLD["cases"][str(seed)][stage], f"seed {seed} {kw}: stage {stage}: not the reference's fingerprint"
    print(f"deblock_ref on {len(cases)} pictures: {model_s:.1f} s")
    return classes


def test_deblock_sweep_as_parsed(pkg):
    """1488 pictures in one batch per stage, split chains wherever the class allows.  (The model's share of the run time, measured on an
    MI355X host: 4.3 s of 7.1 s.)"""
    assert _batch(pkg, corpus.deblock_sweep(GOLD["sweep_cases"]), 0) == set(du.CLASSES)


def test_deblock_sweep_in_decode_order(pkg):
    """the same pictures forced into decode order.  (The model's share: 4.3 s of 5.3 s.)"""
    assert _batch(pkg, corpus.deblock_sweep(GOLD["sweep_cases"]), du.DECODE_ORDER) == set(du.CLASSES)


def test_one_edge_pictures(pkg):
    """300 pictures of 16x8, 8x16 and 16x16 samples - half windows at every border, the one crossing - in both record orders.  (The model's
    share: 0.4 s of 0.5 s.)"""
    for order in (0, du.DECODE_ORDER):
        assert len(_batch(pkg, corpus.deblock_single_edge_cases(), order)) == 5


# (bit depth, chroma format, full range, matrix, output format, bytes per pixel) of the canvas each tile of corpus.deblock_tiles is converted from, and the
# fused tail it must take: (the batch's kind: 0 the integer 4:2:0 chain, 1 the float chain; the kernel launched: 1 / 2 k_tail420 on 8- / 16-bit samples,
# 3 + 2 * (CF - 1) + (16-bit samples) k_tailf<Pix, CF> - test_hooks.cpp: hm_debug_batch_tail)
TILE_CHAINS = [(8, 1, 1, 6, "HM_OUT_RGB", 3, (0, 1)), (8, 1, 1, 6, "HM_OUT_RGB", 3, (0, 1)), (10, 1, 1, 9, "HM_OUT_RGB", 3, (1, 2)), (10, 2, 0, 9, "HM_OUT_RRGGBB_LE", 6, (1, 6))]


def _hook_batch(pkg, hooks):
    """a batch of the test library (conftest.hm_hooks: the shipping library's objects and the test hooks) that tells which fused tail it ran"""
    hooks.hm_debug_batch_tail.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hooks.hm_debug_batch_tail.restype = C.c_int

    class HookBatch(pkg.capi.Batch):
        def __init__(self):
            self.L = hooks
            self.h = C.c_void_p()
            pkg.capi.check(hooks.hm_batch_create(C.byref(self.h)))

        def tail(self):
            """(the fused tail the batch decided on, -1: none; the kernel that fused tails launched since the last call, 0: none)"""
            kernel = C.c_int(-1)
            return hooks.hm_debug_batch_tail(self.h, C.byref(kernel)), kernel.value

    return HookBatch()


@pytest.mark.parametrize("tile", range(4), ids=["8bit_420_one_slice", "8bit_420_40_slices", "10bit_420", "10bit_422"])
def test_tiles_in_the_fused_tails(pkg, hm_hooks, tile):
    """corpus.deblock_tiles, one 512 x 512 picture each: the fused tail (k_tail420 with the block map's copy in LDS, the same with the general
    edge derivation, its 16-bit instantiation, k_tailf<uint16_t, 2>) with deblocking alone and with no filter == the separate kernels, pixel for
    pixel of the converted image; hm_batch_tail_fused tells that a fused kernel ran, and the test hook hm_debug_batch_tail that it was the one
    this tile is here for - noted where the kernel is launched, so a 10-bit 4:2:0 tile that went through k_tailf<uint16_t, 1> instead of
    k_tail420's 16-bit instantiation is red; and the separate kernels' deblocking-stage planes are deblock_ref of their reconstruction-stage
    planes.  What the comparison of the converted images can see: the 8-bit tiles and the 4:2:2 tile (RRGGBB keeps ten bits) are converted at
    the samples' own precision; the 10-bit 4:2:0 tile is shifted to 8 bits on its way to RGB24, so a fused kernel's deblocked sample that is
    one 10-bit step off shows only where the step crosses a multiple of four - the planes held to the model sample by sample are those of the
    separate kernels.  (The model's share: less than 0.1 s per tile.)"""
    import torch
    capi, L = pkg.capi, pkg.lib()
    seed, kw = corpus.deblock_tiles()[tile]
    bd, cf, full, matrix, fmt, obpp, fused_tail = TILE_CHAINS[tile]
    assert (kw.get("bit_depth", 8), kw.get("chroma_format", 1), kw["full_range"], kw["matrix"]) == (bd, cf, full, matrix)
    data = synthutil.picture(seed, **kw)
    blob = capi.parse_hevc(data)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    w = h = 512
    bps = 2 if bd > 8 else 1
    ys, cs, os_ = L.hm_plane_stride(w, bps), L.hm_plane_stride((w + 1) // 2, bps), L.hm_plane_stride(w, obpp)
    ch = h // 2 if cf == 1 else h
    for stages in (1, 0):
        out = []
        for group in (0, -1):  # 0: fused where possible, -1: never
            batch = _hook_batch(pkg, hm_hooks)
            im = dict(y=torch.zeros((h, ys), dtype=torch.uint8, device=dev), cb=torch.zeros((max(64, ch), cs), dtype=torch.uint8, device=dev),
                      cr=torch.zeros((max(64, ch), cs), dtype=torch.uint8, device=dev), rgb=torch.zeros((h, os_), dtype=torch.uint8, device=dev))
            d = capi.TileDest()
            d.plane[0], d.plane[1], d.plane[2] = im["y"].data_ptr(), im["cb"].data_ptr(), im["cr"].data_ptr()
            d.pitch[0], d.pitch[1], d.pitch[2] = ys, cs, cs
            d.canvas_width, d.canvas_height, d.x0, d.y0 = w, h, 0, 0
            if bd == 8:  # bench.GridBatch's description: the tile items carry the profile, the integer 4:2:0 operation converts
                d.tile_has_nclx, d.tile_full_range, d.tile_matrix = 1, full, matrix
                desc = capi.ColourDesc(w, h, 8, 1, 0, 0, 0, 0, capi.HM_OUT_RGB, ys, cs, cs, os_)
            else:        # test_fused_float_tail_equals_separate_kernels': the canvas carries the tile's profile, nothing is rescaled
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
    before, after = (gpudecode.decode_pictures(pkg, [blob], bits)[0] for bits in (0, 1))
    P = rr.Picture(capi.parse_hevc(data, record_order=du.DECODE_ORDER))
    bad = du.first_mismatch(seed, P, before, after, du.quirks_for(default_build=True))
    assert bad is None, f"{kw}: {bad}"
    assert _fp(before) == GOLD["cases"][str(seed)]["recon"] and _fp(after) == GOLD["cases"][str(seed)]["deblock"]
