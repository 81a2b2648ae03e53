"""GPU: hm_batch_execute's automatic overlap (csrc/hm_overlap_plan.h, batch.cpp) - the images of a batch in two groups on streams
of their own - gives the pixels of the single stream wherever the cut falls, execute after execute; a batch of one image stays
on one stream; the per-kernel timings stay filled and honest under overlap (union spans); a refused execute leaves nothing
behind.  Batches of 5 images of 2 x 2 pictures of 128 x 128 (CTB 32) on a 256 x 192 canvas: deblocking, SAO and a 128 x 64 tail
tile all occur.  The knobs overlap_min_pics / overlap_cut (test library only) make the schedule engage on so few pictures."""
import ctypes as C
import time

import pytest

import synthutil

pytestmark = pytest.mark.gpu

N_IMAGES, COLS, ROWS, TILE, OUT_W, OUT_H = 5, 2, 2, 128, 256, 192


def _batch_class(pkg, hooks):
    class HookBatch(pkg.capi.Batch):
        """a batch of the test library (its knobs are its own: conftest.hm_hooks)"""

        def __init__(self):
            self.L = hooks
            self.h = C.c_void_p()
            pkg.capi.check(hooks.hm_batch_create(C.byref(self.h)))

        def groups(self):
            cut = C.c_int(-1)
            return hooks.hm_debug_batch_groups(self.h, C.byref(cut)), cut.value

    hooks.hm_debug_batch_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hooks.hm_debug_batch_groups.restype = C.c_int
    return HookBatch


@pytest.fixture(scope="module")
def blobs(pkg):
    return [pkg.capi.parse_hevc(synthutil.picture(9300000 + 13 * k, width=TILE, height=TILE, log2_ctb=5, qp=30)) for k in range(N_IMAGES * COLS * ROWS)]


def _grid_batch(pkg, hooks, blobs, n_images, tile=TILE, out_w=OUT_W, out_h=OUT_H):
    import bench
    import torch
    st = torch.cuda.current_stream().cuda_stream
    gb = bench.GridBatch(pkg, torch.device("cuda:0"), COLS, ROWS, tile, out_w, out_h)
    gb.batch.close()
    gb.batch = _batch_class(pkg, hooks)()
    for j in range(n_images):
        gb.add_image(blobs[j * COLS * ROWS:(j + 1) * COLS * ROWS])
    gb.finish(st, 0)
    return gb, st


def _knobs(hooks, **kw):
    for name, v in kw.items():
        assert hooks.hm_debug_set(name.encode(), v) == 0, name


@pytest.fixture(scope="module")
def single(pkg, hm_hooks, blobs):
    """the batch and what it gives on one stream (hm_batch_set_concurrency(1)): computed once, never written again"""
    import torch
    gb, st = _grid_batch(pkg, hm_hooks, blobs, N_IMAGES)
    gb.batch.set_concurrency(1)
    gb.batch.execute(3, st)
    torch.cuda.synchronize()
    gb.batch.check()
    assert gb.batch.tail_fused() and gb.batch.groups() == (1, 0)
    want = [im["rgb"].clone() for im in gb.images]
    assert all(w[:OUT_H].any() for w in want)
    yield gb, st, want
    gb.batch.close()


@pytest.mark.parametrize("cut", [1, 2, 4])
def test_overlapped_groups_equal_single_stream(hm_hooks, single, cut):
    import torch
    gb, st, want = single
    try:
        _knobs(hm_hooks, overlap_min_pics=1, overlap_cut=cut)
        gb.batch.set_concurrency(0)
        for _ in range(3):
            for im in gb.images:
                im["rgb"].zero_()
            gb.batch.execute(3, st)
            torch.cuda.synchronize()
            assert gb.batch.groups() == (2, cut)
            for j in range(N_IMAGES):
                assert torch.equal(gb.images[j]["rgb"], want[j]), f"cut {cut}, image {j}"
        gb.batch.check()
    finally:
        _knobs(hm_hooks, overlap_min_pics=0, overlap_cut=0)
        gb.batch.set_concurrency(1)


def test_few_pictures_and_single_images_stay_on_one_stream(pkg, hm_hooks, blobs, single):
    import torch
    gb, st, want = single
    one = None
    try:
        # the threshold as it ships: 20 small pictures are far below it
        gb.batch.set_concurrency(0)
        gb.batch.execute(3, st)
        torch.cuda.synchronize()
        assert gb.batch.groups() == (1, 0)
        assert all(torch.equal(gb.images[j]["rgb"], want[j]) for j in range(N_IMAGES))
        # one image: one group whatever the knobs say
        _knobs(hm_hooks, overlap_min_pics=1, overlap_cut=1)
        one, st1 = _grid_batch(pkg, hm_hooks, blobs, 1)
        one.batch.execute(3, st1)
        torch.cuda.synchronize()
        assert one.batch.tail_fused() and one.batch.groups() == (1, 0)
        assert torch.equal(one.images[0]["rgb"], want[0])
    finally:
        if one is not None:
            one.batch.close()
        _knobs(hm_hooks, overlap_min_pics=0, overlap_cut=0)
        gb.batch.set_concurrency(1)


def test_timings_stay_filled_under_overlap(hm_hooks, single):
    """every profiled step: k_residual [4], k_chain [0] and the fused tail [2] > 0, the empty slots [1], [3] == 0, and no entry longer
    than the step's wall time (host clock around the execute and a synchronise)"""
    import torch
    gb, st, want = single
    try:
        _knobs(hm_hooks, overlap_min_pics=1, overlap_cut=2)
        gb.batch.set_concurrency(0)
        gb.batch.execute(3, st)  # (the streams and events of the groups exist from here on)
        torch.cuda.synchronize()
        gb.batch.set_profiling(3)
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gb.batch.execute(3, st)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            assert gb.batch.groups() == (2, 2)
        for i in range(3):
            ms = gb.batch.timings5_ms(i)
            print(f"step {i}: timings5_ms {ms}, wall {wall[i]:.4f} ms")
            assert ms[4] > 0 and ms[0] > 0 and ms[2] > 0, ms
            assert ms[1] == 0 and ms[3] == 0, ms
            assert max(ms) <= wall[i], (ms, wall[i])
            ms4 = gb.batch.timings4_ms(i)
            assert abs(ms4[0] - (ms[0] + ms[4])) <= 1e-6 * max(1.0, ms4[0]) and ms4[2] == ms[2]
    finally:
        gb.batch.set_profiling(0)
        _knobs(hm_hooks, overlap_min_pics=0, overlap_cut=0)
        gb.batch.set_concurrency(1)


def test_refused_execute_after_a_grouped_one_is_harmless(pkg, hm_hooks, single):
    """batch_fail_width: a host-side refusal of the execute (no GPU fault involved) on a batch that has just run in groups, not
    synchronised in between; the next single-stream execute gives the same pixels.  The refusal comes before the fork, so this
    does not reach the join of the grouped path's own error returns: it shows that a refused execute leaves a batch whose last
    execute ran on two streams usable."""
    import torch
    gb, st, want = single
    try:
        _knobs(hm_hooks, overlap_min_pics=1, overlap_cut=2)
        gb.batch.set_concurrency(0)
        gb.batch.execute(3, st)
        assert gb.batch.groups() == (2, 2)
        _knobs(hm_hooks, batch_fail_width=TILE)
        with pytest.raises(pkg.capi.HmError):
            gb.batch.execute(3, st)
        _knobs(hm_hooks, batch_fail_width=0)
        gb.batch.set_concurrency(1)
        for im in gb.images:
            im["rgb"].zero_()
        gb.batch.execute(3, st)
        torch.cuda.synchronize()
        gb.batch.check()
        assert gb.batch.groups() == (1, 0)
        for j in range(N_IMAGES):
            assert torch.equal(gb.images[j]["rgb"], want[j]), f"image {j}"
    finally:
        _knobs(hm_hooks, batch_fail_width=0, overlap_min_pics=0, overlap_cut=0)
        gb.batch.set_concurrency(1)


# ---- the automatic path as it ships: no knob, the chain launcher asked through hm_chain_plan ----
BIG_IMAGES, BIG_TILE = 3000, 64  # 12 000 pictures of 64 x 64 (2 CTB rows: a wave per picture at any count), 2 x 2 per image


def _expected_cut(n, per, resident, fraction=4, min_rounds=2):
    """the rule of DESIGN.md 7 written out on its own: -> image index of the cut, 0 = one stream"""
    def partial(m):
        k, r = divmod(m, resident)
        return m > resident and r > 0 and fraction * k * r <= resident
    pics = n * per
    if n < 2 or pics < min_rounds * resident:
        return 0
    rounds = max(1, (pics // 2 + resident // 2) // resident)  # half of the batch in rounds, to the nearest
    for c in (n // 2, rounds * resident // per):
        if 1 <= c <= n - 1 and not partial(c * per) and not partial(pics - c * per):
            return c
    return 0


def test_automatic_schedule_follows_the_chain_launcher(pkg, hm_hooks, capfd):
    """No overlap knob set: hm_batch_execute asks the chain launcher (hm_chain_plan) and cuts the batch by the rule.  The launcher's
    own debug print (knob chain_debug) of a single-stream execute gives the waves per CU of the wave-per-picture cut, hence the
    resident waves; the cut expected from them - worked out here, not by the library - must be the one the execute took, the two
    k_chain launches must be a wave per picture of exactly the groups' picture counts, and the pixels those of one stream."""
    import re
    import torch
    few = [pkg.capi.parse_hevc(synthutil.picture(9400000 + 7 * k, width=BIG_TILE, height=BIG_TILE, log2_ctb=5, qp=30)) for k in range(8)]
    gb = None
    try:
        gb, st = _grid_batch(pkg, hm_hooks, [few[(3 * k + k // 4) % 8] for k in range(BIG_IMAGES * 4)], BIG_IMAGES, BIG_TILE, 2 * BIG_TILE, 2 * BIG_TILE)
        pics = BIG_IMAGES * 4
        line = re.compile(r"\[k_chain\] (\d+) pictures, (\d+) waves \(one per picture\).* (\d+) waves per CU")
        _knobs(hm_hooks, chain_debug=1)
        gb.batch.set_concurrency(1)
        capfd.readouterr()
        gb.batch.execute(3, st)
        torch.cuda.synchronize()
        gb.batch.check()
        assert gb.batch.tail_fused() and gb.batch.groups() == (1, 0)
        launches = line.findall(capfd.readouterr().err)
        assert [int(m[0]) for m in launches] == [pics], launches
        resident = torch.cuda.get_device_properties(0).multi_processor_count * int(launches[0][2])
        want = [gb.images[j]["rgb"].clone() for j in range(0, BIG_IMAGES, 97)]
        cut = _expected_cut(BIG_IMAGES, 4, resident)
        print(f"resident {resident} waves, {pics / resident:.2f} rounds, expected cut {cut}")
        assert cut > 0, "the batch was sized for two groups on an MI355X"
        gb.batch.set_concurrency(0)
        for j in range(0, BIG_IMAGES, 97):
            gb.images[j]["rgb"].zero_()
        gb.batch.execute(3, st)
        torch.cuda.synchronize()
        gb.batch.check()
        assert gb.batch.groups() == (2, cut)
        launches = line.findall(capfd.readouterr().err)
        assert sorted(int(m[0]) for m in launches) == sorted([4 * cut, pics - 4 * cut]), launches
        for k, j in enumerate(range(0, BIG_IMAGES, 97)):
            assert torch.equal(gb.images[j]["rgb"], want[k]), f"image {j}"
    finally:
        _knobs(hm_hooks, chain_debug=0)
        if gb is not None:
            gb.batch.close()
