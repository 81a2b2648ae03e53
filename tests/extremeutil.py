"""Helpers of test_extreme.py / test_extreme_gpu.py: the single-CTB pictures with what tests/residual_ref.py expects of their
first blocks, and the census of arithmetic edges that the extreme streams reach - all of it computed from command-stream
records with residual_ref alone, never from the code under test."""
import collections
import struct

import numpy as np

import corpus
import residual_ref as rr
import synthutil

DECODE_ORDER, SPLIT_ORDER = 2, 1  # HM_RECORDS_DECODE_ORDER / HM_RECORDS_SPLIT (capi.parse_hevc record_order)
N_PER_SHAPE, N_WRAP_PER_SHAPE = 600, 60  # 5 shapes: 3000 + 300 pictures of one CTB
EDGES = ("clip_hi", "clip_lo", "stage1_clip", "dc_only_clipped", "edge_and_in_range")
LARGE_EDGES = ("top_left_only", "last_group")


def note(census, bd, rec, ev, exp=None):
    """count the edges of one unit; exp: its expected samples where they are observable (single-CTB pictures)"""
    key = (bd, rec["log2"])
    clipped = ev["clip_hi"] or ev["clip_lo"]
    for k in ("wrap", "clip_hi", "clip_lo", "stage1_clip", "stage2_beyond_int16", "top_left_only", "last_group"):
        census[key + (k,)] += bool(ev[k])
    census[key + ("dc_only_clipped",)] += ev["dc_only"] and clipped and ev["kind"] in ("dct", "dst")
    census[key + (ev["kind"],)] += 1
    if exp is not None:
        mx = (1 << bd) - 1
        inside = int(((exp > 0) & (exp < mx)).sum())
        census[key + ("edge_and_in_range",)] += (clipped or ev["wrap"]) and inside > 0
        census[key + ("wrap_and_in_range",)] += ev["wrap"] and inside > 0
        census["samples"] += exp.size
        census["samples_in_range"] += inside


def single_ctb_pictures(capi, n_per_shape=N_PER_SHAPE):
    """[(seed, kw, stream, [(cidx, expected samples of the component's first block)])], census"""
    census = collections.Counter()
    out = []
    for seed, kw in corpus.single_ctb_cases(n_per_shape, n_wrap_per_shape=N_WRAP_PER_SHAPE):
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(capi.parse_hevc(data, record_order=DECODE_ORDER))
        assert P.n_ctbs == 1
        mid, mx = 1 << (P.bit_depth - 1), (1 << P.bit_depth) - 1
        firsts = []
        for rec in P.records(0):
            if any(c == rec["cidx"] for c, _ in firsts):
                continue
            assert rec["x"] == 0 and rec["y"] == 0 and not rec["pcm"]
            nT = 1 << rec["log2"]
            if rec["cbf"]:
                r, ev = rr.residual(rec, P.bit_depth, P.scaling, P.flags)
                exp = np.clip(mid + r, 0, mx).astype(np.uint16)
                note(census, P.bit_depth, rec, ev, exp)
            else:
                exp = np.full((nT, nT), mid, np.uint16)
            firsts.append((rec["cidx"], exp))
        out.append((seed, kw, data, firsts))
    return out, census


def first_mismatch(planes, firsts):
    """None, or a description of the first block of `planes` that is not what residual_ref expects"""
    for cidx, exp in firsts:
        got = planes[cidx][:exp.shape[0], :exp.shape[1]]
        if not np.array_equal(got, exp):
            y, x = np.argwhere(got != exp)[0]
            return f"component {cidx}, {exp.shape[0]}x{exp.shape[0]}: {int((got != exp).sum())} samples differ, first (y,x)=({y},{x}) got {int(got[y, x])} expected {int(exp[y, x])}"
    return None


def sweep_census(capi, cases):
    """the edges in ALL units of the sweep's pictures (transformed or transform-skip units outside implicit RDPCM; the
    residual itself is not observable there - the reference decoder's pictures hold it), and the QpY walk"""
    census = collections.Counter()
    qp = dict(lowest=False, highest=False, wrap_up=False, wrap_down=False)
    for seed, kw in cases:
        P = rr.Picture(capi.parse_hevc(synthutil.picture(seed, **kw), record_order=DECODE_ORDER))
        off = 6 * (P.bit_depth - 8)
        # (8-283): QpY = ((qPY_PRED + CuQpDeltaVal + 52 + 2 * QpBdOffset) % (52 + QpBdOffset)) - QpBdOffset.  qPY_PRED is the slice QP,
        # an earlier QpY or the mean of two, so it lies between the lowest and the highest of those; |CuQpDeltaVal| <= 26 + QpBdOffset / 2.
        # A QpY further than that below all of them went round the top of the range, one further above round the bottom.
        assert P.n_slices == 1
        lo = hi = struct.unpack_from("<b", P.blob, P.off_slices + 10)[0]  # hm_slice.slice_qp
        reach = 26 + off // 2
        for rec in P.records():
            if rec["cidx"] == 0 and not rec["pcm"]:
                q = rec["qpy"]
                qp["lowest"] |= q == -off
                qp["highest"] |= q == 51
                qp["wrap_up"] |= q < lo - reach
                qp["wrap_down"] |= q > hi + reach
                lo, hi = min(lo, q), max(hi, q)
            if not rec["cbf"] or rec["pcm"] or rec["bypass"]:
                continue
            if (P.flags & rr.PIC_IMPLICIT_RDPCM) and rec["tskip"] and rec["mode"] in (10, 26):
                continue
            _, ev = rr.residual(rec, P.bit_depth, P.scaling, P.flags)
            note(census, P.bit_depth, rec, ev)
    return census, qp
