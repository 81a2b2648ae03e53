"""Helpers of test_intra.py / test_intra_gpu.py: the check of every observable block of a picture against tests/intra_ref.py,
and the census of the branches of intra prediction that corpus.intra_sweep reaches - computed from decode-order records and
the reference decoder's reconstruction-stage planes with intra_ref alone, never from the code under test."""
import collections

import numpy as np

import intra_ref as ir
import residual_ref as rr

DECODE_ORDER = 2  # HM_RECORDS_DECODE_ORDER (capi.parse_hevc record_order)
CLASSES = ("8bit_split", "8bit_decode", "deep_split", "deep_decode")
KINDS = ("luma", "chroma")
SIZES = (4, 8, 16, 32)
ANGULAR = tuple(range(2, 35))


def kernel_class(bit_depth, split):
    return ("8bit" if bit_depth == 8 else "deep") + ("_split" if split else "_decode")


def describe(seed, rec, ev):
    nT = 1 << rec["log2"]
    return (f"seed {seed} component {rec['cidx']} block (x,y)=({rec['x']},{rec['y']}) {nT}x{nT} mode {rec['mode']} cbf {int(rec['cbf'])} "
            f"avail L/BL/T/TR/TL {rec['avail_left']}/{rec['avail_bottom_left']}/{rec['avail_top']}/{rec['avail_top_right']}/{int(rec['avail_tl'])} "
            f"smoothing {ev['smoothing']} edge {ev['edge']}")


def first_mismatch(seed, P, planes, note=None, quirks=rr.REFERENCE, tools_note=None, pcm_bits=None):
    """None, or a description of the first block of `planes` (reconstruction stage, one array per component) that is not what
    intra_ref predicts from the block's neighbours IN THESE PLANES plus residual_ref's residual - implicit RDPCM and the
    cross-component term included: the walk carries the luma residual of the current transform unit along, so every block is
    observable - or, for a PCM block, not the record's samples.  note(rec, ev, observable) is called for every block that is
    not PCM; tools_note(rec, ev) for every block, PCM included (ev["tools"]: residual_ref's range-extension events).  pcm_bits:
    (luma, chroma) PCM bit depths where the caller knows them (the shift is then restated)."""
    planes = [p.astype(np.int64) for p in planes]
    carry = rr.LumaCarry()
    for rec in P.records():
        obs = ir.observable(rec, P, carry)
        assert obs
        exp, ev = ir.expected_block(rec, planes, P, carry, quirks, pcm_bits)
        if note is not None and not rec["pcm"]:
            note(rec, ev, obs)
        if tools_note is not None:
            tools_note(rec, ev)
        nT = 1 << rec["log2"]
        got = planes[rec["cidx"]][rec["y"]:rec["y"] + nT, rec["x"]:rec["x"] + nT]
        if not np.array_equal(got, exp):
            y, x = np.argwhere(got != exp)[0]
            what = f"seed {seed} component {rec['cidx']} PCM block (x,y)=({rec['x']},{rec['y']}) {nT}x{nT}" if rec["pcm"] else describe(seed, rec, ev)
            t = ev["tools"]
            if t["own"]:
                what += f" {t['own']['kind']} rdpcm {t['own']['rdpcm']}" + (" rotated" if t["own"]["rotated"] else "")
            if t["ccp"]:
                what += f" scale {t['ccp']['scale']} over luma {rr.luma_kind(t['luma'])}"
            return f"{what}: {int((got != exp).sum())} samples differ, first (y,x)=({y},{x}) got {int(got[y, x])} expected {int(exp[y, x])}"
    return None


def cells_of(rec, ev):
    """the census cells one block counts in"""
    out = [("mode", ev["mode"]), ("smooth", ev["smoothing"])]
    if rec["cbf"] and ev["mode"] >= 2:
        out.append(("mode_cbf", ev["mode"]))
    out += [("avail", p) for p in ev["patterns"]]
    out += [("source", s) for s in ev["sources"]]
    st = ev["strong"]
    if st:
        if st["decision"] and not st["constant"]:
            out.append(("strong", "true_nonconstant"))
        if st["decision"] and st["visible"]:
            out.append(("strong", "true_visible"))
        if st["left_ok"] and not st["top_ok"]:
            out.append(("strong", "false_top_only"))
        if st["top_ok"] and not st["left_ok"]:
            out.append(("strong", "false_left_only"))
        if st["at_limit"]:
            out.append(("strong", "at_limit"))
    if ev["edge"]:
        out.append(("edge", ev["edge"]))
        if ev["edge"] in ("h", "v"):
            out += [("edge_clip", ev["edge"] + "_" + k) for k in ("lo", "hi") if ev["edge_clip_" + k]]
    out += [("rail", k) for k in ("lo", "hi") if ev.get("rail_" + k)]
    return out


class Census:
    """counts[(class, kind, nT, cell)] = [blocks, observable blocks]"""

    def __init__(self):
        self.counts = collections.defaultdict(lambda: [0, 0])
        self.blocks = self.observable = 0

    def noter(self, cls):
        def note(rec, ev, obs):
            self.blocks += 1
            self.observable += obs
            key = (cls, "chroma" if rec["cidx"] else "luma", 1 << rec["log2"])
            for cell in cells_of(rec, ev):
                c = self.counts[key + (cell,)]
                c[0] += 1
                c[1] += obs
        return note

    def seen(self, cls, kind, nT, cell):
        return self.counts.get((cls, kind, nT, cell), [0, 0])[1]

    def table(self):
        lines = [f"prediction blocks {self.blocks}, observable {self.observable} ({self.observable / max(1, self.blocks):.3f})",
                 "class kind size cell: blocks / observable blocks"]
        for key in sorted(self.counts, key=str):
            cls, kind, nT, cell = key
            lines.append(f"{cls} {kind} {nT}x{nT} {cell[0]}={cell[1]}: {self.counts[key][0]} / {self.counts[key][1]}")
        return "\n".join(lines) + "\n"


# ---- what must be reached, and what cannot occur ---------------------------------------------------------------------------
PATTERNS = ("nothing", "top_missing_only", "left_missing_only", "complete", "bl_none", "bl_partial", "bl_full", "tr_none", "tr_partial", "tr_full",
            "top_missing_tr_present", "corner_missing_only", "left_missing_inside")
SOURCES = ("default", "BL", "L", "TL", "T", "TR")


def exists(cls, kind, nT):
    """block sizes a class holds: chroma 32x32 needs 4:4:4 (a 32x32 chroma block of 4:2:0 / 4:2:2 would belong to a 64x64 luma
    transform, and the largest is 32x32), and 4:4:4 pictures go out in decode order"""
    return not (kind == "chroma" and nT == 32 and cls.endswith("_split"))


def smoothed(cls, kind):
    """chroma reference samples are filtered in 4:4:4 only, i.e. in decode-order pictures only"""
    return kind == "luma" or cls.endswith("_decode")


def impossible(cls, kind, nT):
    """{cell: reason} of the cells that cannot occur in (class, kind, size); the test asserts them to be zero"""
    out = {}
    if not exists(cls, kind, nT):
        return None
    for k in ("121", "bilinear", "off_by_flag"):
        if nT == 4:
            out[("smooth", k)] = "8.4.4.2.3: no filtering of the reference samples of 4x4 blocks"
        elif not smoothed(cls, kind):
            out[("smooth", k)] = "chroma reference samples are filtered in 4:4:4 only: decode-order pictures"
        elif k == "bilinear" and (nT != 32 or kind == "chroma"):
            out[("smooth", k)] = "the bilinear filter is one of 32x32 luma blocks"
    for k in ("true_nonconstant", "true_visible", "false_top_only", "false_left_only", "at_limit"):
        if nT != 32 or kind == "chroma":
            out[("strong", k)] = "the bilinear decision is taken for 32x32 luma blocks only"
    for k in ("dc", "h", "v", "suppressed"):
        if kind == "chroma" or nT == 32:
            out[("edge", k)] = "edge filters: luma blocks smaller than 32x32"
    out[("edge", "not_32")] = "luma 32x32 only" if (kind == "chroma" or nT != 32) else None
    out[("edge", "not_chroma")] = "chroma only" if kind == "luma" else None
    for k in ("h_lo", "h_hi", "v_lo", "v_hi"):
        if kind == "chroma" or nT == 32:
            out[("edge_clip", k)] = "edge filters: luma blocks smaller than 32x32"
    if nT == 4 or (nT == 8 and kind == "luma"):
        why = "a run cut by the picture edge: plane sizes are multiples of 8 luma / 4 chroma samples, so runs of that length end at the edge or inside"
        out[("avail", "bl_partial")] = out[("avail", "tr_partial")] = out[("source", "BL")] = why
    if nT == 4 or (nT == 8 and kind == "luma"):
        out[("source", "TR")] = ("the above-right run fills something only where it is cut, or where nothing before it is available: the first block "
                                 "of a slice's or tile's CTB row and as wide as its CTB, and no CTB is narrower than 16 luma / 8 chroma samples")
    out[("source", "TL")] = ("the corner is available only where the left column and the top row are (its CTB precedes theirs in the slice and "
                             "lies in their tile): it never fills anything - census_of asserts the implication on every block")
    return {k: v for k, v in out.items() if v}


def excluded(cls, kind, nT):
    """{cell: reason} of the cells that the standard allows but that are zero by a choice of the product's parser or of this sweep - no
    proofs, unlike impossible(); asserted zero as well, so that a change of either choice shows"""
    out = {}
    if impossible(cls, kind, nT) is None:
        return out
    if nT > 4 and smoothed(cls, kind) and cls.endswith("_split"):
        out[("smooth", "off_by_flag")] = "the parser sends pictures with intra_smoothing_disabled (rare syntax) in decode order"
    if kind == "luma" and nT < 32 and cls != "deep_decode":
        out[("edge", "suppressed")] = ("implicit RDPCM is rare syntax (decode order), and the sweep draws transquant bypass at 10 / 12 bit only: at 8 bit the "
                                       "reference's builds disagree on deblocking such pictures")
    return out


def required(cls, kind, nT):
    """the cells that must be non-zero among observable blocks of (class, kind, size)"""
    imp = impossible(cls, kind, nT)
    if imp is None:
        return []
    cells = [("mode", m) for m in range(35)]
    if cls == "8bit_split" and kind == "luma" and nT in (16, 32):
        cells += [("mode_cbf", m) for m in ANGULAR]  # predict_pairs8 with its fused residual
    cells += [("avail", p) for p in PATTERNS]
    cells += [("source", s) for s in SOURCES]
    cells += [("smooth", k) for k in ("none", "121", "bilinear", "off_by_flag")]
    cells += [("strong", k) for k in ("true_nonconstant", "true_visible", "false_top_only", "false_left_only")]  # (at_limit: reported only)
    cells += [("edge", k) for k in ("dc", "h", "v", "suppressed", "not_32", "not_chroma")]
    cells += [("edge_clip", k) for k in ("h_lo", "h_hi", "v_lo", "v_hi")]
    cells += [("rail", k) for k in ("lo", "hi")]
    exc = excluded(cls, kind, nT)
    return [c for c in cells if c not in imp and c not in exc]


