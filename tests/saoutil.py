"""Helpers of test_sao.py / test_sao_gpu.py: the comparison of SAO-stage planes with tests/sao_ref.py, naming the first wrong sample with
its event record, and the census of the branches of sample adaptive offset that the SAO corpora reach - computed from sao_ref's event
records and from positions alone, never from the code under test."""
import collections

import numpy as np

import sao_ref as sr
from test_decode_gpu import RARE_SYNTAX  # HM_PIC_RARE_SYNTAX (hm_stream.h): the one copy the tests keep

DECODE_ORDER = 2  # HM_RECORDS_DECODE_ORDER (capi.parse_hevc record_order)
# the instantiation of k_sao_paste a picture meets (hm_launch_sao_paste: Pix by the bit depth, RARE by the picture's rare syntax)
CLASSES = ("8bit_common", "deep_common", "8bit_rare", "deep_rare")
KINDS = ("luma", "chroma")
# (input stage, output stage) of the product / (flags of the reference's input, of its output): deblocked input, and SAO alone on the reconstruction
PAIRS = ("1to3", "0to2")
SIDES = ("left", "right", "top", "bottom")
G = 8  # samples of one group of k_sao_paste


def kernel_class(flags, bit_depth):
    return ("8bit" if bit_depth == 8 else "deep") + ("_rare" if flags & RARE_SYNTAX else "_common")


def uncrop_window(P, c):
    """(y0, y1, x0, x1) of the conformance window in plane c"""
    cl, cr, ct, cb = P.crop
    sw, sh = ((1 if P.chroma_format == 3 else 2), (2 if P.chroma_format == 1 else 1)) if c else (1, 1)
    return ct // sh, (P.height - cb) // sh, cl // sw, (P.width - cr) // sw


def crop(planes, P):
    out = []
    for c, p in enumerate(planes):
        y0, y1, x0, x1 = uncrop_window(P, c)
        out.append(np.ascontiguousarray(p[y0:y1, x0:x1]))
    return out


def first_mismatch(seed, P, data, before, after, quirks=None, note=None, cropped_after=False):
    """None, or a description of the first sample of `after` (SAO stage) that is not sao_ref of `before` (the stage SAO reads; the whole coded
    picture), with its event record.  cropped_after: `after` holds the conformance window only.  note(events) is called with the model's records."""
    exp, events = sr.sao(before, P, data, quirks, record=note is not None)
    if note is not None:
        note(events)
    for c in range(len(exp)):
        y0, y1, x0, x1 = uncrop_window(P, c) if cropped_after else (0, exp[c].shape[0], 0, exp[c].shape[1])
        e = exp[c][y0:y1, x0:x1]
        got = np.asarray(after[c], np.int64)
        assert got.shape == e.shape, (seed, c, got.shape, e.shape)
        bad = np.argwhere(got != e)
        if bad.size:
            y, x = (int(v) for v in bad[0])
            return (f"seed {seed} plane {c}: {len(bad)} samples differ from sao_ref, first (y,x)=({y + y0},{x + x0}) of the coded picture got {int(got[y, x])}; " +
                    sr.describe(events[c], y + y0, x + x0))
    return None


def largest_offset(P, c):
    """the largest |SaoOffsetVal| the plane's bit depth allows (7.4.9.3.2: sao_offset_abs up to (1 << (Min(bitDepth, 10) - 5)) - 1, << log2OffsetScale)"""
    bd, scale = (P.bit_depth_c, P.sao_scale_c) if c else (P.bit_depth, P.sao_scale_y)
    return ((1 << (min(bd, 10) - 5)) - 1) << scale, scale


def cells_of(ev, P):
    """{cell: number of samples} of one plane of one picture"""
    c = ev["plane"]
    out = collections.Counter()
    H, W = ev["type"].shape
    bd = P.bit_depth_c if c else P.bit_depth
    maxv = (1 << bd) - 1
    y, x = np.arange(H)[:, None] + np.zeros((1, W), np.int64), np.arange(W)[None, :] + np.zeros((H, 1), np.int64)
    sw = ((1 if P.chroma_format == 3 else 2) if c else 1)
    l2w = P.log2_ctb - (sw - 1)

    def put(cell, mask):
        n = int(np.count_nonzero(mask))
        if n:
            out[cell] += n

    typ, kept = ev["type"], ev["kept"]
    live = ~kept
    band, edge = (typ == 1) & live, (typ == 2) & live
    offset = ev["raw"] - ev["before"]
    # ---- off / on ----
    put(("off", "slice_flag"), ~ev["on"])
    put(("off", "type_0"), ev["on"] & (typ == 0))
    if P.chroma_format:
        if c == 0:
            put(("slice", "luma_on_chroma_off"), ev["on_luma"] & ~ev["on_chroma"] & (typ > 0))
        else:
            put(("slice", "chroma_on_luma_off"), ev["on_chroma"] & ~ev["on_luma"] & (typ > 0))
            put(("cb_cr_offsets_differ",), (typ > 0) & ev["cb_cr_differ"])
    put(("ctb", "cut_right"), (typ > 0) & ev["cut_right"])
    put(("ctb", "cut_bottom"), (typ > 0) & ev["cut_bottom"])
    # ---- band offset ----
    big, scale = largest_offset(P, c)
    hit = band & (ev["band_idx"] > 0)
    for k in range(1, 5):
        put(("band", "hit", k), band & (ev["band_idx"] == k))
    put(("band", "none"), band & (ev["band_idx"] == 0))
    put(("band", "wrapped_hit"), hit & (ev["band_position"] >= 29) & (ev["band"] < ev["band_position"]))
    put(("band", "offset_positive"), hit & (offset > 0))
    put(("band", "offset_negative"), hit & (offset < 0))
    put(("band", "largest"), hit & (np.abs(offset) == big))
    if scale:
        put(("band", "largest_scaled"), hit & (np.abs(offset) == big))
    put(("band", "clip_0"), band & (ev["raw"] < 0))
    put(("band", "clip_max"), band & (ev["raw"] > maxv))
    # ---- edge offset ----
    avail = ev["available"]
    for cl in range(4):
        e = edge & (ev["eo_class"] == cl)
        for k in range(5):
            put(("edge", cl, "edgeIdx", k), e & avail & (ev["edge_idx"] == k))
        put(("edge", cl, "largest"), e & avail & (offset != 0) & (np.abs(offset) == big))
        put(("edge", cl, "clip_0"), e & (ev["raw"] < 0))
        put(("edge", cl, "clip_max"), e & (ev["raw"] > maxv))
        for n in "ab":
            ox, oy = ev[n + "_outside_x"], ev[n + "_outside_y"]
            put(("edge", cl, n, "picture_left"), e & (ox < 0))
            put(("edge", cl, n, "picture_right"), e & (ox > 0))
            put(("edge", cl, n, "picture_top"), e & (oy < 0))
            put(("edge", cl, n, "picture_bottom"), e & (oy > 0))
            for r in (sr.EARLIER_SLICE, sr.LATER_SLICE, sr.TILE_BORDER):
                put(("edge", cl, n, sr.REASONS[r]), e & (ev[n + "_reason"] == r))
        if cl >= 2:
            put(("edge", cl, "diagonal_blocked_sides_usable"), e & (ev["a_diag_blocked_sides_ok"] | ev["b_diag_blocked_sides_ok"]))
            put(("edge", cl, "diagonal_usable_side_blocked"), e & (ev["a_diag_ok_side_blocked"] | ev["b_diag_ok_side_blocked"]))
        # kernel geometry, from positions: the first / last sample of a group of 8 looks into another CTB column and gets another answer than its neighbour in the group
        if cl != 1:
            other_l = (x > 0) & (x % G == 0) & ((x >> l2w) != ((x - 1) >> l2w))
            other_r = (x + 1 < W) & (x % G == G - 1) & ((x >> l2w) != ((x + 1) >> l2w))
            put(("group", cl, "first_differs"), e & other_l & (avail != np.roll(avail, -1, 1)))
            put(("group", cl, "last_differs"), e & other_r & (avail != np.roll(avail, 1, 1)))
        if cl >= 1:
            put(("row", cl, "first"), e & (y == 0))
            put(("row", cl, "last"), e & (y == H - 1))
    e = edge
    put(("q13", "mask_differs"), e & ev["decided_by_chroma_slice_lookup"])
    put(("q13", "ring_blocked_by_own_ctb"), e & (ev["a_own_ctb_blocked"] | ev["b_own_ctb_blocked"]))
    put(("fast_path", "other_slice_used"), e & ev["decided_by_pps_fast_path"])
    put(("slice_order", "by_address_differs"), e & ev["decided_by_slice_order_by_address"])
    put(("in_place_would_differ",), e & ev["in_place_would_differ"])
    # ---- lossless units ----
    put(("lossless", "pcm_kept"), (typ > 0) & kept & ev["pcm"])
    put(("lossless", "pcm_filtered"), (typ > 0) & live & ev["pcm"] & (ev["after"] != ev["before"]))
    put(("lossless", "bypass_kept"), (typ > 0) & kept & ev["bypass"])
    put(("lossless", "kept_neighbour_of_filtered"), e & avail & (ev["a_kept"] | ev["b_kept"]) & (ev["after"] != ev["before"]))
    # ---- the per-sample path of k_sao_paste, for its three reasons (positions inside the conformance window, which is what is pasted) ----
    y0, y1, x0, x1 = uncrop_window(P, c)
    inside = (y >= y0) & (y < y1) & (x >= x0) & (x < x1) & (typ > 0)
    put(("per_sample", "offset_not_multiple_of_8"), inside if x0 % G else np.zeros((H, W), bool))
    put(("per_sample", "partial_group"), inside & (x - x0 >= (x1 - x0) // G * G) if x0 % G == 0 else np.zeros((H, W), bool))
    put(("per_sample", "q13_redo"), inside & (typ == 2) & ev["own_ctb_blocked"] if c else np.zeros((H, W), bool))
    return out


class Census:
    """counts[(class, kind, stage pair, cell)] = samples"""

    def __init__(self):
        self.counts = collections.Counter()
        self.pictures = collections.Counter()
        self.samples = 0

    def noter(self, cls, pair, P):
        def note(events):
            self.pictures[(cls, pair)] += 1
            for ev in events:
                self.samples += ev["type"].size
                key = (cls, "chroma" if ev["plane"] else "luma", pair)
                for cell, n in cells_of(ev, P).items():
                    self.counts[key + (cell,)] += n
        return note

    def seen(self, cls, kind, pair, cell):
        return self.counts.get((cls, kind, pair, cell), 0)

    def table(self):
        lines = [f"samples {self.samples}; pictures per class and stage pair " + ", ".join(f"{c} {p} {self.pictures[(c, p)]}" for c in CLASSES for p in PAIRS),
                 "class kind stages cell: samples"]
        for key in sorted(self.counts, key=str):
            cls, kind, pair, cell = key
            lines.append(f"{cls} {kind} {pair} {' '.join(str(v) for v in cell)}: {self.counts[key]}")
        return "\n".join(lines) + "\n"


# ---- what must be reached, and what cannot occur ---------------------------------------------------------------------------
def rare(cls):
    return cls.endswith("_rare")


# the picture edges neighbour a / b of each class can lie beyond (Table 8-13: a = (x + hPos[0], y + vPos[0]), b the opposite)
EDGES_OF = {0: {"a": ("left",), "b": ("right",)}, 1: {"a": ("top",), "b": ("bottom",)}, 2: {"a": ("left", "top"), "b": ("right", "bottom")},
            3: {"a": ("right", "top"), "b": ("left", "bottom")}}


def impossible(cls, kind, pair):
    """{cell: reason} of the cells that cannot occur in (class, kind, stage pair); the test asserts them to be zero"""
    out = {}
    for cl in range(4):
        for n in "ab":
            for side in SIDES:
                if side not in EDGES_OF[cl][n]:
                    out[("edge", cl, n, "picture_" + side)] = "Table 8-13: this neighbour of the class does not lie in that direction"
    if not rare(cls):
        for k in ("pcm_kept", "pcm_filtered", "bypass_kept", "kept_neighbour_of_filtered"):
            out[("lossless", k)] = "PCM and transquant bypass are rare syntax"
    if kind == "luma":
        for cell in (("q13", "mask_differs"), ("q13", "ring_blocked_by_own_ctb"), ("per_sample", "q13_redo")):
            out[cell] = "Q13: luma is looked up at its own position; a neighbour inside the own CTB lies in the own slice and tile"
    if cls.startswith("8bit"):
        out[("band", "largest_scaled")] = "log2_sao_offset_scale is at most bitDepth - 10"
    return out


def excluded(cls, kind, pair):
    """{cell: reason} of cells that the standard allows but that are zero by a choice of the parser or of the corpora; asserted zero too"""
    return {}


def required(cls, kind, pair):
    """the cells that must be non-zero in (class, kind, stage pair)"""
    cells = [("off", "slice_flag"), ("off", "type_0"), ("ctb", "cut_right"), ("ctb", "cut_bottom")]
    cells += [("slice", "luma_on_chroma_off")] if kind == "luma" else [("slice", "chroma_on_luma_off"), ("cb_cr_offsets_differ",)]
    cells += [("band", "hit", k) for k in range(1, 5)]
    cells += [("band", k) for k in ("none", "wrapped_hit", "offset_positive", "offset_negative", "largest", "clip_0", "clip_max")]
    if cls.startswith("deep"):
        cells.append(("band", "largest_scaled"))
    for cl in range(4):
        cells += [("edge", cl, "edgeIdx", k) for k in range(5)]
        cells += [("edge", cl, "largest"), ("edge", cl, "clip_0"), ("edge", cl, "clip_max")]
        for n in "ab":
            cells += [("edge", cl, n, "picture_" + side) for side in EDGES_OF[cl][n]]
            cells += [("edge", cl, n, "tile_border")]
        # (chroma of the common classes is sub-sampled: under Q13 the reference compares the neighbour's slice address with the one found at CTB (x >> 1, y >> 1 or y),
        #  which without tiles is never the larger one - neighbour a is then stopped as one of a "later" slice, by ITS slice's flag)
        cells += [("edge", cl, "a", "later_slice" if kind == "chroma" and not rare(cls) else "earlier_slice"), ("edge", cl, "b", "later_slice")]
        if cl >= 2:
            cells += [("edge", cl, "diagonal_blocked_sides_usable"), ("edge", cl, "diagonal_usable_side_blocked")]
        if cl != 1:
            cells += [("group", cl, "first_differs"), ("group", cl, "last_differs")]
        if cl >= 1:
            cells += [("row", cl, "first"), ("row", cl, "last")]
    cells += [("fast_path", "other_slice_used"), ("in_place_would_differ",), ("per_sample", "offset_not_multiple_of_8"), ("per_sample", "partial_group")]
    if kind == "chroma":
        cells += [("q13", "mask_differs"), ("q13", "ring_blocked_by_own_ctb"), ("per_sample", "q13_redo")]
    if rare(cls):
        cells += [("lossless", k) for k in ("pcm_kept", "pcm_filtered", "bypass_kept", "kept_neighbour_of_filtered")]
    imp, exc = impossible(cls, kind, pair), excluded(cls, kind, pair)
    return [c for c in dict.fromkeys(cells) if c not in imp and c not in exc]


# ---- the reference decoder's planes -------------------------------------------------------------------------------------------
def reference_stages(data, kw):
    """{stage: planes} of the live reference decoder (stage bits: 1 deblocking, 2 SAO; the conformance window only) in the build that is the truth for
    the picture: the scalar build for the Q9 class, the default build for 8-bit pictures of the "pcmf" branch (input and output alike), and
    everywhere else the scalar build, which the default build must equal at every stage - asserted"""
    import corpus
    import orc
    q9, pcmf8 = corpus.sao_class_q9(kw), corpus.sao_class_pcmf8(kw)
    assert not (q9 and pcmf8), "a picture in both classes of the reference's builds"
    flags = {0: orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO, 1: orc.REF_F_NO_SAO, 2: orc.REF_F_NO_DEBLOCK, 3: 0}
    build = 0 if pcmf8 else orc.REF_F_SCALAR
    out = {s: orc.ref_decode(data, f | build)[0] for s, f in flags.items()}
    if not q9 and not pcmf8:
        for s in (2, 3):
            other = orc.ref_decode(data, flags[s])[0]
            assert all(np.array_equal(a, b) for a, b in zip(other, out[s])), f"{kw}: the reference's builds differ at stage {s} outside the Q9 and pcmf classes"
    return out


def fingerprint(planes):
    import orc
    h = 0
    for p in planes:
        a = np.ascontiguousarray(p if p.max() > 255 else p.astype(np.uint8))
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


WINDOW_KEYS = ("conf_left", "conf_right", "conf_top", "conf_bottom")


def reference_whole(seed, kw, data, P):
    """{stage: planes of the WHOLE coded picture} of the live reference decoder.  The reference hands out the conformance window alone; the
    whole planes of a windowed picture come from its twin, the same seed and parameters without the window (the window is a field of the SPS:
    the slice data are the same bytes - asserted through the parser's records), and what the reference hands out for the windowed stream is held
    to the twin's planes cropped.  One class is not: with more than 8 bits and a left or top offset the reference computes the window's first
    sample in BYTES of 16-bit storage (image.cc:406-410), so the planes it hands out start at half the offset and are no window of the
    picture; the standard's window - what the product hands out - is the twin's planes cropped, and that is what is recorded."""
    import orc
    import synthutil
    if not any(P.crop):
        return reference_stages(data, kw)
    twin = synthutil.picture(seed, **{k: v for k, v in kw.items() if k not in WINDOW_KEYS})
    whole = reference_stages(twin, kw)
    assert all([p.shape for p in whole[s]] == sr.planes_shape(P) for s in whole)
    if not (P.bit_depth > 8 and (P.crop[0] or P.crop[2])):
        handed = reference_stages(data, kw)
        for s in whole:
            assert all(np.array_equal(a, b) for a, b in zip(crop(whole[s], P), handed[s])), f"seed {seed} {kw}: the reference's window is not the window of its whole picture at stage {s}"
    return whole


def hold_picture(seed, kw, data, P, C=None, quirks=None):
    """sao_ref against the live reference decoder, both stage pairs, every sample of the whole coded picture; the census taken on the way.  Returns
    {stage: fingerprint of the reference's planes, the conformance window}."""
    ref = reference_whole(seed, kw, data, P)
    cls = kernel_class(P.flags, P.bit_depth)
    for pair, (s_in, s_out) in zip(PAIRS, ((1, 3), (0, 2))):
        bad = first_mismatch(seed, P, data, ref[s_in], ref[s_out], quirks, C.noter(cls, pair, P) if C is not None else None)
        assert bad is None, f"{kw} stages {pair}: sao_ref is not the reference decoder: {bad}"
    return {str(s): fingerprint(crop(ref[s], P)) for s in ref}
