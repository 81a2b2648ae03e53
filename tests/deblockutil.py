"""Helpers of test_deblock.py / test_deblock_gpu.py: the comparison of deblocked planes with tests/deblock_ref.py, naming the first
wrong unit, and the census of the decisions of the deblocking filter that the deblocking corpora reach - computed from
deblock_ref's event records on the reference decoder's planes, never from the code under test."""
import collections

import numpy as np

import deblock_ref as dr
import residual_ref as rr
from test_decode_gpu import RARE_SYNTAX  # HM_PIC_RARE_SYNTAX (hm_stream.h): the one copy the tests keep

DECODE_ORDER = 2  # HM_RECORDS_DECODE_ORDER (capi.parse_hevc record_order)
# which filters of filters.hip a picture meets (hm_launch_deblock, window_filter): the packed 8-bit ones, the packed 16-bit ones
# (maxv < 2048), the plain scalar ones at 12 bit and - with their "pcmf" branches - for every picture with rare syntax
CLASSES = ("8bit_packed", "deep_packed", "deep_scalar", "8bit_rare", "deep_rare")
KINDS = ("luma", "chroma")
DIRS = ("V", "H")
CAUSES = ("pcm_nolf", "pcm_lf", "bypass")
WINDOWS = ("interior", "first_half", "second_half")  # V: top / bottom half windows, H: left / right
STRONG_POSITIONS = ("p0", "p1", "p2", "q0", "q1", "q2")


def kernel_class(flags, bit_depth):
    if flags & RARE_SYNTAX:
        return "8bit_rare" if bit_depth == 8 else "deep_rare"
    return "8bit_packed" if bit_depth == 8 else "deep_packed" if bit_depth < 12 else "deep_scalar"


def quirks_for(default_build):
    """the model's switches for a comparison with the reference's default (SIMD) build or its scalar build; the product follows the
    default build (which at more than 8 bits is the scalar code: the model tells by the picture's bit depth)"""
    return dr.Quirks(pcmf_luma="simd" if default_build else "scalar")


def first_mismatch(seed, P, before, after, quirks=None, note=None):
    """None, or a description of the first sample of `after` (deblocking stage) that is not deblock_ref of `before` (reconstruction
    stage), with the event records of the units that hold it.  note(events) is called with the model's records."""
    exp, events = dr.deblock(before, P, quirks)
    if note is not None:
        note(events)
    for c in range(len(exp)):
        bad = np.argwhere(np.asarray(after[c], np.int64) != exp[c])
        if bad.size:
            y, x = (int(v) for v in bad[0])
            units = dr.units_at(events, c, y, x) or ["no unit of the model holds this sample"]
            return (f"seed {seed} plane {c}: {len(bad)} samples differ from deblock_ref, first (y,x)=({y},{x}) got {int(after[c][y, x])} expected {int(exp[c][y, x])} "
                    f"reconstruction {int(before[c][y, x])}; " + "; ".join(units))
    return None


def cells_of(ev, P):
    """{cell: number of units} of one (plane, direction) of one picture"""
    luma = ev["plane"][0] == 0
    out = collections.Counter()
    on = ev["bS"] > 0

    def put(cell, mask):
        n = int(np.count_nonzero(mask))
        if n:
            out[cell] += n

    put(("bS", 0), ~on)
    put(("bS", 2), on)
    put(("window", WINDOWS[0]), on & (ev["window"] == 0))
    put(("window", WINDOWS[1]), on & (ev["window"] == 1))
    put(("window", WINDOWS[2]), on & (ev["window"] == 2))
    if "reads_filtered" in ev:
        put(("crossing",), ev["reads_filtered"] & ev["changed"])
    put(("segment_differs",), on & ev["segment_differs"])
    other = ev["slice_p"] != ev["slice_q"]
    put(("off", "q_side"), ev["tu_edge"] & other & ev["off_q"] & ~ev["off_p"])
    put(("off", "p_side"), on & other & ev["off_p"])
    dropped = ev["tu_edge"] & ~ev["allowed"] & ~ev["off_q"]
    put(("dropped", "slice_border"), dropped & other & ~ev["lf_across_slices"])
    put(("dropped", "tile_border"), dropped & ~(other & ~ev["lf_across_slices"]))
    put(("slice_offsets_differ",), on & other & ((ev["beta_offset"] != 0) | (ev["tc_offset"] != 0)) &
        ((ev["beta_offset"] != ev["beta_offset_p"]) | (ev["tc_offset"] != ev["tc_offset_p"])))
    put(("Qtc", "below_0"), on & (ev["Q_tc"] < 0))
    put(("Qtc", "above_53"), on & (ev["Q_tc"] > 53))
    put(("qp", "odd_sum"), on & (ev["QpP"] != ev["QpQ"]) & ((ev["QpP"] + ev["QpQ"]) % 2 != 0))
    put(("delta", "lo"), ev["delta_lo"])
    put(("delta", "hi"), ev["delta_hi"])
    put(("res", "lo"), ev["res_lo"])
    put(("res", "hi"), ev["res_hi"])
    # PCM / bypass units: which sides are held back
    any_pcm, any_bypass = ev["pcm_p"] | ev["pcm_q"], ev["bypass_p"] | ev["bypass_q"]
    touched = {"pcm_nolf": any_pcm & ~any_bypass & bool(P.pcm_loop_filter_disabled), "pcm_lf": any_pcm & ~any_bypass & (not P.pcm_loop_filter_disabled),
               "bypass": any_bypass & ~any_pcm, "pcm_and_bypass": any_pcm & any_bypass}
    acts = on & (ev["dE"] > 0)
    for cause, m in touched.items():
        for hp in (0, 1):
            for hq in (0, 1):
                put(("held", cause, hp, hq), acts & m & (ev["filterP"] != hp) & (ev["filterQ"] != hq))
    if P.flags & rr.PIC_PCMF:
        for hp in (0, 1):
            put(("held", "ordinary_in_pcmf_picture", hp, hp), acts & ~(any_pcm | any_bypass) & (ev["filterP"] != hp) & (ev["filterQ"] != hp))
    if luma:
        b2 = on
        put(("tc0_beta_pos",), b2 & (ev["tc"] == 0) & (ev["beta"] > 0))
        put(("beta0",), b2 & (ev["beta"] == 0))
        put(("dE", 0), b2 & (ev["beta"] > 0) & (ev["dE"] == 0))
        for a in (0, 1):
            for b in (0, 1):
                put(("normal", a, b), (ev["dE"] == 1) & (ev["dEp"] == a) & (ev["dEq"] == b))
        put(("strong",), ev["dE"] == 2)
        n_true = ev["preds"].sum(1)
        for k in range(6):
            put(("near_strong", k), (ev["dE"] == 1) & (n_true == 5) & ~ev["preds"][:, k])
        put(("d", "beta-1"), b2 & (ev["beta"] > 0) & (ev["d"] == ev["beta"] - 1))
        put(("d", "beta"), b2 & (ev["beta"] > 0) & (ev["d"] == ev["beta"]))
        put(("skip10",), (ev["lines_skipped"] > 0) & (ev["lines_filtered"] > 0))
        for k in ("dp", "dq"):
            put((k, "lo"), ev[k + "_lo"])
            put((k, "hi"), ev[k + "_hi"])
        for k, name in enumerate(STRONG_POSITIONS):
            put(("strong_clip", name, "lo"), ev["strong_lo"][:, k])
            put(("strong_clip", name, "hi"), ev["strong_hi"][:, k])
        put(("Qbeta", "below_0"), b2 & (ev["Q_beta"] < 0))
        put(("Qbeta", "above_51"), b2 & (ev["Q_beta"] > 51))
        put(("peak", "above_16384"), ev["peak"] > 16384)
    else:
        f = on & (ev["filterP"] | ev["filterQ"])
        put(("filtered",), f)
        if P.chroma_format == 1:
            put(("qpc", "below_30"), f & (ev["qPi"] < 30))
            put(("qpc", "30_43"), f & (ev["qPi"] >= 30) & (ev["qPi"] <= 43))
            put(("qpc", "above_43"), f & (ev["qPi"] > 43))
            # the two 4-line units of one 8-sample segment with QpC of their own
            nk = len(np.unique(ev["x"] if ev["vertical"][0] else ev["y"]))
            nj = len(ev["x"]) // nk
            if nj >= 2:
                q = ev["QpC"].reshape(nj, nk)[:nj // 2 * 2].reshape(nj // 2, 2, nk)
                b = (ev["bS"] == 2).reshape(nj, nk)[:nj // 2 * 2].reshape(nj // 2, 2, nk)
                put(("segment_qpc_differs",), b.all(1) & (q[:, 0] != q[:, 1]))
        else:
            put(("qpc", "capped_at_51"), f & (ev["qPi"] > 51))
        put(("offsets_opposite",), f & (P.cb_qp_offset * P.cr_qp_offset < 0))
        if ev["vertical"][0]:
            put(("vpq", "p_only"), on & ev["lossless_p"] & ~ev["lossless_q"])
            put(("vpq", "q_only"), on & ev["lossless_q"] & ~ev["lossless_p"])
    return out


class Census:
    """counts[(class, kind, direction, cell)] = units"""

    def __init__(self):
        self.counts = collections.Counter()
        self.pictures = collections.Counter()
        self.units = 0

    def noter(self, cls, P):
        def note(events):
            self.pictures[cls] += 1
            for ev in events:
                self.units += len(ev["x"])
                key = (cls, "chroma" if ev["plane"][0] else "luma", "V" if ev["vertical"][0] else "H")
                for cell, n in cells_of(ev, P).items():
                    self.counts[key + (cell,)] += n
        return note

    def seen(self, cls, kind, d, cell):
        return self.counts.get((cls, kind, d, cell), 0)

    def table(self):
        lines = [f"units on the 8-sample grid {self.units}; pictures per class " + ", ".join(f"{c} {self.pictures[c]}" for c in CLASSES),
                 "class kind direction cell: units"]
        for key in sorted(self.counts, key=str):
            cls, kind, d, cell = key
            lines.append(f"{cls} {kind} {d} {' '.join(str(v) for v in cell)}: {self.counts[key]}")
        return "\n".join(lines) + "\n"


# ---- what must be reached, and what cannot occur ---------------------------------------------------------------------------
def rare(cls):
    return cls.endswith("_rare")


def impossible(cls, kind, d):
    """{cell: reason} of the cells that cannot occur in (class, kind, direction); the test asserts them to be zero"""
    out = {("segment_differs",): "the two units of an 8-sample segment lie in one 8x8 block on either side (luma: one coding unit, one QpY) and in one CTB (one slice)"}
    for cause in CAUSES:
        for hp in (0, 1):
            for hq in (0, 1):
                cell = ("held", cause, hp, hq)
                if not rare(cls):
                    out[cell] = "PCM and transquant bypass are rare syntax"
                elif kind == "luma":
                    if hp and hq:
                        out[cell] = "the reference's luma path filters exactly the PCM / bypass sides of a segment that touches one (quirk pcmf_luma): one side at least is one"
                elif cause == "pcm_lf":
                    if hp or hq:
                        out[cell] = "chroma: a PCM unit is held back only with pcm_loop_filter_disabled"
                elif d == "V":
                    if hp != hq:
                        out[cell] = "a vertical chroma edge writes both sides under the P side's flag (quirk vchroma_p_for_both)"
                elif not hp and not hq:
                    out[cell] = "a horizontal chroma edge that touches a lossless unit holds that side back"
    for hp in (0, 1):
        cell = ("held", "ordinary_in_pcmf_picture", hp, hp)
        if not rare(cls):
            out[cell] = "PCM and transquant bypass are rare syntax"
        elif kind == "luma" and (cls == "8bit_rare") == bool(hp):
            out[cell] = "between ordinary units of a pcmf picture the 8-bit SIMD filter modifies both sides, the scalar filter of deeper pictures neither (quirk pcmf_luma)"
        elif kind == "chroma" and hp:
            out[cell] = "chroma between ordinary units is always filtered"
    if kind == "chroma":
        for k in ("p_only", "q_only"):
            if not rare(cls):
                out[("vpq", k)] = "PCM and transquant bypass are rare syntax"
    if kind == "luma" and cls.startswith("8bit"):
        out[("peak", "above_16384")] = "8 bit: |9 (q0 - p0) - 3 (q1 - p1) + 8| <= 12 * 255 + 8"
    return out


def excluded(cls, kind, d):
    """{cell: reason} of cells that the standard allows but that are zero by a choice of the parser or of the corpora; asserted zero too"""
    return {}


def required(cls, kind, d):
    """the cells that must be non-zero in (class, kind, direction)"""
    cells = [("bS", 0), ("bS", 2), ("crossing",) if d == "H" else ("bS", 2), ("off", "q_side"), ("off", "p_side"), ("dropped", "slice_border"), ("dropped", "tile_border"),
             ("delta", "lo"), ("delta", "hi"), ("res", "lo"), ("res", "hi")]
    cells += [("window", w) for w in WINDOWS]
    if kind == "luma":
        cells += [("tc0_beta_pos",), ("beta0",), ("dE", 0), ("strong",), ("d", "beta-1"), ("d", "beta"), ("skip10",), ("qp", "odd_sum"), ("slice_offsets_differ",)]
        cells += [("normal", a, b) for a in (0, 1) for b in (0, 1)]
        cells += [("near_strong", k) for k in range(6)]
        cells += [(k, r) for k in ("dp", "dq") for r in ("lo", "hi")]
        cells += [("strong_clip", n, r) for n in STRONG_POSITIONS for r in ("lo", "hi")]
        cells += [("Qbeta", "below_0"), ("Qbeta", "above_51"), ("Qtc", "below_0"), ("Qtc", "above_53")]
        if cls == "deep_packed":
            cells.append(("peak", "above_16384"))
    else:
        cells += [("filtered",), ("qpc", "below_30"), ("qpc", "30_43"), ("qpc", "above_43"), ("qpc", "capped_at_51"), ("offsets_opposite",), ("segment_qpc_differs",)]
    if rare(cls):
        cells += [("held", c, hp, hq) for c in CAUSES for hp in (0, 1) for hq in (0, 1)]
        cells += [("held", "ordinary_in_pcmf_picture", hp, hp) for hp in (0, 1)]
        if kind == "chroma" and d == "V":
            cells += [("vpq", "p_only"), ("vpq", "q_only")]
    imp, exc = impossible(cls, kind, d), excluded(cls, kind, d)
    return [c for c in dict.fromkeys(cells) if c not in imp and c not in exc]
