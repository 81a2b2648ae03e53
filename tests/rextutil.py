"""Helpers of test_rext_residual.py / test_rext_residual_gpu.py: the census of the branches of the range-extension residual tools
(implicit RDPCM, transform-skip rotation, cross-component prediction, the reference's 16-bit arm, PCM) that corpus.rext_residual_sweep
and corpus.rext_residual_single_ctb_cases reach - computed from decode-order records and the reference decoder's reconstruction-stage
planes with residual_ref / intra_ref alone, never from the code under test - and what these corpora share: the case lists, the build
of the reference that holds each stage, the fingerprint of a set of planes."""
import collections

import numpy as np

import corpus
import intrautil as iu
import orc
import residual_ref as rr

DECODE_ORDER = iu.DECODE_ORDER
N_SWEEP = 1254  # 144 crossed cases + 54 of each of nine aimed families + 120 more of three of them + 108 at 8 bit + 156 of the tenth family
KINDS = ("luma", "chroma")
SIZES = (4, 8, 16, 32)
CTBS = (16, 32, 64)
CLASSES = tuple(f"{d}_rare_ctb{c}" for d in ("8bit", "deep") for c in CTBS)  # the six k_recon<Pix, log2 CTB, true> instances
STAGES = (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO, 0), ("deblock", orc.REF_F_NO_SAO, 1), ("full", 0, 3))
SKIPS = ("tskip", "bypass")
LUMA_KINDS = ("dst", "dct", "tskip", "bypass", "tskip_rdpcm", "bypass_rdpcm")
OWN_KINDS = ("none", "dct", "tskip", "bypass", "tskip_rdpcm", "bypass_rdpcm")


def kernel_class(P):
    return ("8bit" if P.bit_depth == 8 else "deep") + f"_rare_ctb{1 << P.log2_ctb}"


def corpora():
    """{name: [(seed, parameters)]} of the block-by-block corpora"""
    return dict(sweep=corpus.rext_residual_sweep(N_SWEEP), single=corpus.rext_residual_single_ctb_cases(), lock=corpus.rext_residual_lock_pictures())


def pcm_bits(kw):
    return (kw.get("pcm_bits_y", 8), kw.get("pcm_bits_c", 8)) if kw.get("pcm") else None


def default_build_holds(name, kw):
    """8-bit pictures of the "pcmf" deblocking branch (corpus.rext_pcmf8) with loop filters: the sweep's families of their own.  The one-CTB
    pictures have no loop filters and stay with the scalar build."""
    return name != "single" and corpus.rext_pcmf8(kw)


def ref_build(name, kw, stage_bits):
    """the flag of the reference's build that holds a picture of corpus `name` at a stage: its scalar build (an 8-bit 4x4 transform-skip block
    differs in the default one: Q10), but the default build from the deblocking stage on where default_build_holds()"""
    return 0 if (stage_bits and default_build_holds(name, kw)) else orc.REF_F_SCALAR


def fingerprint(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype(np.uint8)
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


def syntax_cells(P):
    """cells counted from the records alone, before the model runs: what the syntax (or the product's parser) promises never to send"""
    out = []
    last_luma = None
    for rec in P.records():
        if rec["cidx"] == 0:
            last_luma = rec
            continue
        scale = rec["qpy"] if (P.flags & rr.PIC_CROSS_COMPONENT) and not rec["pcm"] else 0
        if scale == 0:
            continue
        if P.chroma_format != 3:
            out.append((rec, ("ccp_syntax", "outside_444")))
        if scale not in rr.RES_SCALE_VALUES:
            out.append((rec, ("ccp_syntax", "no_power_of_two")))
        L = last_luma
        if L is None or (L["x"], L["y"], L["log2"]) != (rec["x"], rec["y"], rec["log2"]) or not L["cbf"] or L["pcm"]:
            out.append((rec, ("ccp_syntax", "luma_without_cbf")))
        elif L["tskip"] and not L["bypass"] and P.bit_depth == 8 and L["log2"] == 2:
            out.append((rec, ("ccp_syntax", "q17_unit")))
    return out


def cells_of(rec, ev):
    """the census cells one block counts in (ev: intra_ref.expected_block's events)"""
    t = ev["tools"]
    out = []
    own, ccp, pcm = t["own"], t["ccp"], t["pcm"]
    tooled = False
    if own is not None:
        k = own["kind"]
        if k in SKIPS:
            if own["rdpcm"]:
                tooled = True
                out.append(("rdpcm", f"{k}_{own['rdpcm']}"))
                if own["run_beyond_int16"]:
                    out.append(("rdpcm_beyond_int16", k))
                if own["rotated"]:
                    out.append(("rdpcm_rot", k))
            else:
                out.append(("plain", k))
                if own["rotated"]:
                    tooled = True
                    out.append(("rot", k))
        elif own["rotated"] or own["rdpcm"]:
            out.append(("transform", "rotated_or_rdpcm"))
        if own["rotated"] and rec["log2"] != 2:
            out.append(("rot", "not_4x4"))
        if own["res16"]:
            out.append(("res16", "arm"))
            if own["res16_acts"]:
                out.append(("res16", "acts"))
    if ccp is not None:
        tooled = True
        out.append(("ccp_scale", ccp["scale"]))
        out.append(("ccp_luma", rr.luma_kind(t["luma"])))
        out.append(("ccp_own", "none" if own is None else rr.luma_kind(own)))
        if ccp["neg_odd"]:
            out.append(("ccp", "neg_odd"))
        if ccp["wrap"]:
            out.append(("ccp", "wrap"))
        if ccp["res16_acts"]:
            out.append(("res16", "acts"))
    if pcm is not None:
        out.append(("pcm", "block"))
        if pcm["zero"]:
            out.append(("pcm", "zero"))
        if pcm["top"]:
            out.append(("pcm", "top"))
    if tooled:
        out += [("tool_rail", k) for k in ("lo", "hi") if ev["rail_" + k]]
    return out


class Census:
    """counts[(class, kind, nT, cell)] = blocks; blocks / observable: every record of the corpora, and those the model computed"""

    def __init__(self):
        self.counts = collections.Counter()
        self.blocks = self.observable = 0

    def count_syntax(self, cls, P):
        self.blocks += P.n_tus
        for rec, cell in syntax_cells(P):
            self.counts[(cls, "chroma", 1 << rec["log2"], cell)] += 1

    def noter(self, cls):
        def note(rec, ev):
            self.observable += 1
            key = (cls, "chroma" if rec["cidx"] else "luma", 1 << rec["log2"])
            for cell in cells_of(rec, ev):
                self.counts[key + (cell,)] += 1
        return note

    def seen(self, cls, kind, nT, cell):
        return self.counts.get((cls, kind, nT, cell), 0)

    def table(self):
        lines = [f"blocks {self.blocks}, observable {self.observable}", "class kind size cell: blocks"]
        for key in sorted(self.counts, key=str):
            cls, kind, nT, cell = key
            lines.append(f"{cls} {kind} {nT}x{nT} {cell[0]}={cell[1]}: {self.counts[key]}")
        return "\n".join(lines) + "\n"


# ---- what must be reached, what cannot occur, what the sweep leaves out -----------------------------------------------------
def exists(cls, kind, nT):
    """a transform block is at most 32x32 and no larger than its CTB (chroma 32x32: 4:4:4 with CTB 32 / 64)"""
    return nT <= int(cls.rsplit("ctb", 1)[1])


def all_cells():
    """the cross product of the events that the census counts: every cell that a block of any (class, kind, size) can count in.  required, impossible
    and excluded partition it for every (class, kind, size) that exists - test_the_branches_are_reached holds them to that"""
    cells = [("rdpcm", f"{k}_{d}") for k in SKIPS for d in "hv"] + [("plain", k) for k in SKIPS]
    cells += [("rot", k) for k in SKIPS] + [("rdpcm_rot", k) for k in SKIPS] + [("rot", "not_4x4"), ("transform", "rotated_or_rdpcm")]
    cells += [("rdpcm_beyond_int16", k) for k in SKIPS] + [("res16", "arm"), ("res16", "acts")]
    cells += [("tool_rail", k) for k in ("lo", "hi")] + [("pcm", k) for k in ("block", "zero", "top")]
    cells += [("ccp_scale", s) for s in rr.RES_SCALE_VALUES] + [("ccp_luma", k) for k in LUMA_KINDS] + [("ccp_own", k) for k in OWN_KINDS]
    cells += [("ccp", "neg_odd"), ("ccp", "wrap")] + [("ccp_syntax", k) for k in ("outside_444", "no_power_of_two", "luma_without_cbf", "q17_unit")]
    return cells


def impossible(cls, kind, nT):
    """{cell: reason} of the cells that cannot occur in (class, kind, size); asserted zero.  None: the size does not exist in the class."""
    if not exists(cls, kind, nT):
        return None
    deep = cls.startswith("deep")
    out = {("transform", "rotated_or_rdpcm"): "rotation and implicit RDPCM act on transform-skip and bypass blocks only (7.3.8.12, 8.6.2); explicit RDPCM is one of "
                                              "inter units (7.3.8.12: explicit_rdpcm_flag needs CuPredMode == MODE_INTER), and these are intra pictures",
           ("rot", "not_4x4"): "8.6.2: the rotation needs nTbS == 4",
           ("res16", "acts"): "the 16-bit arm holds 8-bit 4x4 transform-skip blocks: |element| <= (32767 << 7 + 2048) >> 12 = 1024, a run sum of four <= 4096; a chroma block's "
                              "cross-component term comes from a 4x4 luma block that is a DST block (|rY| <= 242 * 32768 >> 12 = 1936; a skip luma block there is a Q17 unit, "
                              "refused, and behind a bypass luma block the chroma block is bypass too), |8 * 1936 >> 3| = 1936: |sum| <= 6032 < 32768 - the int16 stores never "
                              "change a value"}
    if kind == "luma":
        for s in rr.RES_SCALE_VALUES:
            out[("ccp_scale", s)] = "7.3.8.12: cross_comp_pred( ) is one of the chroma components"
        for k in LUMA_KINDS:
            out[("ccp_luma", k)] = "a chroma cell"
        for k in OWN_KINDS:
            out[("ccp_own", k)] = "a chroma cell"
        out[("ccp", "neg_odd")] = out[("ccp", "wrap")] = "a chroma cell"
        for k in ("outside_444", "no_power_of_two", "luma_without_cbf", "q17_unit"):
            out[("ccp_syntax", k)] = "a chroma cell"
        if nT == 4:
            for k in ("block", "zero", "top"):
                out[("pcm", k)] = "a PCM coding unit is 8x8 at least (7.4.3.2.1: Log2MinIpcmCbSizeY >= 3), so its luma block is; 4x4 PCM blocks are chroma blocks of 4:2:0 / 4:2:2"
    else:
        for why, cell in (("7.3.8.12: a scale is sent in ChromaArrayType == 3 only", "outside_444"), ("7.4.9.12: ResScaleVal is +-(1 << 0 .. 3)", "no_power_of_two"),
                          ("7.3.8.12: a scale is sent only behind cbf_luma", "luma_without_cbf"),
                          ("Q17: the product's parser refuses a scale behind an 8-bit 4x4 transform-skip luma block", "q17_unit")):
            out[("ccp_syntax", cell)] = why
        if nT == 4:
            out[("ccp_luma", "dct")] = "a 4x4 luma block of an intra unit is a DST block"
            if not deep:
                out[("ccp_luma", "tskip")] = out[("ccp_luma", "tskip_rdpcm")] = "Q17 units: refused by the parser"
        else:
            out[("ccp_luma", "dst")] = "the DST is one of 4x4 luma blocks"
        if not deep or nT < 16:
            out[("ccp", "wrap")] = ("(rY << BitDepthC) wraps int32 for |rY| >= 2^(31 - BitDepthC): 2^23 at 8 bit, 2^21 at 10 bit, 2^19 at 12 bit (11 bit is not in these corpora). "
                                    "The largest |rY| is an RDPCM run sum: of bypass levels nT * 32767 (< 2^19 up to 16x16, < 2^20 at 32x32), of rounded transform-skip elements "
                                    "nT * ((32767 << (5 + log2)) >> (20 - BitDepth)) < 2^(2 log2 + BitDepth) - so the pair wraps at 12 bit alone, behind skip luma blocks of 16x16 "
                                    "and 32x32 and bypass luma blocks of 32x32")
    if nT > 4:
        for k in SKIPS:
            out[("rot", k)] = out[("rdpcm_rot", k)] = "8.6.2: the rotation needs nTbS == 4"
        out[("res16", "arm")] = "transform.cc:577: bit_depth == 8 && nT == 4"
    if deep:
        out[("res16", "arm")] = "transform.cc:577: bit_depth == 8 && nT == 4"
    if not deep and nT <= 8:
        out[("rdpcm_beyond_int16", "tskip")] = ("a rounded transform-skip element is at most (32767 << (5 + log2)) >> (20 - BitDepth) < 2^(log2 + BitDepth): a run of nT of them "
                                                "stays below 2^(2 log2 + BitDepth) <= 2^14 at 8 bit up to 8x8")
    return {k: v for k, v in out.items() if v}


def excluded(cls, kind, nT):
    """{cell: reason} of cells that the standard allows but that are zero by a choice of these corpora or of the synthesiser; asserted zero too"""
    return {}  # (nothing: every cell that can occur in these corpora is required or reported)


def required(cls, kind, nT):
    """the cells that must be non-zero in (class, kind, size): every cell of the cross product that is neither impossible nor excluded"""
    imp = impossible(cls, kind, nT)
    if imp is None:
        return []
    exc = excluded(cls, kind, nT)
    return [c for c in all_cells() if c not in imp and c not in exc]
