"""Generate the committed test fixtures.  Runs only in the build container (needs /root/reference
and the reference decoder build oracle/_ref):

  tests/data/*.hevc         coded pictures as [u32 BE length][NAL] records (what a libheif decoder
                            plugin receives through push_data) - DATA files taken from the
                            reference's own test material, re-framed, never source code
  tests/golden/decode.json  FNV-1a-64 fingerprints of the planes the REAL reference decoder
                            (libde265, oracle/_ref) produces for each fixture, per stage
  tests/golden/extreme.json (a plain run rewrites it with the others; `make_fixtures.py extreme` writes this file alone) the same fingerprints of the reference's
                            SCALAR build for corpus.extreme_sweep - levels, QPs and scaling factors at the edges of the
                            residual arithmetic -, and beside them where its default (SIMD) build decodes otherwise
  tests/golden/intra.json   (`make_fixtures.py intra` writes it, and only that sub-command) the same for corpus.intra_sweep
  tests/golden/deblock.json (`make_fixtures.py deblock`, and only that sub-command) fingerprints of the reconstruction and deblocking stages for
                            corpus.deblock_sweep / deblock_single_edge_cases / deblock_tiles: the reference's scalar build, and its default build for
                            8-bit pictures of the "pcmf" branch; with it profiles/deblock_census.txt, the census of tests/deblockutil.py
  tests/golden/sao.json     (`make_fixtures.py sao`, and only that sub-command) fingerprints of all four stages (none, deblocking, SAO alone, both) for
                            corpus.sao_sweep / sao_small_cases / sao_tiles: the reference's scalar build, its default build for 8-bit pictures of the
                            "pcmf" branch; with it profiles/sao_census.txt, the census of tests/saoutil.py
  tests/golden/rext_residual.json (`make_fixtures.py rext`, and only that sub-command) fingerprints of the three stages for corpus.rext_residual_sweep /
                            rext_residual_single_ctb_cases / rext_residual_lock_pictures / rext_residual_tiles: the reference's scalar build, its default build from
                            the deblocking stage on for 8-bit pictures of the "pcmf" branch, and which pictures its builds decode differently at the
                            reconstruction stage; with it profiles/rext_residual_census.txt, the census of tests/rextutil.py (the model must reproduce
                            the reference's planes block by block: asserted)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402

REF = "/root/reference"


def annexb_to_lp(data):
    out = bytearray()
    i = 0
    n = len(data)
    starts = []
    while i + 3 <= n:
        if data[i] == 0 and data[i + 1] == 0 and data[i + 2] == 1:
            starts.append(i + 3)
            i += 3
        else:
            i += 1
    for k, s in enumerate(starts):
        e = (starts[k + 1] - 3) if k + 1 < len(starts) else n
        while e > s and data[e - 1] == 0:
            e -= 1
        nal = data[s:e]
        out += len(nal).to_bytes(4, "big") + nal
    return bytes(out)


def fingerprint(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype("uint8")
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


def main():
    os.makedirs(os.path.join(ROOT, "tests", "data"), exist_ok=True)
    golden = {}
    srcs = {
        "basketball_1080p_qp32": f"{REF}/third-party/libde265/testfile/BasketballDrive_1920x1080_32.265",
        "basketball_1080p_qp25": f"{REF}/third-party/libde265/testfile/BasketballDrive_1920x1080_25.265",
        "basketball_1080p_qp1": f"{REF}/third-party/libde265/testfile/BasketballDrive_1920x1080_1.265",
    }
    for name, path in srcs.items():
        lp = annexb_to_lp(open(path, "rb").read())
        open(os.path.join(ROOT, "tests", "data", name + ".hevc"), "wb").write(lp)
        entry = {"source": os.path.relpath(path, REF), "bytes": len(lp)}
        for stage, flags in (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO), ("deblock", orc.REF_F_NO_SAO), ("full", 0)):
            planes, info = orc.ref_decode(lp, flags)
            entry[stage] = fingerprint(planes)
            entry["width"], entry["height"] = int(planes[0].shape[1]), int(planes[0].shape[0])
            entry["info"] = info
        golden[name] = entry
        print(name, entry)
    json.dump(golden, open(os.path.join(ROOT, "tests", "golden", "decode.json"), "w"), indent=1, sort_keys=True)

    # synthetic corpus: blessed by the reference decoder (SIMD build = the oracle configuration, and
    # its scalar build must agree - the two differ for 8-bit SAO on 8-sample-wide chroma CTBs, which
    # the corpus therefore avoids)
    import corpus
    synth = {}
    for name in sorted(corpus.CASES):
        data = corpus.stream(name)
        entry = {"bytes": len(data), "stream_fnv": f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}"}
        for stage, flags in (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO), ("deblock", orc.REF_F_NO_SAO), ("full", 0)):
            planes, info = orc.ref_decode(data, flags)
            if name not in corpus.SIMD_BUILD_ONLY:
                scalar, _ = orc.ref_decode(data, flags | orc.REF_F_SCALAR)
                assert all((a == b).all() for a, b in zip(planes, scalar)), f"{name}: reference SIMD != scalar"
            entry[stage] = fingerprint(planes)
        entry["width"], entry["height"] = int(planes[0].shape[1]), int(planes[0].shape[0])
        entry["info"] = info
        synth[name] = entry
        print(name, entry["bytes"], entry["full"])
    json.dump(synth, open(os.path.join(ROOT, "tests", "golden", "synth.json"), "w"), indent=1, sort_keys=True)


EXTREME_CASES = 144


def extreme():
    """corpus.extreme_sweep: fingerprints of the reference's scalar build at the three stages; and, at the reconstruction
    stage, in which plane and block class its default build differs (every class is a quirk of DESIGN.md 3)"""
    import collections
    import numpy as np
    import corpus
    import residual_ref as rr
    import synthutil
    import __graft_entry__ as g
    capi = g.load_package().capi
    cases, classes, differing = {}, collections.Counter(), []
    for seed, kw in corpus.extreme_sweep(EXTREME_CASES):
        data = synthutil.picture(seed, **kw)
        entry = {"bytes": len(data), "stream_fnv": f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}"}
        for stage, flags in (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO), ("deblock", orc.REF_F_NO_SAO), ("full", 0)):
            planes, _ = orc.ref_decode(data, flags | orc.REF_F_SCALAR)
            entry[stage] = fingerprint(planes)
            if stage == "recon":
                simd, _ = orc.ref_decode(data, flags)
                if any(not np.array_equal(a, b) for a, b in zip(simd, planes)):
                    differing.append(seed)
                    P = rr.Picture(capi.parse_hevc(data, record_order=2))
                    origin = set()
                    for rec in P.records():  # per plane, the first block in decode order in which a sample differs (later ones may inherit it through prediction)
                        if rec["cidx"] in origin:
                            continue
                        nT = 1 << rec["log2"]
                        a, b = (p[rec["cidx"]][rec["y"]:rec["y"] + nT, rec["x"]:rec["x"] + nT] for p in (simd, planes))
                        if not np.array_equal(a, b):
                            kind = "pcm" if rec["pcm"] else "no residual" if not rec["cbf"] else "bypass" if rec["bypass"] else \
                                "transform skip" if rec["tskip"] else "DST" if nT == 4 and rec["cidx"] == 0 else "DCT"
                            origin.add(rec["cidx"])
                            classes[f"{P.bit_depth}-bit plane {rec['cidx']} {nT}x{nT} {kind}"] += 1
        cases[str(seed)] = entry
    out = {"cases": cases,
           "simd_vs_scalar": {"stage": "recon", "cases": len(cases), "cases_that_differ": len(differing), "seeds": differing,
                              "blocks_that_differ_by_class": dict(sorted(classes.items()))}}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "extreme.json"), "w"), indent=1, sort_keys=True)
    print("extreme:", len(cases), "cases;", len(differing), "decoded differently by the default build:", dict(sorted(classes.items())))


INTRA_CASES = 1104


def intra():
    """corpus.intra_sweep: fingerprints of the reference's scalar build at the three stages (level_span is in play: DESIGN.md
    Q10); and, at the reconstruction stage, the class of the first block per plane in which its default build differs"""
    import collections
    import numpy as np
    import corpus
    import residual_ref as rr
    import synthutil
    import __graft_entry__ as g
    capi = g.load_package().capi
    cases, classes, differing = {}, collections.Counter(), []
    for seed, kw in corpus.intra_sweep(INTRA_CASES):
        data = synthutil.picture(seed, **kw)
        entry = {"stream_fnv": f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}"}
        for stage, flags in (("recon", orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO), ("deblock", orc.REF_F_NO_SAO), ("full", 0)):
            planes, _ = orc.ref_decode(data, flags | orc.REF_F_SCALAR)
            entry[stage] = fingerprint(planes)
            if stage == "recon":
                simd, _ = orc.ref_decode(data, flags)
                if any(not np.array_equal(a, b) for a, b in zip(simd, planes)):
                    differing.append(seed)
                    P = rr.Picture(capi.parse_hevc(data, record_order=2))
                    origin = set()
                    for rec in P.records():  # per plane, the first block in decode order in which a sample differs
                        nT = 1 << rec["log2"]
                        a, b = (p[rec["cidx"]][rec["y"]:rec["y"] + nT, rec["x"]:rec["x"] + nT] for p in (simd, planes))
                        if rec["cidx"] not in origin and not np.array_equal(a, b):
                            origin.add(rec["cidx"])
                            kind = "pcm" if rec["pcm"] else "no residual" if not rec["cbf"] else "bypass" if rec["bypass"] else \
                                "transform skip" if rec["tskip"] else "DST" if nT == 4 and rec["cidx"] == 0 else "DCT"
                            classes[f"level_span {kw['level_span']}: {kind}"] += 1
        cases[str(seed)] = entry
    out = {"cases": cases,
           "simd_vs_scalar": {"stage": "recon", "cases": len(cases), "cases_that_differ": len(differing), "seeds": differing,
                              "first_blocks_that_differ_by_class": dict(sorted(classes.items()))}}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "intra.json"), "w"), indent=0, sort_keys=True, separators=(",", ":"))
    print("intra:", len(cases), "cases;", len(differing), "decoded differently by the default build:", dict(sorted(classes.items())))


DEBLOCK_SWEEP_CASES = 1488


def deblock():
    """the three deblocking corpora: fingerprints of the reference decoder at the reconstruction and deblocking stages, and the census of the
    filter's decisions taken with tests/deblock_ref.py on the reference's planes (the model must reproduce them: asserted)"""
    import corpus
    import deblockutil as du
    import residual_ref as rr
    import synthutil
    import __graft_entry__ as g
    capi = g.load_package().capi
    cases, C = {}, du.Census()
    todo = corpus.deblock_sweep(DEBLOCK_SWEEP_CASES) + corpus.deblock_single_edge_cases() + corpus.deblock_tiles()
    for seed, kw in todo:
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(capi.parse_hevc(data, record_order=du.DECODE_ORDER))
        pcmf8 = P.bit_depth == 8 and bool(P.flags & rr.PIC_PCMF)
        build = 0 if pcmf8 else orc.REF_F_SCALAR
        before, _ = orc.ref_decode(data, orc.REF_F_NO_DEBLOCK | orc.REF_F_NO_SAO | build)
        after, _ = orc.ref_decode(data, orc.REF_F_NO_SAO | build)
        bad = du.first_mismatch(seed, P, before, after, du.quirks_for(default_build=pcmf8), C.noter(du.kernel_class(P.flags, P.bit_depth), P))
        assert bad is None, bad
        assert str(seed) not in cases
        cases[str(seed)] = {"stream_fnv": f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}", "recon": fingerprint(before), "deblock": fingerprint(after)}
    json.dump({"sweep_cases": DEBLOCK_SWEEP_CASES, "cases": cases}, open(os.path.join(ROOT, "tests", "golden", "deblock.json"), "w"), indent=0, sort_keys=True,
              separators=(",", ":"))
    open(os.path.join(ROOT, "profiles", "deblock_census.txt"), "w").write(C.table())
    print("deblock:", len(cases), "pictures,", C.units, "units on the grid")


SAO_SWEEP_CASES = 660


def sao():
    """the three SAO corpora: fingerprints of the reference decoder at all four stages, and the census of the branches of sample adaptive offset taken with
    tests/sao_ref.py on the reference's planes (the model must reproduce them: asserted)"""
    import corpus
    import residual_ref as rr
    import saoutil as su
    import synthutil
    import __graft_entry__ as g
    capi = g.load_package().capi
    cases, C = {}, su.Census()
    for seed, kw in corpus.sao_sweep(SAO_SWEEP_CASES) + corpus.sao_small_cases() + corpus.sao_tiles():
        data = synthutil.picture(seed, **kw)
        P = rr.Picture(capi.parse_hevc(data, record_order=su.DECODE_ORDER))
        assert str(seed) not in cases
        cases[str(seed)] = dict(su.hold_picture(seed, kw, data, P, C), stream_fnv=f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}")
    json.dump({"sweep_cases": SAO_SWEEP_CASES, "cases": cases}, open(os.path.join(ROOT, "tests", "golden", "sao.json"), "w"), indent=0, sort_keys=True,
              separators=(",", ":"))
    open(os.path.join(ROOT, "profiles", "sao_census.txt"), "w").write(C.table())
    missing = [(cls, kind, pair) + cell for cls in su.CLASSES for kind in su.KINDS for pair in su.PAIRS for cell in su.required(cls, kind, pair)
               if not C.seen(cls, kind, pair, cell)]
    print("sao:", len(cases), "pictures,", C.samples, "samples; required cells still empty:", missing)


def rext():
    """the range-extension residual corpora: fingerprints of the reference decoder at the three stages, which pictures its default build reconstructs otherwise
    (the class of the first differing block per plane), and the census of tests/rextutil.py taken with residual_ref / intra_ref on the reference's planes"""
    import collections
    import numpy as np
    import corpus
    import intrautil as iu
    import residual_ref as rr
    import rextutil as xu
    import synthutil
    import __graft_entry__ as g
    capi = g.load_package().capi
    cases, C, classes, differing = {}, xu.Census(), collections.Counter(), []
    todo = dict(xu.corpora(), tiles=corpus.rext_residual_tiles())
    for name, lst in todo.items():
        for seed, kw in lst:
            data = synthutil.picture(seed, **kw)
            P = rr.Picture(capi.parse_hevc(data, record_order=xu.DECODE_ORDER))
            assert str(seed) not in cases
            entry = {"stream_fnv": f"{orc.load().orc_fnv1a64(data, len(data), 0):016x}"}
            for stage, flags, bits in xu.STAGES:
                planes, _ = orc.ref_decode(data, flags | xu.ref_build(name, kw, bits))
                entry[stage] = fingerprint(planes)
                if bits:
                    continue
                if name != "tiles":
                    cls = xu.kernel_class(P)
                    C.count_syntax(cls, P)
                    bad = iu.first_mismatch(seed, P, planes, tools_note=C.noter(cls), pcm_bits=xu.pcm_bits(kw))
                    assert bad is None, f"{kw}: the model is not the reference decoder: {bad}"
                simd, _ = orc.ref_decode(data, flags)
                if any(not np.array_equal(a, b) for a, b in zip(simd, planes)):
                    assert not xu.default_build_holds(name, kw), f"seed {seed} {kw}: a picture held to the default build differs from the scalar one at the reconstruction stage"
                    differing.append(seed)
                    origin = set()
                    for rec in P.records():  # per plane, the first block in decode order in which a sample differs
                        nT = 1 << rec["log2"]
                        a, b = (p[rec["cidx"]][rec["y"]:rec["y"] + nT, rec["x"]:rec["x"] + nT] for p in (simd, planes))
                        if rec["cidx"] not in origin and not np.array_equal(a, b):
                            origin.add(rec["cidx"])
                            kind = "pcm" if rec["pcm"] else "no residual" if not rec["cbf"] else "bypass" if rec["bypass"] else \
                                "transform skip" if rec["tskip"] else "DST" if nT == 4 and rec["cidx"] == 0 else "DCT"
                            classes[f"{P.bit_depth}-bit {nT}x{nT} {kind}"] += 1
            cases[str(seed)] = entry
    out = {"sweep_cases": xu.N_SWEEP, "cases": cases,
           "simd_vs_scalar": {"stage": "recon", "cases": len(cases), "cases_that_differ": len(differing), "seeds": differing,
                              "first_blocks_that_differ_by_class": dict(sorted(classes.items()))}}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "rext_residual.json"), "w"), indent=0, sort_keys=True, separators=(",", ":"))
    open(os.path.join(ROOT, "profiles", "rext_residual_census.txt"), "w").write(C.table())
    missing = [(cls, kind, nT) + cell for cls in xu.CLASSES for kind in xu.KINDS for nT in xu.SIZES for cell in xu.required(cls, kind, nT) if not C.seen(cls, kind, nT, cell)]
    print("rext:", len(cases), "pictures,", C.blocks, "blocks;", len(differing), "decoded differently by the default build:", dict(sorted(classes.items())),
          "; required cells still empty:", missing)


if __name__ == "__main__":
    if sys.argv[1:] == ["rext"]:
        sys.path.insert(0, ROOT)
        rext()
    elif sys.argv[1:] == ["sao"]:
        sys.path.insert(0, ROOT)
        sao()
    elif sys.argv[1:] == ["deblock"]:
        sys.path.insert(0, ROOT)
        deblock()
    elif sys.argv[1:] == ["extreme"]:
        sys.path.insert(0, ROOT)
        extreme()
    elif sys.argv[1:] == ["intra"]:
        sys.path.insert(0, ROOT)
        intra()
    else:
        main()
        sys.path.insert(0, ROOT)
        extreme()
