"""Helper of test_chain_modes_gpu.py (run as a script, a process per set of tuning / fault-injection knobs, which the
script takes from its environment and sets through the library's test hook): reconstruct a few corpus pictures on the GPU and compare with the oracle.
Prints OK, or the first difference; exit status 0 / 1; 3 = hm_batch_check reported a wave that gave up.

Besides corpus names and the special pictures below, the arguments may name a SET of corpus pictures: `structure` (several slices,
dependent segments, tiles, WPP with slices, conformance windows - the non-rare structure cases and the 512 x 512 tiles with
structure), `rare512` (the rare-syntax 512 x 512 tiles); `extreme_sweep`, `extreme512`, `extreme_large` are the pictures of
corpus.extreme_sweep / extreme_tiles / extreme_large; every picture of `extreme_sweep` is also held against the fingerprints of the
reference's scalar build (tests/golden/extreme.json); `intra512` are the tiles of corpus.intra_tiles.  A picture of the corpus is also held against the reference decoder's
fingerprint of it (tests/golden/synth.json) at stages 0, 1 and 3.  More variables of the environment:
  HM_CHECK_COPIES    copies of every picture in its batch (default 3)
  HM_CHECK_STAGES    the stages to run, comma-separated (default 3)
  HM_CHECK_EXECUTES  executes of the one uploaded batch, every output compared each time (default 1)
  HM_CHECK_ORDER     record order of the parser (HM_RECORDS_*; default: the parser's own choice)
  HM_CHECK_CUTS      a JSON list of knob settings ({"chain_ring": 4, ...}): the whole check once per entry, in one process, the
                     cut knobs back at their defaults in between; "[check] cut <n> <settings>" goes to stderr before entry n
and "[check] <name> stages <s>" before every decode: the launchers' HM_CHAIN_DEBUG lines of that decode follow it."""
import json
import os
import sys

import numpy as np

import __graft_entry__ as g
import corpus
import gpudecode
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
SYNTH = json.load(open(os.path.join(HERE, "golden", "synth.json")))
EXTREME = json.load(open(os.path.join(HERE, "golden", "extreme.json")))["cases"]  # corpus.extreme_sweep: the reference's scalar build
STAGE_NAMES = {0: "recon", 1: "deblock", 3: "full"}

TILE512_STRUCTURE = ["tile512_slices", "tile512_slices_dependent_nolf", "tile512_tiles_uniform_slices", "tile512_tiles_explicit_slices",
                     "tile512_wpp_slices", "tile512_422_10_ctb64_tiles", "tile512_mono_ctb16_slices"]
RARE512 = ["tile512_rare", "tile512_rare_422_10_slices"]
# the pictures with structure that take the split chains: every slices* / tiles_* / wpp_* / conf_window* case but the one with
# 4:4:4 and PCM (rare syntax: k_recon), the CU chroma QP offsets with slices, and the 512 x 512 tiles above
STRUCTURE = sorted(n for n in corpus.CASES if (n.split("_")[0] in ("slices", "tiles", "wpp") or n.startswith("conf_window"))
                   and n != "slices_444_pcm") + ["rext_chroma_qp_list"] + TILE512_STRUCTURE
SETS = {"structure": STRUCTURE, "rare512": RARE512}
# the cut knobs and their defaults (csrc/common.cpp), set again before every entry of HM_CHECK_CUTS
CUT_DEFAULTS = {"chain_pairs": -1, "chain_share": 0, "chain_ring": -1, "chain_alt": 1, "chain_np": 0, "resid_segs": 0, "recon_waves": 0,
                "chain_early": 1}


def main():
    import knobs
    pkg = g.load_package(test_knobs="always" if os.environ.get("HM_CHECK_CUTS") else True)
    # the cuts and the fault-injection knobs are library test hooks (hm_debug_set), not environment variables of the product: the
    # test hands them to this script through the environment and load_package(test_knobs=True) sets them (tests/knobs.py)
    hm = pkg.lib()
    names = []
    for a in sys.argv[1:] or ["tile512_a", "ctb64_wpp", "hi422_10", "mono8", "ragged"]:
        names += SETS.get(a, [a])
    copies = int(os.environ.get("HM_CHECK_COPIES", "3"))  # (hundreds: the cuts the launcher chooses for mid-size batches)
    stages_list = [int(s) for s in os.environ.get("HM_CHECK_STAGES", "3").split(",")]
    executes = int(os.environ.get("HM_CHECK_EXECUTES", "1"))
    order = os.environ.get("HM_CHECK_ORDER")
    cuts = json.loads(os.environ["HM_CHECK_CUTS"]) if os.environ.get("HM_CHECK_CUTS") else [None]
    env_knobs = knobs.apply_env(hm) if cuts != [None] else {}  # (what the environment set: the base of every entry)

    def parse(data):
        blob = pkg.capi.parse_hevc(data) if order is None else pkg.capi.parse_hevc(data, record_order=int(order))
        if order == "2":
            assert not pkg.capi.stream_header(blob)["flags"] & 0x1000, "HM_PIC_SPLIT_CHAINS in a decode-order record stream"
        return blob

    batches = {}  # name -> the batch's blobs (one parse per picture for all entries)
    for name in names:
        if name == "wide16k":  # the widest picture class: CTB 64, 16-bit storage, 4:2:2, 16384 columns, two CTU rows
            import synthutil
            batches[name] = [parse(synthutil.picture(515151, width=16384, height=128, log2_ctb=6, bit_depth=10, chroma_format=2, qp=32, density=30))] * copies
        elif name == "big422":  # BASELINE config 4's picture: 2048x1536 10-bit 4:2:2, 48 rows of 64 CTUs - a long wavefront
            import synthutil
            batches[name] = [parse(synthutil.picture(4220010, width=2048, height=1536, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30, vui=1,
                                                     full_range=0, matrix=9, primaries=9))] * copies
        elif name == "mono10_wide":  # 16-bit monochrome, CTBs of 32, 512 columns: luma of four rows per wave = 15 KB of LDS
            import synthutil
            batches[name] = [parse(synthutil.picture(4001032, width=512, height=192, chroma_format=0, bit_depth=10, log2_ctb=5, qp=30))] * copies
        elif name == "rare_sweep":  # PCM / transquant bypass / scaling lists of every chroma format, depth and CTB size (k_recon with rare syntax)
            import synthutil
            batches[name] = [parse(synthutil.picture(seed, **kw)) for seed, kw in corpus.rare_syntax_sweep(48)]
        elif name == "structure_sweep":  # slices, tiles, WPP of every chroma format, depth and CTB size in one batch
            import synthutil
            batches[name] = [parse(synthutil.picture(seed, **kw)) for seed, kw in corpus.structure_sweep(64)]
        elif name in ("extreme_sweep", "extreme512", "extreme_large"):  # levels / QPs / scaling factors at the edges of the residual arithmetic
            import synthutil
            cases = {"extreme_sweep": lambda: corpus.extreme_sweep(len(EXTREME)), "extreme512": corpus.extreme_tiles, "extreme_large": corpus.extreme_large}[name]()
            batches[name] = [parse(synthutil.picture(seed, **kw)) for seed, kw in cases] * (1 if name == "extreme_sweep" else copies)
        elif name == "intra512":  # corpus.intra_tiles: half of the coding units calm - smooth borders cross every cut
            import synthutil
            batches[name] = [parse(synthutil.picture(seed, **kw)) for seed, kw in corpus.intra_tiles()] * copies
        elif name == "mixed":  # pictures of one class and different sizes in one launch (the cut follows the tallest; short ones leave waves idle)
            batches[name] = [parse(corpus.stream(n)) for n in ("tile512_a", "ragged", "dense_lowqp", "no_deblock", "tile512_b", "ragged")] * 2
        elif name == "mixed_structure":  # ... the same with slices, dependent segments, tiles and WPP with slices (8-bit 4:2:0, CTB 32)
            batches[name] = [parse(corpus.stream(n)) for n in ("tile512_slices", "slices", "tiles_3x2_nolf", "tile512_tiles_explicit_slices", "ragged",
                                                               "wpp_slices_dependent", "tile512_wpp_slices", "slices_headers", "tiles_explicit_slices",
                                                               "tile512_slices_dependent_nolf")] * 2
        else:
            batches[name] = [parse(corpus.stream(name))] * copies
    expected = {}  # (id of a blob, stages) -> the oracle's planes

    for n_cut, cut in enumerate(cuts):
        tag = ""
        if cut is not None:
            for k, v in {**CUT_DEFAULTS, **env_knobs, **cut}.items():
                knobs.set_knob(hm, k, v)
            tag = f"cut {n_cut} {json.dumps(cut, sort_keys=True)}: "
            print(f"[check] cut {n_cut} {json.dumps(cut, sort_keys=True)}", file=sys.stderr, flush=True)
        for name, blobs in batches.items():
            for stages in stages_list:
                print(f"[check] {name} stages {stages}", file=sys.stderr, flush=True)
                try:
                    runs = gpudecode.decode_pictures_repeatedly(pkg, blobs, stages, executes)
                except RuntimeError as e:
                    print(f"{tag}{name}: CHECK FAILED:", e)
                    return 3
                for k, got in enumerate(runs):
                    for i, pic in enumerate(got):
                        key = (id(blobs[i]), stages)
                        if key not in expected:
                            expected[key] = orc.oracle_decode(blobs[i], stages, crop=True)[0]
                        exp = expected[key]
                        if len(pic) != len(exp):
                            print(f"{tag}{name}: stages {stages}, execute {k}, picture {i}: {len(pic)} planes, the oracle {len(exp)}")
                            return 1
                        for c in range(len(exp)):
                            if not np.array_equal(pic[c], exp[c]):
                                bad = np.argwhere(pic[c] != exp[c])
                                print(f"{tag}{name}: stages {stages}, execute {k}, picture {i} plane {c} differs ({len(bad)} samples, first (y,x)={bad[0].tolist()})")
                                return 1
                # one picture of the corpus against the reference decoder's fingerprint (the oracle is held against it by the CPU suite)
                if name in corpus.CASES and stages in STAGE_NAMES and fingerprint(runs[0][0]) != SYNTH[name][STAGE_NAMES[stages]]:
                    print(f"{tag}{name}: stages {stages}: not the reference decoder's fingerprint")
                    return 1
                # every picture of the extreme sweep against the fingerprint of the reference's scalar build - in whatever record order
                # HM_CHECK_ORDER forced, which the CPU suite's comparison of parser + oracle with the reference does not cover
                if name == "extreme_sweep" and stages in STAGE_NAMES:
                    for (seed, _), pic in zip(corpus.extreme_sweep(len(EXTREME)), runs[0]):
                        if fingerprint(pic) != EXTREME[str(seed)][STAGE_NAMES[stages]]:
                            print(f"{tag}{name}: stages {stages}: seed {seed}: not the fingerprint of the reference's scalar build")
                            return 1
    print("OK")
    return 0


def fingerprint(planes):
    h = 0
    for p in planes:
        a = p if p.max() > 255 else p.astype(np.uint8)
        buf = a.tobytes()
        h = orc.load().orc_fnv1a64(buf, len(buf), h)
    return f"{h:016x}"


if __name__ == "__main__":
    sys.exit(main())
