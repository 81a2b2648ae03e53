"""CPU: error behaviour of the host side (no GPU needed): malformed HEIF / HEVC input must produce an
error status (never a crash), invalid grids report the reference's error conditions
(context.cc:2142-2153, 2321-2337), and without a GPU the decode entry points fail loudly
(HM_ERR_NO_DEVICE) instead of falling back to a CPU path."""
import ctypes as C
import os
import random
import struct

import pytest

import corpus
import heifwriter
import hevcutil
import pipeline

HERE = os.path.dirname(os.path.abspath(__file__))


def _tiles(n, **kw):
    import synthutil
    return [synthutil.picture(300 + i, width=64, height=64, **kw) for i in range(n)]


def test_truncated_and_corrupted_hevc_never_crashes(hm):
    rng = random.Random(1234)
    base = [corpus.stream(n) for n in ("tiny", "ragged", "ctb64_wpp", "hi422_10", "pcm_nofilter", "pcm_bypass_sl_wpp", "sl_pps_422_10")]
    ok = err = 0
    for data in base:
        for _ in range(150):
            b = bytearray(data)
            mode = rng.randrange(4)
            if mode == 0:
                b = b[:rng.randrange(1, len(b))]
            elif mode == 1:
                for _ in range(rng.randrange(1, 6)):
                    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            elif mode == 2:
                i = rng.randrange(len(b))
                b[i:i + rng.randrange(1, 16)] = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 16)))
            else:
                b += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 64)))
            try:
                hevcutil.parse(hm, bytes(b))
                ok += 1
            except RuntimeError:
                err += 1
    assert ok + err == 150 * len(base) and err > 100


def test_damaged_slice_data_is_accepted_only_where_the_reference_is_defined(hm):
    """1-2 bit flips in the slice data (the classes of tools/fuzz_ref.py).  The parser takes a damaged slice exactly when what
    the reference decodes from it is defined by the data: every CTB parsed from bits inside the slice data, a missing
    end_of_slice_segment_flag at the picture's last CTB included (slice.cc:5107-5115: a warning, the picture kept).  Every
    accepted stream must give the reference's picture (oracle/_ref where it is built); the others fail with HM_ERR_BITSTREAM."""
    import numpy as np
    import orc
    rng = random.Random(5)
    accepted = refused = 0
    for name in ("ragged", "ctb64_wpp", "hi420_10", "slices_headers", "dense_lowqp"):
        data = corpus.stream(name)
        for _ in range(40):
            b = bytearray(data)
            for _ in range(rng.randrange(1, 3)):
                b[rng.randrange(len(data) // 3, len(b))] ^= 1 << rng.randrange(8)
            b = bytes(b)
            try:
                blob = hevcutil.parse(hm, b)
            except RuntimeError as e:
                refused += 1
                assert "failed: -3:" in str(e) or "failed: -2:" in str(e), e  # HM_ERR_BITSTREAM (a flipped header bit may also name unsupported syntax)
                continue
            accepted += 1
            if orc.have_ref():
                mine, _ = orc.oracle_decode(blob, 3, crop=True)
                try:
                    ref, _ = orc.ref_decode(b, 0)
                except RuntimeError:
                    continue  # (the reference refuses what this parser takes: a damaged header field it checks and the product does not need)
                assert len(mine) == len(ref) and all(np.array_equal(m, r) for m, r in zip(mine, ref)), f"{name}: accepted damaged stream decodes differently"
    assert accepted >= 15 and refused >= 40, (accepted, refused)


def _ctb_grid(blob):
    import struct
    w, h = struct.unpack_from("<HH", blob, 8)
    crop = struct.unpack_from("<4H", blob, 12)
    ctb = 1 << blob[23]
    return w, h, crop, ctb, (w + ctb - 1) // ctb, (h + ctb - 1) // ctb


def _assert_ctbs_equal_reference(blob, mine, ref, ctbs, what):
    """the luma samples of the CTBs `ctbs` (raster addresses) of the oracle's picture `mine` (whole coded picture) against the
    reference decoder's (conformance window)"""
    import numpy as np
    w, h, (cl, cr, ct, cb), ctb, ctb_w, ctb_h = _ctb_grid(blob)
    for c in ctbs:
        x0, y0 = (c % ctb_w) * ctb, (c // ctb_w) * ctb
        x1, y1 = min(x0 + ctb, w - cr), min(y0 + ctb, h - cb)
        x0, y0 = max(x0, cl), max(y0, ct)
        if x1 <= x0 or y1 <= y0:
            continue
        assert np.array_equal(mine[0][y0:y1, x0:x1], ref[0][y0 - ct:y1 - ct, x0 - cl:x1 - cl]), f"{what}: CTB {c} differs from the reference"


def test_damaged_slice_data_is_concealed_like_the_reference_keeps_the_picture(hm):
    """HM_PARSE_CONCEAL (r05; VERDICT r04 "missing" 2).  The reference hands out a picture whose slice data is damaged (libde265
    marks the slice as processed, decctx.cc:876-995; the plugin returns the picture, decoder_libde265.cc:311-336) - the CTBs it
    could not decode hold whatever its image memory held.  The product, asked to conceal, decodes every CTB in front of the damage
    exactly and writes the rest as plain intra CTUs; without the option it refuses the stream as before.  Two kinds of damage
    whose effect on the reference is deterministic:
      * a LOST slice (its NAL dropped) of a picture of many slices: every CTB that is not the lost slice's, nor next to one of
        them (the loop filters reach across), equals the real libde265's;
      * a TRUNCATED last slice: the CTBs up to one CTB row + 2 in front of the first concealed one equal the reference's."""
    import numpy as np
    import orc
    import synthutil
    # 16 x 12 CTBs of 16 x 16 in a dozen or more independent slices with their own filter switches
    data = bytes(synthutil.picture(6100077, width=256, height=192, log2_ctb=4, slices=120, slice_lf_random=1, deblock_override=1, slice_sao_random=1, slice_qp_random=1))
    nals = hevcutil.split_nals(data)
    vcl = [i for i, n in enumerate(nals) if ((n[0] >> 1) & 0x3F) <= 21]
    assert len(vcl) >= 6, len(vcl)
    intact = hevcutil.parse(hm, data)
    w, h, crop, ctb, ctb_w, ctb_h = _ctb_grid(intact)
    # ---- a lost slice in the middle of the picture ----
    for k in (len(vcl) // 3, len(vcl) // 2):
        damaged = hevcutil.join_nals([n for i, n in enumerate(nals) if i != vcl[k]])
        with pytest.raises(RuntimeError):
            hevcutil.parse(hm, damaged)
        blob, n_conc, first = hevcutil.parse_concealing(hm, damaged)
        assert n_conc > 0 and first >= 0
        import struct
        assert struct.unpack_from("<I", blob, 48)[0] == ctb_w * ctb_h  # hm_pic.n_ctbs: the whole picture
        mine, _ = orc.oracle_decode(blob, 3)
        if orc.have_ref():
            ref, _ = orc.ref_decode(damaged, 0)
            lost = set(range(first, first + n_conc))  # (one gap: consecutive CTBs)
            near = set()
            for c in lost:
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        x, y = c % ctb_w + dx, c // ctb_w + dy
                        if 0 <= x < ctb_w and 0 <= y < ctb_h:
                            near.add(x + y * ctb_w)
            # CTBs coded BEHIND the lost slice predict from nothing of it only if they start a new slice row ...: keep to the ones in front
            safe = [c for c in range(first) if c not in near]
            assert len(safe) > 3
            _assert_ctbs_equal_reference(blob, mine, ref, safe, f"lost slice {k}")
    # ---- the last slice cut short ----
    cut = hevcutil.join_nals(nals[:-1] + [nals[-1][:max(8, len(nals[-1]) // 2)]])
    with pytest.raises(RuntimeError):
        hevcutil.parse(hm, cut)
    blob, n_conc, first = hevcutil.parse_concealing(hm, cut)
    assert n_conc > 0 and first + n_conc == ctb_w * ctb_h  # concealed to the picture's end
    mine, _ = orc.oracle_decode(blob, 3)
    if orc.have_ref():
        ref, _ = orc.ref_decode(cut, 0)
        _assert_ctbs_equal_reference(blob, mine, ref, range(max(0, first - ctb_w - 2)), "truncated last slice")
    # ---- an intact stream is untouched by the option ----
    blob, n_conc, first = hevcutil.parse_concealing(hm, data)
    assert n_conc == 0 and first == -1 and blob == intact
    # ---- bit flips in the slice data: every stream comes back as a picture the executors take ----
    rng = random.Random(11)
    concealed = 0
    for name in ("ragged", "ctb64_wpp", "hi422_10", "mono10", "tiles_3x2_nolf", "pcm_bypass_sl_wpp", "dense_lowqp"):
        base = bytes(corpus.stream(name))
        for _ in range(12):
            b = bytearray(base)
            for _ in range(rng.randrange(1, 3)):
                b[rng.randrange(len(base) // 3, len(b))] ^= 1 << rng.randrange(8)
            try:
                blob, n_conc, first = hevcutil.parse_concealing(hm, bytes(b))
            except RuntimeError as e:
                assert "failed: -3:" in str(e) or "failed: -2:" in str(e), e  # (damaged parameter sets / first slice header stay errors)
                continue
            assert hm.hm_stream_validate(blob, len(blob)) == 0
            orc.oracle_decode(blob, 3)
            concealed += n_conc > 0
    assert concealed >= 30, concealed


def test_the_validator_accepts_whatever_the_parser_emits(hm):
    """mutated slice data that the parser takes must come out as a command stream every field of which is in range
    (hm_stream_validate is what hm_batch_add runs on foreign streams) - the invariant of tools/asan/fuzz_host.cpp, which found a
    5-bit field read as 45 from an arithmetic decoder that started with an offset of 510 (refused since: 9.3.2.5)"""
    import ctypes as C
    hm.hm_stream_validate.argtypes = [C.c_char_p, C.c_size_t]
    rng = random.Random(670)
    taken = 0
    for name in ("rext_cross_444_all", "pcm_bypass_sl_wpp", "slices_headers", "wpp_tiles_slices", "rext_ts_bypass_422_10"):
        data = corpus.stream(name)
        for _ in range(250):
            b = bytearray(data)
            for _ in range(rng.randrange(1, 4)):
                i = rng.randrange(len(b) // 4, len(b))
                b[i] = rng.randrange(256) if rng.random() < 0.3 else b[i] ^ (1 << rng.randrange(8))
            try:
                blob = hevcutil.parse(hm, bytes(b))
            except RuntimeError:
                continue
            taken += 1
            assert hm.hm_stream_validate(blob, len(blob)) == 0, f"{name}: {hm.hm_last_error().decode()}"
    assert taken > 50


def test_truncated_heif_is_an_error(hm):
    data = heifwriter.write_heic(_tiles(1), (64, 64))
    for cut in (0, 4, 11, 40, len(data) // 2):
        with pytest.raises(RuntimeError):
            f = pipeline.HeifFile(hm, data[:cut])
            f.info(f.primary())
    with pytest.raises(RuntimeError):
        pipeline.HeifFile(hm, b"\x00\x00\x00\x10ftypheic\x00\x00\x00\x00")  # no meta box


def _decode_status(hm, data, host_threads=1):
    f = pipeline.HeifFile(hm, data)
    prm = pipeline.DecodeParams(10, host_threads, 0, 0, None, None, 0, 0)
    d = pipeline.Decoded()
    rc = hm.hm_decode_item(f.h, f.primary(), C.byref(prm), C.byref(d))
    msg = hm.hm_last_error().decode()
    f.close()
    return rc, msg


def test_invalid_grids_report_reference_errors(hm):
    t = _tiles(4)
    # fewer tiles than rows*cols (context.cc:2142-2153)
    bad = heifwriter.write_heic(t[:3], (64, 64), grid=(2, 2, 128, 128))
    with pytest.raises(RuntimeError, match="dimg"):
        pipeline.HeifFile(hm, bad).info(4)
    # tiles do not cover the output (context.cc:2321-2326)
    rc, msg = _decode_status(hm, heifwriter.write_heic(t, (64, 64), grid=(2, 2, 200, 128)))
    assert rc == -3 and "cover" in msg
    # tiles of different declared size (context.cc:2333-2337)
    import synthutil
    mixed = t[:3] + [synthutil.picture(399, width=64, height=72)]
    data = heifwriter.write_heic(mixed, (64, 64), grid=(2, 2, 128, 128), sizes=[(64, 64)] * 3 + [(64, 72)])
    rc, msg = _decode_status(hm, data)
    assert rc == -3 and "different sizes" in msg


def mixed_tile_grid(case):
    """Grids of 64x64 tiles whose tiles disagree with tile 0 (context.cc:2333-2337, 2430-2492): (file, expected status, expected text).
    Tiles are compared with tile 0 of the WHOLE grid one by one, the declared size first, then the chroma format, then the depth: the first
    tile that fails names the error."""
    import synthutil
    odd = {"depth": dict(bit_depth=10), "chroma": dict(chroma_format=3), "both": dict(bit_depth=10, chroma_format=3)}

    def grid(rows, cols, other, sizes=None):  # other: {tile index: key of odd}
        n = rows * cols
        pics = [synthutil.picture(300 + i, width=64, height=72 if sizes and sizes[i] == (64, 72) else 64, **odd.get(other.get(i), {})) for i in range(n)]
        return heifwriter.write_heic(pics, (64, 64), grid=(rows, cols, 64 * cols, 64 * rows), sizes=sizes,
                                     bit_depth=[odd.get(other.get(i), {}).get("bit_depth", 8) for i in range(n)],
                                     chroma_format=[odd.get(other.get(i), {}).get("chroma_format", 1) for i in range(n)])
    tall = [(64, 64)] * 3 + [(64, 72)]
    return {
        "depth_last_row": lambda: (grid(4, 2, {6: "depth"}), -3, "different pixel depth"),
        "chroma_last_row": lambda: (grid(4, 2, {6: "chroma"}), -3, "different chroma format"),
        # a whole tile row unlike tile 0: as a slab of its own it is consistent in itself, only the comparison with tile 0 of the grid refuses it
        "depth_whole_last_row": lambda: (grid(4, 2, {6: "depth", 7: "depth"}), -3, "different pixel depth"),
        "chroma_whole_last_row": lambda: (grid(4, 2, {6: "chroma", 7: "chroma"}), -3, "different chroma format"),
        "chroma_and_depth_same_tile": lambda: (grid(2, 2, {1: "both"}), -3, "different chroma format"),
        "depth_then_size": lambda: (grid(2, 2, {1: "depth"}, sizes=tall), -3, "different pixel depth"),
        "size_then_depth": lambda: (grid(2, 2, {3: "depth"}, sizes=[(64, 64), (64, 72), (64, 64), (64, 64)]), -3, "Grid tiles have different sizes"),
    }[case]()


@pytest.mark.parametrize("case", ["depth_last_row", "chroma_last_row", "depth_whole_last_row", "chroma_whole_last_row", "chroma_and_depth_same_tile", "depth_then_size",
                                  "size_then_depth"])
def test_mixed_tile_grids_report_reference_errors(hm, case):
    """host_threads=16: no more tiles than threads, the one-batch decode.  (With fewer threads than tiles the first five grids are cut
    into slabs of tile rows, which needs a device: the test below.)"""
    data, want_rc, want_msg = mixed_tile_grid(case)
    rc, msg = _decode_status(hm, data, host_threads=16)
    assert rc == want_rc and want_msg in msg, (rc, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["depth_last_row", "chroma_last_row", "depth_whole_last_row", "chroma_whole_last_row", "chroma_and_depth_same_tile"])
def test_mixed_tile_grids_are_refused_slab_by_slab(hm, case):
    """ADVICE.md (round 6), first item: host_threads=1, more tiles than threads - the grid is decoded in slabs of one tile row, each queued
    as soon as it is parsed, and every tile is still compared with tile 0 of the WHOLE grid: the status and message of the one-batch decode,
    nothing handed out, and the next decode in the same process unharmed.  The two *_whole_last_row grids are the ones that need that
    comparison (grid_tile_picture in decode_grid_cut's take_blobs): rows 0-2 as tile 0, row 3 another depth or chroma format throughout, so
    the last slab agrees with itself and its own decode finds nothing wrong - without the comparison the call returned HM_OK with mixed
    content under tile 0's metadata.  In the other three the odd tile shares a slab with an ordinary one, and the slab's decode refuses too."""
    data, want_rc, want_msg = mixed_tile_grid(case)
    f = pipeline.HeifFile(hm, data)
    prm = pipeline.DecodeParams(10, 1, 0, 0, None, None, 0, 0)
    d = pipeline.Decoded()
    rc = hm.hm_decode_item(f.h, f.primary(), C.byref(prm), C.byref(d))
    msg = hm.hm_last_error().decode()
    f.close()
    assert rc == want_rc and want_msg in msg, (rc, msg)
    assert not d.plane[0]
    import numpy as np
    g = pipeline.HeifFile(hm, heifwriter.write_heic(_tiles(8), (64, 64), grid=(4, 2, 128, 256)))
    slabs, meta = g.decode(g.primary(), 10, threads=1)
    batch, _ = g.decode(g.primary(), 10, threads=16)
    g.close()
    assert (meta["width"], meta["height"]) == (128, 256)
    np.testing.assert_array_equal(slabs[0][:256, :384], batch[0][:256, :384])


def test_no_gpu_means_loud_failure_not_cpu_fallback(hm):
    if hm.hm_device_count() > 0:
        pytest.skip("a GPU is present")
    rc, msg = _decode_status(hm, heifwriter.write_heic(_tiles(1), (64, 64)))
    assert rc == -4, (rc, msg)  # HM_ERR_NO_DEVICE
    b = C.c_void_p()
    assert hm.hm_batch_create(C.byref(b)) == -4
    with pytest.raises(RuntimeError, match="-4"):
        pipeline.Pipeline(hm, 10)


def test_unsupported_syntax_is_reported(hm):
    """syntax outside the GPU path: HM_ERR_UNSUPPORTED with a reason, not garbage (here: 14-bit samples)"""
    import synthutil
    data = synthutil.picture(5, width=64, height=64, bit_depth=14)
    with pytest.raises(RuntimeError, match="-2.*bit depth"):
        hevcutil.parse(hm, data)


def test_mutated_heif_boxes_never_crash(hm):
    """byte-level mutations of valid .heic files (real fuzz-corpus files of the reference and a synthetic grid with
    irot / clap): every entry point of the container side either succeeds or reports an error."""
    rng = random.Random(99)
    seeds = [open(os.path.join(HERE, "data", n), "rb").read() for n in ("colors-no-alpha.heic", "colors-with-alpha.heic")]
    seeds.append(heifwriter.write_heic(_tiles(4), (64, 64), grid=(2, 2, 120, 100),
                                       transforms=[("irot", 1), ("clap", (100, 1, 80, 1, 0, 1, 0, 1))]))
    ok = err = 0
    for data in seeds:
        meta_end = min(len(data), 4096)  # the box structure sits at the start; payload mutations are covered above
        for _ in range(400):
            b = bytearray(data)
            for _ in range(rng.randrange(1, 5)):
                i = rng.randrange(meta_end)
                if rng.random() < 0.5:
                    b[i] ^= 1 << rng.randrange(8)
                else:
                    b[i] = rng.randrange(256)
            try:
                f = pipeline.HeifFile(hm, bytes(b))
                try:
                    ids = f.top_level() if hasattr(f, "top_level") else [f.primary()]
                    for iid in ids[:4]:
                        info = f.info(iid)
                        if not info.is_grid:
                            hevcutil.parse(hm, f.hevc_data(iid))
                finally:
                    f.close()
                ok += 1
            except RuntimeError:
                err += 1
    assert ok + err == 1200 and err > 50 and ok > 50


def test_foreign_command_streams_are_validated(hm):
    """hm_stream_validate (run by hm_batch_add on every stream it is given): streams of the parser pass; corrupting any
    field the kernels use as an index or a size is caught on the host; the validator itself survives arbitrary bytes."""
    import ctypes as C
    import struct
    hm.hm_stream_validate.argtypes = [C.c_char_p, C.c_size_t]
    names = ("tiny", "ragged", "ctb64_wpp", "hi422_10", "pcm_bypass_sl_wpp", "yuv444_rare", "mono10")
    blobs = [hevcutil.parse(hm, corpus.stream(n)) for n in names]
    for b in blobs:
        assert hm.hm_stream_validate(b, len(b)) == 0, hm.hm_last_error()
    # hm_pic (include/hm_stream.h): n_slices, n_ctbs, n_tus, n_coeffs at 0x2C.., off_slices, off_ctbs, off_tus, off_coeffs at 0x3C..
    def mutations(b, compact):
        off = {name: struct.unpack_from("<I", b, pos)[0] for name, pos in (("ctbs", 0x40), ("tus", 0x44), ("coeffs", 0x48))}

        def bad(mut):
            m = bytearray(b)
            mut(m)
            return hm.hm_stream_validate(bytes(m), len(m)) != 0

        def put(fmt, pos, val):
            return lambda m: struct.pack_into(fmt, m, pos, val)

        tus, cfs, ctbs = off["tus"], off["coeffs"], off["ctbs"]
        assert bad(put("<I", 4, len(b) + 1))                       # total_bytes beyond the buffer
        assert bad(put("<I", 0x34, 0xFFFFFFF))                     # n_tus
        assert bad(put("<I", 0x44, len(b) - 4))                    # off_tus
        assert bad(put("<I", ctbs, 7))                             # tu_first of CTB 0 (records not contiguous)
        assert bad(put("<H", ctbs + 6, 9))                         # slice index
        assert bad(put("<B", ctbs + 12, 9))                        # SAO type
        if compact:  # hm_tu6: pos, info, pred_mode, qp, count
            assert bad(put("<B", tus + 1, 7))                      # block size 2^7
            assert bad(put("<B", tus + 2, 63))                     # prediction mode 63
            assert bad(put("<B", tus + 2, 0x80 | 1))               # PCM flag in a picture without rare syntax
            assert bad(put("<H", tus + 4, 0x07FF))                 # more levels than the block has positions
            assert bad(put("<H", tus + 4, 0xE000))                 # reserved bits
            info0 = struct.unpack_from("<B", b, tus + 1)[0]
            assert bad(put("<B", tus + 1, info0 | 0x80))           # reserved bit of info (hm_tu's top-left flag: derived, not stored)
            assert bad(put("<B", ctbs + 42, 0x08))                 # CTB 0 claims a usable CTB to its left (outside the picture)
            assert bad(put("<B", ctbs + 42, 0x10))                 # reserved bits of hm_ctb.nb_avail
            assert bad(put("<I", ctbs + 44, 7))                    # level index of the CTB's first record
            size0 = info0 & 7
            assert bad(put("<B", tus + 0, 0xFF)) or size0 == 2    # block outside its CTB (a 4x4 block at 60,60 of a 64 CTB is inside)
            counts = [struct.unpack_from("<H", b, tus + 6 * t + 4)[0] & 0x7FF for t in range(64)]
            first_cf = sum(counts[:next(t for t in range(64) if counts[t])])
        else:        # hm_tu
            assert bad(put("<B", tus + 2, 7))                      # block size 2^7
            assert bad(put("<B", tus + 0, 200))                    # block outside its CTB
            assert bad(put("<B", tus + 3, 63))                     # prediction mode 63
            assert bad(put("<H", tus + 6, 5000))                   # n_coeff > nT^2
            assert bad(put("<I", tus + 8, 0x7FFFFFFF))             # coeff_first
            assert bad(put("<B", tus + 12, 250))                   # avail_left > nT
            first_cf = next(struct.unpack_from("<I", b, tus + 16 * t + 8)[0] for t in range(64) if struct.unpack_from("<H", b, tus + 16 * t + 6)[0])
        assert bad(put("<H", cfs + 4 * first_cf, 60000))           # level position outside the block

    mutations(bytearray(blobs[2]), True)    # compact records (split chains)
    mutations(bytearray(blobs[4]), False)   # rare syntax: full records in decode order
    rng = random.Random(7)
    for _ in range(3000):                                      # arbitrary corruption: any verdict, no crash
        m = bytearray(blobs[rng.randrange(len(blobs))])
        for _ in range(rng.randrange(1, 8)):
            m[rng.randrange(len(m))] = rng.randrange(256)
        hm.hm_stream_validate(bytes(m), len(m))
        cut = rng.randrange(len(m))
        hm.hm_stream_validate(bytes(m[:cut]), cut)


def _nals(data):
    out, p = [], 0
    while p < len(data):
        n = struct.unpack_from(">I", data, p)[0]
        out.append(data[p + 4:p + 4 + n])
        p += 4 + n
    return out


def _frame(nals):
    return b"".join(struct.pack(">I", len(n)) + n for n in nals)


def test_sps_replaced_after_pps_invalidates_the_pps(hm):
    """SPS(64x64), PPS, SPS(larger, same id), slice.  The PPS scan tables were derived from the first
    SPS; a slice that walks the larger picture with them indexed past their end.  The PPS must be invalid now."""
    import synthutil
    small = _nals(synthutil.picture(11, width=64, height=64))
    big = _nals(synthutil.picture(12, width=512, height=320))
    kind = lambda n: (n[0] >> 1) & 0x3F
    sps_big = [n for n in big if kind(n) == 33]
    slices_big = [n for n in big if kind(n) <= 21]
    assert sps_big and slices_big
    evil = _frame([n for n in small if kind(n) in (32, 33, 34)] + sps_big + slices_big)
    with pytest.raises(RuntimeError, match="missing PPS|scan tables"):
        hevcutil.parse(hm, evil)
    # re-sending the PPS after the new SPS is legal and decodes the large picture
    good = _frame([n for n in small if kind(n) in (32, 33, 34)] + [n for n in big if kind(n) in (33, 34)] + slices_big)
    blob = hevcutil.parse(hm, good)
    assert struct.unpack_from("<HH", blob, 8) == (512, 320)


def test_parameter_set_ranges_are_checked(hm):
    """out-of-range PPS / SPS fields are refused at parse time (H.265 7.4.3.2.1, 7.4.3.3.1)."""
    import synthutil
    for kw in (dict(cb_qp_offset=13), dict(cr_qp_offset=-13), dict(beta_offset_div2=7), dict(tc_offset_div2=-7)):
        # the synthesiser reads its own parameter sets back with the product's parser (parse_pps): -2 = it refused them
        with pytest.raises(RuntimeError, match="out of range|synth failed: -2"):
            hevcutil.parse(hm, synthutil.picture(3, width=64, height=64, **kw))


def _parse_opts(hm, data, threads, conceal):
    o = hevcutil._ParseOptions(0, threads, hevcutil.HM_PARSE_CONCEAL if conceal else 0)
    hm.hm_hevc_parse_opts.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(hevcutil._ParseOptions), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    hm.hm_last_error.restype = C.c_char_p
    blob, size = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = hm.hm_hevc_parse_opts(data, len(data), C.byref(o), C.byref(blob), C.byref(size))
    if rc:
        raise RuntimeError(f"hm_hevc_parse_opts failed: {rc}: {hm.hm_last_error().decode()}")
    out = C.string_at(blob, size.value)
    hm.hm_free(blob)
    return out


def test_a_second_coded_picture_behind_an_intact_one_is_ignored_when_concealing(hm):
    """with concealment on (the default of the plugin / facade / hm_decode_item) the slice segments of a SECOND coded picture
    behind an intact one must not take CTBs of the finished picture back (they did: every segment but the first one of that picture,
    with no warning).  The item's picture is the first one, byte for byte the strict parse's, and nothing counts as concealed."""
    a = hevcutil.split_nals(corpus.stream("slices"))
    b = hevcutil.split_nals(corpus.stream("slices_headers"))
    ref = hevcutil.parse(hm, corpus.stream("slices"))
    two = hevcutil.join_nals(a + [n for n in b if ((n[0] >> 1) & 63) <= 21])  # + the slice segments of another picture (first, then five more)
    blob, n_conc, first = hevcutil.parse_concealing(hm, two)
    assert blob == ref and n_conc == 0 and first == -1
    # ... also when the first picture WAS damaged (its last segment lost): the other picture's segments do not fill the gap
    cut = hevcutil.join_nals(a[:-1] + [n for n in b if ((n[0] >> 1) & 63) <= 21])
    blob_cut, n_cut, first_cut = hevcutil.parse_concealing(hm, hevcutil.join_nals(a[:-1]))
    assert n_cut > 0
    try:
        got = hevcutil.parse_concealing(hm, cut)
    except RuntimeError:  # (a first_slice_segment_in_pic inside an unfinished picture, or its header read with the wrong PPS: refused, as before)
        pass
    else:
        assert got == (blob_cut, n_cut, first_cut)


def test_overlapping_segments_of_a_picture_parsed_in_parallel_keep_their_levels(hm, oracle):
    """a rare-syntax (records in decode order) WPP picture parsed with several threads keeps its levels in per-row lists that
    are merged afterwards; a later independent segment that starts inside what has been parsed takes those CTBs back - the picture's
    level list was cut at a mark the parallel rows never set (0: every earlier CTB lost its levels while its records still pointed at
    them).  A duplicated middle segment must give the picture of the stream without the duplicate, with 1 and with 4 threads."""
    import numpy as np
    import orc
    import synthutil
    d = synthutil.picture(9102, width=256, height=256, log2_ctb=5, wpp=1, slices=20, pcm=200, pcm_bits_y=8, pcm_bits_c=8)
    nals = hevcutil.split_nals(d)
    segs = [n for n in nals if ((n[0] >> 1) & 63) <= 21]
    assert len(segs) >= 4
    ref, _ = orc.oracle_decode(_parse_opts(hm, d, 1, False), 3)
    hm.hm_parse_parallel_segments.restype = C.c_long
    for k in range(1, len(segs) - 1):
        i = nals.index(segs[k])
        dup = hevcutil.join_nals(nals[:i + 1] + [segs[k]] + nals[i + 1:])
        for threads in (1, 4):
            before = hm.hm_parse_parallel_segments(0)
            blob = _parse_opts(hm, dup, threads, True)
            assert threads == 1 or hm.hm_parse_parallel_segments(0) > before  # (the rows of these segments did run side by side)
            n_tus, n_coeffs = struct.unpack_from("<II", blob, 56)
            assert struct.unpack_from("<II", blob, 80) == (0, 0)  # nothing made up
            got, _ = orc.oracle_decode(blob, 3)
            assert all(np.array_equal(x, y) for x, y in zip(ref, got)), (k, threads)
