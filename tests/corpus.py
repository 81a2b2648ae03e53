"""The synthetic test corpus: named (seed, parameter) cases for tests/synth.  Every case is
blessed by the real reference decoder in the build container (tools/make_fixtures.py writes its
fingerprints to tests/golden/synth.json); streams are regenerated deterministically from the
seed wherever the tests run."""

# BASELINE configs: 512x512 tiles, CTB 32, QP 27 +- cu_qp_delta, SAO, deblock, SDH
TILE = dict(width=512, height=512, log2_ctb=5, qp=27, cu_qp_delta=1, sao=1, sign_hiding=1, density=60)

CASES = {
    # config 2 tiles: VUI full_range=1 matrix=6, and the no-VUI variant (limited-range paste rescale)
    "tile512_a": dict(seed=1200000, vui=1, full_range=1, matrix=6, **TILE),
    "tile512_b": dict(seed=1200001, vui=1, full_range=1, matrix=6, **TILE),
    "tile512_novui": dict(seed=1200002, vui=0, **TILE),
    # config 4: 10-bit 4:2:2 (small variant; the full 2048x1536 one is generated in the bench / slow tests)
    "hi422_10": dict(seed=4220010, width=256, height=192, chroma_format=2, bit_depth=10, log2_ctb=5, qp=30,
                     vui=1, full_range=0, matrix=9, primaries=9),
    "hi422_10_full": dict(seed=4220011, width=192, height=128, chroma_format=2, bit_depth=10, log2_ctb=5, qp=24,
                          vui=1, full_range=1, matrix=1, primaries=1, cb_qp_offset=3, cr_qp_offset=-2),
    "hi420_10": dict(seed=4200010, width=128, height=128, chroma_format=1, bit_depth=10, log2_ctb=4, qp=33),
    "hi422_12": dict(seed=4220012, width=128, height=64, chroma_format=2, bit_depth=12, log2_ctb=5, qp=35),
    # structure / tool coverage
    "ctb64": dict(seed=64001, width=192, height=136, log2_ctb=6, qp=25),
    "ctb64_wpp": dict(seed=64002, width=256, height=192, log2_ctb=6, wpp=1, qp=31),
    "ctb16_nosao": dict(seed=16001, width=128, height=72, log2_ctb=4, sao=0, qp=29),
    "ctb32_wpp_422": dict(seed=32002, width=160, height=96, log2_ctb=5, wpp=1, chroma_format=2, qp=28),
    "no_deblock": dict(seed=7001, width=128, height=128, deblock_disable=1),
    "no_sao_no_sdh": dict(seed=7002, width=128, height=96, sao=0, sign_hiding=0, transform_skip=0, strong_intra=0),
    "offsets": dict(seed=7003, width=128, height=128, beta_offset_div2=3, tc_offset_div2=-2, cb_qp_offset=-4, cr_qp_offset=5, qp=36),
    "dense_lowqp": dict(seed=7004, width=96, height=96, density=95, qp=12),
    "sparse_highqp": dict(seed=7005, width=96, height=96, density=25, qp=47),
    "tiny": dict(seed=7006, width=8, height=8, log2_ctb=4),
    "ragged": dict(seed=7007, width=72, height=40, log2_ctb=5),
    "min_cb16": dict(seed=7008, width=128, height=64, log2_ctb=5, log2_min_cb=4, log2_min_tb=3, max_th_depth_intra=1),
    "flat_qp": dict(seed=7009, width=128, height=128, cu_qp_delta=0, max_th_depth_intra=0),
    # monochrome (4:0:0): alpha planes written by libheif-style encoders, depth / gain maps
    "mono8": dict(seed=4000001, width=160, height=104, chroma_format=0, log2_ctb=5, qp=29),
    "mono8_ctb64_wpp": dict(seed=4000002, width=192, height=136, chroma_format=0, log2_ctb=6, wpp=1, qp=24),
    "mono10": dict(seed=4000010, width=128, height=96, chroma_format=0, bit_depth=10, log2_ctb=4, qp=33),
    # scaling lists (transform.cc:507-545): default lists, random lists in the SPS, lists in the PPS overriding the SPS
    "sl_default": dict(seed=5100001, width=128, height=96, log2_ctb=5, qp=30, scaling_list=1),
    "sl_sps": dict(seed=5100002, width=192, height=128, log2_ctb=5, qp=26, scaling_list=2),
    "sl_pps_422_10": dict(seed=5100003, width=128, height=128, log2_ctb=5, chroma_format=2, bit_depth=10, qp=34, scaling_list=3),
    "sl_sps_ctb64_lowqp": dict(seed=5100004, width=192, height=136, log2_ctb=6, qp=8, density=90, scaling_list=2),
    "sl_sps_12bit_highqp": dict(seed=5100005, width=64, height=64, log2_ctb=4, bit_depth=12, qp=50, scaling_list=2),
    # PCM and transquant-bypass coding units (slice.cc:4462-4536, transform.cc:431-449) and the reference's "pcmf"
    # loop-filter branches (deblock.cc:723-786, 1635-1756; sao.cc:356-363)
    "pcm_nofilter": dict(seed=5200001, width=128, height=96, log2_ctb=5, qp=30, pcm=300, pcm_bits_y=7, pcm_bits_c=5, pcm_loop_filter_disable=1),
    "pcm_filtered": dict(seed=5200002, width=128, height=96, log2_ctb=5, qp=30, pcm=300, pcm_bits_y=8, pcm_bits_c=6, pcm_loop_filter_disable=0),
    "pcm_422_10": dict(seed=5200003, width=128, height=64, log2_ctb=5, chroma_format=2, bit_depth=10, qp=32, pcm=250, pcm_bits_y=10, pcm_bits_c=8,
                       pcm_loop_filter_disable=1, pcm_log2_max=4),
    "tq_bypass": dict(seed=5200004, width=128, height=96, log2_ctb=5, qp=28, tq_bypass=400),
    "lossless_all": dict(seed=5200005, width=96, height=64, log2_ctb=4, bit_depth=10, qp=22, tq_bypass=1000),
    "pcm_bypass_mono12": dict(seed=5200006, width=96, height=72, log2_ctb=5, chroma_format=0, bit_depth=12, qp=36, pcm=200, pcm_bits_y=11,
                              pcm_bits_c=12, pcm_loop_filter_disable=1, tq_bypass=250),
    "pcm_bypass_sl_wpp": dict(seed=5200007, width=192, height=128, log2_ctb=6, bit_depth=10, qp=29, wpp=1, scaling_list=2, pcm=200,
                              pcm_bits_y=9, pcm_bits_c=9, pcm_loop_filter_disable=0, tq_bypass=200),
    # 4:4:4 (chroma blocks as large as luma ones, chroma reference samples smoothed like luma: intrapred.cc:307-311)
    "yuv444_8": dict(seed=5300001, width=160, height=96, chroma_format=3, log2_ctb=5, qp=28, matrix=0),
    "yuv444_10_ctb64_wpp": dict(seed=5300002, width=192, height=136, chroma_format=3, bit_depth=10, log2_ctb=6, wpp=1, qp=31),
    "yuv444_12_ctb16": dict(seed=5300003, width=96, height=64, chroma_format=3, bit_depth=12, log2_ctb=4, qp=36),
    "yuv444_rare": dict(seed=5300004, width=128, height=96, chroma_format=3, log2_ctb=5, qp=30, scaling_list=2, pcm=200, pcm_bits_y=8,
                        pcm_bits_c=7, pcm_loop_filter_disable=1, tq_bypass=200),
}

# slice / tile structure (slice.cc:5004-5083, 5350-5406; deblock.cc:160-196; sao.cc:336-424): several slices, dependent
# slice segments, tiles (uniform / explicit), loop filters stopped at slice / tile borders, per-slice deblocking
# override, SAO flags, QP and chroma QP offsets, WPP together with slices / tiles, conformance windows
CASES.update({
    "slices": dict(seed=6100001, width=256, height=192, slices=60),
    "slices_dependent": dict(seed=6100002, width=256, height=192, slices=60, dependent=500),
    "slices_nolf": dict(seed=6100003, width=256, height=192, slices=80, pps_lf_across_slices_off=1),
    "slices_headers": dict(seed=6100004, width=256, height=192, slices=80, slice_lf_random=1, deblock_override=1, slice_sao_random=1,
                           slice_qp_random=1, slice_chroma_qp=1, dependent=300),
    "tiles_3x2": dict(seed=6100005, width=256, height=192, tile_cols=3, tile_rows=2),
    "tiles_3x2_nolf": dict(seed=6100006, width=256, height=192, tile_cols=3, tile_rows=2, lf_across_tiles=0),
    "tiles_explicit_slices": dict(seed=6100007, width=320, height=256, tile_cols=4, tile_rows=3, tiles_uniform=0, lf_across_tiles=0, slices=100,
                                  dependent=400, slice_lf_random=1),
    "wpp_slices_dependent": dict(seed=6100008, width=256, height=192, wpp=1, slices=100, dependent=600),
    "wpp_tiles_slices": dict(seed=6100009, width=256, height=192, wpp=1, tile_cols=2, tile_rows=2, slices=50, dependent=300, lf_across_tiles=0),
    "tiles_422_10_ctb64": dict(seed=6100010, width=256, height=192, log2_ctb=6, tile_cols=2, tile_rows=2, slices=300, chroma_format=2, bit_depth=10,
                               lf_across_tiles=0, slice_lf_random=1),
    "slices_444_pcm": dict(seed=6100011, width=192, height=128, chroma_format=3, slices=120, dependent=300, slice_lf_random=1, pcm=200,
                           pcm_loop_filter_disable=1, tq_bypass=150, slice_sao_random=1),
    "slices_mono_ctb16": dict(seed=6100012, width=160, height=96, chroma_format=0, log2_ctb=4, slices=60, dependent=400, pps_lf_across_slices_off=1),
    "conf_window": dict(seed=6100013, width=200, height=136, conf_left=2, conf_right=6, conf_top=4, conf_bottom=2),
    "conf_window_422_10": dict(seed=6100014, width=200, height=136, conf_right=8, conf_bottom=6, chroma_format=2, bit_depth=10),
})

# slice / tile structure at the bench's tile shape (16 CTU rows of CTB 32: rings of 4 and 8 bands of k_chain get bands of their
# own): slices that end in the middle of a CTU row - the CTU above-right of the next row's CTUs unavailable, no OP_FAR block
# in their records -, dependent segments, loop filters stopped at slice / tile borders, uniform and explicit tiles, WPP with
# slices; 10-bit 4:2:2 with CTB 64 and 4:0:0 with CTB 16; and two rare-syntax tiles (PCM, transquant bypass, scaling lists)
CASES.update({
    "tile512_slices": dict(seed=6300001, slices=40, **TILE),
    "tile512_slices_dependent_nolf": dict(seed=6300002, slices=80, dependent=400, pps_lf_across_slices_off=1, **TILE),
    "tile512_tiles_uniform_slices": dict(seed=6300003, tile_cols=4, tile_rows=4, lf_across_tiles=0, slices=30, slice_lf_random=1, **TILE),
    "tile512_tiles_explicit_slices": dict(seed=6300004, tile_cols=3, tile_rows=5, tiles_uniform=0, lf_across_tiles=0, slices=100, dependent=300,
                                          **TILE),
    "tile512_wpp_slices": dict(seed=6300005, wpp=1, slices=100, dependent=500, slice_qp_random=1, **TILE),
    "tile512_422_10_ctb64_tiles": dict(seed=6300006, **dict(TILE, log2_ctb=6), chroma_format=2, bit_depth=10, tile_cols=2, tile_rows=2,
                                       lf_across_tiles=0, slices=60),
    "tile512_mono_ctb16_slices": dict(seed=6300007, **dict(TILE, log2_ctb=4), chroma_format=0, slices=50, dependent=300),
    "tile512_rare": dict(seed=6300008, scaling_list=2, pcm=200, pcm_bits_y=7, pcm_bits_c=6, pcm_loop_filter_disable=0, tq_bypass=150, **TILE),
    "tile512_rare_422_10_slices": dict(seed=6300009, **dict(TILE, log2_ctb=6), chroma_format=2, bit_depth=10, scaling_list=3, pcm=200,
                                       pcm_bits_y=9, pcm_bits_c=8, pcm_loop_filter_disable=1, tq_bypass=200, slices=60),
})

# range-extension coding tools (sps.cc:1375-1390, pps.cc:47-142; slice.cc:3143-3177, 3425-3432, 3565-3655, 3774-3805,
# 3809-3864, 3928-3957; transform.cc:251-285, 427-466, 566-643; intrapred.cc:307-326 of the reference).  rext_sps bits:
# 1 transform_skip_rotation, 2 transform_skip_context, 4 implicit_rdpcm, 8 explicit_rdpcm, 16 extended_precision,
# 32 intra_smoothing_disabled, 64 high_precision_offsets, 128 persistent_rice, 256 cabac_bypass_alignment
CASES.update({
    "rext_ts_tools": dict(seed=6200001, width=128, height=96, rext_sps=1 | 2 | 4, log2_max_ts=4, qp=26),
    "rext_ts_bypass_422_10": dict(seed=6200002, width=128, height=96, chroma_format=2, bit_depth=10, rext_sps=1 | 2 | 4, log2_max_ts=5, tq_bypass=250, qp=30),
    "rext_nosmooth_rice": dict(seed=6200003, width=160, height=96, log2_ctb=6, rext_sps=32 | 128, big_levels=300, qp=22),
    "rext_chroma_qp_list": dict(seed=6200004, width=128, height=128, chroma_qp_list=2, chroma_qp_depth=1, cb_qp_offset=2, slices=80),
    "rext_chroma_qp_list6_422": dict(seed=6200005, width=128, height=64, chroma_format=2, bit_depth=10, chroma_qp_list=6, chroma_qp_depth=0, wpp=1),
    "rext_cross_444": dict(seed=6200006, width=128, height=96, chroma_format=3, cross_component=1, qp=27),
    "rext_cross_444_all": dict(seed=6200007, width=128, height=96, chroma_format=3, bit_depth=10, cross_component=1, rext_sps=1 | 2 | 4 | 32 | 128,
                               log2_max_ts=5, tq_bypass=150, chroma_qp_list=3, big_levels=200, qp=24, wpp=1),
    "rext_ignored_flags": dict(seed=6200008, width=96, height=64, rext_sps=8 | 16 | 64 | 256, qp=30),
    "rext_sao_scale_12": dict(seed=6200009, width=96, height=64, bit_depth=12, sao_scale_y=2, sao_scale_c=1, qp=34),
    "rext_mono_rice_rdpcm": dict(seed=6200010, width=96, height=72, chroma_format=0, bit_depth=12, rext_sps=4 | 128 | 1, big_levels=250, tq_bypass=200, qp=33),
})

# 8-bit pictures in which the reference takes its "pcmf" deblocking branch: its SIMD build (the configuration of
# oracle/_ref, and what x86 / ARM users run) filters luma edges between ordinary units with the SSE / NEON kernel, its
# scalar build leaves them unfiltered (fallback-postfilter.h:85-124 reads the flags with the opposite polarity).  The
# fixtures and the product follow the SIMD build; tools/make_fixtures.py does not require the scalar build to agree.
SIMD_BUILD_ONLY = {"pcm_nofilter", "tq_bypass", "yuv444_rare", "slices_444_pcm", "tile512_rare"}


def stream(name):
    import synthutil
    kw = dict(CASES[name])
    seed = kw.pop("seed")
    return synthutil.picture(seed, **kw)


def rare_syntax_sweep(n, first_seed=2000):
    """(seed, parameters) of a seeded sweep over the rarely used syntax: PCM and transquant-bypass units with every
    loop-filter flag combination, scaling lists, WPP, 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4, 8-12 bit, every CTB size."""
    out = []
    for seed in range(first_seed, first_seed + n):
        kw = dict(width=[64, 96, 72, 128][seed % 4], height=[64, 40, 72][seed % 3], log2_ctb=[5, 4, 6, 5][seed % 4] if seed % 5 else 5,
                  chroma_format=[1, 2, 3, 0][seed % 4], bit_depth=[8, 10, 8, 12, 9][seed % 5], pcm=[200, 0, 300][seed % 3],
                  tq_bypass=[0, 300, 150, 1][seed % 4], pcm_loop_filter_disable=seed % 2, wpp=int(seed % 7 == 0), cu_qp_delta=1,
                  scaling_list=[0, 0, 2][seed % 3])
        if kw["log2_ctb"] == 4 and kw["bit_depth"] == 8 and kw["chroma_format"] in (1, 2):
            kw["log2_ctb"] = 5  # 8-bit SAO on 8-sample-wide chroma CTBs: the reference's SIMD quirk Q9, not a corpus subject
        kw["pcm_bits_y"] = max(1, kw["bit_depth"] - seed % 3)
        kw["pcm_bits_c"] = max(1, kw["bit_depth"] - seed % 4)
        out.append((seed, kw))
    return out


def structure_sweep(n, first_seed=7000):
    """(seed, parameters) of a seeded sweep over slice / tile structures: slices, dependent segments, uniform / explicit
    tiles, loop filters stopped at slice / tile borders, per-slice headers, WPP, all chroma formats, CTB sizes, depths."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        kw = dict(width=pick(0, [128, 192, 256, 160]), height=pick(2, [128, 96, 192, 64]), log2_ctb=pick(4, [5, 5, 4, 6]),
                  chroma_format=pick(6, [1, 1, 2, 3, 0]), bit_depth=pick(9, [8, 8, 10, 12]),
                  slices=pick(11, [0, 40, 100, 300]), dependent=pick(13, [0, 300, 1000]),
                  tile_cols=pick(15, [1, 1, 2, 3]), tile_rows=pick(17, [1, 2, 3]), tiles_uniform=pick(19, [1, 0]),
                  lf_across_tiles=pick(20, [1, 0]), pps_lf_across_slices_off=pick(21, [0, 0, 1]), slice_lf_random=pick(23, [0, 1]),
                  deblock_override=pick(24, [0, 1]), slice_sao_random=pick(25, [0, 1]), slice_qp_random=pick(26, [0, 1]),
                  slice_chroma_qp=pick(27, [0, 1]), wpp=pick(28, [0, 0, 1]), cu_qp_delta=1, diff_cu_qp_delta_depth=pick(30, [1, 0, 2]))
        if seed % 9 == 0:
            kw.update(pcm=200, pcm_loop_filter_disable=seed % 2, tq_bypass=150)
            kw["pcm_bits_y"] = kw["pcm_bits_c"] = kw["bit_depth"]
        if kw["log2_ctb"] == 4 and kw["bit_depth"] == 8 and kw["chroma_format"] in (1, 2):
            kw["log2_ctb"] = 5  # quirk Q9 (see rare_syntax_sweep)
        if kw["wpp"] and (kw["tile_cols"] > 1 or kw["tile_rows"] > 1):
            # WPP together with tiles: the reference accepts at most one entry point per tile and per remaining CTB row
            # (slice.cc:813-829) and takes its row tables from picture column 1 - only short slices in full-width tiles
            kw["tile_cols"] = 1
            kw["slices"] = max(kw["slices"], 300)
        kw["diff_cu_qp_delta_depth"] = min(kw["diff_cu_qp_delta_depth"], kw["log2_ctb"] - 3)
        out.append((seed, kw))
    return out


def rext_sweep(n, first_seed=11000):
    """(seed, parameters) of a seeded sweep over the range-extension tools, alone and combined with each other and with
    transquant bypass, scaling lists, WPP, slices, tiles, every chroma format / bit depth / CTB size."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        kw = dict(width=pick(0, [64, 96, 128, 72]), height=pick(2, [64, 40, 96, 72]), log2_ctb=pick(4, [5, 5, 4, 6]),
                  chroma_format=pick(6, [1, 3, 2, 3, 0]), bit_depth=pick(9, [8, 8, 10, 12]), cu_qp_delta=1,
                  rext_sps=pick(11, [0, 1, 2, 4, 32, 128, 7, 135, 167, 511, 39, 5]), log2_max_ts=pick(15, [0, 0, 3, 4, 5]),
                  tq_bypass=pick(18, [0, 0, 200, 500]), chroma_qp_list=pick(20, [0, 0, 1, 2, 6]), chroma_qp_depth=pick(23, [0, 1, 2]),
                  big_levels=pick(25, [0, 200, 400]), wpp=pick(27, [0, 0, 1]), slices=pick(29, [0, 0, 100]),
                  scaling_list=pick(30, [0, 0, 0, 2]), qp=pick(12, [27, 22, 33, 38]))
        kw["cross_component"] = int(kw["chroma_format"] == 3 and seed % 3 != 0)
        kw["chroma_qp_depth"] = min(kw["chroma_qp_depth"], kw["log2_ctb"] - 3)
        if kw["chroma_format"] == 0:
            kw["chroma_qp_list"] = 0
        if seed % 11 == 0:
            kw.update(tile_cols=2, tile_rows=2, wpp=0)
        if seed % 13 == 0 and not (kw["rext_sps"] & 128):
            kw.update(dependent=500, slices=max(kw["slices"], 100))  # (persistent_rice + dependent segments: refused, see below)
        if kw["bit_depth"] == 12 and seed % 2:
            kw.update(sao_scale_y=seed % 3, sao_scale_c=(seed // 3) % 3)
        if kw["log2_ctb"] == 4 and kw["bit_depth"] == 8 and kw["chroma_format"] in (1, 2):
            kw["log2_ctb"] = 5  # quirk Q9 (see rare_syntax_sweep)
        if kw["tq_bypass"] and kw["bit_depth"] == 8:
            pass  # (the "pcmf" deblocking branch: the SIMD build of the reference is the oracle, as for SIMD_BUILD_ONLY)
        out.append((seed, kw))
    return out


def rext_large():
    """larger pictures with 32x32 transform-skip / bypass blocks and CTB 64: RDPCM runs of 32 samples, cross-component
    prediction of 32x32 blocks"""
    return [(12000 + i, dict(width=192, height=128, log2_ctb=[6, 5][i % 2], chroma_format=[3, 1, 3, 2][i % 4], bit_depth=[8, 10, 12][i % 3],
                             rext_sps=[7, 135, 167, 39][i % 4], log2_max_ts=5, tq_bypass=[0, 300][i % 2], cross_component=int(i % 4 in (0, 2)),
                             chroma_qp_list=[0, 3][i % 2], big_levels=200, wpp=i % 2, qp=[24, 30, 36][i % 3], max_th_depth_intra=[0, 1, 2][i % 3]))
            for i in range(12)]


def extreme_sweep(n, first_seed=13000, pcmf_8bit=False):
    """(seed, parameters) of a seeded sweep over the arithmetic edges of the residual path: levels over the whole range a
    conforming stream may carry (level_span), QpY over -QpBdOffset .. 51 with its wrap (qp_span), scaling matrices pinned
    at 1 and 255 (scaling_span) - crossed with what selects a kernel path: bit depth, chroma format, CTB size, slice QP
    (1 / 26 / 51), 16x16 and 32x32 blocks (no_split), density from DC-only blocks to every group of four, transform skip
    (rotation, context, implicit RDPCM, blocks up to 32x32), persistent Rice, cross-component prediction, scaling lists, PCM
    and transquant bypass next to ordinary units.  The reference's SCALAR build is the ground truth (tests/golden/
    extreme.json): its SIMD build differs where 16-bit saturating instructions round otherwise.
    8-bit pictures whose draws hold transquant bypass or unfiltered PCM (9 of the first 144 cases) take the reference's "pcmf"
    deblocking branch, where its two builds disagree and the product follows the SIMD build (SIMD_BUILD_ONLY above): in the
    sweep proper they run without those two tools (which run at 10 and 12 bit); pcmf_8bit=True returns exactly these cases WITH
    their draws - the residual is held against the scalar build at the reconstruction stage, where the builds' deblocking
    does not enter, and the kernels against the oracle at every stage."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        i = seed - first_seed
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        # (the three depths, four chroma formats and three CTB sizes in turn: all 36 combinations within 36 cases)
        kw = dict(bit_depth=[8, 10, 12][i % 3], chroma_format=[1, 3, 0, 2][(i // 3) % 4], log2_ctb=[5, 4, 6][(i // 12) % 3],
                  width=pick(0, [64, 96, 128, 72]), height=pick(2, [64, 40, 96, 72]), qp=pick(4, [1, 26, 51, 26, 12, 40]),
                  no_split=pick(7, [0, 1, 0]), density=pick(9, [3, 20, 60, 100, 90]), transform_skip=pick(12, [1, 0, 1]),
                  scaling_list=pick(14, [0, 0, 2, 3, 0]), scaling_span=500, cu_qp_delta=1, qp_span=pick(17, [1, 1, 0]),
                  diff_cu_qp_delta_depth=pick(18, [1, 0, 2]), level_span=pick(20, [60, 250, 600, 1000]),
                  rext_sps=pick(22, [0, 1 | 2 | 4, 128, 0, 1 | 2 | 4 | 128, 4, 1]), log2_max_ts=pick(25, [0, 0, 3, 5]),
                  pcm=pick(27, [0, 0, 150]), tq_bypass=pick(29, [0, 0, 200]), wpp=pick(31, [0, 1]), sign_hiding=pick(6, [1, 1, 0]))
        kw["cross_component"] = int(kw["chroma_format"] == 3 and seed % 3 != 0)
        kw["diff_cu_qp_delta_depth"] = min(kw["diff_cu_qp_delta_depth"], kw["log2_ctb"] - 3)
        if (i // 36) % 2 == 0:
            # every other run of 36 cases: no rare syntax, so that whatever is not 4:4:4 takes the split chains (k_residual + k_chain);
            # the others go out in decode order (k_recon)
            kw.update(scaling_list=0, pcm=0, tq_bypass=0, log2_max_ts=0, rext_sps=kw["rext_sps"] & 128)
        if not kw["transform_skip"]:
            kw["log2_max_ts"] = 0
        if kw["pcm"]:
            kw.update(pcm_bits_y=max(1, kw["bit_depth"] - seed % 3), pcm_bits_c=max(1, kw["bit_depth"] - seed % 4), pcm_loop_filter_disable=seed % 2)
        pcmf = kw["bit_depth"] == 8 and bool(kw["tq_bypass"] or (kw["pcm"] and kw["pcm_loop_filter_disable"]))
        if pcmf_8bit:
            if pcmf:
                out.append((seed, kw))
            continue
        if kw["bit_depth"] == 8:
            kw.update(tq_bypass=0, pcm_loop_filter_disable=0)  # (the "pcmf" branch: see above)
        out.append((seed, kw))
    return out


def single_ctb_cases(n_per_shape, first_seed=14000, n_wrap_per_shape=60):
    """(seed, parameters) of pictures of ONE CTB whose first transform block of every component has no neighbours at all: every intra
    mode then predicts the constant 1 << (bit_depth - 1) (8.4.4.2.2), and the block's samples are clip(that + residual) -
    the residual arithmetic alone, observable (tests/residual_ref.py).  The smallest pictures that hold a first block of 4x4
    (8x8 picture, NxN allowed), 8x8, 16x16 (no_split) and 32x32 (32x32 and 64x64 pictures: CTB 32 and CTB 64), every bit depth
    and chroma format, the slice QP over its whole range, flat scaling and pinned scaling lists, transform skip with
    rotation, transquant bypass.  No implicit RDPCM, cross-component prediction or PCM (the sweep holds those).
    Behind them n_wrap_per_shape pictures per shape of the one regime in which the flat product wraps int32: 12 bit, slice QP 51
    (qP up to 75), every coded remaining level over the whole range, no rare syntax - so that all but 4:4:4 go out as split
    chains and the wrap reaches k_residual's DC-only, 4x4, 8x8 and large-block paths where residual_ref sees it."""
    shapes = [dict(width=8, height=8, log2_ctb=4, no_split=0), dict(width=8, height=8, log2_ctb=4, no_split=1),
              dict(width=16, height=16, log2_ctb=4, no_split=1), dict(width=32, height=32, log2_ctb=5, no_split=1),
              dict(width=64, height=64, log2_ctb=6, no_split=1)]
    out = []
    seed = first_seed
    for shape in shapes:
        for k in range(n_per_shape):
            r = seed * 2654435761 % (1 << 32)
            pick = lambda s, opts: opts[(r >> s) % len(opts)]
            bd = [8, 10, 12][k % 3]
            kw = dict(shape, bit_depth=bd, chroma_format=[1, 3, 2, 0][(k // 3) % 4], qp=pick(3, [1, 8, 17, 26, 35, 44, 51, 51]),
                      density=pick(7, [100, 60, 30, 100]), level_span=pick(10, [30, 120, 400, 1000]), qp_span=pick(12, [0, 1]), cu_qp_delta=1,
                      diff_cu_qp_delta_depth=0, transform_skip=pick(14, [1, 0]), rext_sps=pick(16, [0, 1, 128]), log2_max_ts=pick(18, [0, 0, 5]),
                      scaling_list=pick(21, [0, 0, 2]), scaling_span=600, tq_bypass=pick(23, [0, 0, 0, 150]) if bd > 8 else 0,
                      sao=0, deblock_disable=1, sign_hiding=pick(25, [1, 0]))
            if not kw["transform_skip"]:
                kw["log2_max_ts"] = 0
            out.append((seed, kw))
            seed += 1
    seed = first_seed + 100000
    for shape in shapes:
        for k in range(n_wrap_per_shape):
            out.append((seed, dict(shape, bit_depth=12, chroma_format=[1, 2, 0, 3][k % 4], qp=51, density=[100, 60, 30][k % 3], level_span=1000,
                                   qp_span=k % 2, cu_qp_delta=1, diff_cu_qp_delta_depth=0, transform_skip=(k // 4) % 2, rext_sps=[0, 128][(k // 8) % 2],
                                   sao=0, deblock_disable=1, sign_hiding=(k // 2) % 2)))
            seed += 1
    return out


def extreme_tiles():
    """512 x 512 tiles of the classes that take the split chains, with levels, QPs and 16x16 / 32x32 blocks at the edges of the
    residual arithmetic: the int16 residual slab and the hand-over lines between waves carry rail values"""
    base = dict(width=512, height=512, cu_qp_delta=1, qp_span=1, sao=1, sign_hiding=1)
    return [(15000, dict(base, log2_ctb=5, qp=30, density=60, level_span=250)),
            (15001, dict(base, log2_ctb=5, bit_depth=12, qp=51, density=90, level_span=600, no_split=1, transform_skip=0)),
            (15002, dict(base, log2_ctb=6, bit_depth=10, chroma_format=2, qp=12, density=60, level_span=400, rext_sps=128)),
            (15003, dict(base, log2_ctb=4, chroma_format=0, qp=44, density=100, level_span=1000, no_split=1))]


def extreme_large():
    """one large single picture per class with the same knobs (many waves per picture)"""
    return [(15100, dict(width=1600, height=1024, log2_ctb=5, qp=26, density=50, level_span=300, qp_span=1, cu_qp_delta=1)),
            (15101, dict(width=1536, height=1024, log2_ctb=6, bit_depth=12, chroma_format=2, qp=51, density=70, level_span=600, qp_span=1, cu_qp_delta=1, no_split=1)),
            (15102, dict(width=1920, height=1080, log2_ctb=4, bit_depth=10, qp=8, density=60, level_span=400, qp_span=1, cu_qp_delta=1, rext_sps=128)),
            (15103, dict(width=1536, height=1024, log2_ctb=6, chroma_format=0, qp=40, density=90, level_span=1000, qp_span=1, cu_qp_delta=1))]


def intra_sweep(n, first_seed=16000):
    """(seed, parameters) of a seeded sweep for intra sample prediction: small pictures whose sizes cut blocks at the right and
    bottom edges (72, 40, 136, 200), calm coding units (no residual: the picture holds the prediction itself, and smooth but
    non-flat borders for the units next to them) among noisy ones, crossed with what selects a path of the prediction: bit
    depth, chroma format, CTB size, whole 16x16 / 32x32 blocks (no_split, with 32x32 or 16x16 as the largest transform),
    strong intra smoothing, intra_smoothing_disabled, implicit RDPCM with transquant bypass (10 / 12 bit), level_span on a
    share of the cases (predictions from neighbours at 0 and at the maximum), slices with and without dependent segments,
    tiles that stop prediction at their borders, WPP.  Every other run of 48 cases has no rare syntax and takes the split
    chains unless it is 4:4:4; the others go out in decode order.  Quirk Q9 and the 8-bit "pcmf" branch stay excluded, as in
    extreme_sweep."""
    out = []
    for seed in range(first_seed, first_seed + n):
        # (a multiplicative hash alone leaves its low bits a function of the seed's low bits, which choose depth, format and CTB size below)
        r = seed * 2654435761 % (1 << 32)
        r = (r ^ (r >> 15)) * 2246822519 % (1 << 32)
        r ^= r >> 13
        i = seed - first_seed
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        # (8 bit in every other case - its split chains are the class with the packed-pair kernels -, the four chroma formats and three
        # CTB sizes in turn: all combinations within 48 cases)
        kw = dict(bit_depth=[8, 10, 8, 12][i % 4], chroma_format=[1, 3, 0, 2][(i // 4) % 4], log2_ctb=[5, 4, 6][(i // 16) % 3],
                  no_split=pick(5, [0, 1, 1, 1]), calm=pick(7, [0, 300, 700, 500]), density=pick(9, [20, 60, 100]), strong_intra=pick(11, [1, 1, 0]),
                  qp=pick(13, [22, 30, 38, 27]), cu_qp_delta=1, level_span=pick(15, [0, 300, 1000, 600]), rext_sps=pick(17, [4, 32, 36, 4]),
                  tq_bypass=pick(20, [0, 250]), slices=pick(22, [0, 60, 150, 300]), dependent=pick(24, [0, 400]), log2_max_tb=pick(26, [5, 5, 4]),
                  sign_hiding=pick(28, [1, 0]), mode_span=pick(29, [0, 800, 800, 400]))
        if kw["level_span"] == 1000:
            kw.update(density=100, qp=45)  # residuals far beyond the sample range: neighbours at 0 and at the maximum side by side
        # whole blocks on the larger pictures (few blocks each), split ones on the smaller
        kw.update(width=pick(0, [136, 192, 200, 72]), height=pick(3, [128, 56, 72, 104])) if kw["no_split"] else \
            kw.update(width=pick(0, [64, 72, 40, 72]), height=pick(3, [64, 40, 56, 72]))
        if (i // 48) % 2 == 0:
            kw.update(rext_sps=0, tq_bypass=0)  # no rare syntax: split chains (k_residual + k_chain) for all but 4:4:4
        if not kw["no_split"]:
            kw["log2_max_tb"] = 5
        if not kw["slices"]:
            kw["dependent"] = 0
        elif kw["slices"] == 300 and not kw["no_split"]:
            # two CTBs a row and short slices: a slice that starts above-right of a row's first CTB leaves it that neighbour alone
            kw.update(width=2 << kw["log2_ctb"], height=72)
        if i % 5 == 3:
            kw.update(tile_cols=2, tile_rows=2, lf_across_tiles=0, tiles_uniform=i % 2)
        elif i % 7 == 2:
            kw.update(wpp=1)
        if i >= 768:
            # behind the crossed cases, two families aimed at the cells of the census that 768 crossed cases leave empty
            j = i - 768
            if j % 2 == 0:  # small split pictures with neighbours at both rails and short slices: the clip of modes 10 / 26, missing corners
                kw = dict(bit_depth=[8, 10, 8, 12][(j // 2) % 4], chroma_format=[1, 0, 2, 1][(j // 8) % 4], log2_ctb=[5, 4, 6][(j // 2) % 3], width=72, height=72,
                          calm=300, density=100, qp=45, level_span=1000, cu_qp_delta=1, slices=150, rext_sps=[0, 4][(j // 4) % 2])
                if j % 8 == 2:  # ... and the same on whole 16x16 luma blocks of 8-bit split chains (32x32 units, 16x16 transforms)
                    kw.update(bit_depth=8, chroma_format=[1, 0][(j // 8) % 2], log2_ctb=5, no_split=1, log2_max_tb=4, rext_sps=0, width=136, height=72)
                if j % 16 == 6:  # ... and on 8x8 luma blocks of the deeper split chains (32x32 units, 8x8 transforms)
                    kw.update(bit_depth=[10, 12][(j // 16) % 2], chroma_format=[1, 0][(j // 32) % 2], log2_ctb=5, no_split=1, log2_max_tb=3, rext_sps=0, width=136, height=72)
            else:           # whole 32x32 luma / 16x16 chroma blocks with residuals, modes drawn whole
                kw = dict(bit_depth=[8, 10][(j // 2) % 2], chroma_format=1, log2_ctb=5, width=200, height=128, no_split=1, calm=200, density=100,
                          qp=30, cu_qp_delta=1, mode_span=800)
        if kw["log2_ctb"] == 4 and kw["bit_depth"] == 8 and kw["chroma_format"] in (1, 2):
            kw["log2_ctb"] = 5  # quirk Q9 (see rare_syntax_sweep)
        if kw["bit_depth"] == 8:
            kw["tq_bypass"] = 0  # (the "pcmf" branch: see extreme_sweep)
        out.append((seed, kw))
    return out


def intra_single_ctb_cases(n, first_seed=17000):
    """(seed, parameters) of pictures of ONE CTB - the smallest shape at which each block size exists: CTB 16 / 32 / 64, every bit
    depth and chroma format, whole blocks and split ones, most coding units calm"""
    out = []
    for i in range(n):
        ctb = [4, 5, 6][i % 3]
        kw = dict(width=1 << ctb, height=1 << ctb, log2_ctb=ctb, bit_depth=[8, 10, 12][(i // 3) % 3], chroma_format=[1, 3, 0, 2][(i // 9) % 4],
                  no_split=(i // 36) % 2, calm=[800, 600][(i // 72) % 2], density=[60, 100][i % 2], strong_intra=1, qp=[24, 34][(i // 2) % 2], cu_qp_delta=1)
        if ctb == 4 and kw["bit_depth"] == 8 and kw["chroma_format"] in (1, 2):
            kw.update(sao=0)  # (quirk Q9 is one of SAO: these pictures are compared at the reconstruction stage only)
        out.append((first_seed + i, kw))
    return out


def intra_tiles():
    """512 x 512 tiles for the forced cuts of the prediction chains: half of their coding units calm, so that what a wave hands
    to the next one - border lines, corner samples - is a smooth ramp or a smear and not noise"""
    base = dict(width=512, height=512, cu_qp_delta=1, sao=1, sign_hiding=1, calm=500, density=60)
    return [(18000, dict(base, log2_ctb=5, qp=27, no_split=1)),
            (18001, dict(base, log2_ctb=6, bit_depth=10, chroma_format=2, qp=30)),
            (18002, dict(base, log2_ctb=4, chroma_format=0, qp=33, no_split=1)),
            (18003, dict(base, log2_ctb=5, qp=27, slices=40, dependent=300))]


def deblock_sweep(n, first_seed=19000):
    """(seed, parameters) of a seeded sweep for the deblocking filter (tests/deblock_ref.py holds it, decision by decision): pictures of
    64-200 samples a side whose sizes cut a window at the right and bottom border (72, 40, 136, 200), calm coding units next to noisy ones
    (smooth sides: the strong filter, dEp / dEq), QpY over its range with cu_qp_delta (QpP != QpQ, odd sums, the table indices clipped
    at both ends), slice offsets up to +-6 with per-slice overrides and disables, loop filters stopped at slice and tile borders, chroma
    QP offsets up to +-12, neighbours at both rails (level_span), PCM with and without pcm_loop_filter_disable and transquant bypass
    (every other run of 72 cases), whole blocks, every chroma format and CTB size, 8, 9, 10, 11 and 12 bit.  The comparisons are at the
    reconstruction and deblocking stages only, so quirk Q9 (one of SAO) does not enter, and 8-bit pictures of the "pcmf" branch are in:
    compared with the reference's default build (see SIMD_BUILD_ONLY).  Behind the 288 crossed cases follow cases aimed at the cells of
    the census (tests/deblockutil.py) that the crossed ones leave empty."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        r = (r ^ (r >> 15)) * 2246822519 % (1 << 32)
        r ^= r >> 13
        i = seed - first_seed
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        kw = dict(bit_depth=[8, 10, 11, 12, 8, 9][i % 6], chroma_format=[1, 2, 3, 0][(i // 6) % 4], log2_ctb=[5, 4, 6][(i // 24) % 3],
                  width=pick(0, [72, 136, 64, 200, 96, 40]), height=pick(3, [72, 40, 64, 136, 96]), calm=pick(6, [0, 500, 800, 300]),
                  qp=pick(8, [22, 30, 38, 45, 12, 51, 27, 34]), qp_span=pick(11, [0, 1, 0]), cu_qp_delta=1, diff_cu_qp_delta_depth=pick(13, [1, 0, 2]),
                  beta_offset_div2=pick(15, [0, -6, 6, 3, -2]), tc_offset_div2=pick(18, [0, 6, -6, -3, 2]), deblock_override=pick(21, [0, 1]),
                  slice_lf_random=pick(22, [0, 1]), pps_lf_across_slices_off=pick(23, [0, 0, 1]), slices=pick(25, [0, 0, 60, 150]),
                  dependent=pick(27, [0, 400]), cb_qp_offset=pick(1, [0, 12, -12, 5, -7]), cr_qp_offset=pick(4, [0, -12, 12, -3, 8]),
                  chroma_qp_list=pick(7, [0, 0, 2]), level_span=pick(9, [0, 0, 300, 1000]), no_split=pick(12, [0, 0, 1]),
                  log2_max_tb=pick(14, [5, 5, 4, 3]), density=pick(16, [20, 60, 100]), sign_hiding=pick(29, [1, 0]))
        kw["diff_cu_qp_delta_depth"] = min(kw["diff_cu_qp_delta_depth"], kw["log2_ctb"] - 3)
        if kw["chroma_format"] == 0:
            kw["chroma_qp_list"] = 0
        if not kw["slices"]:
            kw["dependent"] = 0
        if (i // 72) % 2 == 1:  # rare syntax: the plain scalar filters with their "pcmf" branches
            kw.update(pcm=pick(19, [0, 200, 300]), pcm_loop_filter_disable=pick(24, [1, 0]), tq_bypass=pick(26, [0, 250, 0, 150]), pcm_log2_max=pick(28, [5, 3, 4]))
            kw.update(pcm_bits_y=max(1, kw["bit_depth"] - seed % 3), pcm_bits_c=max(1, kw["bit_depth"] - seed % 4))
        if i % 5 == 3:
            kw.update(tile_cols=2, tile_rows=2, lf_across_tiles=i % 2, tiles_uniform=(i // 2) % 2, width=max(kw["width"], 136), height=max(kw["height"], 136))
        elif i % 7 == 2:
            kw.update(wpp=1)
        if i >= 288:
            # aimed cases, five families in turn: (0) flat pictures at the edges of QpY - both ends of both table indices, tc 0 beside beta > 0, QpC
            # in its three ranges and capped at 51; (1) calm pictures at the rails, half of them at 11 bit - the packed 16-bit filters one bit from
            # overflow; (2) short slices with overrides and disables, or tiles that stop the filter; (3) PCM (samples of one bit: flat runs that
            # the filter accepts) and bypass units next to calm ones under a large beta; (4) a large beta over a small tc on smooth ramps - the
            # strong filter against its 2 tc clip
            j = i - 288
            fam, k = j % 5, j // 5
            bd, cf, ctb = [8, 12, 10, 8, 11, 9, 12, 8][k % 8], pick(1, [1, 2, 3, 0, 1]), pick(4, [4, 5, 6])
            if fam == 0:
                kw = dict(bit_depth=bd, chroma_format=cf, log2_ctb=ctb, width=72, height=72, calm=[300, 600][k % 2], qp=[1, 51, 17, 20, 44, 30][k % 6], qp_span=(k // 6) % 2,
                          cu_qp_delta=1, diff_cu_qp_delta_depth=min(1, ctb - 3), beta_offset_div2=[6, -6, 0, -6, 6, 2][k % 6], tc_offset_div2=[-6, 6, 0, 6, -6, -1][k % 6],
                          cb_qp_offset=[12, -12, 6][k % 3], cr_qp_offset=[-12, 12, -6][k % 3], density=60)
            elif fam == 1:
                kw = dict(bit_depth=[11, 8, 11, 10, 11, 12, 11, 9][k % 8], chroma_format=cf, log2_ctb=ctb, width=72, height=72, calm=[200, 500][k % 2], qp=[45, 51, 38][k % 3], level_span=1000,
                          density=100, cu_qp_delta=1, tc_offset_div2=[6, 0][(k // 2) % 2], beta_offset_div2=[6, 0][(k // 2) % 2])
            elif fam == 2:
                kw = dict(bit_depth=bd, chroma_format=cf, log2_ctb=ctb, width=136, height=72, calm=500, qp=[27, 34, 40][k % 3], cu_qp_delta=1, slices=300, deblock_override=1,
                          slice_lf_random=1, slice_qp_random=1, density=60, scaling_list=[0, 2][(k // 4) % 2])  # (scaling lists: the rare classes)
                if k % 3 == 2:
                    kw.update(tile_cols=2, tile_rows=2, lf_across_tiles=0, slices=0, deblock_override=0, slice_lf_random=0)
            elif fam == 3:
                kw = dict(bit_depth=bd, chroma_format=cf, log2_ctb=ctb, width=72, height=72, calm=700, qp=[45, 51][k % 2], beta_offset_div2=6, tc_offset_div2=6, cu_qp_delta=1,
                          pcm=[700, 0, 600][k % 3], pcm_loop_filter_disable=[1, 0, 0][k % 3], tq_bypass=[0, 300, 150][k % 3], pcm_log2_max=3 + (k // 3) % 2,
                          pcm_bits_y=1, pcm_bits_c=[1, bd][(k // 6) % 2], density=60)
                if k % 3 != 1:
                    kw.update(width=136, height=136)  # (two PCM units side by side, both flat on the lines the decision reads: one unit in 256)
            else:
                kw = dict(bit_depth=[8, 12, 8, 12, 10, 8, 11, 9][k % 8], chroma_format=cf, log2_ctb=ctb, width=136, height=72, calm=[800, 600][k % 2], qp=[32, 38, 44][k % 3], beta_offset_div2=6, tc_offset_div2=-6,
                          cu_qp_delta=1, density=[30, 60][(k // 2) % 2], mode_span=[0, 800][(k // 4) % 2], scaling_list=[0, 2][(k // 8) % 2])  # (scaling lists: the rare classes)
        if kw["bit_depth"] == 8:
            kw["transform_skip"] = 0  # (Q10: the reference's builds round 8-bit 4x4 transform-skip blocks differently where levels are large - not a subject here)
        out.append((seed, kw))
    return out


def deblock_single_edge_cases(first_seed=22000):
    """(seed, parameters) of the smallest pictures that hold each kind of window of the one-pass deblocking kernels: 16x8 (one vertical edge
    in a top and a bottom half window), 8x16 (one horizontal edge in a left and a right half window) and 16x16 (the one crossing, where the
    horizontal edge reads what the vertical edge wrote; the corner windows hold no edge) - one CTB 16 of 8x8 units whose transform tree is
    not split any further (an NxN unit's 4x4 blocks meet off the 8-sample grid), no SAO, every bit depth and chroma format, QP over its range"""
    out = []
    seed = first_seed
    for w, h in ((16, 8), (8, 16), (16, 16)):
        for bd in (8, 9, 10, 11, 12):
            for cf in (1, 2, 3, 0):
                for k, qp in enumerate((1, 14, 27, 40, 51)):
                    out.append((seed, dict(width=w, height=h, log2_ctb=4, max_th_depth_intra=0, sao=0, bit_depth=bd, chroma_format=cf, qp=qp, cu_qp_delta=1,
                                           calm=[0, 500, 800][(seed + k) % 3], density=[60, 100][seed % 2], beta_offset_div2=[0, 3, -3][(seed // 5) % 3],
                                           tc_offset_div2=[0, -3, 3][(seed // 7) % 3], level_span=[0, 0, 1000][(seed // 3) % 3], transform_skip=int(bd > 8))))  # (8 bit: Q10, see deblock_sweep)
                    seed += 1
    return out


def deblock_tiles():
    """512 x 512 tiles for the deblocking phase of the fused tails, half of their coding units calm: 8-bit 4:2:0 of one slice (k_tail420
    with the edge parameters from the block map's copy in LDS), the same in 40 slices (the general derivation inside the fused tail), 10-bit
    4:2:0 (k_tail420's 16-bit instantiation) and 10-bit 4:2:2 limited range BT.2020 (k_tailf)"""
    return [(23000, dict(TILE, calm=500, vui=1, full_range=1, matrix=6)),
            (23001, dict(TILE, calm=500, vui=1, full_range=1, matrix=6, slices=40)),
            (23002, dict(TILE, calm=500, bit_depth=10, vui=1, full_range=1, matrix=9, primaries=9)),
            (23003, dict(TILE, calm=500, bit_depth=10, chroma_format=2, vui=1, full_range=0, matrix=9, primaries=9))]


def sao_class_q9(kw):
    """quirk Q9: 8-bit pictures with CTBs of 16 and sub-sampled chroma, SAO on - the reference's default build overruns there, its scalar build is the truth"""
    return kw.get("bit_depth", 8) == 8 and kw.get("log2_ctb", 5) == 4 and kw.get("chroma_format", 1) in (1, 2) and kw.get("sao", 1) != 0


def sao_class_pcmf8(kw):
    """8-bit pictures of the "pcmf" branch of the deblocking filter (SIMD_BUILD_ONLY tells why): the reference's default build for input and output alike"""
    return kw.get("bit_depth", 8) == 8 and bool((kw.get("pcm", 0) and kw.get("pcm_loop_filter_disable", 0)) or kw.get("tq_bypass", 0))


def _sao_settle(kw):
    if kw["bit_depth"] == 8:
        kw["transform_skip"] = 0  # (Q10, see deblock_sweep)
    if sao_class_pcmf8(kw) and sao_class_q9(kw):
        kw["log2_ctb"] = 5        # no picture is in both classes of the reference's builds
    if kw.get("chroma_format", 1) == 0:
        kw.pop("sao_scale_c", None)
    return kw


def sao_sweep(n, first_seed=24000):
    """(seed, parameters) of a seeded sweep for sample adaptive offset (tests/sao_ref.py holds it, sample by sample): pictures of 64x64 to
    128x96 samples - a sample goes wrong at a border or a rail, not at size.  120 crossed cases over bit depth 8-12, every chroma format and
    CTB size, with slices whose filter and SAO flags are drawn per slice, tiles, PCM / bypass units every other run of 60, offsets and band
    positions at the ends of their ranges (sao_span) and levels at the rails.  Behind them follow families aimed at the cells of the census
    (tests/saoutil.py): (0) short slices with staircase borders inside a CTB row, flags per slice, the PPS flag off in every third; (1) tiles,
    uniform and not, the filters crossing their borders or not; (2) tiles and slices together; (3) PCM with and without
    pcm_loop_filter_disable and bypass units; (4) scaled offsets at 11 and 12 bit; (5) samples at both rails under the largest offsets;
    (6) conformance windows whose left offset is and is not a multiple of 8 in each plane; (7) sizes that are no multiple of the CTB, chroma
    widths of 8 k + 4; (8) two tiles one above the other whose border the filters cross, cut into slices of a few CTBs with flags of their own: with tiles
    the reference leaves its fast path, and only there do the slices' flags differ inside a picture without PCM / bypass units - a diagonal neighbour CTB
    stopped between usable ones and the reverse."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        r = (r ^ (r >> 15)) * 2246822519 % (1 << 32)
        r ^= r >> 13
        i = seed - first_seed
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        if i < 120:
            kw = dict(bit_depth=[8, 9, 10, 11, 12][i % 5], chroma_format=[1, 2, 3, 0][(i // 5) % 4], log2_ctb=[4, 5, 6][(i // 20) % 3],
                      width=pick(0, [64, 72, 96, 104, 128, 88]), height=pick(3, [64, 72, 96, 80]), calm=pick(6, [0, 500, 300]), qp=pick(8, [22, 30, 38, 45, 27, 34]),
                      cu_qp_delta=1, slices=pick(11, [0, 60, 150]), slice_lf_random=pick(13, [0, 1]), slice_sao_random=pick(14, [0, 1]),
                      pps_lf_across_slices_off=pick(15, [0, 0, 1]), dependent=pick(17, [0, 400]), level_span=pick(19, [0, 0, 300, 1000]),
                      sao_span=pick(21, [0, 300, 600]), density=pick(23, [20, 60, 100]), sign_hiding=pick(25, [1, 0]))
            if not kw["slices"]:
                kw["dependent"] = 0
            if (i // 60) % 2 == 1:  # rare syntax
                kw.update(pcm=pick(26, [0, 200, 300]), pcm_loop_filter_disable=pick(28, [1, 0]), tq_bypass=pick(29, [0, 250, 0, 150]), pcm_log2_max=pick(30, [5, 3, 4]),
                          pcm_bits_y=max(1, kw["bit_depth"] - seed % 3), pcm_bits_c=max(1, kw["bit_depth"] - seed % 4))
            if i % 7 == 3:
                kw.update(tile_cols=2, tile_rows=2, lf_across_tiles=(i // 7) % 2, tiles_uniform=(i // 14) % 2, width=128, height=96)
        else:
            j = i - 120
            fam, k = j % 9, j // 9
            bd, cf, ctb = [8, 12, 10, 8, 11, 9, 8, 10][k % 8], [1, 2, 3, 0, 1, 2, 1][k % 7], [4, 5, 6, 4, 5][k % 5]
            rare = dict(scaling_list=[0, 0, 0, 2][k % 4])  # (scaling lists: the rare classes without PCM / bypass units)
            kw = dict(bit_depth=bd, chroma_format=cf, log2_ctb=ctb, width=128, height=96, qp=pick(8, [27, 34, 40, 22]), cu_qp_delta=1, density=60,
                      calm=pick(6, [0, 300]), sao_span=pick(21, [0, 300, 600]))
            if fam == 0:
                kw.update(rare, slices=[300, 500, 150][k % 3], slice_lf_random=1, slice_sao_random=(k // 2) % 2, pps_lf_across_slices_off=int(k % 3 == 2), dependent=[0, 300][(k // 3) % 2],
                          width=[128, 96, 112][k % 3], height=[96, 64, 80][(k // 3) % 3])
            elif fam == 1:
                kw.update(rare, tile_cols=[2, 3, 2][k % 3], tile_rows=[2, 2, 3][(k // 3) % 3], lf_across_tiles=k % 2, tiles_uniform=(k // 2) % 2)
            elif fam == 2:
                kw.update(rare, tile_cols=2, tile_rows=2, lf_across_tiles=int(k % 3 != 0), tiles_uniform=(k // 2) % 2, slices=[150, 300][k % 2], slice_lf_random=1,
                          slice_sao_random=(k // 4) % 2, dependent=[0, 300][(k // 3) % 2])
            elif fam == 3:
                kw.update(pcm=[300, 0, 400][k % 3], pcm_loop_filter_disable=[1, 0, 0][k % 3], tq_bypass=[0, 300, 150][k % 3], pcm_log2_max=3 + (k // 3) % 3,
                          pcm_bits_y=max(1, bd - k % 3), pcm_bits_c=max(1, bd - k % 4), slices=[0, 150][(k // 2) % 2], slice_lf_random=1, width=96, height=72,
                          level_span=[0, 1000][(k // 4) % 2], sao_span=600)
            elif fam == 4:
                deep = [12, 11, 12][k % 3]
                kw.update(rare, bit_depth=deep, sao_scale_y=[deep - 10, 1, 0][(k // 3) % 3], sao_scale_c=[deep - 10, 0, 1][(k // 3) % 3], sao_span=[700, 400][k % 2], level_span=[1000, 300][(k // 2) % 2],
                          width=96, height=64)
            elif fam == 5:
                kw.update(rare, level_span=1000, qp_span=(k // 2) % 2, qp=[51, 45, 48][k % 3], sao_span=[800, 500][k % 2], density=100, calm=0, width=96, height=64,
                          slices=[0, 100][(k // 4) % 2], slice_lf_random=1)
                if bd == 12:
                    kw.update(sao_scale_y=[0, 2][(k // 2) % 2], sao_scale_c=[2, 0][(k // 2) % 2])
            elif fam == 6:
                kw.update(rare, conf_left=[8, 0, 6, 16, 2, 24, 12][k % 7], conf_right=[4, 10, 0, 8, 2][k % 5], conf_top=[0, 2, 8, 6][(k // 3) % 4], conf_bottom=[0, 6, 2][(k // 5) % 3],
                          slices=[0, 150, 300][(k // 2) % 3], slice_lf_random=1, width=[128, 96, 104][k % 3], height=[96, 72][(k // 3) % 2])
                if (k // 4) % 3 == 2:
                    kw.update(tile_cols=2, tile_rows=2, lf_across_tiles=0, slices=0)
            elif fam == 8:
                kw.update(scaling_list=[0, 2][k % 2], bit_depth=[8, 8, 10, 8, 12, 8, 11, 9][k % 8], log2_ctb=[4, 4, 5][k % 3], tile_cols=1, tile_rows=2, lf_across_tiles=1, slices=[500, 700, 350][k % 3], slice_lf_random=1, sao_span=300,
                          level_span=[0, 1000][(k // 2) % 2])
            else:
                kw.update(rare, width=[72, 88, 104, 120, 80][k % 5], height=[72, 80, 88, 72][(k // 5) % 4], slices=[0, 200][(k // 2) % 2], slice_lf_random=1, slice_sao_random=(k // 4) % 2,
                          level_span=[0, 1000][(k // 3) % 2])
        out.append((seed, _sao_settle(kw)))
    return out


def sao_small_cases(first_seed=26000):
    """(seed, parameters) of pictures of exactly one CTB of 16, 32 and 64 samples (every neighbour CTB is missing: each edge class meets the picture's
    border on both sides), of 2 x 2 CTBs (one crossing of CTB borders, sliced so that the diagonal CTB and the ones beside it get answers of their own) and
    of strips one CTB wide / one CTB high, at every bit depth and chroma format"""
    out = []
    seed = first_seed
    for ctb in (4, 5, 6):
        n = 1 << ctb
        for shape, (w, h) in enumerate(((n, n), (2 * n, 2 * n), (n, 4 * n if ctb < 6 else 2 * n), (4 * n if ctb < 6 else 2 * n, n))):
            for bd in (8, 9, 10, 11, 12):
                for cf in (1, 2, 3, 0):
                    kw = dict(width=w, height=h, log2_ctb=ctb, bit_depth=bd, chroma_format=cf, qp=[27, 38, 45][seed % 3], cu_qp_delta=1, density=[60, 100][seed % 2],
                              sao_span=[0, 500, 800][(seed // 2) % 3], level_span=[0, 0, 1000][(seed // 3) % 3], calm=[0, 300][(seed // 5) % 2])
                    if shape:
                        kw.update(slices=[0, 400, 600][(seed // 4) % 3], slice_lf_random=1, slice_sao_random=(seed // 8) % 2)
                    out.append((seed, _sao_settle(kw)))
                    seed += 1
    return out


SAO_TILE_W, SAO_TILE_H = 192, 144


def sao_tiles():
    """tiles for the SAO phase of the fused tails, one per instance that the test hook hm_debug_batch_tail can name, 192 x 144 samples each (one and a half
    cells of the fused kernels wide, CTBs cut at the bottom; test_sao_gpu.py tells why this is the smallest useful canvas): k_tail420 on 8-bit samples with
    CTBs of 16 (UNI off), with CTBs of 32 in one slice (UNI; all_ok in the CTBs off the picture's border), with CTBs of 32 in several slices whose flags stop
    the filters at their borders (the batch fuses such a picture only while the PPS flag is on: SAO then takes the reference's fast path, and the mask is not
    0xFF at the picture's border alone), its 16-bit instantiation (a 10-bit picture, compared after its shift to 8 bits: offsets at their largest let most
    changes survive it), and k_tailf<uint8_t / uint16_t, 4:2:0 / 4:2:2>"""
    base = dict(width=SAO_TILE_W, height=SAO_TILE_H, log2_ctb=5, qp=30, cu_qp_delta=1, sao=1, sign_hiding=1, calm=300, density=60, vui=1, sao_span=500, transform_skip=0)
    deep = dict(base, bit_depth=10, transform_skip=1)
    return [(27000, dict(base, log2_ctb=4, full_range=1, matrix=6)),
            (27001, dict(base, full_range=1, matrix=6)),
            (27002, dict(base, full_range=1, matrix=6, slices=40, slice_lf_random=1)),
            (27003, dict(deep, full_range=1, matrix=9, primaries=9, sao_span=900)),
            (27004, dict(base, full_range=0, matrix=1)),
            (27005, dict(deep, full_range=1, matrix=1)),
            (27006, dict(base, chroma_format=2, full_range=1, matrix=6)),
            (27007, dict(deep, chroma_format=2, full_range=0, matrix=9, primaries=9))]


def rext_pcmf8(kw):
    """8-bit pictures of the "pcmf" deblocking branch (see SIMD_BUILD_ONLY): held to the reference's default build from the deblocking stage on"""
    return sao_class_pcmf8(kw)


def _rext_settle(kw, pcmf8_family=False):
    if kw.get("chroma_format", 1) != 3:
        kw["cross_component"] = 0
    if kw.get("pcm"):
        kw.setdefault("pcm_bits_y", kw["bit_depth"])
        kw.setdefault("pcm_bits_c", kw["bit_depth"])
    if kw["bit_depth"] == 8 and not pcmf8_family:
        kw.update(tq_bypass=0, pcm_loop_filter_disable=0)  # (the "pcmf" branch runs in a family of its own: see rext_residual_sweep)
    if kw["log2_ctb"] == 4 and kw["bit_depth"] == 8 and kw.get("chroma_format", 1) in (1, 2):
        kw["sao"] = 0  # (quirk Q9 is one of SAO on such pictures)
    return kw


def rext_residual_sweep(n, first_seed=28000):
    """(seed, parameters) of a seeded sweep for the range-extension residual tools (tests/residual_ref.py holds them block by block:
    implicit RDPCM, transform-skip rotation, cross-component prediction, PCM), pictures of 64x64 to 128x96 samples (128x128 where whole
    32x32 blocks need full CTBs of 64).  Every picture carries rare syntax, so all of them go out in decode order (k_recon's rare
    instances).  144 crossed cases over bit depth 8 / 10 / 12, the four chroma formats, CTB 16 / 32 / 64 and the tools - implicit RDPCM
    in all of them, rotation, log2_max_transform_skip_block_size 2-5, transquant bypass, PCM, scaling lists, whole blocks, modes drawn
    whole (mode_span: mode 10 is no most-probable mode) -, then ten aimed families (the first nine in turn, more of some of them and the tenth behind), each over the three depths and CTB sizes and, where
    it draws whole blocks, over 32x32, 16x16 and 8x8 as the largest transform:
      (0) whole 32x32 blocks (16x16 with CTB 16) of both skip kinds with levels over their whole range: RDPCM runs of 32;
      (1) 4:4:4 with cross-component prediction over every luma kind, whole and split blocks;
      (2) the same at 12 bit with every unit bypassed, whole 32x32 blocks and most levels at +-32767 (level_sat): |rY| up to 32 x 32767, the
          one regime in which the reference's 32-bit shift pair can wrap, at |rY| >= 2^19;
      (3) 8-bit 4:4:4 split pictures at a low QP with levels over their whole range: 4x4 transform-skip chroma blocks (the reference's
          16-bit arm) under the largest luma residuals a 4x4 luma block can have;
      (4) PCM of every size from 8x8 to 32x32 with PCM bit depths from 1 to the sample depth, next to bypass and ordinary units;
      (5) scaling lists (pinned at 1 and 255 in places) together with skip and RDPCM blocks;
      (6) 8 bit WITH transquant bypass and unfiltered PCM: the "pcmf" deblocking branch, on which the reference's two builds disagree
          (see SIMD_BUILD_ONLY) - these pictures are held to its scalar build at the reconstruction stage and to its default build from
          the deblocking stage on, and draw large levels only where they draw no transform skip (Q10 would make the builds differ at the
          reconstruction stage too);
      (7) every unit bypassed, levels over their whole range and many at +-32767 (level_sat): RDPCM run sums beyond 16 bits at every size, bypass luma under bypass chroma blocks
          with a cross-component term (8 bit: as family 6, without transform skip);
      (8) 4:4:4 with cross-component prediction and transform skip up to 32x32, modes drawn whole: skip chroma blocks with RDPCM under skip luma
          blocks with RDPCM.
      (9) transform skip up to 32x32 without bypass, full blocks of levels at +-32767 (level_sat) at 8 and 12 bit: RDPCM run sums of rounded skip
          elements beyond 16 bits, and in 4:4:4 at 12 bit the shift pair wrapping behind skip luma blocks of 16x16 and 32x32.
    Everywhere else 8-bit pictures run without bypass and with filtered PCM."""
    out = []
    for seed in range(first_seed, first_seed + n):
        r = seed * 2654435761 % (1 << 32)
        r = (r ^ (r >> 15)) * 2246822519 % (1 << 32)
        r ^= r >> 13
        i = seed - first_seed
        pick = lambda k, opts: opts[(r >> k) % len(opts)]
        fam = None
        if i < 144:
            kw = dict(bit_depth=[8, 10, 12][i % 3], chroma_format=[1, 3, 0, 2][(i // 3) % 4], log2_ctb=[5, 4, 6][(i // 12) % 3],
                      width=pick(0, [64, 96, 128, 72]), height=pick(2, [64, 40, 96, 72]), qp=pick(4, [27, 22, 33, 38]), cu_qp_delta=1,
                      rext_sps=pick(6, [4, 5, 7, 4 | 128, 5 | 32, 7]), log2_max_ts=pick(9, [5, 3, 4, 5, 0]), tq_bypass=pick(12, [0, 250, 0, 500]),
                      pcm=pick(14, [0, 0, 200]), pcm_loop_filter_disable=seed % 2, no_split=pick(16, [0, 1, 0]), level_span=pick(18, [0, 300, 0, 1000]),
                      scaling_list=pick(20, [0, 0, 2]), mode_span=pick(22, [0, 500, 800]), density=pick(24, [60, 100, 30]), wpp=pick(26, [0, 0, 1]),
                      slices=pick(28, [0, 0, 100]), sign_hiding=pick(30, [1, 0]), cross_component=int(seed % 3 != 0))
            kw.update(pcm_bits_y=max(1, kw["bit_depth"] - seed % 3), pcm_bits_c=max(1, kw["bit_depth"] - seed % 4))
        else:
            j = i - 144
            fam, k = j % 9, j // 9
            bd, ctb, cf = [8, 10, 12][k % 3], [5, 4, 6][(k // 3) % 3], [1, 3, 0, 2][(k // 9) % 4]
            tb = [5, 4, 3][(k // 9) % 3]
            fill = j >= 9 * 54
            if fill:
                # behind the nine families, more 4:4:4 pictures of whole blocks of families 7, 8 and 4 (in that order), two thirds of them 8 bit,
                # CTB 32 / 64 before CTB 16: the cells of large blocks, which hold few blocks a picture
                j -= 9 * 54
                fam, k = [7, 8, 4][j % 3], j // 3
                bd, ctb, cf, tb = [8, 10, 8, 12, 8][k % 5], [6, 5, 6, 4][(k // 5) % 4], 3, [4, 5, 3, 2][(k // 20) % 4]  # (2: a split picture)
                if j >= 360:  # ... and behind those, families 8 and 7 at 8 bit alone, CTB 32 / 64
                    j -= 360
                    fam, k = [8, 7][j % 2], j // 2
                    bd, ctb, tb = 8, [6, 5, 6][k % 3], [5, 4, 2, 3, 4, 3][(k // 3) % 6]
                    if j >= 108:  # ... and last, family 9: 8 and 12 bit, every CTB size, the largest transform 16x16, 32x32, 4x4 (split pictures) and 8x8 in turn
                        j -= 108
                        fam, k = 9, j
                        bd, ctb, tb, cf = [8, 12, 12][k % 3], [5, 6, 4][(k // 3) % 3], [4, 5, 2, 3][(k // 9) % 4], [3, 1, 3, 3][(k // 36) % 4]
                        if k >= 144:  # (the one cell that 144 cases leave empty: 32x32 chroma skip blocks with RDPCM at 8 bit under CTB 64, 72 blocks a picture)
                            bd, ctb, tb, cf = 8, 6, 5, 3
            # whole blocks of 32x32, 16x16 and 8x8 in turn (the largest transform; CTB 16: 16x16 at most)
            whole = dict(width=128, height=128 if ctb == 6 else 96, no_split=1, log2_max_tb=tb)
            if ctb > 4 and whole["log2_max_tb"] == 5:
                whole.update(width=192, height=128)  # (24 blocks of 32x32: mode 10 is one mode in 32 where modes are drawn whole)
            kw = dict(bit_depth=bd, chroma_format=cf, log2_ctb=ctb, qp=pick(4, [27, 22, 33, 38]), cu_qp_delta=1, density=100)
            if fam == 0:
                kw.update(whole, rext_sps=[4, 5, 4 | 128][k % 3], log2_max_ts=5, level_span=[600, 1000][k % 2], level_sat=[0, 500][(k // 2) % 2], tq_bypass=[0, 400][(k // 2) % 2],
                          mode_span=800, cross_component=(k // 4) % 2)
            elif fam == 1:
                kw.update(chroma_format=3, cross_component=1, rext_sps=[0, 4, 5, 7][k % 4], log2_max_ts=[5, 4, 0, 3][(k // 2) % 4], tq_bypass=[0, 300][(k // 4) % 2],
                          mode_span=[0, 800][k % 2], level_span=[0, 300][(k // 2) % 2], width=[64, 96, 128][k % 3], height=[64, 96][(k // 3) % 2])
                if k % 2:
                    kw.update(whole)
            elif fam == 2:
                kw.update(whole, bit_depth=12, chroma_format=3, log2_ctb=[5, 6][k % 2], cross_component=1, rext_sps=4, tq_bypass=1000, level_span=1000, level_sat=[1000, 800][(k // 2) % 2],
                          mode_span=[0, 0, 400][(k // 4) % 3], log2_max_tb=5, width=192, height=128)  # (without mode_span mode 26 is a most-probable mode everywhere)
            elif fam == 3:
                kw.update(bit_depth=8, chroma_format=3, cross_component=1, rext_sps=[5, 4, 7][k % 3], log2_max_ts=[0, 3][k % 2], qp=[1, 8, 17][(k // 2) % 3], level_span=[1000, 600][(k // 3) % 2],
                          width=64, height=64, max_th_depth_intra=2)
            elif fam == 4:
                kw.update(pcm=[300, 500, 800][k % 3], pcm_log2_max=[5, 3, 4][(k // 2) % 3], pcm_log2_min=3, pcm_bits_y=1 + (k * 5) % bd, pcm_bits_c=1 + (k * 7 + 3) % bd,
                          pcm_loop_filter_disable=k % 2, tq_bypass=[200, 0][(k // 3) % 2], rext_sps=[4, 0, 5][(k // 2) % 3], cross_component=k % 2, width=[96, 128, 64][k % 3],
                          height=[64, 96][(k // 3) % 2], no_split=(k // 2) % 2)
                if kw["pcm_log2_max"] < min(ctb, 5):
                    kw["no_split"] = 0  # (whole coding units would be larger than the largest PCM unit: a picture without rare syntax after all)
                if (k // 9) % 2:
                    kw.update(pcm_bits_y=[1, bd][k % 2], pcm_bits_c=[bd, 1][k % 2])
                if fill:
                    kw.update(whole, log2_max_tb=5, pcm=900, pcm_log2_max=5, pcm_log2_min=[5, 3][k % 2], width=128, height=128, no_split=int(ctb < 6))  # (a PCM unit is 32x32 at most)
            elif fam == 5:
                kw.update(scaling_list=[2, 3][k % 2], scaling_span=500, rext_sps=[5, 4, 7][k % 3], log2_max_ts=[5, 4][(k // 2) % 2], level_span=[0, 300, 1000][(k // 2) % 3],
                          tq_bypass=[0, 200][(k // 4) % 2], mode_span=[800, 0][(k // 3) % 2], cross_component=k % 2, no_split=(k // 3) % 2, width=[96, 128][k % 2], height=[64, 96][(k // 2) % 2])
            elif fam == 7:
                kw.update(chroma_format=[3, 1, 3, 2, 0][(k // 9) % 5], cross_component=1, rext_sps=[4, 5][k % 2], tq_bypass=1000, level_span=1000, level_sat=[600, 1000][k % 2],
                          mode_span=[800, 400][(k // 2) % 2], width=[64, 96][k % 2], height=64)
                if ((k // 27) % 2 == 0 or k % 2) if not fill else tb > 2:
                    kw.update(whole)
                if bd == 8:
                    kw.update(transform_skip=0)
            elif fam == 8:
                kw.update(chroma_format=3, cross_component=1, rext_sps=[4, 5][k % 2], log2_max_ts=5, mode_span=800, level_span=[0, 300][(k // 2) % 2], width=[64, 96][k % 2], height=64)
                if ((k // 27) % 2 == 0 or k % 2) if not fill else tb > 2:
                    kw.update(whole)
            elif fam == 9:
                kw.update(cross_component=1, rext_sps=[4, 5][k % 2], log2_max_ts=5, level_span=1000, level_sat=[1000, 700][(k // 2) % 2], mode_span=[0, 800][(k // 4) % 2],
                          width=64, height=64)
                if tb > 2:
                    kw.update(whole)
            else:
                kw.update(bit_depth=8, log2_ctb=[5, 4, 6][k % 3], chroma_format=[1, 3, 0, 2, 3][(k // 3) % 5], tq_bypass=[300, 600, 1000][k % 3], pcm=[300, 0, 500][(k // 2) % 3],
                          pcm_loop_filter_disable=1, pcm_bits_y=[8, 5, 1][(k // 3) % 3], pcm_bits_c=[7, 8, 2][(k // 4) % 3], rext_sps=[4, 5, 7][(k // 2) % 3], log2_max_ts=[5, 0, 4][k % 3],
                          cross_component=1, mode_span=[800, 0][(k // 2) % 2], no_split=(k // 4) % 2, width=[96, 128, 64][k % 3], height=[64, 96][(k // 3) % 2])
                if kw["no_split"]:
                    kw.update(width=128, height=128 if kw["log2_ctb"] == 6 else 96)
                if k % 2:  # no transform skip at all: large levels are then safe (Q10 is one of 8-bit 4x4 transform-skip blocks) - bypass run sums beyond 16 bits
                    kw.update(transform_skip=0, level_span=1000)
        out.append((seed, _rext_settle(kw, pcmf8_family=fam == 6 or (fam == 7 and kw["bit_depth"] == 8))))
    return out


def rext_residual_single_ctb_cases(n_per_shape=36, first_seed=32000):
    """(seed, parameters) of pictures of ONE CTB whose first transform block of every component predicts the constant 1 << (bit_depth - 1): its
    samples are clip(that + residual), the residual of the range-extension tools alone.  The shapes of single_ctb_cases (first block 4x4, 8x8,
    16x16, and 32x32 with CTB 32 and CTB 64), every bit depth and chroma format, log2_max_transform_skip_block_size up to 5, rotation on and
    off, cross-component prediction, PCM, transquant bypass - at 8 bit too: these pictures have no loop filters (sao = 0, deblocking disabled),
    so the "pcmf" branch on which the reference's builds disagree does not exist in them."""
    shapes = [dict(width=8, height=8, log2_ctb=4, no_split=0), dict(width=8, height=8, log2_ctb=4, no_split=1),
              dict(width=16, height=16, log2_ctb=4, no_split=1), dict(width=32, height=32, log2_ctb=5, no_split=1),
              dict(width=64, height=64, log2_ctb=6, no_split=1)]
    out = []
    seed = first_seed
    for shape in shapes:
        for k in range(n_per_shape):
            r = seed * 2654435761 % (1 << 32)
            r = (r ^ (r >> 15)) * 2246822519 % (1 << 32)
            r ^= r >> 13
            pick = lambda s, opts: opts[(r >> s) % len(opts)]
            bd = [8, 10, 12][k % 3]
            kw = dict(shape, bit_depth=bd, chroma_format=[1, 3, 2, 0][(k // 3) % 4], qp=pick(3, [1, 17, 26, 35, 44, 51]), density=100, cu_qp_delta=1, diff_cu_qp_delta_depth=0,
                      level_span=pick(6, [0, 120, 400, 1000]), rext_sps=[4, 5, 7][(k // 12) % 3], log2_max_ts=pick(9, [5, 5, 3]), tq_bypass=pick(11, [0, 0, 300, 1000]),
                      cross_component=k % 2, pcm=pick(14, [0, 0, 300]), pcm_bits_y=1 + (k * 5) % bd, pcm_bits_c=1 + (k * 7 + 3) % bd, pcm_loop_filter_disable=k % 2,
                      mode_span=pick(16, [0, 800]), scaling_list=pick(18, [0, 0, 2]), sao=0, deblock_disable=1, sign_hiding=pick(20, [1, 0]))
            if kw["chroma_format"] != 3:
                kw["cross_component"] = 0
            out.append((seed, kw))
            seed += 1
    return out


def rext_residual_lock_pictures():
    """pictures whose every CTB row is full of whole 32x32 blocks with residuals (no_split, density 100), 64x128 with CTB 32 and 128x192 with CTB 64:
    in k_recon every wave of a workgroup takes the workgroup's one 32x32 staging area for such a block - nothing smaller has two waves contend"""
    base = dict(no_split=1, density=100, cu_qp_delta=1, rext_sps=5, log2_max_ts=5, mode_span=800)
    return [(30000, dict(base, width=64, height=128, log2_ctb=5, bit_depth=8, chroma_format=3, cross_component=1, qp=27)),
            (30001, dict(base, width=128, height=192, log2_ctb=6, bit_depth=10, chroma_format=3, cross_component=1, tq_bypass=300, qp=30, level_span=300)),
            (30002, dict(base, width=128, height=192, log2_ctb=6, bit_depth=12, chroma_format=1, tq_bypass=300, qp=33))]


def rext_residual_tiles():
    """four 192 x 144 tiles with the range-extension residual tools, through the full path"""
    base = dict(width=SAO_TILE_W, height=SAO_TILE_H, cu_qp_delta=1, sao=1, density=60, log2_max_ts=5)
    return [(31000, dict(base, log2_ctb=5, bit_depth=8, chroma_format=3, cross_component=1, rext_sps=5, qp=27)),
            (31001, dict(base, log2_ctb=6, bit_depth=10, chroma_format=3, cross_component=1, rext_sps=7, tq_bypass=200, qp=30, level_span=300)),
            (31002, dict(base, log2_ctb=4, bit_depth=12, chroma_format=1, rext_sps=4, tq_bypass=200, pcm=200, pcm_bits_y=9, pcm_bits_c=7, pcm_loop_filter_disable=1, qp=33)),
            (31003, dict(base, log2_ctb=5, bit_depth=10, chroma_format=2, rext_sps=5, pcm=200, pcm_bits_y=10, pcm_bits_c=8, scaling_list=2, qp=25, no_split=1))]
