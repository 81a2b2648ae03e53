/* heif_mi355x.h — C ABI of the MI355X (gfx950) HEIC hot path.
 *
 * Drop-in boundary for the path  heif_decode_image() -> grid -> per-tile HEVC-intra
 * reconstruction -> deblock -> SAO -> paste -> YCbCr->RGB  of aliyun/heif-decoder-lib.
 * Plain pointers and sizes only; no C++/torch types.  Device pointers are raw HIP
 * device addresses (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed
 * as void* (NULL = the default stream).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   hm_colour_convert        <- convert_colorspace()               libheif/color-conversion/colorconversion.cc:487-596
 *                               Op_YCbCr420_to_RGB24/32            libheif/color-conversion/yuv2rgb.cc:306-366, 416-495
 *                               Op_YCbCr_to_RGB<u8/u16> + repack   yuv2rgb.cc:79-254, rgb2rgb.cc:66-143,189-272,676-729
 *                               Op_YCbCr420_to_RRGGBBaa            yuv2rgb.cc:550-643
 *   hm_plane_stride          <- HeifPixelImage::ImagePlane::alloc  libheif/pixelimage.cc:139-218
 *   hm_ycbcr_coefficients    <- get_YCbCr_to_RGB_coefficients      libheif/nclx.cc:152-171
 *   hm_hevc_parse / hm_stream_* <- libde265 slice-data parsing     third-party/libde265/libde265/slice.cc:2886-5600
 *                               (CABAC stays on the host; output = the GPU command stream, hm_stream.h)
 *   hm_batch_* / hm_decode_* <- decode_full_grid_image + decode_and_paste_tile_image
 *                                                                  libheif/context.cc:2120-2539
 *                               and libde265's reconstruction      transform.cc, intrapred.{h,cc}, deblock.cc, sao.cc
 *
 * Every function returns HM_OK (0) or a negative hm_status; nothing falls back to a
 * CPU implementation: if the HIP runtime / device is missing the call fails with
 * HM_ERR_NO_DEVICE.
 */
#ifndef HEIF_MI355X_H
#define HEIF_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define HM_API __attribute__((visibility("default")))
#else
#define HM_API
#endif

typedef enum hm_status {
  HM_OK = 0,
  HM_ERR_INVALID_ARG = -1,
  HM_ERR_UNSUPPORTED = -2,     /* syntax / format outside the supported hot path      */
  HM_ERR_BITSTREAM = -3,       /* malformed HEVC / HEIF input                           */
  HM_ERR_NO_DEVICE = -4,       /* no HIP device, or a HIP call failed                   */
  HM_ERR_NOMEM = -5,
  HM_ERR_INTERNAL = -6,
} hm_status;

HM_API const char* hm_status_string(int status);
/* last error detail for the calling thread (static storage, never NULL) */
HM_API const char* hm_last_error(void);
/* What kind of failure the calling thread's last error was, where callers branch on more than the status: the decoder plugin
 * maps HM_DETAIL_END_OF_DATA - a [length][NAL] record that runs past the pushed bytes - to heif_suberror_End_of_data as the
 * reference's plugin does (libheif/plugins/decoder_libde265.cc:276-292).  Set by the call that failed, HM_DETAIL_NONE otherwise. */
typedef enum hm_error_detail { HM_DETAIL_NONE = 0, HM_DETAIL_END_OF_DATA = 1,
  HM_DETAIL_NO_COLOUR_CHAIN = 2 /* convert_colorspace() finds no chain: heif_suberror_Unsupported_color_conversion */,
  HM_DETAIL_INVALID_OVERLAY_DATA = 3 /* an 'iovl' payload that is truncated, has a zero canvas size or too few offsets: heif_suberror_Invalid_overlay_data */,
  HM_DETAIL_UNSUPPORTED_DATA_VERSION = 4 /* an 'iovl' payload of another version than 0: heif_suberror_Unsupported_data_version */ } hm_error_detail;
HM_API int hm_last_error_detail(void);
HM_API const char* hm_version(void);
/* number of visible HIP devices (0 if none); does not initialise a context */
HM_API int hm_device_count(void);

/* ------------------------------------------------------------------------- */
/* Colour conversion                              */
/* ------------------------------------------------------------------------- */

/* values equal enum heif_chroma (libheif/api/libheif/heif.h:481-494) */
enum {
  HM_CHROMA_MONO = 0, HM_CHROMA_420 = 1, HM_CHROMA_422 = 2, HM_CHROMA_444 = 3,
  HM_OUT_RGB = 10, HM_OUT_RGBA = 11, HM_OUT_RRGGBB_BE = 12, HM_OUT_RRGGBBAA_BE = 13, HM_OUT_RRGGBB_LE = 14, HM_OUT_RRGGBBAA_LE = 15,
  /* planar YCbCr at the chroma format the caller asks for (heif_colorspace_YCbCr with heif_chroma_420 / _422 / _444): the
   * decoded planes go through the chain convert_colorspace() finds for that target; a target that equals the image's own
   * format converts nothing.  Low two bits = HM_CHROMA_* of the target. */
  HM_OUT_YCBCR_420 = 0x101, HM_OUT_YCBCR_422 = 0x102, HM_OUT_YCBCR_444 = 0x103,
  /* or-ed to a planar code where no convert_hdr_to_8bit field exists (hm_colour_desc, hm_pipeline_config):
   * convert_colorspace()'s output_bpp = 8.  hm_decode_params callers may set convert_hdr_to_8bit instead. */
  HM_OUT_YCBCR_8BIT = 0x200,
};

typedef struct hm_colour_desc {
  int32_t width, height;        /* luma size in pixels                                         */
  int32_t bit_depth;            /* 8..16; planes are uint8 (8) or uint16 little-endian (>8)    */
  int32_t chroma;               /* HM_CHROMA_MONO (d_cb / d_cr unused) / _420 / _422 / _444      */
  int32_t has_nclx;             /* 0: image carries no nclx (every grid canvas) => defaults     */
  int32_t matrix, primaries, full_range; /* the attached nclx (ignored when !has_nclx)          */
  int32_t out_format;           /* HM_OUT_* (a planar HM_OUT_YCBCR_* code: hm_colour_convert_planar only)  */
  int32_t y_stride, cb_stride, cr_stride, out_stride; /* bytes                                  */
  int32_t chroma_upsampling;    /* 0 / HM_UPSAMPLE_NEAREST: whatever convert_colorspace() would pick (nearest
                                   neighbour ops); HM_UPSAMPLE_BILINEAR: the caller set
                                   only_use_preferred_chroma_algorithm with heif_chroma_upsampling_bilinear
                                   (heif.h:1546-1562) => Op_YCbCr420/422_bilinear_to_YCbCr444 first           */
  int32_t has_alpha;            /* the image carries an alpha plane.  The planes converted here do not include it (the
                                   callers add it to the pixels afterwards), but it decides the reference's chain for one
                                   case: an 8-bit 4:2:0 image reaches RRGGBBAA through Op_to_hdr_planes +
                                   Op_YCbCr420_to_RRGGBBaa only when it has an alpha plane - without one that op ends in
                                   RRGGBB and the float op on 8 bits comes first (different arithmetic)            */
} hm_colour_desc;
enum { HM_UPSAMPLE_NEAREST = 1, HM_UPSAMPLE_BILINEAR = 2 }; /* == enum heif_chroma_upsampling_algorithm */

/* which reference op chain convert_colorspace() picks for this state: the product runs the reference's pipeline SEARCH
 * (colorconversion.cc:266-420, restated in colour_search.cpp) and reports the chain's shape */
enum { HM_PIPE_INT420 = 1, HM_PIPE_FLOAT = 2, HM_PIPE_BILINEAR_FLOAT = 3, HM_PIPE_TO_HDR_FLOAT = 4, HM_PIPE_MONO = 5,
       HM_PIPE_SDR_INT420 = 6,  /* Op_to_sdr_planes -> Op_YCbCr420_to_RGB24/32: > 8-bit full-range 4:2:0 to 8-bit RGB      */
       HM_PIPE_FLOAT_SDR = 7,   /* Op_YCbCr_to_RGB<u16> -> Op_to_sdr_planes -> Op_RGB_to_RGB24_32: other > 8-bit images     */
       HM_PIPE_FLOAT_HDR = 8,   /* Op_YCbCr_to_RGB<u8> -> Op_to_hdr_planes -> Op_RGB_HDR_to_RRGGBBaa_BE [-> swap]          */
       HM_PIPE_GENERIC = 9,     /* any other combination of [depth change] [bilinear] core op [depth change]               */
       HM_PIPE_PLANAR = 10 };   /* a planar HM_OUT_YCBCR_* target: the chain runs operation by operation (hm_colour_convert_planar) */
HM_API int hm_colour_pipeline(const hm_colour_desc* d); /* HM_PIPE_* or negative status */
/* the chain itself: the reference's operations by their position in its pool (ColorConversionPipeline::init_ops,
 * colorconversion.cc:218-255); returns the number of operations (0: nothing to convert), -1 when there is no chain */
HM_API int hm_colour_chain(const hm_colour_desc* d, int* ops, int max_ops);

/* Observable libheif plane stride for a plane `width` pixels wide (pixelimage.cc:139-218). */
HM_API int hm_plane_stride(int width, int bytes_per_pixel);
/* bytes per output pixel of an interleaved HM_OUT_* format (3,4,6,8); the planar codes have none (HM_ERR_UNSUPPORTED) */
HM_API int hm_out_bytes_per_pixel(int out_format);

/* float32 coefficients exactly as nclx.cc:152-171 computes them: r_cr, g_cb, g_cr, b_cb */
HM_API int hm_ycbcr_coefficients(int has_nclx, int matrix, int primaries, float out[4]);

/* Convert device planes to the interleaved device buffer. Asynchronous on `stream` (the forced-bilinear chain
 * works through two temporary 4:4:4 chroma planes and returns after the stream has drained). */
HM_API int hm_colour_convert(const hm_colour_desc* d, const void* d_y, const void* d_cb,
                             const void* d_cr, void* d_out, void* stream);
/* The same for n images that share one descriptor (e.g. the 12 MP canvases of a batch of grids): arrays of n device
 * pointers (host arrays).  The integer 4:2:0 chain covers up to 32 images per kernel launch. */
HM_API int hm_colour_convert_batch(const hm_colour_desc* d, int n, const void* const* d_y, const void* const* d_cb,
                                   const void* const* d_cr, void* const* d_out, void* stream);

/* Planar targets (d->out_format = HM_OUT_YCBCR_* [| HM_OUT_YCBCR_8BIT]): device planes to device planes through the
 * reference's chain for that target, operation by operation - chroma up-sampling (bilinear) and down-sampling (average),
 * Op_YCbCr_to_RGB / Op_RGB_to_YCbCr on planes, Op_mono_to_YCbCr420, the depth changes.  A chain that holds any other
 * operation is refused with HM_ERR_UNSUPPORTED and a message that names it; no chain: HM_ERR_UNSUPPORTED with
 * hm_last_error_detail() == HM_DETAIL_NO_COLOUR_CHAIN.
 * in / out: [0..2] Y, Cb, Cr, [3] the alpha plane (NULL: none; d->has_alpha says whether the image has one, and a
 * depth change converts it like the others).  in_alpha_bits: the alpha plane's sample depth (0 = the image's); the
 * planes of `out` have the target's size and depth: chroma (w+1)/2 and (h+1)/2 where sub-sampled, 8 bits with
 * HM_OUT_YCBCR_8BIT, else d->bit_depth; d->y_stride / cb_stride / cr_stride describe `in`.  Quirk kept from
 * Op_YCbCr444_to_YCbCr422_average (chroma_sampling.cc:398-403): with an odd width the reference never writes the last
 * chroma sample of the last row; the copied sample is written there.
 * flags: HM_PLANAR_UNFUSED runs Op_YCbCr_to_RGB -> Op_RGB_to_YCbCr as two kernels over planar RGB instead of the
 * fused one (same pixels; the checker's second path).  Asynchronous on `stream` except for chains that need
 * temporaries, which return after the stream has drained. */
typedef struct hm_planes {
  void*   plane[4];
  int32_t stride[4];
} hm_planes;
enum { HM_PLANAR_UNFUSED = 1 };
HM_API int hm_colour_convert_planar(const hm_colour_desc* d, const hm_planes* in, int in_alpha_bits, const hm_planes* out, int flags, void* stream);

/* ------------------------------------------------------------------------- */
/* Host entropy decode: HEVC intra picture -> GPU command stream (hm_stream.h) */
/* ------------------------------------------------------------------------- */

/* Parse one coded picture.  `data` is what a heif_decoder_plugin receives through push_data():
 * a concatenation of [u32 big-endian length][NAL unit] records, parameter sets first
 * (libheif/plugins/decoder_libde265.cc:269-303); with annexb != 0 it is an Annex-B byte stream
 * (00 00 01 start codes) instead.  On success *out_blob (free with hm_free) holds the picture's
 * command stream (struct hm_pic at offset 0).  CABAC / parsing run on the calling CPU thread -
 * as in the reference (slice.cc) - and are thread-safe across different calls.
 * Returns HM_ERR_UNSUPPORTED for syntax outside the GPU hot path (inter slices, multilayer / 3D / screen-content
 * extensions, separate colour planes, more than 12 bits, range-extension corners undefined in the reference). */
HM_API int hm_hevc_parse(const uint8_t* data, size_t size, int annexb, uint8_t** out_blob, size_t* out_size);
/* the same with up to `threads` host threads for ONE picture: slice segments coded with wavefront parallel processing
 * (entry points per CTB row) are entropy-decoded row-parallel like the reference's WPP threads (decctx.cc:1004-1116);
 * the command stream is the same byte for byte */
HM_API int hm_hevc_parse_mt(const uint8_t* data, size_t size, int annexb, int threads, uint8_t** out_blob, size_t* out_size);
/* the same with every choice spelled out.  record_order decides the order of the block records in the command stream
 * (hm_stream.h), i.e. which reconstruction kernels the picture runs: HM_RECORDS_AUTO - by picture class, tuned for
 * batches of thousands of tiles -, HM_RECORDS_SPLIT - separate luma / chroma chains whenever the picture's syntax allows
 * (the faster choice when a batch holds few pictures: their rows then become the parallel work) -, HM_RECORDS_DECODE_ORDER.
 * The same bytes always parse to the same stream for the same options: nothing depends on who calls. */
enum { HM_RECORDS_AUTO = 0, HM_RECORDS_SPLIT = 1, HM_RECORDS_DECODE_ORDER = 2 };
/* ... | HM_PARSE_CONCEAL (r05): a picture whose SLICE DATA is damaged is not refused - the reference keeps such pictures
 * (libde265 notes the error and hands the picture out, third-party/libde265/libde265/decctx.cc:876-995,
 * libheif/plugins/decoder_libde265.cc:311-336).  Every CTB in front of the error is decoded from the data, exactly; every
 * other CTB - the rest of the damaged slice segment, segments that depended on it, CTBs no segment covers - is written as a
 * plain intra CTU without a residual (the reference's samples there are whatever its image memory held: nothing to match).
 * hm_pic.concealed_ctbs / first_concealed_ctb of the command stream say how much was made up.  Damaged parameter sets and a
 * damaged first slice header remain errors.  hm_decode_item / the facade / the plugin set it unless strict decoding is asked. */
#define HM_PARSE_CONCEAL 0x100
typedef struct hm_parse_options {
  int32_t annexb;        /* 0: [u32 length][NAL] records, 1: Annex-B start codes */
  int32_t threads;       /* host threads for the rows of a WPP-coded picture     */
  int32_t record_order;  /* HM_RECORDS_*                                          */
} hm_parse_options;
HM_API int hm_hevc_parse_opts(const uint8_t* data, size_t size, const hm_parse_options* opts, uint8_t** out_blob, size_t* out_size);
HM_API void hm_free(void* p);

/* ------------------------------------------------------------------------- */
/* GPU tile decode: reconstruction -> deblocking -> SAO -> paste               */
/* ------------------------------------------------------------------------- */

/* Where a decoded picture goes: a (grid) canvas on the device.  Mirrors the arguments of
 * HeifContext::decode_and_paste_tile_image (libheif/context.cc:2407-2411) plus the tile's
 * colour profile, which decides the limited->full range rescale of context.cc:2504-2528.
 * For a single (non-grid) image use x0 = y0 = 0 and canvas size = picture size. */
typedef struct hm_tile_dest {
  void*   plane[3];          /* device pointers to the canvas Y, Cb, Cr planes (origin of the canvas) */
  int32_t pitch[3];          /* bytes                                                              */
  int32_t canvas_width, canvas_height; /* luma size of the canvas                                   */
  int32_t x0, y0;            /* tile origin in the canvas, luma samples                             */
  int32_t tile_has_nclx;     /* the tile image carries an nclx (VUI or 'colr')                      */
  int32_t tile_full_range, tile_matrix;
} hm_tile_dest;

typedef struct hm_batch hm_batch;

HM_API int  hm_batch_create(hm_batch** out);
HM_API void hm_batch_destroy(hm_batch* b);
HM_API void hm_batch_clear(hm_batch* b);
/* queue one picture (command stream from hm_hevc_parse; copied); returns its index (>= 0) or a status */
/* Structural check of a command stream that did not come straight out of hm_hevc_parse (everything the kernels use
 * as an index or a size); hm_batch_add runs it on every stream it is given.  HM_OK or HM_ERR_INVALID_ARG. */
HM_API int  hm_stream_validate(const uint8_t* blob, size_t size);
HM_API int  hm_batch_add(hm_batch* b, const uint8_t* blob, size_t size, const hm_tile_dest* dest);
HM_API int  hm_batch_size(const hm_batch* b);
/* copy the queued command streams to the device and build the job descriptors (synchronous) */
HM_API int  hm_batch_upload(hm_batch* b, void* stream);
/* launch the kernels for all queued pictures (asynchronous on `stream`, repeatable).
 * stages: bit0 = deblocking, bit1 = SAO; pass 3.  Pictures of a batch are independent: this is
 * the data-parallel replacement of the reference's std::async tile fan-out (context.cc:2361-2401). */
HM_API int  hm_batch_execute(hm_batch* b, int stages, void* stream);
/* Attach the YCbCr -> RGB conversion of the images' canvases to the batch (convert_colorspace of the decoded grids,
 * context.cc:1516-1600): one hm_batch_execute is then the whole hot path.  images_per_group > 0 runs the filters and the
 * conversion group of images by group of images (Infinity-Cache blocking; measured not to pay for 12 MP grids, see
 * batch.cpp), 0 = one group, < 0 = one group and never the fused kernel described below.  The pictures must have been queued image by image, equally many per image; arrays of
 * n_images device pointers (copied).  n_images 0 detaches.
 * With a conversion attached the batch's result is the conversion's output; the canvases are an intermediate that the
 * batch may skip: for the mainstream shape (8-bit 4:2:0 pictures of one slice, canvases fully covered, integer matrix
 * chain to RGB24 / RGBA32) deblocking, SAO, paste and conversion run as ONE kernel that reads the reconstruction once
 * and writes the pixels once (filters.hip: k_tail420) and the canvases are not written.  hm_batch_tail_fused tells. */
HM_API int  hm_batch_set_colour(hm_batch* b, const hm_colour_desc* d, int n_images, const void* const* d_y, const void* const* d_cb,
                                const void* const* d_cr, void* const* d_out, int images_per_group);
/* hm_batch_upload + hm_batch_execute in one call, the command streams split into `chunks` parts: the H2D copy of part
 * i+1 (on `copy_stream`) runs under the kernels of part i (on `stream`).  Asynchronous. */
HM_API int  hm_batch_upload_execute(hm_batch* b, int stages, int chunks, void* copy_stream, void* stream);
/* per-kernel timing with HIP events on the launch streams: `slots` execute calls are kept (ring),
 * 0 switches it off (default) */
HM_API int  hm_batch_set_profiling(hm_batch* b, int slots);
/* The images of a batch whose tail is fused can be executed as groups, each on a stream of its own, joined on the caller's
 * stream - the tail kernel of one group runs while the reconstruction of the other drains.
 * groups = 0 (the default): automatic - two groups of whole images once the batch holds two rounds or more of the chain
 * kernel's resident waves (about 10 000 tiles of 512 x 512 on an MI355X), one stream below that: single images and small
 * batches run exactly as with 1; 1: always the caller's stream alone; 2..8: that many equal groups.
 * The pixels are the same in every mode. */
HM_API int  hm_batch_set_concurrency(hm_batch* b, int groups);
/* kernel times in ms of the execute call in `slot` (call index mod slots):
 * [0] reconstruction, [1] deblocking (V+H), [2] SAO+paste.  Waits for that call to finish.
 * An execute that ran in groups: each entry is the time during which at least one kernel of its kind was running on any
 * of the groups' streams (the union of the groups' intervals), so the entries add up to more than the step. */
HM_API int  hm_batch_get_timings(hm_batch* b, int slot, float ms[3]);
/* the same plus [3] the colour conversion attached with hm_batch_set_colour (summed over the groups of images) */
HM_API int  hm_batch_get_timings4(hm_batch* b, int slot, float ms[4]);
/* the same with the two kernels of the split-chain reconstruction apart: [0] the prediction chains (k_chain; for other
 * picture classes the whole reconstruction), [4] the residual pre-pass (k_residual; 0 where it does not run) */
HM_API int  hm_batch_get_timings5(hm_batch* b, int slot, float ms[5]);
/* 1 when the executes of this batch run the fused tail kernel: its time is reported in slot [2], [1] and [3] are 0 */
HM_API int  hm_batch_tail_fused(const hm_batch* b);
/* waits for the batch's work; HM_ERR_INTERNAL when a reconstruction wave had to give up a (bounded) wait for the rows
 * above it - the pictures of that execute are then not valid.  Never on a healthy device. */
HM_API int  hm_batch_check(hm_batch* b);
/* algorithmic bytes of the queued pictures: command streams read, reconstructed samples written */
HM_API int  hm_batch_algorithmic_bytes(const hm_batch* b, uint64_t* stream_bytes, uint64_t* sample_bytes);
/* the same per kernel of the split-chain reconstruction: out[0] command streams, [1] reconstructed samples, [2] the
 * levels inside the streams (read by the residual pre-pass only), [3] residual samples (written by the pre-pass, read
 * by the prediction chains) */
HM_API int  hm_batch_algorithmic_bytes4(const hm_batch* b, uint64_t out[4]);

/* ------------------------------------------------------------------------- */
/* Plugin level: one coded picture -> host planes                              */
/* ------------------------------------------------------------------------- */

/* What heif_decoder_plugin::decode_image produces (libheif/plugins/decoder_libde265.cc:88-157, 311-369): the planes of
 * the last pushed picture at the conformance-window size, chroma planes width / SubWidthC x height / SubHeightC
 * (de265_get_image_width/height(img, c)), one plane for 4:0:0, all planes of one bit depth, plus the VUI colour
 * description (defaults 2,2,2, limited).  `data` is the push_data() byte string ([u32 BE length][NAL]...). */
typedef struct hm_picture hm_picture;
typedef struct hm_picture_info {
  int32_t chroma, bit_depth, n_planes;       /* enum heif_chroma value; 8..12; 1 (4:0:0) or 3             */
  int32_t plane_width[3], plane_height[3];   /* samples                                                   */
  int32_t primaries, transfer, matrix, full_range;
} hm_picture_info;
/* host entropy decode (CABAC on the calling thread); *out owns the command stream */
HM_API int  hm_picture_parse(const uint8_t* data, size_t size, hm_picture** out, hm_picture_info* info);
/* ... with strict != 0: a picture with damaged slice data is refused (HM_ERR_BITSTREAM) instead of concealed (HM_PARSE_CONCEAL:
 * what hm_picture_parse does, as the reference's plugin hands such pictures out); *concealed_ctbs (may be NULL): how many CTBs of
 * the picture are concealment */
HM_API int  hm_picture_parse_opts(const uint8_t* data, size_t size, int strict, hm_picture** out, hm_picture_info* info, int32_t* concealed_ctbs);
/* reconstruction + in-loop filters on the GPU, then rows of plane_width * bytes_per_sample bytes into plane[c]
 * (host memory, e.g. heif_image_get_plane()); returns after the copy has completed */
HM_API int  hm_picture_decode_to_host(hm_picture* p, uint8_t* const plane[3], const int32_t stride[3], void* stream);
/* the same in two halves: begin hands the picture to the device (stream == NULL: to the device's shared worker, where
 * concurrent callers - the tile threads of context.cc:2361-2401 - meet in one batch) and returns; finish waits, copies
 * the planes out and frees the job, also when it fails.  The plugin's decode_image allocates its heif_image in between.
 * A job that was begun must be finished (plane == NULL: abandon it), before hm_picture_free. */
typedef struct hm_picture_job hm_picture_job;
HM_API int  hm_picture_decode_begin(hm_picture* p, void* stream, hm_picture_job** out);
HM_API int  hm_picture_decode_finish(hm_picture_job* job, uint8_t* const plane[3], const int32_t stride[3]);
HM_API void hm_picture_free(hm_picture* p);

/* ------------------------------------------------------------------------- */
/* Image level: HEIF file -> pixels (host box parsing + CABAC, GPU everything else) */
/* ------------------------------------------------------------------------- */

typedef struct hm_file hm_file;

typedef struct hm_image_info {
  int32_t width, height;       /* output size (grid: the grid's output size; image, 'iden', 'iovl': ispe) */
  int32_t bit_depth, chroma;   /* from the (first tile's) hvcC; a derived item ('iden', 'iovl'): of its first non-virtual
                                  child, found through the first reference of every derived item on the way (context.cc:1377-1407);
                                  is_grid and has_alpha are 0 for a derived item (context.cc:1370-1373)   */
  int32_t is_grid, grid_rows, grid_cols, tile_width, tile_height;
  int32_t has_transforms;      /* irot / imir / clap present on the item                         */
  int32_t has_alpha;           /* an alpha auxiliary image is attached (heif_image_handle_has_alpha_channel) */
  int32_t coded_width, coded_height; /* size before the transformative properties (ispe / grid output size);
                                        width / height above are what heif_image_handle_get_width/height report
                                        (context.cc:810-838: clap size, swapped by a 90 / 270 degree irot)       */
  int32_t has_nclx;            /* the item carries a 'colr' nclx (a grid without one: its first tile's, context.cc:1087)    */
} hm_image_info;

typedef struct hm_decode_params {
  int32_t out_format;          /* 0 = native planar YCbCr, else HM_OUT_* (interleaved: == enum heif_chroma; planar:
                                  HM_OUT_YCBCR_420 / _422 / _444)                                  */
  int32_t host_threads;        /* entropy-decode threads (heif_context_set_threads semantics)    */
  int32_t ignore_transformations;
  int32_t chroma_upsampling;   /* 0 = default op selection, HM_UPSAMPLE_BILINEAR = forced bilinear (see hm_colour_desc) */
  void*   stream;              /* hipStream_t or NULL                                            */
  void*   ext_dst;             /* optional caller buffer for interleaved output (fork API:       */
  uint32_t ext_dst_len;        /*   heif_decoding_options_add_external_dest, heif.h:1605-1615)   */
  uint32_t ext_dst_stride;
  int32_t strict_decoding;     /* heif_decoding_options.strict_decoding (heif.h:1591): an unknown VUI colour code is an
                                  error instead of a warning (HEIF_WARN_OR_FAIL, heif_plugin.h:290-301)              */
  int32_t convert_hdr_to_8bit; /* heif_decoding_options.convert_hdr_to_8bit (heif.h:1577, context.cc:1550)          */
} hm_decode_params;

typedef struct hm_decoded {
  int32_t width, height, bit_depth, chroma;
  int32_t out_format;          /* as requested                                                    */
  int32_t has_nclx, primaries, transfer, matrix, full_range; /* profile attached to the result   */
  int32_t used_ext_dst;
  uint8_t* plane[3];           /* pinned host memory (owned by the library: release with hm_decoded_free or
                                  hm_host_free), libheif plane layout (pixelimage.cc:139-218);      */
  int32_t stride[3];           /*   interleaved output uses plane[0] only                          */
  int32_t plane_width[3], plane_height[3];
  /* alpha channel of the image (an auxiliary image item, context.cc:2029-2078): interleaved RGBA output carries it in
   * byte 3; native planar output gets it as a fourth plane (same size as the image, same sample width) */
  int32_t has_alpha;
  uint8_t* alpha;              /* pinned host memory like plane[], NULL unless has_alpha and the output is planar */
  int32_t alpha_stride;
  int32_t warnings;            /* HM_WARN_*: what heif_image_get_decoding_warnings reports (heif.cc:1223-1245)     */
} hm_decoded;
/* non-strict decoding replaces an unknown colour code of the VUI by "unspecified" and records a warning
 * (decoder_libde265.cc:339-357 via heif_nclx_color_profile_set_*, heif.cc:1811-1905) */
enum { HM_WARN_UNKNOWN_PRIMARIES = 1, HM_WARN_UNKNOWN_TRANSFER = 2, HM_WARN_UNKNOWN_MATRIX = 4,
       HM_WARN_CONCEALED = 8 /* damaged slice data: part of the picture (of one of a grid's tiles) is concealment, HM_PARSE_CONCEAL */ };
/* 1 if `value` is a code point libheif knows for kind 0 = colour primaries, 1 = transfer characteristics,
 * 2 = matrix coefficients (the known_* sets of heif.cc:1795-1885) */
HM_API int hm_nclx_code_known(int kind, int value);

/* parse the box structure (the bytes are copied).  Replaces heif_context_read_from_memory. */
HM_API int      hm_file_open(const uint8_t* data, size_t size, hm_file** out);
HM_API void     hm_file_close(hm_file* f);
HM_API uint32_t hm_file_primary_item(const hm_file* f);
HM_API int      hm_file_top_level_images(const hm_file* f, uint32_t* ids, int max_ids); /* returns the count */
HM_API int      hm_file_image_info(const hm_file* f, uint32_t id, hm_image_info* info);
/* what kind of item `id` is: HM_ITEM_*, or a negative status (no such item) */
enum { HM_ITEM_OTHER = 0, HM_ITEM_HVC1 = 1, HM_ITEM_GRID = 2, HM_ITEM_IDEN = 3, HM_ITEM_IOVL = 4,
       HM_ITEM_TMAP = 5 /* a tone-map derived item (ISO 21496-1 gain map): "Gain" below */,
       HM_ITEM_UNCI = 6 /* an uncompressed image (ISO/IEC 23001-17): "Uncompressed items" below */,
       HM_ITEM_MSKI = 7 /* a mask item ('mski') that carries its 'mskC' property: "Regions and masks" below; one without stays HM_ITEM_OTHER */ };
HM_API int      hm_file_item_kind(const hm_file* f, uint32_t id);
/* A 'tmap' item: an SDR base image, a gain-map image and the parameters that take the base to its alternate (HDR) rendition.  It
 * has exactly two 'dimg' references, [0] the base image and [1] the gain-map image (anything else: HM_ERR_BITSTREAM).  These
 * references do not hide their targets: the base stays a top-level image, the map is listed or not as its own hidden flag says, and
 * the 'tmap' item itself is never listed by hm_file_top_level_images.  hm_decode_item on a 'tmap' id is HM_ERR_UNSUPPORTED: the item
 * is rendered by hm_decode_item_to_device_gain.
 * The payload, big-endian (the contract of this reader):
 *   u8  version                          0, anything else HM_ERR_UNSUPPORTED
 *   u16 minimum_version                  0, anything else HM_ERR_UNSUPPORTED
 *   u16 writer_version
 *   u8  flags                            0x80 is_multichannel, 0x40 use_base_colour_space
 *   u32 / u32  base_hdr_headroom         numerator / denominator
 *   u32 / u32  alternate_hdr_headroom
 *   per channel - 3 channels if is_multichannel, else 1 that stands for all three -, each numerator / u32 denominator:
 *     s32 gain_map_min, s32 gain_map_max, u32 gamma, s32 base_offset, s32 alternate_offset
 * HM_ERR_BITSTREAM: a zero denominator, a zero gamma, a truncated payload.  Headrooms, gain_map_min and gain_map_max are log2 values.
 * Every fraction is handed out as (double)numerator / (double)denominator. */
typedef struct hm_gain_params {
  double  base_headroom, alternate_headroom;        /* Hb, Ha: log2 */
  double  map_min[3], map_max[3], gamma[3];         /* per colour channel R, G, B; min and max are log2 */
  double  base_offset[3], alternate_offset[3];
  int32_t use_base_primaries;                       /* the gain is applied in the base image's primaries (flag 0x40) */
  int32_t reserved;                                 /* 0 */
} hm_gain_params;
typedef struct hm_gain_map_info {
  uint32_t base_item, map_item;
  hm_gain_params params;
  int32_t alt_has_nclx, alt_primaries, alt_transfer; /* the 'tmap' item's own colr (nclx): the alternate rendition's profile */
} hm_gain_map_info;
HM_API int      hm_file_gain_map_info(const hm_file* f, uint32_t tmap_id, hm_gain_map_info* info);
/* the first 'tmap' item (in item-ID order) whose base image is `base_id`, 0 if there is none */
HM_API uint32_t hm_file_gain_map_of(const hm_file* f, uint32_t base_id);
/* The URN of item `id`'s auxC property as a NUL-terminated string in out[0 .. cap) (cut to cap - 1 characters); returns its full
 * length, 0 for an item without one, or a negative status.  With it a caller finds a vendor gain map among the 'auxl' items of an image. */
HM_API int      hm_file_item_aux_type(const hm_file* f, uint32_t id, char* out, int cap);
/* An 'iovl' item (ImageOverlay, context.cc:318-369): the canvas, the 16-bit R G B A background (the canvas is filled with
 * R G B >> 8; A is ignored) and the layers in reference order, bottom first.  children[i] / offsets[2 i], offsets[2 i + 1]: item ID
 * and signed (x, y) offset of layer i, for i < min(n_children, max_children); either array may be NULL.
 * HM_ERR_BITSTREAM: a truncated payload, a zero canvas size; HM_ERR_UNSUPPORTED: a payload version other than 0. */
typedef struct hm_overlay_info {
  int32_t canvas_width, canvas_height;
  int32_t n_children;
  uint16_t background[4];
} hm_overlay_info;
HM_API int      hm_file_overlay_info(const hm_file* f, uint32_t id, hm_overlay_info* info, uint32_t* children, int32_t* offsets, int max_children);
/* the one image an 'iden' item derives from (context.cc:2542-2576).  HM_ERR_BITSTREAM: not exactly one reference, or one to itself */
HM_API int      hm_file_derived_child(const hm_file* f, uint32_t id, uint32_t* child);
/* the auxiliary image item that is the alpha channel of image `id` (context.cc:885-945), 0 if there is none */
HM_API uint32_t hm_file_alpha_item(const hm_file* f, uint32_t id);
/* The raw ('prof' / 'rICC') colour profile that goes with image `id` (passed through untouched; *data points into the
 * file object and stays valid until hm_file_close).  for_handle != 0: what an image handle reports - the item's own
 * 'colr', a grid without one inherits its first tile's (context.cc:780-800, 1075-1090); for_handle == 0: what the
 * decoded image carries - the item's own 'colr' for a coded image, nothing for a grid (context.cc:1844-1852; the
 * conversion keeps it, colorconversion.cc:456).  *type = the profile's fourcc as a big-endian number, 0 = none. */
HM_API int      hm_file_item_icc(const hm_file* f, uint32_t id, int for_handle, uint32_t* type, const uint8_t** data, size_t* size);
/* the byte string a decoder plugin gets through push_data for an hvc1 item (free with hm_free) */
HM_API int      hm_file_item_hevc_data(const hm_file* f, uint32_t id, uint8_t** out, size_t* out_size);
/* decode an hvc1 image, a grid, a derived item or an uncompressed ('unci') item - "Uncompressed items" at the end of this header says
 * what such an item decodes to.  Replaces heif_decode_image (heif.cc:1150-1186 ->
 * context.cc:1516-1600, 2120-2404, 2542-2675).  Free the result with hm_decoded_free.
 * Derived items: an 'iden' item is its child decoded with the transformation list child ++ iden; an 'iovl' item is composed on the
 * device (its layers clipped to the canvas; layers off the canvas are not decoded) and decodes to HM_OUT_RGB / HM_OUT_RGBA only.
 * HM_ERR_UNSUPPORTED, before any work is queued: pictures or alpha planes deeper than 8 bits under a derived item, an alpha
 * auxiliary image attached to the derived item itself, an 'iovl' item to out_format 0 / HM_OUT_YCBCR_* / RRGGBB*, an 'iden' item
 * over a 4:4:4 hvc1 image to out_format 0 / HM_OUT_YCBCR_*.  HM_ERR_BITSTREAM: a bad 'iovl' payload, 'iden' without exactly one
 * other reference, a reference to a missing item, a reference cycle, nesting deeper than 8.   */
HM_API int      hm_decode_item(const hm_file* f, uint32_t id, const hm_decode_params* params, hm_decoded* out);
/* The same with ONE GRID OVER SEVERAL DEVICES of this process: the grid's tile rows are cut into contiguous slabs, one per
 * entry of `devices` (HIP device indices; an index may repeat), each slab is decoded and converted on its device and copied
 * from there straight into its rows of params->ext_dst / of the pinned output plane - the in-process tile fan-out of the
 * reference (context.cc:2281-2294, 2361-2401) across GPUs, without any exchange between them.  Items that do not cut this
 * way (single images, derived items, planar output, alpha, transformed grids, forced bilinear up-sampling) are decoded on devices[0].
 * params->stream must be NULL (every slab runs on a stream of its own).  hm_plan_device_slabs: the cut it uses. */
HM_API int      hm_decode_item_devices(const hm_file* f, uint32_t id, const hm_decode_params* params, const int32_t* devices, int n_devices, hm_decoded* out);
HM_API int      hm_plan_device_slabs(int grid_rows, int n_devices, int32_t* first_row, int32_t* row_count);
HM_API void     hm_decoded_free(hm_decoded* d);
/* release one plane taken out of an hm_decoded (ownership transfer, used by the libheif facade) */
HM_API void     hm_host_free(void* plane);

/* ------------------------------------------------------------------------- */
/* Image sequences: the fork's movie mode (a 'moov' track of HEVC-intra samples) */
/* ------------------------------------------------------------------------- */

/* A file whose ftyp lists the compatible brand 'hevc' or 'hevx' and that holds a 'moov' box is read the way the fork reads it
 * (libheif/file.cc:474-483, context.cc:646-700): every sample of the track is a top-level image, IDs 1..frame_count, ID 1 the
 * primary one; 'meta' is ignored.  hm_file_image_info, hm_file_item_hevc_data and hm_decode_item work on the frames like on
 * hvc1 items (width / height: the track header's, the decoded image: the picture's own size). */
typedef struct hm_sequence_info {
  int32_t  is_sequence;        /* 1: movie mode                                                               */
  uint32_t frame_count;        /* samples_per_chunk of the track's one 'stsc' entry                            */
  uint64_t duration;           /* 'mvhd' duration, in its timescale (libheif_parameters.movie_duration)         */
} hm_sequence_info;
/* fills *info; a file that is not a sequence gives is_sequence = 0 (not an error) */
HM_API int hm_file_sequence_info(const hm_file* f, hm_sequence_info* info);
/* where one frame of hm_decode_sequence goes: the role of params->ext_dst for that frame (NULL = pinned host memory) */
typedef struct hm_frame_dest {
  void*    ext_dst;
  uint32_t ext_dst_len;
  uint32_t ext_dst_stride;
} hm_frame_dest;
/* Decode frames first .. first + count - 1 of a sequence in ONE device batch on params->stream: their entropy decode shares
 * params->host_threads, one upload, the reconstruction and filter kernels (and the colour conversion) run once over all
 * frames; out[k] receives frame first + k exactly as hm_decode_item would give it (free each with hm_decoded_free).
 * dests (NULL, or `count` entries) replaces params->ext_dst, which must be NULL.  A frame whose data fails fails the call
 * with that frame's status and message (hm_last_error) before anything is queued - no caller buffer is written -, and
 * *failed_frame (may be NULL) = its index k; -1 when the failure is not one frame's.  On any failure every out[k] is
 * empty; after a device failure the caller buffers' contents are undefined. */
HM_API int hm_decode_sequence(const hm_file* f, uint32_t first, int32_t count, const hm_decode_params* params, const hm_frame_dest* dests,
                              hm_decoded* out, int32_t* failed_frame);

/* ------------------------------------------------------------------------- */
/* Pipelined decode: many HEIF files in flight (host parse || H2D || kernels || D2H) */
/* ------------------------------------------------------------------------- */

/* The throughput form of heif_decode_image: what a server that decodes a stream of files does with the reference is a
 * loop over heif_context_read_from_memory + heif_decode_image with heif_context_set_threads(n) (README.md:47-62 of the
 * reference); there the tiles of ONE image fan out (context.cc:2361-2401) and images are serial.  Here the coded
 * pictures of ALL submitted images share one crew of host entropy-decode threads, and each image's device work runs on
 * its own HIP stream, so parsing image k+1, the kernels of image k and the D2H copy of image k-1 overlap. */
typedef struct hm_pipeline hm_pipeline;
typedef struct hm_pipeline_config {
  int32_t host_threads;        /* entropy-decode crew (heif_context_set_threads semantics, shared by all images)  */
  int32_t max_in_flight;       /* images that may hold device + pinned memory at once (back-pressure of submit)   */
  int32_t out_format;          /* as hm_decode_params                                                              */
  int32_t chroma_upsampling, ignore_transformations, strict_decoding;
  int32_t device;              /* HIP device index, -1 = the calling thread's current device                       */
  int32_t cpu_first, cpu_count; /* the crew's CPUs: [cpu_first, cpu_first + cpu_count), 0 count = wherever the caller may
                                  run.  One pipeline per GPU, each with the CPUs (NUMA node) next to its GPU, is how a
                                  node of 8 GPUs is fed: the entropy decode of one GPU's images never migrates away     */
} hm_pipeline_config;
typedef struct hm_pipeline_result {
  uint64_t   tag;              /* the caller's tag of hm_pipeline_submit                                            */
  int32_t    status;           /* HM_OK or the hm_status of this image (detail: hm_last_error() of the calling thread) */
  hm_decoded image;            /* valid when status == HM_OK, until hm_pipeline_release                            */
  void*      handle;           /* internal                                                                         */
} hm_pipeline_result;
HM_API int  hm_pipeline_create(const hm_pipeline_config* cfg, hm_pipeline** out);
HM_API void hm_pipeline_destroy(hm_pipeline* p);
/* queue one HEIF file (the bytes are copied; item_id 0 = the primary item).  Returns HM_OK, a negative status (the file
 * is malformed / unsupported: nothing was queued), or HM_PIPELINE_FULL when max_in_flight images are pending: take a
 * result (hm_pipeline_next + hm_pipeline_release) and submit again */
enum { HM_PIPELINE_FULL = 1 };
HM_API int  hm_pipeline_submit(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag);
/* number of submitted images whose result has not been taken yet */
HM_API int  hm_pipeline_pending(hm_pipeline* p);
/* wait for the oldest pending image (results come in submission order; several consumers each get a different image);
 * a failed image is reported in res->status */
HM_API int  hm_pipeline_next(hm_pipeline* p, hm_pipeline_result* res);
/* give the image's pinned planes and its slot back */
HM_API void hm_pipeline_release(hm_pipeline* p, hm_pipeline_result* res);

/* ------------------------------------------------------------------------- */
/* Device-resident output: decode into caller-owned GPU memory, with tensor layouts */
/* ------------------------------------------------------------------------- */

/* The image-level entry points above end in a copy to host memory.  These put the pixels of an interleaved RGB target
 * (HM_OUT_RGB / _RGBA / _RRGGBB_* / _RRGGBBAA_*) into device memory of the caller instead - in the target's own
 * interleaving (HWC) or one plane per channel (CHW), as the target's integers or as float32 / float16 with a scale and a
 * bias per channel - for callers that go on working on the same GPU.  A "sample" is a byte of an 8-bit target, a 16-bit
 * word of a 16-bit target.
 *   HWC with the target's integer type: exactly the bytes hm_decode_item puts into plane[0] (byte order of _BE included).
 *   CHW, or a float dtype: samples are taken as values - _BE targets are refused (ask for _LE), an integer dtype must be
 *   the target's (HM_DEV_U8 / HM_DEV_U16); floats are  __fadd_rn(__fmul_rn((float)v, scale[c]), bias[c])  (no fused
 *   multiply-add), HM_DEV_F16 that value through __float2half_rn (denormals kept).
 * Refused with HM_ERR_INVALID_ARG, before any work is queued and without a byte of the destination written: a pointer
 * that is not device memory of the decoding device, len below hm_device_dest_bytes, pitches below the tight value,
 * ptr or pitches that are not multiples of the element size.  HM_ERR_UNSUPPORTED ("not supported with a device
 * destination"): out_format 0 and the planar HM_OUT_YCBCR_* targets.  Only the width x height x channels elements of
 * the image are written: no pitch padding, nothing behind the last row. */
enum { HM_DEV_LAYOUT_HWC = 0,   /* the out_format's own interleaving: rows of pixels                     */
       HM_DEV_LAYOUT_CHW = 1 }; /* one plane per channel (R, G, B[, A])                                   */
enum { HM_DEV_U8 = 0, HM_DEV_U16 = 1, HM_DEV_F16 = 2, HM_DEV_F32 = 3 };
typedef struct hm_device_dest {
  void*    ptr;          /* device memory of the device the decode runs on                              */
  uint64_t len;          /* bytes available at ptr                                                      */
  int32_t  layout, dtype;
  int64_t  row_pitch;    /* bytes between rows; 0 = tight                                               */
  int64_t  plane_pitch;  /* CHW: bytes between channel planes; 0 = row_pitch * height                   */
  float    scale[4], bias[4]; /* float dtypes only: out = sample * scale[c] + bias[c]                   */
} hm_device_dest;
/* bytes the destination must hold for a width x height image (last-row / last-plane form: HWC
 * row_pitch * (h-1) + w*C*elem, CHW plane_pitch * (C-1) + row_pitch * (h-1) + w*elem), or the negative status of a
 * combination that is refused.  Pure host arithmetic: no device needed; d->ptr and d->len are not looked at. */
HM_API int64_t hm_device_dest_bytes(int out_format, int width, int height, const hm_device_dest* d);
/* The tensor step on its own, for callers of the low-level API (hm_colour_convert / hm_batch_set_colour leave interleaved
 * pixels on the device): rows of width * bytes-per-pixel bytes at d_src, src_stride bytes apart, go to `dest` under the
 * rules above.  Asynchronous on `stream`. */
HM_API int hm_to_tensor(int out_format, int width, int height, const void* d_src, int src_stride, const hm_device_dest* dest, void* stream);
/* hm_decode_item with the pixels going to `dest`: returns when they are in place (the work runs on params->stream).
 * `out` is filled as for an ext_dst decode: used_ext_dst = 1, every plane[] NULL, stride[0] = the row pitch in use.
 * params->ext_dst must be NULL.  A derived item ('iden', 'iovl') is decoded as by hm_decode_item and refused for the same
 * reasons, before a device is needed. */
HM_API int hm_decode_item_to_device(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_dest* dest, hm_decoded* out);
/* hm_decode_sequence with one hm_device_dest per frame (e.g. `count` offsets into one N x C x H x W allocation) */
HM_API int hm_decode_sequence_to_device(const hm_file* f, uint32_t first, int32_t count, const hm_decode_params* params, const hm_device_dest* dests,
                                        hm_decoded* out, int32_t* failed_frame);
/* hm_pipeline_submit with a destination (copied): when hm_pipeline_next hands the result out, the pixels are complete in
 * device memory, which must stay valid until then.  A destination that is refused fails the submit or the image's result. */
HM_API int hm_pipeline_submit_to_device(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag, const hm_device_dest* dest);

/* ------------------------------------------------------------------------- */
/* Device-resident planar YCbCr: I420 / NV12 / P010 and their kin in caller-owned GPU memory */
/* ------------------------------------------------------------------------- */

/* The other half of what the library decodes to - out_format 0 (the picture as coded), HM_OUT_YCBCR_420 / _422 / _444 (the
 * reference's chain to that chroma format, optionally with convert_hdr_to_8bit), a Y plane alone for 4:0:0 - into device memory of
 * the caller, one destination per plane, separate or with Cb and Cr interleaved: what an encoder behind a transcode, a video
 * pipeline that takes NV12 / P010 surfaces or a model that works on luma wants on the device.  hm_device_dest stays an interleaved
 * RGB destination and hm_decode_item_to_device keeps refusing the planar formats; these entry points take the planar formats only.
 *   Format and size: the planes written are those hm_decode_item with the same hm_decode_params hands out in plane[0 .. 2] / alpha.
 *   bits and the chroma format are the result's (out->bit_depth, out->chroma), the plane sizes out->plane_width / height[c] (chroma
 *   (w + 1) / 2 and (h + 1) / 2 where sub-sampled); the alpha plane has the image's size.  The interleaved plane of
 *   HM_DEV_PLANES_SEMI has 2 * chroma_width elements per row, Cb first.  A 4:0:0 result writes Y only: plane[1] and plane[2] must be
 *   all zero then.
 *   Integer dtypes store the sample: HM_DEV_U8 needs bits == 8, HM_DEV_U16 bits > 8 (little-endian words); msb_aligned stores
 *   v << (16 - bits), the P010 / P012 convention.  The result's depth is known for certain only after the decode: a mismatch is
 *   HM_ERR_INVALID_ARG before anything is written, and at the entry point already where hm_image_info decides it.
 *   Float dtypes:  __fadd_rn(__fmul_rn((float)v, scale[c]), bias[c])  with c = 0 Y, 1 Cb, 2 Cr, 3 alpha (no fused multiply-add),
 *   HM_DEV_F16 that value through __float2half_rn (denormals kept) - hm_device_dest's rule.
 *   Alpha: written to plane[3] at the alpha plane's own depth (msb_aligned: v << (16 - that depth)) when plane[3].ptr is non-NULL,
 *   not written and not looked at otherwise.  With an integer dtype the alpha depth must be in the dtype's class (8, or more than 8
 *   bits), else HM_ERR_UNSUPPORTED; plane[3] given for an image without alpha: HM_ERR_INVALID_ARG.
 *   Only plane_width x plane_height elements per plane are written: no pitch padding, nothing behind the last row.
 * Refused with HM_ERR_INVALID_ARG before any work is queued, every plane unwritten: an unknown layout or dtype, non-zero reserved,
 * msb_aligned without HM_DEV_U16, a ptr or pitch that is not a multiple of the element size, a pitch below the tight value, len
 * below the last-row form row_pitch * (rows - 1) + tight, a NULL ptr of a plane that is written, a pointer that is not device
 * memory of the decoding device, an interleaved HM_OUT_RGB* target (that is hm_decode_item_to_device's), params->ext_dst, two
 * planes whose byte ranges overlap, and with HM_DEV_PLANES_SEMI a plane[2] that is not all zero.
 * Views (hm_device_view) with a planar destination: the _planes_view entry points behind hm_device_view, below. */
enum { HM_DEV_PLANES_SEPARATE = 0,  /* Y, Cb, Cr[, A]: one plane each (I420 / I422 / I444 and their 16-bit forms) */
       HM_DEV_PLANES_SEMI     = 1 };/* Y, CbCr interleaved (Cb first)[, A]: NV12 / NV16 / NV24, P010-style with 16 bits */
typedef struct hm_device_plane {
  void*    ptr;          /* device memory of the device the decode runs on                              */
  uint64_t len;          /* bytes available at ptr                                                      */
  int64_t  row_pitch;    /* bytes between rows; 0 = tight                                               */
} hm_device_plane;
typedef struct hm_device_planes {
  hm_device_plane plane[4];   /* [0] Y, [1] Cb (SEMI: CbCr), [2] Cr (SEMI: must be all zero), [3] alpha (ptr NULL: not written) */
  int32_t layout, dtype;      /* HM_DEV_PLANES_*, HM_DEV_U8 / _U16 / _F16 / _F32 */
  int32_t msb_aligned;        /* HM_DEV_U16 only: store v << (16 - bits), the P010 / P012 convention; otherwise 0 */
  int32_t reserved;           /* 0 */
  float   scale[4], bias[4];  /* float dtypes, per component Y, Cb, Cr, A */
} hm_device_planes;
/* Bytes the planes must hold for a result of this chroma format (HM_CHROMA_*), depth and luma size: need[c] (may be NULL) =
 * row_pitch * (rows - 1) + tight per plane - 0 for a plane that does not exist (Cb / Cr of 4:0:0, Cr of HM_DEV_PLANES_SEMI);
 * need[3] is what an alpha plane takes.  Returns need[0] + need[1] + need[2], plus need[3] when d->plane[3].ptr is non-NULL, or the
 * negative status of a combination that is refused.  Pure host arithmetic: no device needed; no len and no other ptr is looked at. */
HM_API int64_t hm_device_planes_bytes(int chroma, int bits, int width, int height, const hm_device_planes* d, int64_t need[4]);
/* The step on its own, on planes that are on the device already (the sibling of hm_to_tensor): d_src[0 .. 2] Y, Cb, Cr (Cb / Cr
 * unused for HM_CHROMA_MONO), d_src[3] the alpha plane with alpha_bits > 0 (alpha_bits 0: none), src_stride in bytes; samples are
 * bytes for 8 bits, little-endian 16-bit words above.  Asynchronous on `stream`. */
HM_API int hm_planes_to_tensor(int chroma, int bits, int width, int height, int alpha_bits, const void* const d_src[4], const int32_t src_stride[4],
                               const hm_device_planes* planes, void* stream);
/* hm_decode_item with the planes going to `planes`: returns when they are in place (the work runs on params->stream).  params->
 * out_format: 0 or HM_OUT_YCBCR_*.  `out` is filled as for an ext_dst decode: used_ext_dst = 1, every plane[] and alpha NULL,
 * stride[c] / alpha_stride = the pitches in use (SEMI: stride[2] = 0); plane_width / height, chroma, bit_depth, the nclx fields
 * and warnings exactly as hm_decode_item sets them. */
HM_API int hm_decode_item_to_device_planes(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_planes* planes, hm_decoded* out);
/* The sequence form: frames[0 .. count) are 1-based frame IDs in any order, repeats allowed, decoded in ONE device batch as by
 * hm_decode_frames_to_device_view, planes[k] the destination of frames[k] (one launch of the plane kernel per frame).  A frame whose
 * data or destination fails fails the call before anything is written, *failed_frame (may be NULL) = its index k, -1 otherwise. */
HM_API int hm_decode_frames_to_device_planes(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                             const hm_device_planes* planes, hm_decoded* out, int32_t* failed_frame);
/* hm_pipeline_submit with a planar destination (copied); the pipeline's out_format must be 0 or HM_OUT_YCBCR_* [| HM_OUT_YCBCR_8BIT].
 * The planes are complete when hm_pipeline_next hands the result out. */
HM_API int hm_pipeline_submit_to_device_planes(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                               const hm_device_planes* planes);

/* ------------------------------------------------------------------------- */
/* Views: a rectangle of the image, at a size of the caller's choice, into the destination */
/* ------------------------------------------------------------------------- */

/* "This rectangle of the image, at this size, in this tensor": crop and resampling are fused into the step that writes the
 * destination, and of a grid only the tiles the rectangle touches are entropy-decoded, uploaded and reconstructed (where that
 * provably changes no pixel: no transformation applied on the item or a covered tile, no alpha image, default chroma
 * up-sampling, a sub-grid origin that is even in every subsampled direction - hm_plan_view tells; everything else decodes the
 * whole item and applies the view at the end, with identical bytes).  A coded picture outside the sub-grid is not looked at:
 * damage there neither fails the call nor sets HM_WARN_CONCEALED.
 * Per axis, n = crop extent, m = output extent, a = the filter's support (1 HM_VIEW_TRIANGLE, 2 HM_VIEW_CUBIC, 3 HM_VIEW_LANCZOS3),
 * in double:  s = n / m, fs = max(s, 1), c = (j + 0.5) * s, lo = max(0, (int)(c - a * fs + 0.5)), hi = min(n, (int)(c + a * fs + 0.5)),
 * w_i = k((i + 0.5 - c) / fs) for i in [lo, hi), table entry (float)(w_i / W) with W the sum of the w_i in increasing i (taps never
 * leave the crop: "crop, then resize").  The kernel function k of x, with every operation rounded on its own, on |x|:
 *   HM_VIEW_TRIANGLE  max(0, 1 - x): the antialiased bilinear filter of PIL and of torch.nn.functional.interpolate(mode="bilinear",
 *                     antialias=True);
 *   HM_VIEW_CUBIC     Keys' cubic with a = -0.5, PIL's BICUBIC and torch's interpolate(mode="bicubic", antialias=True):
 *                     x < 1: (1.5 * x - 2.5) * x * x + 1;  1 <= x < 2: ((-0.5 * x + 2.5) * x - 4) * x + 2;  otherwise 0;
 *   HM_VIEW_LANCZOS3  x == 0: 1;  x < 3: (sin(p) / p) * (sin(q) / q) with p = pi * x (pi = 3.14159265358979323846), q = p / 3 and the
 *                     C library's sin;  otherwise 0.
 * Per channel (alpha like any other; premultiplication: "Alpha" below), in float32 without fused multiply-add: horizontally
 * t = 0, t = t + w * (float)v for i increasing, then vertically the same over the t, giving r; integer destinations store
 * min(max((int)(r + 0.5f), 0), peak) with peak 255 / 65535, float destinations r * scale[c] + bias[c] (r not rounded first).
 * The cubic and Lanczos weights are negative in places, so r can lie below 0 and above the peak (overshoot at hard edges): the
 * conversion (int)(r + 0.5f) is towards zero - a negative r + 0.5f above -1 becomes 0 - and both clamps act; a float destination
 * receives the overshoot as it is.
 * HM_VIEW_NEAREST moves the sample at j * n / m (int arithmetic).  out_w == out_h == 0 is the crop alone: the bytes of the full
 * decode's rectangle.  The crop alone and HM_VIEW_NEAREST to HWC with the target's own integer type move bytes: _BE targets allowed.
 * Refused with HM_ERR_INVALID_ARG before any work is queued, the destination unwritten: a crop with a non-positive extent or
 * not inside the image, an output extent below 1 or above 32768, a reduction n / m on an axis above 256 (HM_VIEW_TRIANGLE,
 * HM_VIEW_NEAREST), above 128 (HM_VIEW_CUBIC) or above 85 (HM_VIEW_LANCZOS3) - no output has more than 2 * 256 + 2 taps -, an
 * unknown filter, a resampling filter (every one but HM_VIEW_NEAREST) with a _BE target (ask for _LE), and whatever
 * hm_decode_item_to_device refuses, judged against out_w x out_h. */
enum { HM_VIEW_TRIANGLE = 0,   /* antialiased bilinear, defined above */
       HM_VIEW_NEAREST  = 1,   /* the reference's scale_nearest_neighbor index rule (pixelimage.cc:1232-1251) */
       HM_VIEW_CUBIC    = 16,  /* antialiased bicubic (Keys, a = -0.5), defined above */
       HM_VIEW_LANCZOS3 = 17 };/* antialiased Lanczos with three lobes, defined above */
typedef struct hm_device_view {
  int32_t crop_x, crop_y, crop_w, crop_h;  /* rectangle of the image as hm_decode_item hands it out (after irot / imir /
                                              clap unless ignore_transformations); crop_w == crop_h == 0: the whole image */
  int32_t out_w, out_h;                    /* size written to the destination; 0, 0 = the crop's own size (crop only) */
  int32_t filter;
} hm_device_view;
/* hm_decode_item_to_device with `dest` sized for out_w x out_h (hm_device_dest_bytes of that size); out->width / height: the
 * size written.  warnings: of the coded pictures that were decoded; a grid's profile fields: of the first tile decoded. 
 * A derived item: the view is taken of the composed image; layers of an 'iovl' item without transformations that do not touch
 * the crop are not decoded (hm_plan_overlay). */
HM_API int hm_decode_item_to_device_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                         const hm_device_dest* dest, hm_decoded* out);
/* the pipeline form: images of different sizes into the slices of one N x C x H x W allocation */
HM_API int hm_pipeline_submit_to_device_view(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                             const hm_device_view* view, const hm_device_dest* dest);
/* The sequence form: frames[0 .. count) are 1-based frame IDs of a sequence, in any order, repeats allowed (every k-th frame of
 * a track: a temporal stride).  All of them are decoded in ONE device batch, as by hm_decode_sequence_to_device, and the ONE view
 * is taken of every frame - resolved against that frame's own decoded size - into dests[k], which is sized for out_w x out_h (the
 * crop's size when out_w == out_h == 0); out[k].width / height: the size written.  Frames that agree in crop, output size and in
 * their destination's layout, dtype, pitches, scale, bias and 16-byte alignment (the frames of a clip into the slices of one
 * T x C x H x W allocation do) share their two tap tables and one kernel launch per resampling pass; the bytes are those of `count`
 * calls of hm_decode_item_to_device_view.  view == NULL: hm_decode_sequence_to_device on those frames.
 * Refused before anything is queued, every destination unwritten: what hm_decode_sequence_to_device and
 * hm_decode_item_to_device_view refuse (HM_ERR_UNSUPPORTED for out_format 0 and the planar HM_OUT_YCBCR_* targets), a frame ID
 * outside 1 .. frame_count, a file that is not a sequence.  *failed_frame (may be NULL) = the index k into frames[] when the
 * failure is one frame's - its data, its destination, a view that does not fit that frame's size -, -1 otherwise. */
HM_API int hm_decode_frames_to_device_view(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                           const hm_device_view* view, const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame);
/* The step on its own, on interleaved pixels that are on the device already (as hm_to_tensor).  Asynchronous on `stream`. */
HM_API int hm_resample_to_tensor(int out_format, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                                 const hm_device_dest* dest, void* stream);
/* Host arithmetic: tiles[] = first tile row, row count, first tile column, column count a view decode of this item will
 * entropy-decode; a single image, or a view that is not reduced: the whole grid (0, rows, 0, cols). */
HM_API int hm_plan_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t tiles[4]);
/* which layers of overlay `id` a decode (view NULL) or a decode under `view` would decode: decoded[i] = 1 / 0 for i < max_children
 * (a layer that does not touch the canvas - under a view without transformations on the overlay: the crop - is not decoded).
 * Returns the number of layers, or a negative status: everything a decode refuses without looking at a picture. */
HM_API int hm_plan_overlay(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t* decoded, int max_children);
/* Host arithmetic: the taps of output index j on one axis of n_in -> n_out.  Returns their count (or a negative status),
 * *first = the first source index, weights[0 .. min(count, cap)) = the weights the kernels use. */
HM_API int hm_view_filter_taps(int n_in, int n_out, int filter, int j, int32_t* first, float* weights, int cap);

/* ------------------------------------------------------------------------- */
/* Light: linear-light output, a change of primaries, views that average light */
/* ------------------------------------------------------------------------- */

/* The entry points above hand out the transfer-encoded code values of the colour stage.  A light step in the write of the
 * destination turns them into linear light, optionally changes the primaries, and stores linear floats or re-encodes; a view
 * then resamples LIGHT, not code values (a one-pixel black / white checkerboard in sRGB halved with HM_VIEW_TRIANGLE is code 188,
 * not 128).  No transcendental function runs on the device: the transfer functions are tables built on the host in double, the
 * re-encoding is a search in a threshold table, and every float32 operation is rounded on its own - a float32 restatement on the
 * host is exact.
 * Transfer codes (H.273), in both directions: 1, 6, 14, 15 the BT.709 curve with the exact constants alpha = 1.09929682680944,
 * beta = 0.018053968510807 (E' < 4.5 beta: E' / 4.5, else ((E' + alpha - 1) / alpha)^(1 / 0.45); the rounded 1.099 / 0.081 pair is
 * not monotone across the knee at 12 bits);  4 gamma 2.2;  5 gamma 2.8;  8 linear;  13 sRGB (IEC 61966-2-1: E' <= 0.04045:
 * E' / 12.92, else ((E' + 0.055) / 1.055)^2.4);  16 PQ, the ST 2084 EOTF, 1.0 = 10000 cd/m2;  18 HLG, the INVERSE OETF of BT.2100
 * only: scene light, no OOTF is applied - that is a step of its own, "OOTF" below - (E' <= 0.5: E'^2 / 3, else
 * (exp((E' - c) / a) + b) / 12, a = 0.17883277, b = 1 - 4 a, c = 0.5 - a log(4 a)).
 * Primaries: 1, 5, 6, 7, 9, 12 - all with a D65 white; no chromatic adaptation.  Any other code: HM_ERR_UNSUPPORTED.
 *   bits = the target's sample depth: 8 for HM_OUT_RGB / _RGBA, hm_decoded.bit_depth for the _LE 16-bit targets (at most 12: both
 *   tables sit in the kernels' local memory; deeper: HM_ERR_UNSUPPORTED);  peak = (1 << bits) - 1;  F_t = the code-to-light function
 *   of transfer t on [0, 1];  g = (double)gain.
 *   Tables, in double with the C library's pow / exp / log:  lin[c] = (float)(g * F_from(c / peak)), c = 0 .. peak;
 *   enc[c] = (float)(g * F_to((c - 0.5) / peak)), c = 1 .. peak.
 *   Colour channels: a source sample v becomes a = lin[min(v, peak)].  Under a view a replaces (float)v in the sums stated under
 *   "Views" (same tap tables, horizontal first, tap 0 first, __fmul_rn / __fadd_rn), giving r; without a view, with the crop alone
 *   or HM_VIEW_NEAREST r = a of the sample that is moved.  The alpha channel is not light: a = (float)v, finished as without a light
 *   step (no premultiplication; with an alpha step beside the light step: "Alpha" below).
 *   Gamut: when to_primaries is non-zero and differs from the source's, per output pixel, after the resampling:
 *   R' = fadd(fadd(fmul(m0, R), fmul(m1, G)), fmul(m2, B)), G' and B' with m3 .. m5 and m6 .. m8; m = hm_light_matrix's, derived in
 *   double from the H.273 chromaticities as (to -> XYZ)^-1 (from -> XYZ), then rounded to float32.
 *   Finish: HM_LIGHT_LINEAR stores fadd(fmul(r, scale[c]), bias[c]), HM_DEV_F16 through __float2half_rn; integer dtypes are refused.
 *   Otherwise code = |{c in 1 .. peak : enc[c] <= r}| - negative values and overshoot clamp to 0 and peak by themselves -; an integer
 *   dtype (the target's own) stores code, a float dtype fadd(fmul((float)code, scale[c]), bias[c]).  With to_transfer ==
 *   from_transfer, no view and no matrix the codes are the source's: enc[c] <= lin[c] < enc[c + 1] holds for every table.
 * Refused before any work is queued, the destination unwritten: reserved != 0, a gain that is not finite or not above 0,
 * HM_LIGHT_LINEAR with an integer dtype, a _BE target (all HM_ERR_INVALID_ARG), an unknown or unsupported code
 * (HM_ERR_UNSUPPORTED), and everything the view and the destination checks refuse.  What depends on the image's own profile or
 * depth (from_* == 0) is refused before a byte of the destination is written.  Planar targets stay refused: light is an RGB notion. */
enum { HM_LIGHT_LINEAR = 8 };              /* H.273 transfer code 8 */
typedef struct hm_device_light {
  int32_t from_transfer, from_primaries;   /* H.273 codes; 0 = the image's own: what this call's hm_decoded reports
                                              (has_nclx == 0 or code 2: transfer 13, primaries 1; an ICC profile is not read);
                                              HM_LIGHT_FROM_ICC in BOTH: the item's ICC profile ("ICC" below) */
  int32_t to_transfer;                     /* HM_LIGHT_LINEAR: linear light, float dtypes only; another supported code: re-encoded */
  int32_t to_primaries;                    /* 0 = keep the source's */
  float   gain;                            /* finite, > 0: multiplies linear light (PQ: 1.0 = 10000 cd/m2) */
  int32_t reserved[3];                     /* 0 */
} hm_device_light;
/* hm_decode_item_to_device[_view] with a light step; view NULL: the whole image.  The item is decoded as one job (of a grid under
 * a view: the tiles hm_plan_view names). */
HM_API int hm_decode_item_to_device_light(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                          const hm_device_light* light, const hm_device_dest* dest, hm_decoded* out);
/* hm_decode_frames_to_device_view with a light step (view may be NULL): one decode batch; the write is one launch per frame and pass */
HM_API int hm_decode_frames_to_device_light(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                            const hm_device_view* view, const hm_device_light* light, const hm_device_dest* dests, hm_decoded* out,
                                            int32_t* failed_frame);
/* the pipeline form (view may be NULL) */
HM_API int hm_pipeline_submit_to_device_light(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                              const hm_device_view* view, const hm_device_light* light, const hm_device_dest* dest);
/* The step on its own, on interleaved pixels of `bits` bits that are on the device already (as hm_to_tensor / hm_resample_to_tensor;
 * view may be NULL).  from_transfer and from_primaries must be explicit.  Asynchronous on `stream`. */
HM_API int hm_light_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                              const hm_device_light* light, const hm_device_dest* dest, void* stream);
/* Host arithmetic, no device: the 1 << bits entries the kernels use - encode == 0: lin, else enc (entry 0 is 0 and is never looked
 * at).  bits 8 .. 12.  Returns the count, or a negative status. */
HM_API int hm_light_table(int transfer, int bits, float gain, int encode, float* out);
/* Host arithmetic, no device: the row-major float32 matrix from one set of primaries to another (the identity, exactly, for equal codes) */
HM_API int hm_light_matrix(int from_primaries, int to_primaries, float m[9]);

/* ------------------------------------------------------------------------- */
/* ICC: the item's matrix/TRC profile as the source colour description of the light step */
/* ------------------------------------------------------------------------- */

/* HM_LIGHT_FROM_ICC in from_transfer AND from_primaries of hm_device_light (in one only: HM_ERR_INVALID_ARG) makes the light step read
 * the RGB code values through the ICC profile of the item - the profile hm_file_item_icc(f, id, 1, ...) reports, 'prof' or 'rICC'; with
 * a gain step: of the base image.  Every value that was valid before keeps its meaning; 0 still is "the nclx or the default, the profile
 * not read".  An nclx beside the profile keeps deciding the YCbCr -> RGB chain; only the light step's reading of the RGB codes changes.
 * The profile is parsed before anything is queued: an item without one (HM_ERR_INVALID_ARG) or with one the reader refuses (its status)
 * fails there, the destination unwritten.
 * What is read: ICC.1 versions 2.x and 4.x, header signature 'acsp', class 'mntr', 'scnr' or 'spac', connection space 'XYZ ', data
 * colour space 'RGB ' with rXYZ, gXYZ, bXYZ ('XYZ ' type) and rTRC, gTRC, bTRC, or 'GRAY' with kTRC (it stands for all three channels);
 * TRC tags of type 'curv' or 'para'.  Every offset and size is checked against the profile's size field, the size field against the bytes
 * given; nothing outside them is read.  The 'chad' tag is not used: the colorants of a conforming profile are in D50 already.
 * Curves, in double with the C library's pow, X in [0, 1]:
 *   'curv', count 0: Y = X;  count 1: Y = pow(X, g), g = the u8Fixed8 entry / 256;  count n >= 2: t[k] = entry k / 65535.0,
 *   pos = X * (n - 1), i = min((int)pos, n - 2), Y = t[i] + (pos - i) * (t[i + 1] - t[i]).
 *   'para', function type 0 .. 4, parameters g a b c d e f as s15Fixed16 / 65536.0, P(X) = pow(max(a * X + b, 0), g):
 *   0: pow(X, g);  1: X >= -b / a ? P(X) : 0;  2: X >= -b / a ? P(X) + c : c;  3: X >= d ? P(X) : c * X;  4: X >= d ? P(X) + e : c * X + f.
 *   g <= 0, or a == 0 in types 1 and 2: malformed.  Y is clamped to [0, 1].
 *   lin_c[v] = (float)(g * Y_c(v / peak)), v = 0 .. peak, g = (double)gain: hm_icc_table.
 * Matrix (hm_icc_matrix): m = (A T)^-1 M in double, each entry rounded once to float32.  M: the colorant columns (s15Fixed16 / 65536.0).
 *   T: RGB -> XYZ of to_primaries exactly as hm_light_matrix derives it, white xy (0.3127, 0.3290), W = (xw / yw, 1, (1 - xw - yw) / yw).
 *   A: the linear Bradford adaptation from W to the connection-space illuminant I = (0xF6D6, 0x10000, 0xD32D) / 65536:
 *   A = B^-1 diag((B I)_k / (B W)_k) B, B = [0.8951 0.2664 -0.1614; -0.7502 1.7135 0.0367; 0.0389 -0.0685 1.0296].
 *   to_primaries == 0 keeps the profile's own primaries: no matrix.  GRAY: the identity.
 * A 'cicp' tag whose primaries and transfer codes are both ones the light step knows stands for the profile: the source is those H.273
 * codes and the step runs as with explicit codes.  Any other cicp: the curves and colorants are read.
 * Tables on the device: when the three tables are identical at the depth in use one is uploaded and the kernels run as without a profile;
 * otherwise three - red, green, blue - and channel c of a pixel looks up lin[(c << bits) + min(v, peak)].  Everything behind the lookup
 * (sums, matrix, tone step, finish, the alpha and gain steps beside it) is as stated above; an alpha step's background colour goes
 * through its channel's table.  The tone step's rule holds: unit_nits must be given (no profile says what 1.0 stands for).
 * A launch's tables must fit 64 KB of local memory: three distinct 12-bit curves with a 12-bit re-encoding AND a tone step, or any
 * combination above that, is HM_ERR_UNSUPPORTED (the message names the depth and the steps), before a byte of the destination is written.
 * Refused (HM_ERR_UNSUPPORTED, the message names the reason): major version 5 or any other than 2 and 4, connection space Lab, device
 * link, abstract, named-colour and every other class, CMYK and other data spaces, profiles with only A2B0 / lookup-table tags and no
 * matrix/TRC set; an OOTF step beside the profile (it renders HLG scene light, which no matrix/TRC profile describes); the frames family
 * (a track's sample entry profile is not read); the stand-alone forms other than hm_icc_to_tensor (they have no item); a profile as the
 * destination and planar targets stay out of scope.  Malformed (HM_ERR_BITSTREAM): a size field above the bytes given or below the
 * header, a tag table that runs off the end, a tag that overlaps the header or the tag table or runs past the end, a missing tag of the
 * set, a tag whose type signature is not the one its use needs, a bad curve. */
enum { HM_LIGHT_FROM_ICC = -1 };
enum { HM_ICC_RGB = 1, HM_ICC_GRAY = 2 };
enum { HM_ICC_CURVE_IDENTITY = 0, HM_ICC_CURVE_GAMMA = 1, HM_ICC_CURVE_TABLE = 2, HM_ICC_CURVE_PARA = 3 };
typedef struct hm_icc_curve {
  int32_t kind;                            /* HM_ICC_CURVE_* */
  int32_t count;                           /* 'curv': its entry count; 'para': the function type 0 .. 4 */
  double  p[7];                            /* 'para': g a b c d e f (those the type has, the rest 0); GAMMA: p[0] = g; else 0 */
} hm_icc_curve;
typedef struct hm_icc_info {
  int32_t version_major, version_minor;
  int32_t colour_space;                    /* HM_ICC_RGB / HM_ICC_GRAY */
  int32_t same_curves;                     /* the three TRC tags are the same tag data (one offset, or equal bytes); GRAY: 1 */
  int32_t has_cicp;                        /* the profile has a 'cicp' tag: cicp[] = primaries, transfer, matrix, full range */
  int32_t cicp[4];
  int32_t cicp_known;                      /* ... and both its primaries and its transfer are codes the light step knows */
  double  colorant[9];                     /* row-major: column k = the XYZ of r / g / b; GRAY: 0 */
  hm_icc_curve curve[3];                   /* r, g, b; GRAY: kTRC three times */
} hm_icc_info;
/* Host arithmetic, no device.  HM_OK, or the refusal. */
HM_API int hm_icc_parse(const uint8_t* icc, size_t size, hm_icc_info* out);
/* lin_c of channel 0 .. 2 (GRAY: 0) at bits 8 .. 12: 1 << bits floats.  Returns the count, or a negative status. */
HM_API int hm_icc_table(const uint8_t* icc, size_t size, int channel, int bits, float gain, float* out);
/* the row-major float32 matrix from the profile's colorants to to_primaries (a code hm_light_matrix knows) */
HM_API int hm_icc_matrix(const uint8_t* icc, size_t size, int to_primaries, float m[9]);
/* hm_icc_parse on the profile hm_file_item_icc(f, id, 1, ...) reports.  HM_ICC_NO_PROFILE (out zeroed): the item has none. */
enum { HM_ICC_NO_PROFILE = 1 };
HM_API int hm_file_item_icc_info(const hm_file* f, uint32_t id, hm_icc_info* out);
/* (hm_icc_to_tensor, the step on its own with a profile as the source: behind hm_alpha_to_tensor, whose steps it takes) */

/* ------------------------------------------------------------------------- */
/* Tone: the BT.2390 curve by table inside the light step, the content's peak from the file, an 8-bit finish */
/* ------------------------------------------------------------------------- */

/* A tone step exists only beside a light step.  It acts per output pixel on linear light, after the gamut matrix (under a view:
 * after the resampling sums) and before the finish - the same for the pointwise path, HM_VIEW_NEAREST, the crop alone and a
 * resampled view:
 *   N = fmaxf(fmaxf(R, G), B)                   the norm: max RGB in the destination's primaries
 *   k = |{ i in 1 .. 2047 : thr[i] <= N }|      the light step's binary search, 11 steps; N <= 0 gives k = 0
 *   R = fmul(R, sg[k]), G and B likewise        one common factor: the hue is kept, no channel rises above the peak
 * Alpha is untouched.  k is the 11-bit PQ code of the norm's luminance, sg the gain of the curve at that code: the gain is
 * piecewise constant over HM_TONE_STEPS PQ steps.
 * Tables, on the host in double with the C library's pow, each rounded once to float32; g = (double)gain of the light step,
 * U = unit_nits, Uo = out_unit_nits, EOTF the ST 2084 function of transfer 16 above, PQ(y) = ((c1 + c2 y^m1) / (1 + c3 y^m1))^m2
 * its inverse with the same five constants:
 *   thr[0] = 0;  thr[i] = (float)(g * (10000 / U) * EOTF((i - 0.5) / 2047)), i = 1 .. 2047
 *   e = k / 2047, Pw = PQ(src_peak / 10000), E1 = min(e / Pw, 1), maxLum = PQ(dst_peak / 10000) / Pw, KS = 1.5 maxLum - 0.5
 *   maxLum >= 1, E1 < KS or k == 0: ratio = 1, exactly.  Otherwise, with T = (E1 - KS) / (1 - KS):
 *     E2 = (2T^3 - 3T^2 + 1) KS + (T^3 - 2T^2 + T)(1 - KS) + (-2T^3 + 3T^2) maxLum,  ratio = EOTF(E2 Pw) / EOTF(e)
 *   sg[k] = (float)(ratio * U / Uo)
 * This is the EETF of Report ITU-R BT.2390 with both black levels at 0: the black-lift term b (1 - E2)^4 is NOT modelled.
 * dst_peak >= src_peak is not an error: the curve is then the clamp at src_peak.
 * src_peak == 0 is the image's own peak, from the properties of the item that is decoded (of a grid: the grid item): its clli
 * max_content_light_level if non-zero - the field is 16 bits wide and PQ codes no light above 10000 cd/m2: a larger value counts as
 * 10000 -; otherwise its mdcv max_display_mastering_luminance * 0.0001 if the raw value lies in 50000 .. 100000000; otherwise 1000.
 * A frame of a sequence carries no properties: 1000.  (A file without either property can be measured instead: "Light statistics" below.)
 * out_bits == 8, the 8-bit finish: the source samples, lin[] and the sums stay at the target's depth; enc is
 * hm_light_table(to_transfer, 8, gain, 1) and the code counts thresholds over 1 .. 255.  The destination is judged, sized and
 * written as that of the 8-bit sibling target (an HM_OUT_RRGGBB_LE request: hm_device_dest_bytes(HM_OUT_RGB, ...)): HM_DEV_U8 stores
 * the code, float dtypes fadd(fmul((float)code, scale[c]), bias[c]).  With HM_LIGHT_LINEAR there is no code and out_bits only
 * selects the sizing rule; with an 8-bit target it changes nothing.  hm_decoded reports out_format as requested, stride[0] is the
 * row pitch in use.
 * Refused before any work is queued, the destination unwritten - HM_ERR_INVALID_ARG: a null light step, an unknown curve, reserved
 * != 0, a peak or unit that is not finite, not above 0 or above 10000 (0 where it stands for a default), KS < 0 (maxLum < 1 / 3: the
 * knee would lie below black), unit_nits == 0 when the resolved from_transfer is not 16, out_bits other than 0 or 8, out_bits == 8
 * with HM_DEV_U16; HM_ERR_UNSUPPORTED: out_bits == 8 with a four-channel target (bringing a deeper alpha plane to 8 bits under a view
 * is a step of its own; the alpha step's matte has three channels and takes it) - and everything the light, view and destination
 * checks refuse.  One refusal waits for the decoded image, as the light step's from_* == 0 does: whether the resolved from_transfer is 16 is known once the image reports its profile, so a
 * missing unit_nits is refused behind the decode, before a byte of the destination is written (with an explicit from_transfer, and in
 * hm_tone_to_tensor: before any work is queued). */
enum { HM_TONE_BT2390 = 1 };
enum { HM_TONE_STEPS = 2048 };           /* 11-bit PQ codes */
typedef struct hm_device_tone {
  int32_t curve;          /* HM_TONE_BT2390 */
  int32_t out_bits;       /* 0: the target's depth; 8: the 8-bit finish */
  float   src_peak;       /* cd/m2 of the content's peak; 0 = the image's own (rule above) */
  float   dst_peak;       /* cd/m2 of the display's peak, > 0 */
  float   unit_nits;      /* cd/m2 that light value 1.0 (before gain) stands for; 0 = 10000 when the resolved from_transfer is 16 */
  float   out_unit_nits;  /* cd/m2 that light value 1.0 stands for after the step; 0 = dst_peak */
  int32_t reserved[2];    /* 0 */
} hm_device_tone;
/* the light entry points with a tone step */
HM_API int hm_decode_item_to_device_tone(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                         const hm_device_light* light, const hm_device_tone* tone, const hm_device_dest* dest, hm_decoded* out);
HM_API int hm_decode_frames_to_device_tone(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                           const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone,
                                           const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame);
HM_API int hm_pipeline_submit_to_device_tone(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                             const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone,
                                             const hm_device_dest* dest);
/* The step on its own (as hm_light_to_tensor): src_peak, unit_nits and the light step's from_* must be explicit. */
HM_API int hm_tone_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                             const hm_device_light* light, const hm_device_tone* tone, const hm_device_dest* dest, void* stream);
/* Host arithmetic, no device: the HM_TONE_STEPS entries of thr (which == 0) or sg (1) for the light step's gain.  Nothing of the
 * tone step may be left at 0 except out_bits.  Returns HM_TONE_STEPS, or a negative status. */
HM_API int hm_tone_table(const hm_device_tone* tone, float gain, int which, float* out);
/* The raw fields of an item's clli and mdcv properties (ISO/IEC 23008-12; zero where the property is absent) */
typedef struct hm_light_levels {
  int32_t  has_clli, has_mdcv;
  uint16_t max_content_light_level, max_pic_average_light_level;
  uint16_t display_primaries_x[3], display_primaries_y[3];
  uint16_t white_point_x, white_point_y;
  uint32_t max_display_mastering_luminance, min_display_mastering_luminance;
} hm_light_levels;
HM_API int hm_file_item_light_levels(const hm_file* f, uint32_t id, hm_light_levels* out);

/* ------------------------------------------------------------------------- */
/* Alpha: premultiplied sums under a view, straight or premultiplied results, a matte over a colour */
/* ------------------------------------------------------------------------- */

/* Everything above carries the alpha channel "like any other, no premultiplication": a view averages the colour of fully transparent
 * pixels into its sums (dark fringes around a cut-out), and a four-channel result is all a caller can ask for.  An alpha step in the
 * write of a device destination uses alpha: the sums of a view are taken over colour times alpha, and the result is straight colour,
 * premultiplied colour, or the picture composited over a background colour - three channels.  It works alone, under a view, and beside
 * a light step and a tone step, for the four-channel interleaved targets HM_OUT_RGBA and HM_OUT_RRGGBBAA_LE.  A call without the step
 * writes what it wrote before.
 *   bits = the target's sample depth, as in the light step (8 for HM_OUT_RGBA, hm_decoded.bit_depth for HM_OUT_RRGGBBAA_LE; at most 12
 *   when a light step is present);  peak = (1 << bits) - 1;  P = (float)peak.  Every operation is float32 and rounded on its own:
 *   fmul, fadd, fsub, fdiv are __fmul_rn, __fadd_rn, __fsub_rn, __fdiv_rn - never a fused multiply-add, never a reciprocal.
 *   Per source pixel, vR, vG, vB, vA its samples:  a = (float)vA;  x_c = (float)v_c for c = R, G, B - with a light step
 *   x_c = lin[min(v_c, peak)] -;  p_c = fmul(x_c, a).
 *   Where sums are formed - a view with HM_VIEW_TRIANGLE, HM_VIEW_CUBIC or HM_VIEW_LANCZOS3 and out_w, out_h non-zero -, the sums stated
 *   under "Views" are taken over p_c and over a (same tap tables, horizontal first, tap 0 first), giving S_c and S_a.  Per output pixel:
 *     HM_ALPHA_STRAIGHT       r_c = S_a > 0 ? fdiv(S_c, S_a) : 0.0f
 *     HM_ALPHA_PREMULTIPLIED  r_c = fdiv(S_c, P)
 *     HM_ALPHA_MATTE          cov = fminf(fmaxf(fdiv(S_a, P), 0.0f), 1.0f);  r_c = fadd(fdiv(S_c, P), fmul(b_c, fsub(1.0f, cov)))
 *                             with b_c = (float)background[c] - with a light step b_c = lin[background[c]].
 *   Where no sums are formed - no view, the crop alone, HM_VIEW_NEAREST -, S_c = p_c and S_a = a of the pixel that is moved, with one
 *   exception: HM_ALPHA_STRAIGHT is then r_c = x_c - no product and no quotient are taken, and the call writes the bytes of the same
 *   call without the step.
 *   After r_c: without a light step r_c goes through the finish stated under "Views" - an integer dtype stores
 *   min(max((int)(r + 0.5f), 0), peak) with peak 255 / 65535, a float dtype r * scale[c] + bias[c].  With a light step r_c takes the
 *   place of the resampled light: gamut matrix, tone step and the light step's finish follow unchanged.
 *   The alpha element (HM_ALPHA_STRAIGHT, HM_ALPHA_PREMULTIPLIED) is what it is without the step: the sample where the pixel is moved,
 *   the finish of S_a where it is summed.
 *   HM_ALPHA_MATTE writes THREE channels: the destination is judged, sized and written as that of the three-channel sibling target -
 *   HM_OUT_RGB for HM_OUT_RGBA, HM_OUT_RRGGBB_LE for HM_OUT_RRGGBBAA_LE, and HM_OUT_RGB under tone->out_bits == 8 (the tone step's
 *   8-bit finish, whose refusal of a four-channel target does not hold for a matte: its result has no alpha plane).
 *   hm_alpha_dest_format names that target; hm_decoded reports out_format as requested.
 *   A source without an alpha image is accepted: its alpha is peak everywhere.  Alpha that is premultiplied in the file already (a
 *   'prem' reference) is not recognised: the file layer does not read that reference, the samples are taken as straight.
 * Refused with HM_ERR_INVALID_ARG before any work is queued, the destination unwritten: an unknown mode, reserved != 0, a non-zero
 * background outside HM_ALPHA_MATTE, a non-zero background[3], a background value above peak (8-bit targets: at once; 16-bit targets:
 * behind the decode, before a byte is written, like the light step's from_* == 0), a three-channel target, a _BE target,
 * HM_ALPHA_PREMULTIPLIED beside a tone step or beside a light step whose to_transfer is not HM_LIGHT_LINEAR (encoding or tone-mapping
 * premultiplied light is not a defined result) - and everything the view, light, tone and destination checks refuse, for
 * HM_ALPHA_MATTE judged against the sibling target.  Planar targets stay refused. */
enum { HM_ALPHA_STRAIGHT = 1, HM_ALPHA_PREMULTIPLIED = 2, HM_ALPHA_MATTE = 3 };
typedef struct hm_device_alpha {
  int32_t  mode;
  uint16_t background[4];   /* HM_ALPHA_MATTE: R, G, B code values at the target's sample depth; [3] = 0; other modes: all 0 */
  int32_t  reserved[3];     /* 0 */
} hm_device_alpha;
/* Host arithmetic, no device: the target the destination of a request is judged and sized by (hm_device_dest_bytes of it) - out_format,
 * or the three-channel sibling under HM_ALPHA_MATTE -, or the negative status of a request the step itself refuses (tone may be NULL) */
HM_API int hm_alpha_dest_format(int out_format, const hm_device_alpha* alpha, const hm_device_tone* tone);
/* hm_decode_item_to_device_tone with an alpha step; view, light and tone may be NULL (a tone step needs a light step).  Tile
 * reduction under a view stays off for items with alpha images. */
HM_API int hm_decode_item_to_device_alpha(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                          const hm_device_light* light, const hm_device_tone* tone, const hm_device_alpha* alpha,
                                          const hm_device_dest* dest, hm_decoded* out);
/* the pipeline form (no frame-list form: a track's frames carry no alpha image) */
HM_API int hm_pipeline_submit_to_device_alpha(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                              const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone,
                                              const hm_device_alpha* alpha, const hm_device_dest* dest);
/* The step on its own, on interleaved four-channel pixels of `bits` bits that are on the device already (as hm_light_to_tensor /
 * hm_tone_to_tensor, whose explicit from_*, src_peak and unit_nits rules apply; view, light, tone may be NULL).  Asynchronous on `stream`. */
HM_API int hm_alpha_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                              const hm_device_light* light, const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest,
                              void* stream);
/* The light step on its own with a profile as the source (as hm_alpha_to_tensor; view, tone and alpha may be NULL): light must carry
 * HM_LIGHT_FROM_ICC in both fields.  The profile is read before the call returns.  Asynchronous on `stream`. */
HM_API int hm_icc_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                            const uint8_t* icc, size_t icc_size, const hm_device_light* light, const hm_device_tone* tone,
                            const hm_device_alpha* alpha, const hm_device_dest* dest, void* stream);

/* ------------------------------------------------------------------------- */
/* Gain: an SDR base image and its gain map ('tmap', ISO 21496-1) rendered to HDR light for a display's headroom */
/* ------------------------------------------------------------------------- */

/* A gain step exists only beside a light step; a tone step may follow it.  It multiplies the base image's linear light, pixel by
 * pixel, by a factor read from a second, usually smaller, single-channel image - the gain map - weighted by how much headroom the
 * display has.  Targets: HM_OUT_RGB, _RGBA, _RRGGBB_LE, _RRGGBBAA_LE; the alpha element is written as without the step.  A call
 * without the step writes what it wrote before.
 *   Geometry (the planar view's chroma rule with a general factor; the sampling of a gain map is not normative in ISO 21496-1 - this
 *   rule is this library's): the base is W x H, the map MW x MH, both as hm_decode_item hands them out.  sx = (W + MW - 1) / MW must
 *   satisfy MW == (W + sx - 1) / sx, sy likewise with H and MH; a map that fails this is HM_ERR_UNSUPPORTED.  The base takes the crop
 *   (x, y, w, h) to ow x oh exactly as without the step (without a view: the whole image, ow x oh = W x H; the crop alone: ow x oh =
 *   w x h).  x must be a multiple of sx and y of sy, else HM_ERR_INVALID_ARG.  The map takes the crop (x / sx, y / sy,
 *   (w + sx - 1) / sx, (h + sy - 1) / sy) to the same ow x oh under the tap rule stated under "Views" with HM_VIEW_TRIANGLE - or with
 *   HM_VIEW_NEAREST's index rule when the view's filter is HM_VIEW_NEAREST -, whatever filter the base is resampled with.
 *   Tables, on the host in double with the C library's pow / exp2, each entry rounded once to float32:  Hd = (double)headroom,
 *   Hb = base_headroom, Ha = alternate_headroom,  wgt = min(max((Hd - Hb) / (Ha - Hb), 0), 1)  (headroom +inf: 1 for Ha > Hb, 0 for
 *   Ha < Hb).  mbits = the map's sample depth (8 .. 12), mpeak = (1 << mbits) - 1.  Per colour channel c and map code v = 0 .. mpeak:
 *     u = v / mpeak;  when gamma_c != 1: u = pow(u, 1 / gamma_c);  tab_c[v] = (float)exp2(wgt * (min_c + (max_c - min_c) * u)).
 *   When the three channels' parameter sets (min, max, gamma, both offsets) are equal there is one table and one M for all three.
 *   Per output pixel:  M_c = the view sum over tab_c[min(map sample, mpeak)] - horizontal first, tap 0 first, t = 0, t = fadd(t,
 *   fmul(w, a)), then vertically the same over the t; HM_VIEW_NEAREST: tab_c of the sample that is moved.  r_c = the light step's
 *   resampled (or moved) linear light.  With g = (double)gain of the light step, kb_c = (float)(g * base_offset_c) and
 *   ka_c = (float)(g * alternate_offset_c):
 *     r_c = fsub(fmul(fadd(r_c, kb_c), M_c), ka_c)
 *   The update sits before the gamut matrix; the tone step and the light step's finish follow unchanged.
 *   wgt == 0 exactly: the map is not decoded, and the call writes the bytes of the same call without the step.
 * Refused with HM_ERR_UNSUPPORTED, each an open step: an alpha step beside the gain step, a map that is not 4:0:0 (a colour gain
 * map), a map deeper than 12 bits, use_base_primaries == 0 with alternate primaries that differ from the base's (applying the gain in
 * the alternate primaries), planar targets.  Refused with HM_ERR_INVALID_ARG (parameters from a 'tmap' payload: HM_ERR_BITSTREAM)
 * before any work is queued, the destination unwritten: a null light step, a headroom that is NaN or negative, alternate_headroom ==
 * base_headroom, a gamma that is not finite or not above 0, any field that is not finite, reserved != 0 - and everything the light,
 * tone, view and destination checks refuse.  Tile reduction under a view stays off with a gain step (the open step, as for alpha
 * images): the whole base is decoded. */
typedef struct hm_device_gain {
  uint32_t map_item;        /* 0: `id` is a 'tmap' item - base, map and parameters come from the file.  Non-zero: `id` is the base
                               image, map_item any image item of the file (an 'auxl' image with a vendor URN ...), `params` are used */
  float    headroom;        /* log2(display peak / SDR white): >= 0, +inf allowed */
  hm_gain_params params;    /* used with map_item != 0 and by hm_gain_to_tensor; otherwise not looked at */
  int32_t  reserved[4];     /* 0 */
} hm_device_gain;
/* hm_decode_item_to_device_tone with a gain step; view and tone may be NULL.  hm_decoded reports the base image's fields; the tone
 * step's src_peak == 0 reads the properties of item `id`.  Base and map are decoded as ONE job: their pictures share one entropy
 * decode fan-out; the map's own irot / imir / clap apply, and it may be a grid. */
HM_API int hm_decode_item_to_device_gain(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                         const hm_device_light* light, const hm_device_tone* tone, const hm_device_gain* gain,
                                         const hm_device_dest* dest, hm_decoded* out);
/* the pipeline form (no frame-list form: a track carries no 'tmap') */
HM_API int hm_pipeline_submit_to_device_gain(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                             const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone,
                                             const hm_device_gain* gain, const hm_device_dest* dest);
/* The step on its own: interleaved base pixels of `bits` bits and a single-channel map of map_w x map_h samples of map_bits bits (one
 * byte each at 8 bits, else two, little-endian; map_stride in bytes), both on the device already.  gain->map_item is not looked at;
 * the light step's from_* and the tone step's src_peak and unit_nits must be explicit, as in hm_tone_to_tensor; view and tone may be
 * NULL.  Asynchronous on `stream`. */
HM_API int hm_gain_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const void* d_map, int map_stride,
                             int map_w, int map_h, int map_bits, const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone,
                             const hm_device_gain* gain, const hm_device_dest* dest, void* stream);
/* Host arithmetic, no device: the 1 << map_bits entries of tab_channel (channel 0 .. 2) for this headroom.  Returns the count, or a
 * negative status (the step's own refusals of the parameters). */
HM_API int hm_gain_table(const hm_gain_params* params, float headroom, int channel, int map_bits, float* out);

/* ------------------------------------------------------------------------- */
/* OOTF: HLG scene light rendered for a display's peak (the reference OOTF of BT.2100, by table) */
/* ------------------------------------------------------------------------- */

/* The light step turns HLG code values (transfer 18) into SCENE light.  An OOTF step beside it renders that scene light for a display
 * of peak luminance L_W = display_peak: the reference OOTF of Rec. ITU-R BT.2100, F_D = alpha Ys^(gamma - 1) E, with alpha normalised
 * to 1 and the black level at 0, the system gamma adapted to the display's peak.  It exists only beside a light step whose resolved
 * from_transfer is 18.  No transcendental function runs on the device: the factor Ys^(gamma - 1) is a table over the 10-bit HLG codes
 * of the scene luminance, found by the light step's binary search.  A call without the step writes what it wrote before.
 *   Gamma, in double, with L = (double)display_peak:  gamma != 0: the system gamma is (double)gamma, as it is.  Otherwise
 *   400 <= L <= 2000: 1.2 + 0.42 * log10(L / 1000) (BT.2100 Table 5, note 5e); any other L: 1.2 * pow(1.111, log2(L / 1000)) (note 5f).
 *   Luminance weights: y[0 .. 2] = the Y row of the RGB -> XYZ matrix of the SOURCE primaries (the resolved from_primaries), derived in
 *   double from the H.273 chromaticities exactly as hm_light_matrix derives its matrices, each entry rounded once to float32
 *   (primaries 9: 0.2627 / 0.6780 / 0.0593 to four places).
 *   Tables, on the host in double with the C library's pow / exp / log / log10 / log2, each entry rounded once to float32;
 *   g = (double)gain of the light step, F = the code-to-light function of transfer 18 stated under "Light":
 *     thr[0] = 0;  thr[i] = (float)(g * F((i - 0.5) / 1023)), i = 1 .. 1023
 *     sg[k] = (float)pow(F(k / 1023), gamma - 1), k = 1 .. 1023;  sg[0] = sg[1]
 *   Per output pixel, on r_c = the light step's resampled (or moved) linear light - with an alpha step: the alpha step's r_c -, BEFORE
 *   the gamut matrix:
 *     Ys = fadd(fadd(fmul(y[0], R), fmul(y[1], G)), fmul(y[2], B))
 *     k = |{ i in 1 .. 1023 : thr[i] <= Ys }|      a binary search of 10 steps; a negative or NaN Ys gives k = 0
 *     R = fmul(R, sg[k]), G and B likewise
 *   Gamut matrix, tone step and the light step's finish follow unchanged.  Alpha is untouched.
 *   Unit of the result: light value g after the step stands for display_peak cd/m2.
 *   A tone step behind it: unit_nits == 0 resolves to display_peak, src_peak == 0 resolves to display_peak (no file property is
 *   read); everything else of the tone step is as written under "Tone".
 *   Accuracy: the factor is piecewise constant over HM_OOTF_STEPS 10-bit HLG steps of the scene luminance.  With gamma - 1 = 0.2 one
 *   step above E' = 0.5 changes it by about 0.11 %.
 *   Views: under a view the sums are taken over scene light, which is linear; the step follows the sums, as the tone step does.
 * Refused before any work is queued, the destination unwritten - HM_ERR_INVALID_ARG: a null light step, an unknown kind, reserved
 * != 0, a display_peak that is not finite, not above 0 or above 10000, a gamma that is not finite or is negative, a resolved
 * from_transfer other than 18, to_transfer == 18 (display light re-encoded with the OETF alone is not an HLG signal; the inverse
 * OOTF is out of scope), HM_ALPHA_PREMULTIPLIED beside the step; HM_ERR_UNSUPPORTED: a gain step beside it (a gain map's base is
 * SDR) - and everything the light, tone, alpha, view and destination checks refuse.  The from_transfer refusal comes at once where
 * from_transfer is explicit and in hm_ootf_to_tensor; with from_transfer == 0 it comes behind the decode, before a byte of the
 * destination is written (the tone step's unit_nits rule). */
enum { HM_OOTF_HLG = 1 };
enum { HM_OOTF_STEPS = 1024 };          /* 10-bit HLG codes of the scene luminance */
typedef struct hm_device_ootf {
  int32_t kind;            /* HM_OOTF_HLG */
  float   display_peak;    /* L_W, cd/m2 of the display's peak: finite, > 0, <= 10000 */
  float   gamma;           /* 0: the system gamma of display_peak (rule above); else finite, > 0: used as it is */
  int32_t reserved[5];     /* 0 */
} hm_device_ootf;
/* hm_decode_item_to_device_alpha with an OOTF step; view, tone and alpha may be NULL.  ootf == NULL: the bytes of the same call
 * through hm_decode_item_to_device_alpha (alpha given) or hm_decode_item_to_device_tone. */
HM_API int hm_decode_item_to_device_ootf(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                         const hm_device_light* light, const hm_device_ootf* ootf, const hm_device_tone* tone,
                                         const hm_device_alpha* alpha, const hm_device_dest* dest, hm_decoded* out);
/* hm_decode_frames_to_device_tone with an OOTF step; view and tone may be NULL.  ootf == NULL: hm_decode_frames_to_device_tone. */
HM_API int hm_decode_frames_to_device_ootf(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                           const hm_device_view* view, const hm_device_light* light, const hm_device_ootf* ootf,
                                           const hm_device_tone* tone, const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame);
/* the pipeline form; ootf == NULL: hm_pipeline_submit_to_device_alpha (alpha given) or hm_pipeline_submit_to_device_tone */
HM_API int hm_pipeline_submit_to_device_ootf(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                             const hm_device_view* view, const hm_device_light* light, const hm_device_ootf* ootf,
                                             const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest);
/* The step on its own, on interleaved pixels of `bits` bits that are on the device already (as hm_tone_to_tensor / hm_alpha_to_tensor):
 * the light step's from_* must be explicit; view, tone and alpha may be NULL.  ootf == NULL: hm_alpha_to_tensor (alpha given) or
 * hm_tone_to_tensor.  Asynchronous on `stream`. */
HM_API int hm_ootf_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view,
                             const hm_device_light* light, const hm_device_ootf* ootf, const hm_device_tone* tone, const hm_device_alpha* alpha,
                             const hm_device_dest* dest, void* stream);
/* Host arithmetic, no device: the system gamma of the step (the rule above) */
HM_API int hm_ootf_gamma(const hm_device_ootf* ootf, double* gamma);
/* ... the HM_OOTF_STEPS entries of thr (which == 0) or sg (1) for the light step's gain.  Returns HM_OOTF_STEPS, or a negative status. */
HM_API int hm_ootf_table(const hm_device_ootf* ootf, float gain, int which, float* out);
/* ... and the luminance weights y[0 .. 2] of a set of primaries (an unknown code: HM_ERR_UNSUPPORTED) */
HM_API int hm_ootf_luma(int primaries, float out[3]);

/* ------------------------------------------------------------------------- */
/* Views, many of one picture: the crops of a multi-crop training step, the thumbnail sizes of one upload, the face rectangles of a
 * region item - `count` views (hm_device_view, "Views" above) of ONE item from ONE decode.
 *
 * The item is decoded ONCE.  views[k] is resolved against the decoded image and written into dests[k], which is sized for that view's
 * out_w x out_h (the crop's size when out_w == out_h == 0).  out[k].width / height: the sizes written (out[k].stride[0]: the row pitch
 * in use); the other fields of out[k] are those of the one decode.  The bytes in dests[k] are those of
 * hm_decode_item_to_device_view(f, id, params, &views[k], &dests[k], ..), or of its _light / _tone / _alpha / _ootf sibling when steps are
 * given.
 *
 * Steps: light, tone, alpha and ootf may each be NULL; the same steps apply to every view, under the rules of
 * hm_decode_item_to_device_ootf.  HM_LIGHT_FROM_ICC is allowed (the item's profile is at hand).  The entry takes no gain step and no
 * measured tone: those remain on the single-view entries.
 *
 * What is decoded: of a grid, the sub-grid hm_plan_views names - hm_plan_view's rule applied to the bounding rectangle of all crops, taken
 * as one crop (a view without a crop makes that the whole image); under hm_plan_view's conditions that provably changes no pixel, otherwise
 * the whole grid is decoded.  A derived item ('iovl', 'iden') is decoded and composed once, whole, and the views are taken of the result.
 *
 * How it is written: views without a step whose filter resamples (HM_VIEW_TRIANGLE / _CUBIC / _LANCZOS3) are grouped by what a kernel
 * launch has one of - the staged horizontal pass or not, sample format, the destination's layout, dtype, scale, bias and 16-byte
 * alignment - and each group takes one upload and, per bounded chunk of views, ONE launch per resampling pass.  The crop alone and
 * HM_VIEW_NEAREST are written view by view; with a light / tone / OOTF / alpha step every view is written on its own from the one decoded
 * image (the decode is shared; fused stepped passes are not built).
 *
 * Refused before anything is queued, every destination unwritten: count outside 1 .. HM_VIEWS_MOST; a null array; everything the
 * single-view entry refuses for views[k] / dests[k] (*failed_view = k; the message starts with "view k: "); two destinations whose
 * byte ranges - hm_device_dest_bytes of the size written, with row_pitch / plane_pitch as resolved, from ptr - overlap
 * (HM_ERR_INVALID_ARG, the message names both indices); an 'unci' or 'mski' item (HM_ERR_UNSUPPORTED for now: a view of such an item
 * uploads by internal tile, a separate piece - use hm_decode_item_to_device_view per view).  *failed_view (may be NULL) = -1 when the
 * refusal is not one view's. */
enum { HM_VIEWS_MOST = 4096 };
HM_API int hm_decode_item_to_device_views(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* views,
                                          const hm_device_dest* dests, int32_t count, const hm_device_light* light, const hm_device_tone* tone,
                                          const hm_device_alpha* alpha, const hm_device_ootf* ootf, hm_decoded* out /* [count] */,
                                          int32_t* failed_view);
/* The step on its own - the multi form of hm_resample_to_tensor -, on interleaved pixels that are on the device already: no steps.
 * Asynchronous on `stream`.  Refusals as above (a view's message starts with "view k: "). */
HM_API int hm_resample_views_to_tensor(int out_format, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* views,
                                       const hm_device_dest* dests, int32_t count, void* stream);
/* Host arithmetic: hm_plan_view for hm_decode_item_to_device_views - tiles[] = first tile row, row count, first tile column, column count
 * that call will entropy-decode.  count == 1: hm_plan_view's answer. */
HM_API int hm_plan_views(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* views, int32_t count,
                         int32_t tiles[4]);

/* ------------------------------------------------------------------------- */
/* Light statistics: a picture's light levels measured on the device, and a tone step fed from them */
/* ------------------------------------------------------------------------- */

/* The statistic runs over a rectangle of the interleaved pixels: without a view the whole image, with a view the view's crop AT SOURCE
 * RESOLUTION - the source pixels are measured, not the resampled ones (out_w, out_h and filter are checked as the view entries check
 * them and otherwise unused).  Every pixel of the rectangle:
 *   v -> light_in: r_c = lin[min(v_c, peak)]                      the light step's table(s), "Light" above
 *   with an OOTF step: the OOTF step's factor on r                "OOTF" above
 *   with to_primaries set: the gamut matrix on r
 *   N = fmaxf(fmaxf(R, G), B)
 *   k = |{ i in 1 .. 2047 : thr[i] <= N }|                        the tone step's search in the tone step's own thr[] for the light
 *                                                                 step's gain g and U = unit_nits; a negative or NaN N gives k = 0
 * - exactly what the pointwise tone step would compute for that pixel.  Alpha is ignored; to_transfer plays no part.  k is the PQ code
 * of N * U / g cd/m2: it does not depend on g or U.
 * Everything below is an integer count or a maximum: no result depends on the order in which the device's workgroups finish, and
 * two calls give identical structs.
 *   pixels        of the rectangle; the sum of hist[]
 *   hist[k]       pixels whose norm has code k
 *   max_norm      the largest N, bit for bit (0 if no N is above 0)
 *   max_code      the highest k with hist[k] != 0
 *   max_nits      (float)((double)max_norm * U / g)
 *   average_nits  the sum over k, in increasing k, of (double)hist[k] * code_nits(k, 0), in double, divided by pixels, rounded once
 *                 to float: taken on the host from the histogram
 * code_nits(k, edge) = 10000 * EOTF(x / 2047), EOTF the ST 2084 function of transfer 16; edge 0: x = k, the code's own light; edge 1:
 * x = min(k + 0.5, 2047), the upper edge of bin k - no pixel of bin k is brighter.
 * percentile(fraction), fraction in (0, 1]: rank = min(max((uint64_t)ceil(fraction * (double)pixels), 1), pixels); code = the smallest
 * k whose cumulative count reaches rank; nits = (float)code_nits(code, 1).  fraction == 1 gives max_code.
 * unit_nits must be given (finite, above 0, at most 10000), except that 0 stands for 10000 when the resolved from_transfer is 16 and
 * for display_peak beside an OOTF step - the tone step's rule.
 * The measured tone step (hm_decode_item_to_device_measured): the item is decoded once, measured, and written through the tone step
 * with src_peak = the nits of percentile(fraction) - the upper bin edge, always above 0 and at most 10000 - in place of the clli /
 * mdcv / 1000 rule.  Everything else is hm_decode_item_to_device_ootf (without an alpha step): the same plan, the same write, the
 * bytes of that entry called with this src_peak.  tone->src_peak must be 0 there: an explicit peak is the _tone entry's.
 * The gain step has no place in these signatures: the light of a gain-mapped rendition depends on the headroom asked for, and is
 * measured on that rendition's pixels (hm_light_stats_of_tensor) where it is wanted.  Derived items are not supported.
 * Refused before anything is queued, *stats and *out untouched - HM_ERR_INVALID_ARG: a null light, out or stats where it is required,
 * reserved != 0, a fraction that is not finite or outside (0, 1], a unit_nits the tone step would refuse, a _BE target, a src_peak
 * other than 0 in the measured entry; HM_ERR_UNSUPPORTED: a derived item, tables that do not fit a workgroup's local memory (12-bit
 * samples through three distinct ICC curves) - and everything the light, OOTF, view and destination checks refuse.  Behind the
 * decode, before a byte of the destination is written: what waits for the image's profile (the tone step's unit_nits rule), and the
 * knee of the measured peak (KS < 0). */
enum { HM_LIGHT_STATS_BINS = 2048 };   /* == HM_TONE_STEPS */
typedef struct hm_light_stats {
  uint64_t pixels;                      /* of the rectangle; == the sum of hist[] */
  uint32_t hist[HM_LIGHT_STATS_BINS];   /* hist[k] = pixels whose norm has code k */
  float    max_norm;                    /* the largest N (0 if none is above 0), bit-exact */
  int32_t  max_code;                    /* highest k with hist[k] != 0 */
  float    max_nits;                    /* (float)((double)max_norm * U / g) */
  float    average_nits;                /* rule above */
  int32_t  reserved[2];                 /* 0 */
} hm_light_stats;
/* Host arithmetic, no device: code_nits (k in 0 .. 2047, edge 0 or 1) */
HM_API int hm_light_stats_code_nits(int k, int edge, double* nits);
/* ... and the percentile of a statistic; code and nits may each be NULL */
HM_API int hm_light_stats_percentile(const hm_light_stats* stats, double fraction, int32_t* code, float* nits);
/* ... and average_nits of its histogram and pixels, as the entries below fill it in */
HM_API int hm_light_stats_average(const hm_light_stats* stats, float* nits);
/* The statistic of interleaved pixels of `bits` bits that are on the device already (as hm_tone_to_tensor: from_transfer and
 * from_primaries must be explicit); view and ootf may be NULL.  Returns when the numbers are in *out: `stream` has been waited for. */
HM_API int hm_light_stats_of_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride,
                                    const hm_device_view* view, const hm_device_light* light, const hm_device_ootf* ootf, float unit_nits,
                                    hm_light_stats* out, void* stream);
/* Decode and measure, with no destination: from_* == 0 and HM_LIGHT_FROM_ICC resolve as in hm_decode_item_to_device_light; under a
 * view only the tiles hm_plan_view names are decoded.  view and ootf may be NULL.  *out reports the image; it holds no pixels. */
HM_API int hm_decode_item_light_stats(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                      const hm_device_light* light, const hm_device_ootf* ootf, float unit_nits, hm_light_stats* stats,
                                      hm_decoded* out);
/* Decode once, measure, tone-map with what was measured, write (rule above); view, ootf and stats may be NULL. */
HM_API int hm_decode_item_to_device_measured(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                             const hm_device_light* light, const hm_device_ootf* ootf, const hm_device_tone* tone,
                                             double fraction, const hm_device_dest* dest, hm_decoded* out, hm_light_stats* stats);

/* ------------------------------------------------------------------------- */
/* Planar views: a rectangle of the image, at a size of the caller's choice, into I420 / NV12 / P010 planes */
/* ------------------------------------------------------------------------- */

/* A view into hm_device_planes treats EVERY PLANE AS AN IMAGE OF ITS OWN under hm_device_view's rule: the tap table per axis, the
 * filters, the float32 sums (tap 0 first, horizontal pass first, no fused multiply-add) and HM_VIEW_NEAREST's index rule are those
 * stated above; only the geometry per plane and the final store are new.
 *   Geometry: the result has chroma format `chroma` and luma size W x H; the crop is (x, y, w, h) (the whole image when crop_w ==
 *   crop_h == 0), the output size ow x oh (the crop's own size when out_w == out_h == 0).  Y and alpha take the crop (x, y, w, h) to
 *   ow x oh.  Cb and Cr take the crop (x / sx, y / sy, (w + sx - 1) / sx, (h + sy - 1) / sy) of the chroma plane to
 *   ((ow + sx - 1) / sx, (oh + sy - 1) / sy) - exactly the plane size of an ow x oh result -, with sx = 2 for 4:2:0 / 4:2:2, sy = 2
 *   for 4:2:0, otherwise 1.  x must be a multiple of sx and y of sy, else HM_ERR_INVALID_ARG; odd extents are fine.  The chroma
 *   crop always lies inside the chroma plane: (x + w + 1) / 2 <= (W + 1) / 2.  A 4:0:0 result has Y only.  No chroma siting is
 *   modelled: "each plane on its own".
 *   Checks: the filter's reduction limit holds per plane and axis; the destination is checked as hm_device_planes is, against an
 *   ow x oh result: hm_device_planes_bytes(chroma, bits, ow, oh, ...) sizes it.
 *   Final store: integer dtypes store min(max((int)(r + 0.5f), 0), peak) << shift with peak = (1 << bits) - 1 OF THAT PLANE'S OWN
 *   DEPTH (1023 for a 10-bit plane, not 65535; the alpha plane: its own depth) and shift = msb_aligned ? 16 - that depth : 0.  Float
 *   dtypes store r * scale[c] + bias[c], c = Y, Cb, Cr, A, unclamped, rounded as hm_device_planes states.  HM_DEV_PLANES_SEMI:
 *   element 2 x of a row is the resampled Cb, element 2 x + 1 the resampled Cr.  The crop alone and HM_VIEW_NEAREST move samples
 *   (<< shift, or through scale and bias).  Only plane_width x plane_height elements per plane are written: no pitch padding,
 *   nothing behind the last row.  Every refusal happens before any work is queued, with no plane written.
 * Of a grid decoded as coded (out_format 0) only the tiles the crop touches are decoded, under the conditions of hm_plan_view (no
 * transformation, no alpha image, the sub-grid's origin moved out to even): hm_plan_planes_view tells.  HM_OUT_YCBCR_* targets decode
 * the whole item and take the view of the chain's result - the chain's up- and down-sampling operations read neighbours across
 * tile borders; reducing them is the open step. */
/* Host arithmetic, no device needed: crop[c] = x, y, w, h inside plane c and out[c] = w, h written, c = 0 Y, 1 Cb, 2 Cr, 3 alpha
 * (all zero for Cb / Cr of HM_CHROMA_MONO), of `view` on a width x height result of chroma format `chroma`; or the view's refusal. */
HM_API int hm_planes_view_geometry(int chroma, int width, int height, const hm_device_view* view, int32_t crop[4][4], int32_t out[4][2]);
/* hm_decode_item_to_device_planes with `planes` sized for out_w x out_h; out->width / height and plane_width / height[c]: the sizes
 * written.  Crop coordinates are in the image as hm_decode_item hands it out. */
HM_API int hm_decode_item_to_device_planes_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view,
                                                const hm_device_planes* planes, hm_decoded* out);
/* The sequence form (hm_decode_frames_to_device_planes with ONE view of every frame): one decode batch, then one grouped write -
 * frames that agree in the view's geometry and in their destination's layout, dtype, pitches, scale, bias and 16-byte alignment
 * share their tap tables and one launch per pass.  The bytes are those of `count` item calls. */
HM_API int hm_decode_frames_to_device_planes_view(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params,
                                                  const hm_device_view* view, const hm_device_planes* planes, hm_decoded* out, int32_t* failed_frame);
/* the pipeline form: images of different sizes into equally sized surfaces */
HM_API int hm_pipeline_submit_to_device_planes_view(hm_pipeline* p, const uint8_t* heif, size_t size, uint32_t item_id, uint64_t tag,
                                                    const hm_device_view* view, const hm_device_planes* planes);
/* The step on its own, on planes that are on the device already (the sibling of hm_planes_to_tensor and hm_resample_to_tensor):
 * d_src / src_stride / alpha_bits as hm_planes_to_tensor takes them, of a width x height image.  Asynchronous on `stream`. */
HM_API int hm_resample_planes_to_tensor(int chroma, int bits, int width, int height, int alpha_bits, const void* const d_src[4], const int32_t src_stride[4],
                                        const hm_device_view* view, const hm_device_planes* planes, void* stream);
/* hm_plan_view for a planar view decode of this item (hm_plan_view's own answers for planar formats stay "the whole grid") */
HM_API int hm_plan_planes_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t tiles[4]);

/* ------------------------------------------------------------------------- */
/* Uncompressed items: ISO/IEC 23001-17 'unci' (cmpd + uncC)                  */
/* ------------------------------------------------------------------------- */

/* An 'unci' item stores its samples uncompressed, in one of five interleave modes, optionally cut into a grid of equally sized
 * internal tiles.  hm_file_unci_info hands out what its 'cmpd' and 'uncC' properties say, checked; hm_unci_layout.h states the byte
 * layout that follows from it (ISO/IEC 23001-17 5.2) in closed form; hm_unci_unpack gathers the samples on the device.
 * uncC version 1 carries a profile only: 'rgb3' (R, G, B), 'rgba' (R, G, B, A), 'abgr' (A, B, G, R) - 8-bit, pixel-interleaved, one
 * tile, no padding; no cmpd is needed.
 * HM_ERR_UNSUPPORTED: block_size != 0, any of the components_little_endian / block_pad_lsb / block_little_endian / block_reversed
 * flags, a component format other than unsigned, interleave modes above 4 (multi-Y), sampling types above 4:2:0 (4:1:1), a component
 * type above 7 other than padded (12), mixed interleave without sub-sampling, sub-sampling outside component / mixed interleave,
 * generic compression ('cmpC' / 'icbr'), an image size that the tile counts do not divide, pixel_size outside pixel interleave,
 * a component align size below the component's depth, depths above 16, more than HM_UNCI_MAX_COMPONENTS components, a component set
 * that is neither mono [+ alpha], Y Cb Cr [+ alpha] nor R G B [+ alpha] (padded components aside).
 * HM_ERR_BITSTREAM: no uncC / cmpd / ispe, a component index outside cmpd, a size that overflows.
 * Through hm_decode_item and its device forms (not the pipeline, batch and sequence calls; not as a grid tile, a derived item's child,
 * an auxiliary image or a gain map: HM_ERR_UNSUPPORTED) such an item is a leaf without coded pictures:
 *   Y Cb Cr / monochrome items of 8..12 bits are ordinary images of their chroma format and depth - transformations, every HM_OUT_*
 *   chain, ext_dst, device tensors, planes, views and the light / tone / OOTF / alpha steps; an item without a 'colr' nclx converts with
 *   the defaults of an image that carries none.  Other depths are handed out as coded only (out_format 0), any conversion is
 *   HM_ERR_UNSUPPORTED.  Y, Cb and Cr of different depths: HM_ERR_UNSUPPORTED.
 *   R G B items: out_format 0 hands out R, G, B in plane[0..2] and A in alpha, each at its own depth (hm_decoded.bit_depth: the largest;
 *   chroma: HM_CHROMA_444); HM_OUT_YCBCR_* is refused.  R, G, B (and A, for a four-channel target) all 8 bits deep: HM_OUT_RGB / _RGBA;
 *   all 16: HM_OUT_RRGGBB_LE / _RRGGBBAA_LE; opaque alpha where the item has none.  Any other combination: HM_ERR_UNSUPPORTED with
 *   HM_DETAIL_NO_COLOUR_CHAIN.
 *   An alpha component is the image's alpha plane; an alpha auxiliary image attached to the item is HM_ERR_UNSUPPORTED.
 *   hm_plan_view / hm_plan_planes_view answer with the sub-grid of INTERNAL tiles a crop touches; only their bytes are uploaded.
 *   A payload shorter than the layout needs: HM_ERR_BITSTREAM, before anything is queued. */
enum { HM_UNCI_MONO = 0, HM_UNCI_YCBCR = 1, HM_UNCI_RGB = 2 };
enum { HM_UNCI_MAX_COMPONENTS = 8 };
/* component types of ISO/IEC 23001-17 table 1 */
enum { HM_UNCI_TYPE_MONO = 0, HM_UNCI_TYPE_Y = 1, HM_UNCI_TYPE_CB = 2, HM_UNCI_TYPE_CR = 3, HM_UNCI_TYPE_R = 4, HM_UNCI_TYPE_G = 5,
       HM_UNCI_TYPE_B = 6, HM_UNCI_TYPE_ALPHA = 7, HM_UNCI_TYPE_PADDED = 12 };
enum { HM_UNCI_INTERLEAVE_COMPONENT = 0, HM_UNCI_INTERLEAVE_PIXEL = 1, HM_UNCI_INTERLEAVE_MIXED = 2, HM_UNCI_INTERLEAVE_ROW = 3,
       HM_UNCI_INTERLEAVE_TILE_COMPONENT = 4 };
enum { HM_UNCI_SAMPLING_NONE = 0, HM_UNCI_SAMPLING_422 = 1, HM_UNCI_SAMPLING_420 = 2 };
typedef struct hm_unci_component {
  uint16_t type;         /* HM_UNCI_TYPE_* */
  uint8_t  depth;        /* 1..16 */
  uint8_t  align_size;   /* bytes, 0 = packed */
} hm_unci_component;
typedef struct hm_unci_info {
  int32_t  width, height;        /* 'ispe': tile_width * tile_cols, tile_height * tile_rows */
  int32_t  colour_space;         /* HM_UNCI_MONO / _YCBCR / _RGB */
  int32_t  n_components;
  hm_unci_component comp[HM_UNCI_MAX_COMPONENTS]; /* in the order of the uncC box: the order of the data */
  int32_t  sampling, interleave; /* HM_UNCI_SAMPLING_*, HM_UNCI_INTERLEAVE_* */
  uint32_t pixel_size, row_align, tile_align;
  uint32_t tile_cols, tile_rows, tile_width, tile_height;
  uint64_t payload_bytes;        /* the byte length the layout needs */
} hm_unci_info;
HM_API int hm_file_unci_info(const hm_file* f, uint32_t id, hm_unci_info* info);
/* The closed form of the layout, on the host: the position, in bits from the start of the payload, of the most significant bit of
 * sample (x, y) of component `component` (x, y in that component's own plane: chroma planes are sub-sampled).  HM_ERR_INVALID_ARG for
 * a component or a coordinate outside the item; info->payload_bytes is not looked at. */
HM_API int hm_unci_sample_bit(const hm_unci_info* info, int component, int x, int y, uint64_t* bit);
/* info->payload_bytes from the other fields (what hm_file_unci_info stores there), or the refusal of a layout */
HM_API int hm_unci_payload_bytes(const hm_unci_info* info, uint64_t* bytes);
/* The unpack on its own: the item's payload in device memory (d_bytes, 4-byte aligned, n_bytes long) to planes and / or interleaved
 * pixels, ONE launch, asynchronous on `stream`.
 *   tiles: NULL, or first tile row, row count, first tile column, column count of a sub-grid of the internal tiles: d_bytes then holds
 *   only that sub-grid's byte ranges laid end to end in the order of the layout (modes 0..3: its tiles row by row; mode 4: per
 *   component, its tiles row by row), and the output has the sub-grid's size.
 *   out (may be NULL): the mapped components at their own depth - bytes up to 8 bits, little-endian 16-bit words above -, plane[0..2] =
 *   Y Cb Cr / R G B / Y (mono), plane[3] = alpha (not written when NULL or when the item has none).  Strides are multiples of 4 and
 *   pointers 4-byte aligned: rows are written in whole dwords, up to 3 bytes of row padding behind the last sample are zeroed.
 *   interleaved (may be NULL) with out_format: HM_OUT_RGB / _RGBA of an RGB item whose R, G, B (and A) are all 8 bits deep,
 *   HM_OUT_RRGGBB_LE / _RRGGBBAA_LE where they are all 16; HWC with HM_DEV_U8 / HM_DEV_U16 only.  An item without an alpha component
 *   gets opaque alpha.  Only width x height pixels are written.  Anything else: HM_ERR_UNSUPPORTED with HM_DETAIL_NO_COLOUR_CHAIN.
 * n_bytes below what the layout needs: HM_ERR_BITSTREAM, before the launch; nothing behind d_bytes + n_bytes is ever read. */
HM_API int hm_unci_unpack(const hm_unci_info* info, const void* d_bytes, size_t n_bytes, const int32_t tiles[4], const hm_planes* out,
                          int out_format, const hm_device_dest* interleaved, void* stream);

/* ------------------------------------------------------------------------- */
/* Regions and masks: 'rgan' region items and 'mski' mask items (ISO/IEC 23008-12 6.10) */
/* ------------------------------------------------------------------------- */

/* What a file says ABOUT its pixels.  A region item ('rgan') annotates the images its 'cdsc' reference names with up to 255 regions
 * on a canvas of reference_width x reference_height; a mask item ('mski' with an 'mskC' property: HM_ITEM_MSKI) is a monochrome image.
 * File layer (libheif/region.cc, codecs/mask_image.cc, context.cc:1166-1237): the payload of an 'rgan' item is a version byte (not
 * looked at), a flags byte (bit 0: 32-bit fields, else 16-bit), reference width and height, a one-byte region count and per region a
 * type byte and its fields - x, y and point coordinates signed, sizes, radii and point counts unsigned.  The k-th referenced-mask
 * region of an item takes the k-th entry of the item's 'mask' reference; its width or height 0 means the mask item's 'ispe'.
 * A damaged region item does not fail hm_file_open: the calls below that read that item fail.
 *   HM_ERR_BITSTREAM    truncated data (an inline mask holds (w * h + 7) / 8 bytes), fewer 'mask' references than referenced-mask regions
 *   HM_ERR_UNSUPPORTED  a geometry type above 6 (named), an inline mask with mask_coding_method != 0 (deflate), a 'mask' reference to
 *                       an item that is not HM_ITEM_MSKI, a referenced-mask region whose stated size differs from the mask item's
 *                       'ispe' (no mask is scaled), a mask item that is not 8 bits deep, and the magnitude limits, named in the message:
 *                       every coordinate v  -2^28 <= v < 2^28, every size and reference dimension < 2^28, an ellipse radius <= 32767
 *                       (with them the membership tests below are exact in 64-bit integers).
 * An HM_ITEM_MSKI item is listed by hm_file_top_level_images unless it is hidden or the target of a 'mask' reference.  Through
 * hm_decode_item and its device forms an 8-bit mask item is a monochrome 8-bit image whose samples are the payload's bytes, row after
 * row, tight - a leaf without coded pictures that takes the path of a monochrome 8-bit 'unci' item in component interleave and is
 * refused where such an item is (the pipeline, batch and sequence calls; as a grid tile, a derived item's child, an auxiliary image,
 * a gain map).  A payload below width * height bytes: HM_ERR_BITSTREAM before anything is queued.  bits_per_pixel other than 8:
 * HM_ERR_UNSUPPORTED.
 *
 * THE MEMBERSHIP RULES.  The canvas is reference_width x reference_height; pixel (px, py) is the lattice point (px, py).  The reference
 * space is that of the annotated image AFTER its transformative properties: no irot / imir / clap is applied to a region.  A region's
 * value at a pixel is 0 or 255; for a referenced mask it is the mask's sample, 0 .. 255.  All arithmetic is int64.
 *   Point           the pixel (x, y).
 *   Rectangle       x <= px < x + w  and  y <= py < y + h.
 *   Ellipse         centre (x, y), radii rx = w, ry = h:  |px - x| <= rx  and  |py - y| <= ry  and
 *                   (px - x)^2 * ry^2 + (py - y)^2 * rx^2 <= rx^2 * ry^2.  A zero radius gives a line or the centre pixel.
 *   Segment A -> B  dx = bx - ax, dy = by - ay, m = max(|dx|, |dy|): P is on it iff P is inside the segment's closed bounding box and
 *                   2 * |dx * (py - ay) - dy * (px - ax)| <= m.  m = 0: P = A.
 *   Polyline        the union of its n - 1 segments; n = 1: the point; n = 0: empty.
 *   Polygon         the union of (a) the closed polyline - n segments, the last vertex joined to the first - and (b) the even-odd
 *                   interior: an edge counts for P iff (ay <= py) != (by <= py) and, with its ends ordered so that ay < by,
 *                   (px - ax) * (by - ay) < (bx - ax) * (py - ay); P is interior iff the count is odd.
 *   Inline mask     at (x, y), size w x h: bit i = (py - y) * w + (px - x) of the data, most significant bit first, rows not byte
 *                   aligned; a set bit gives 255 (heif_regions.cc:677-690).
 *   Referenced mask at (x, y): the mask item's sample at (px - x, py - y).
 * Everything is clipped to the canvas; geometry off the canvas is legal.
 * Two outputs over the view's rectangle of the canvas:
 *   HM_REGIONS_STACK   one plane per region, in the order given.  HM_DEV_U8 stores the value, HM_DEV_F32 / _F16
 *                      __fadd_rn(__fmul_rn((float)v, scale), bias), HM_DEV_F16 through __float2half_rn - the tensor step's rule.
 *   HM_REGIONS_LABELS  ONE uint8 plane: 1 + the index of the LAST region whose value there is >= 128, or 0.  At most 255 regions
 *                      (more: HM_ERR_INVALID_ARG); HM_DEV_U8 only.
 * The view (hm_device_view): the crop is a rectangle of the canvas - pixels outside it are never generated -; an output size that
 * differs from the crop's resamples STACK planes as monochrome 8-bit planes under the rules of "Planar views" above (integer
 * destinations round and clamp, float ones take r * scale + bias); LABELS takes HM_VIEW_NEAREST's index rule only - averaged labels
 * mean nothing: any other filter with a size other than the crop's is HM_ERR_INVALID_ARG.
 * Only width x height elements of each plane are written.  Every refusal - a destination that is not device memory, too short, of a
 * pitch below the tight value or not a multiple of the element size, an unknown dtype or mode, a bad view, a region beyond the
 * magnitude limits, a NULL data pointer, an inline mask of fewer than (w * h + 7) / 8 bytes, a mask of fewer than w * h - happens
 * before anything is queued, with the destination unwritten. */
enum { HM_REGION_POINT = 0, HM_REGION_RECTANGLE = 1, HM_REGION_ELLIPSE = 2, HM_REGION_POLYGON = 3, HM_REGION_REFERENCED_MASK = 4,
       HM_REGION_INLINE_MASK = 5, HM_REGION_POLYLINE = 6 };
enum { HM_REGIONS_STACK = 0, HM_REGIONS_LABELS = 1 };
enum { HM_REGION_COORD_LIMIT = 1 << 28, HM_REGION_MAX_RADIUS = 32767 };
typedef struct hm_region_item_info {
  uint32_t reference_width, reference_height;
  int32_t  n_regions;
  int32_t  field_bits;       /* 16 / 32: the field size the payload uses */
} hm_region_item_info;
typedef struct hm_region {
  int32_t  type;             /* HM_REGION_* */
  int32_t  x, y;             /* point; top-left corner (rectangle, masks); centre (ellipse); 0 for polygon / polyline */
  uint32_t w, h;             /* size (rectangle, masks: resolved against the mask item's 'ispe'); radii (ellipse) */
  uint32_t n_points;         /* polygon / polyline */
  uint32_t mask_item;        /* referenced mask: the HM_ITEM_MSKI item, else 0 */
  uint64_t mask_bytes;       /* inline mask: (w * h + 7) / 8; referenced mask: w * h; else 0 */
} hm_region;
/* the region items whose 'cdsc' reference names `image_id`, in item-ID order: returns their count, ids[0 .. min(count, max_ids)) filled */
HM_API int hm_file_region_items(const hm_file* f, uint32_t image_id, uint32_t* ids, int max_ids);
HM_API int hm_file_region_item_info(const hm_file* f, uint32_t region_item, hm_region_item_info* info);
HM_API int hm_file_region(const hm_file* f, uint32_t region_item, int index, hm_region* out);
/* xy[2 i], xy[2 i + 1] of point i < min(n_points, max_points); returns n_points or a negative status */
HM_API int hm_file_region_points(const hm_file* f, uint32_t region_item, int index, int32_t* xy, int max_points);
/* the bit string of an inline mask (points into the file object, valid until hm_file_close) */
HM_API int hm_file_region_inline_mask(const hm_file* f, uint32_t region_item, int index, const uint8_t** bits, size_t* len);

typedef struct hm_regions_dest {
  void*    ptr;          /* device memory of the current device                                         */
  uint64_t len;          /* bytes available at ptr                                                      */
  int32_t  dtype;        /* HM_DEV_U8 / _F16 / _F32 (STACK); HM_DEV_U8 (LABELS)                         */
  int32_t  reserved;     /* 0 */
  int64_t  row_pitch;    /* bytes between rows; 0 = tight                                               */
  int64_t  plane_pitch;  /* STACK: bytes between region planes; 0 = row_pitch * height                  */
  float    scale, bias;  /* float dtypes: out = value * scale + bias                                     */
} hm_regions_dest;
/* bytes the destination must hold for n_regions planes (LABELS: one) of width x height: plane_pitch * (planes - 1) + row_pitch *
 * (height - 1) + width * elem, or the negative status of a combination that is refused.  Host arithmetic; ptr and len are not looked at. */
HM_API int64_t hm_regions_dest_bytes(int mode, int n_regions, int width, int height, const hm_regions_dest* d);
/* The rasteriser on its own (the sibling of hm_unci_unpack): n host-side descriptors - for region i, data[i] = its int32 x, y point
 * pairs (polygon / polyline), its bit string (inline mask, mask_bytes long) or its samples (referenced mask: w * h bytes, rows tight;
 * mask_item is not looked at), else ignored - on a canvas_w x canvas_h canvas under `view` (NULL: the whole canvas) into `dest`, sized
 * for the view's output.  Everything travels in one upload; ONE launch rasterises every region.  The host data is copied before the
 * call returns.  Asynchronous on `stream`. */
HM_API int hm_rasterise_regions(const hm_region* regions, const void* const* data, int n, int canvas_w, int canvas_h, const hm_device_view* view,
                                int mode, const hm_regions_dest* dest, void* stream);
typedef struct hm_regions_out {
  int32_t width, height;     /* of each plane written */
  int32_t n_regions;
  int32_t planes;            /* n_regions (STACK) or 1 (LABELS) */
  int64_t bytes;             /* hm_regions_dest_bytes of what was written */
  uint32_t reference_width, reference_height;
} hm_regions_out;
/* The regions of the region items region_items[0 .. n), item after item, gathered from the file - the items must share one reference
 * size, else HM_ERR_UNSUPPORTED; referenced masks are the 'mski' payloads' own bytes - and rasterised as by hm_rasterise_regions on the
 * default stream; returns when the planes are in place. */
HM_API int hm_regions_to_device(const hm_file* f, const uint32_t* region_items, int n, const hm_device_view* view, int mode,
                                const hm_regions_dest* dest, hm_regions_out* out);

#ifdef __cplusplus
}
#endif
#endif /* HEIF_MI355X_H */
