// hm_devdest.h — internal: a caller's device destination (hm_device_dest, include/heif_mi355x.h) resolved for one image.
// devdest.cpp holds the host arithmetic and the checks (no device needed except hm_dest_check_pointer), tensor.hip the kernel.
#ifndef HM_DEVDEST_H
#define HM_DEVDEST_H

#include "hm_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hm_dest_plan {
  int32_t layout, dtype;
  int32_t channels;      // 3 / 4
  int32_t sample_bytes;  // of the out_format: 1 / 2
  int32_t elem;          // bytes per element of the destination
  int32_t raw;           // HWC with the target's own integer type: the bytes as they are (a 2-D device copy, no kernel)
  int64_t row_pitch, plane_pitch, tight_row, bytes;
} hm_dest_plan;

// what does not depend on the image size: the target, layout / dtype combination, alignment of ptr and pitches
int hm_dest_check_static(int out_format, const hm_device_dest* d);
// ... and what does: pitches against the tight values, the byte count (d->len is NOT compared: hm_dest_check_len)
int hm_dest_resolve(int out_format, int w, int h, const hm_device_dest* d, hm_dest_plan* p);
int hm_dest_check_len(const hm_device_dest* d, const hm_dest_plan* p);
// d->ptr is device memory of the current device
int hm_dest_check_pointer(const hm_device_dest* d);
// rows [y0, y0 + rows) of a w x h image from `src` (row 0 of src = image row y0) into the destination; asynchronous on `s`.
// The destination has been checked against w x h.
int hm_dest_write(const hm_device_dest* d, int out_format, int w, int h, int y0, int rows, const void* src, int src_stride, hipStream_t s);

int hm_launch_to_tensor(const hm_dest_plan* p, const void* src, int src_stride, int w, int rows, void* dst, const float scale[4], const float bias[4],
                        hipStream_t s);

// ---- planar YCbCr (hm_device_planes): the decoded planes themselves, one destination per plane.  devdest.cpp holds the checks,
//      planes.hip the kernel ----
typedef struct hm_planes_plan {
  int32_t layout, dtype, elem;
  int32_t chroma, bits, alpha_bits; // of the result; alpha_bits 0: no alpha plane is written
  int32_t shift;                    // msb_aligned: 16 - bits (the alpha plane: 16 - alpha_bits), else 0
  struct {
    int32_t present;                // written: Y always, Cb / Cr (SEMI: CbCr in [1]) unless 4:0:0, alpha when it exists and plane[3].ptr is given
    int32_t width, height;          // samples of the source plane(s)
    int32_t elems;                  // elements of a destination row: width, the interleaved plane 2 * width
    int32_t vec;                    // ptr and pitch take 16-byte stores
    int64_t pitch, tight, bytes;    // bytes: the pitch in use, of a row's elements, pitch * (height - 1) + tight
  } pl[4];
  int64_t bytes;                    // the sum over the planes that are present
} hm_planes_plan;
// what depends on nothing but the destination: layout, dtype, reserved, msb_aligned, alignment of the pointers and pitches
int hm_planes_check_static(const hm_device_planes* d);
// ... and what depends on the result's format: chroma (HM_CHROMA_*), bits, luma size, alpha_bits (0: the image has no alpha plane,
// < 0: not known yet - the plane is sized when plane[3].ptr is given, its depth class is not judged).  d->plane[].len is NOT compared.
int hm_planes_resolve(int chroma, int bits, int w, int h, int alpha_bits, const hm_device_planes* d, hm_planes_plan* p);
// null pointers, len against the plan, and planes whose byte ranges overlap
int hm_planes_check_len(const hm_device_planes* d, const hm_planes_plan* p);
// every plane that is written is device memory of the current device
int hm_planes_check_pointer(const hm_device_planes* d, const hm_planes_plan* p);
// the planes src[0 .. 2] (Y, Cb, Cr) and src[3] (alpha, with alpha_bits > 0) of a w x h image, strides in bytes, samples of 1 byte (8 bits) or
// 2, into the destination: ONE launch of k_planes_to_tensor, asynchronous on `s`.  Everything - resolve, len and overlap, the pointers -
// is checked again before the launch.
// pitches (may be NULL): the pitches in use.
int hm_planes_write(const hm_device_planes* d, int chroma, int bits, int w, int h, int alpha_bits, const void* const src[4], const int32_t stride[4],
                    hipStream_t s, int64_t pitches[4]);

// one plane of a launch; pair: the interleaved CbCr plane (src0 = Cb, src1 = Cr, scale0 / bias0 and scale1 / bias1 theirs)
typedef struct hm_plane_desc {
  const uint8_t* src0; const uint8_t* src1;
  uint8_t* dst;
  long long pitch;
  int32_t stride0, stride1;
  int32_t w, h;            // samples of a source row, rows (0: the plane is absent)
  int32_t sample_bytes, pair, vec, shift;
  float scale0, bias0, scale1, bias1;
} hm_plane_desc;
typedef struct hm_planes_args {
  hm_plane_desc pl[4];
  int32_t y_end[4];        // blockIdx.y below y_end[p] (and not below y_end[p - 1]) works on plane p: running sums of (h + 3) / 4
} hm_planes_args;
int hm_launch_planes_to_tensor(const hm_planes_args* a, int dtype, hipStream_t s);

// ---- views (hm_device_view): a rectangle of the image at a size of the caller's choice.  devdest.cpp holds the checks and the tap
//      tables, resample.hip the kernels ----
typedef struct hm_view_plan {
  int32_t x, y, w, h;    // the crop, inside the source
  int32_t ow, oh;        // the size written
  int32_t filter;
  int32_t crop_only;     // out_w == out_h == 0: the bytes of the rectangle
} hm_view_plan;
// device / pinned blocks a view write works on; they must live until the stream has passed the write (hm_view_scratch_free)
typedef struct hm_view_scratch { void* dev[2]; void* pinned; } hm_view_scratch;
void hm_view_scratch_free(hm_view_scratch* sc);
// a stand-alone entry that returns before its kernels have run: the blocks of sc[0 .. n) go back to the pools once stream `s` has passed
// this point (a later stand-alone call releases them); the entries are emptied
void hm_view_scratch_retire(hipStream_t s, hm_view_scratch* sc, int n);
// the view against a src_w x src_h image and the target: every refusal of the view itself
int hm_view_resolve(int out_format, int src_w, int src_h, const hm_device_view* v, hm_view_plan* vp);
// one frame of a batched view write: the destination, the view resolved against the frame, the frame's interleaved pixels (row 0 = image row 0)
typedef struct hm_view_item { const hm_device_dest* dest; hm_view_plan vp; const void* src; int32_t src_stride; } hm_view_item;
// The view of n frames (a sequence under one view) into their destinations.  Frames that agree in crop, output size, filter, sample format,
// source stride, the destination's layout, dtype, pitches, scale, bias and 16-byte alignment form a group: one pair of tap tables,
// one upload (tables + the frames' pointers), one bounded intermediate, and per chunk of frames one launch per pass
// (hm_view_batch.h holds the arithmetic).  The crop alone and HM_VIEW_NEAREST stay calls of hm_out_write per frame, and so does
// everything with knob view_batch = 0.  Every destination is checked before anything is queued.  sc: n zeroed entries.
int hm_view_write_batch(int out_format, const hm_view_item* items, int n, hipStream_t s, hm_view_scratch* sc);

// one axis' taps as the kernels read them: first[m], count[m], weights[taps][m] (tap-major: consecutive outputs are neighbours)
typedef struct hm_view_axis { const int32_t* first; const int32_t* count; const float* weights; int32_t m, taps; } hm_view_axis;
typedef struct hm_resample_args {
  int32_t sample_bytes, channels;       // of the source
  const void* src; int32_t src_stride;  // at the crop's origin
  int32_t n_w, n_h, ow, oh;
  hm_view_axis ax, ay;                  // device pointers
  float* tmp; int64_t tmp_pitch, tmp_plane; // the horizontal pass' float32 rows (elements), laid out like the destination
  int32_t staged;                       // the horizontal pass stages its source run in LDS (k_resample_h_staged: HM_VIEW_CUBIC, HM_VIEW_LANCZOS3)
  int32_t stage_px;                     // > 0: at most that many pixels per staged chunk (knob view_stage_px: tests)
} hm_resample_args;
int hm_launch_resample(const hm_dest_plan* p, const hm_resample_args* a, void* dst, const float scale[4], const float bias[4], hipStream_t s);
// the frames of one chunk of a batched view write: device arrays of the frames' source origins and destinations
typedef struct hm_resample_batch {
  const void* const* srcs; void* const* dsts;
  int32_t frames;
  int32_t vec;            // every destination takes 16-byte stores
  int64_t frame_stride;   // elements of the intermediate per frame
} hm_resample_batch;
int hm_launch_resample_batch(const hm_dest_plan* p, const hm_resample_args* a, const hm_resample_batch* b, const float scale[4], const float bias[4], hipStream_t s);
// the views of one chunk of a multi-view write (hm_views_write; hm_view_multi.h holds the arithmetic): device pointers into the group's block
typedef struct hm_resample_multi {
  const void* block;                    // the group's block: every tap-table offset of a record counts 32-bit words from here
  const void* recs;                     // hm_view_rec[views]: the chunk's first record
  const int32_t* hsums; const int32_t* vsums; // the chunk's running sums of row groups, horizontal and vertical pass
  int32_t views;
  int32_t sample_bytes, channels, src_stride; // of the one source picture
  int32_t staged, stage_px;             // as hm_resample_args
  int32_t vec;                          // every destination of the group takes 16-byte stores
  int32_t h_groups, v_groups;           // the chunk's last sums: gridDim.y of the passes
  int32_t ow_most, E_most;              // of the chunk's widest view: gridDim.x
  float* tmp;                           // the chunk's intermediate
} hm_resample_multi;
int hm_launch_resample_multi(const hm_dest_plan* p, const hm_resample_multi* m, const float scale[4], const float bias[4], hipStream_t s);
int hm_launch_view_nearest(const hm_dest_plan* p, const void* src, int src_stride, int n_w, int n_h, int ow, int oh, void* dst, const float scale[4],
                           const float bias[4], hipStream_t s);

// ---- the light step (hm_device_light): code values to linear light through a table, a gamut matrix, linear floats or a search in a
//      threshold table.  devdest.cpp holds the tables, the matrix, the checks and the write step, light.hip the kernels ----
enum { HM_LIGHT_MAX_BITS = 12 }; // both tables of a pointwise kernel sit in LDS: 2 x 16 KB
typedef struct hm_light_plan {
  int32_t from_transfer, from_primaries, to_transfer, to_primaries; // H.273 codes, nothing left at 0
  int32_t bits;          // of the target's samples
  int32_t encode;        // to_transfer != HM_LIGHT_LINEAR
  int32_t matrix;        // to_primaries differs from from_primaries
  float gain;
  float m[9];
  // the tone step (hm_device_tone) beside it, resolved: nothing left at 0
  int32_t tone;          // a tone step runs
  int32_t enc_bits;      // of the codes the finish stores: bits, or 8 under the 8-bit finish
  float src_peak, dst_peak, unit_nits, out_unit_nits;
  // the OOTF step (hm_device_ootf) beside it, resolved
  int32_t ootf;          // an OOTF step runs
  float ootf_peak, ootf_gamma; // display_peak and gamma of the request (gamma 0: the system gamma of the peak): what the tables are built from
  float y[3];            // the luminance weights of from_primaries
  // the source is an ICC profile (HM_LIGHT_FROM_ICC, no known cicp tag in it): from_transfer and from_primaries stay HM_LIGHT_FROM_ICC,
  // lin comes from the profile's curves, m from its colorants (hm_icc.h).  The bytes are the request's (hm_out_steps): they outlive the write.
  int32_t icc;
  int32_t lin3;          // the three curves give distinct tables at `bits`: three are uploaded, red, green, blue
  const uint8_t* icc_data; size_t icc_size;
} hm_light_plan;
// (the step's refusals: hm_out_check_static; its plan: hm_out_resolve)
// ---- the tone step (hm_device_tone) inside the light step: two tables of HM_TONE_STEPS entries, built in devdest.cpp ----
// the peak rule of include/heif_mi355x.h on an item's raw properties
float hm_tone_peak_of(int has_clli, unsigned max_cll, int has_mdcv, unsigned mdcv_max);

// what the kernels get: device pointers of lin[1 << bits] (lin3: three of them, one behind the other), (encode) enc[1 << enc_bits], (tone) thr[HM_TONE_STEPS] with sg[HM_TONE_STEPS]
// behind it and (ootf) thr[HM_OOTF_STEPS] with sg[HM_OOTF_STEPS] behind it, y the step's luminance weights; src_bytes: bytes of a source
// sample (the plan's sample_bytes are the destination's sibling target's)
typedef struct hm_light_args {
  const float* lin; const float* enc; const float* tone; int32_t bits, enc_bits, src_bytes, encode, matrix; float m[9];
  const float* ootf; float y[3];
  int32_t lin3;          // lin is three tables of 1 << bits entries - red, green, blue: an ICC profile with distinct curves -, not one
} hm_light_args;
// The one host check of a launch's dynamic LDS (light_step.h: check_light_lds) for the plan, which asks before anything is queued.
// tone: bit 0 a tone step, bit 1 an OOTF step; pass 0: a pointwise or nearest kernel, 1: a horizontal pass, 2: a vertical pass
int hm_light_lds_check(int bits, int enc_bits, int encode, int tone, int lin3, int pass);
int hm_launch_light_tensor(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int w, int rows, void* dst, const float scale[4],
                           const float bias[4], hipStream_t s);
int hm_launch_light_nearest(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int n_w, int n_h, int ow, int oh, void* dst,
                            const float scale[4], const float bias[4], hipStream_t s);
int hm_launch_light_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, void* dst, const float scale[4], const float bias[4],
                             hipStream_t s);

// ---- the alpha step (hm_device_alpha): premultiplied sums, a straight / premultiplied / matte result, alone or beside the light and
//      tone steps.  devdest.cpp holds the checks and the write step, alpha.hip the kernels ----
typedef struct hm_alpha_plan {
  int32_t mode;          // HM_ALPHA_*
  int32_t bits;          // of the target's samples: P = (1 << bits) - 1
  uint16_t background[3];
} hm_alpha_plan;
// what the kernels get beside hm_light_args (la NULL: no light step): bytes of a source sample, P, and the background as the floats b_c
typedef struct hm_alpha_args { int32_t mode, bits, src_bytes; float P; float bg[3]; } hm_alpha_args;
int hm_launch_alpha_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const void* src, int src_stride, int w, int rows, void* dst,
                           const float scale[4], const float bias[4], hipStream_t s);
int hm_launch_alpha_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const void* src, int src_stride, int n_w, int n_h, int ow, int oh,
                            void* dst, const float scale[4], const float bias[4], hipStream_t s);
// r: of a FOUR-channel intermediate (the sums of p_R, p_G, p_B and a), whatever the destination's channel count
int hm_launch_alpha_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const hm_resample_args* r, void* dst, const float scale[4],
                             const float bias[4], hipStream_t s);

// ---- the gain step (hm_device_gain) beside the light step: a gain map's samples through a table, summed under the map's own taps,
//      times the base's linear light.  devdest.cpp holds the tables, the geometry, the checks and the write step, gain.hip the kernels ----
enum { HM_GAIN_MAX_BITS = 12 };
typedef struct hm_gain_plan {
  int32_t active;        // wgt != 0: the map is read.  0: the write is the one without the step
  int32_t nch;           // 1: one table and one M for the three colour channels; 3: one each
  int32_t map_w, map_h, map_bits;
  int32_t sx, sy;        // the geometry's factors
  int32_t mx, my, mw, mh; // the map's crop
  int32_t filter;        // of the map's taps: HM_VIEW_TRIANGLE, or HM_VIEW_NEAREST under a nearest view
  float headroom;
  float kb[3], ka[3];
  hm_gain_params params;
} hm_gain_plan;
// wgt of include/heif_mi355x.h; the parameters have passed hm_gain_check
double hm_gain_weight(const hm_gain_params* g, float headroom);
// the step's own refusals of headroom and parameters; bad: the status of a bad parameter (HM_ERR_INVALID_ARG, a 'tmap' payload's: HM_ERR_BITSTREAM)
int hm_gain_check(const hm_gain_params* g, float headroom, int bad);
// the geometry of include/heif_mi355x.h into gp (sx, sy, the map's crop, the filter of its taps): a W x H base under the resolved view
// vp, an MW x MH map of map_bits bits; every refusal of the geometry and of the map's depth
int hm_gain_geometry(int W, int H, int MW, int MH, int map_bits, const hm_view_plan* vp, hm_gain_plan* gp);
// one output index of a map axis in the pointwise path, where the map is enlarged (n <= m: at most two taps): 16 bytes, one load
typedef struct hm_gain_tap { int32_t first, count; float w0, w1; } hm_gain_tap; // (w1 = 0 where count is 1)
// The map as the kernels see it (device pointers).  Pointwise: xrec[ow] and yrec[oh], M formed in the kernel.  Nearest: the map's crop
// alone.  Summed: the taps of both map axes, mtmp[nch planes][mh rows] and M[nch planes][oh rows] of ow floats, rows of `pitch` elements.
typedef struct hm_gain_args {
  const float* tab;                       // nch tables of 1 << map_bits entries, one behind the other
  int32_t nch, map_bits, map_bytes;
  float kb[3], ka[3];
  const void* map; int32_t map_stride;    // at the map crop's origin
  int32_t mw, mh;                         // the map's crop
  hm_view_axis ax, ay;                    // the map's taps: mw -> ow, mh -> oh (summed; pointwise: m alone)
  const hm_gain_tap* xrec; const hm_gain_tap* yrec; // (pointwise) 16-byte aligned
  float* mtmp; float* M; int64_t pitch;   // (summed)
} hm_gain_args;
int hm_launch_gain_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const void* src, int src_stride, int w, int rows, void* dst,
                          const float scale[4], const float bias[4], hipStream_t s);
int hm_launch_gain_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const void* src, int src_stride, int n_w, int n_h, int ow, int oh,
                           void* dst, const float scale[4], const float bias[4], hipStream_t s);
// the map's two passes into M, the base's horizontal pass (hm_launch_light_h: k_light_h), then the vertical pass that applies the update
int hm_launch_gain_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const hm_resample_args* r, void* dst, const float scale[4],
                            const float bias[4], hipStream_t s);
// k_light_h alone: the horizontal pass of hm_launch_light_resample (light.hip)
int hm_launch_light_h(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, hipStream_t s);

// ---- the device write: the interleaved pixels of one image through the steps of a request - view, light (with tone and the OOTF
//      inside it), alpha, gain - into a hm_device_dest.  One request (hm_out_steps), one plan (hm_out_plan), one writer (hm_out_write); a further step is
//      a case inside them ----
typedef struct hm_out_steps {
  const hm_device_view* view; const hm_device_light* light; const hm_device_tone* tone; const hm_device_alpha* alpha; const hm_device_gain* gain;
  const hm_device_ootf* ootf;
  // the profile a light step with HM_LIGHT_FROM_ICC reads: the item's (resolve_request), hm_icc_to_tensor's; it must live until the
  // write has been queued.  NULL: the request has none - the sentinel is refused
  const uint8_t* icc; size_t icc_size;
  // the light statistics (HM_MEASURE_*): STATS - the request is measured, not written: its destination is a stand-in that sizes
  // nothing real, its pointer is not looked at; TONE - the tone step's src_peak is a stand-in until the measurement replaces it
  int32_t measure;
} hm_out_steps; // any may be NULL
enum { HM_MEASURE_NONE = 0, HM_MEASURE_STATS = 1, HM_MEASURE_TONE = 2 };
// what the image reports (hm_decoded); with a gain step the map beside it (map_w 0: not known yet - the step's geometry is not judged)
typedef struct hm_out_image { int32_t w, h, bits, transfer, primaries; int32_t map_w, map_h, map_bits; } hm_out_image;
// the gain map's samples on the device (one channel; one byte per sample at 8 bits, else two), row 0 = the map's row 0
typedef struct hm_out_map { const void* plane; int32_t stride; } hm_out_map;
typedef struct hm_out_plan {
  int32_t out_format, dest_format; // the source's target; the target the destination is judged, sized and written as
  int32_t w, h;                    // the source image
  int32_t has_view, has_light, has_alpha, has_gain;
  hm_view_plan vp;                 // without a view: the whole image as a crop alone (ow = w, oh = h)
  hm_light_plan lp; hm_alpha_plan ap;
  hm_gain_plan gp;                 // has_gain and a known profile: the tables' weight; and a known map: the geometry
  hm_dest_plan dp;                 // against dest_format at vp.ow x vp.oh; d->len has been compared
} hm_out_plan;
// the target the destination is judged by: hm_alpha_dest_format with an alpha step (negative: the step's own refusals), else with
// tone->out_bits == 8 the 8-bit sibling of a 16-bit three-channel target, else out_format
int hm_out_dest_format(int out_format, const hm_out_steps* st);
// what depends on the request alone: the alpha step's own refusals, then the gain, OOTF and tone steps', the light step's (from_* == 0:
// allowed unless `explicit_from`, which wants src_peak and unit_nits given too - beside an OOTF step both may stay 0: display_peak) and
// the destination's, each against hm_out_dest_format
int hm_out_check_static(int out_format, const hm_device_dest* d, const hm_out_steps* st, int explicit_from);
// ... and what depends on the image.  The size: the view, the destination against the size written, its len.  The profile
// (know_profile != 0): hm_out_check_static again, the depth, the alpha step's background against the peak, the light step's from_* == 0
// as img->transfer / img->primaries, the tone step's units - behind the size (HM_OUT_PROFILE_LAST: the decode entries), or between the
// view and the destination (HM_OUT_PROFILE_FIRST: the order of the stand-alone entries).  know_profile 0: p->lp and p->ap stay empty.
enum { HM_OUT_PROFILE_LAST = 1, HM_OUT_PROFILE_FIRST = 2 };
int hm_out_resolve(int out_format, const hm_out_image* img, int know_profile, const hm_device_dest* d, const hm_out_steps* st, hm_out_plan* p);
// the image at `src` (interleaved pixels of p->out_format, row 0 = image row 0) through the plan into the destination; asynchronous on
// `s`.  Tables and the intermediate hang on sc, which must be a free entry (it is not looked at where nothing is uploaded).
// map: the gain map of an active gain step (p->gp.active), else NULL.
int hm_out_write(const hm_device_dest* d, const hm_out_plan* p, const void* src, int src_stride, const hm_out_map* map, hipStream_t s, hm_view_scratch* sc);

// ---- many views of one picture: n plans against the same image, n destinations ----
// two destinations whose byte ranges overlap (plans[k].dp.bytes from dests[k].ptr: hm_dest_resolve's count, the pitches as resolved): the refusal names both
int hm_dests_check_overlap(const hm_device_dest* dests, const hm_out_plan* plans, int n);
// The views plans[0 .. n) of the image at `src` into dests[0 .. n); asynchronous on `s`.  One statement of the rule:
//   - views whose plan has no step (plain code values) and whose filter is a resampling one are grouped by hm_view_multi_key - staged
//     horizontal pass or not, sample_bytes, channels, layout, dtype, the 16-byte store instance, scale, bias - and a group goes to the
//     multi kernels: one pinned block and one upload (every distinct tap table once, the views' records, the running sums), one
//     bounded intermediate, and per chunk of views one launch per pass (hm_view_multi.h holds the arithmetic);
//   - the crop alone and HM_VIEW_NEAREST stay one hm_out_write each, as hm_view_write_batch keeps them;
//   - every view of a request with a light / tone / OOTF / alpha step stays one hm_out_write each too, from the one picture (fusing the
//     stepped passes is a follow-up);
//   - knob view_multi = 0: hm_out_write per view for everything.
// The plans have been resolved and the destinations checked (overlap included) by the caller.  sc: n zeroed entries.
int hm_views_write(const hm_device_dest* dests, const hm_out_plan* plans, int n, const void* src, int src_stride, hipStream_t s, hm_view_scratch* sc);

// ---- the light statistics (hm_light_stats): the plan's rectangle - the view's crop at source resolution - of the interleaved pixels
//      through the light step up to the tone step's search, counted.  devdest.cpp holds the tables and the host arithmetic, stats.hip the kernel ----
// the destination a statistics request is planned against (HM_MEASURE_STATS): float32 HWC of any size
hm_device_dest hm_stats_stand_in_dest(void);
// U of a statistic: unit_nits as given, or what 0 stands for under the plan (the tone step's rule: display_peak beside an OOTF step,
// 10000 for PQ), or the refusal
int hm_stats_unit_nits(const hm_light_plan* lp, float unit_nits, float* U);
// unit_nits itself: 0, or finite, above 0 and at most 10000
int hm_stats_check_unit(float unit_nits);
// fraction: finite and in (0, 1]
int hm_stats_check_fraction(double fraction);
// The statistic of p's rectangle of the image at `src` for U cd/m2 per unit, into *out: 2048 + 2 words of pool device memory zeroed on
// `s`, one launch, their copy to pool pinned memory - and the stream is waited for: the numbers are in *out when it returns.
int hm_launch_light_stats(const hm_out_plan* p, float U, const void* src, int src_stride, hipStream_t s, hm_light_stats* out);
int hm_launch_light_stats_kernel(const hm_light_args* la, int channels, const void* src, int src_stride, int w, int h, unsigned* out, hipStream_t s);

// ---- planar views: a view (hm_device_view) into planar YCbCr (hm_device_planes), every plane an image of its own.  devdest.cpp
//      holds the checks and the write step, hm_planes_view.h the index arithmetic, planes_view.hip the kernels ----
typedef struct hm_planes_view_plan {
  int32_t crop[4][4], out[4][2]; // per plane (0 Y, 1 Cb, 2 Cr, 3 alpha): the crop x, y, w, h inside that plane and the size written
  int32_t ow, oh;                // the luma size written: what the destination is checked against
  int32_t filter, crop_only;
} hm_planes_view_plan;
// the view against a w x h result of this chroma format: every refusal of the view itself (crop, origin, filter, reduction per plane and axis)
int hm_planes_view_resolve(int chroma, int w, int h, const hm_device_view* v, hm_planes_view_plan* pv);
// one frame of a planar view write: the source planes (row 0 = image row 0) of a result of (chroma, bits, alpha_bits), the view
// resolved against it, the destination; pitches: filled with the pitches in use
typedef struct hm_planes_view_item {
  const hm_device_planes* planes;
  hm_planes_view_plan pv;
  int32_t chroma, bits, alpha_bits;
  const void* src[4]; int32_t stride[4];
  int64_t pitches[4];
} hm_planes_view_item;
// n >= 1 frames.  Frames that agree in the key of hm_planes_view.h form a group: the tap tables of its at most four distinct axes and
// the frames' pointer records in ONE pinned block and one upload, one bounded float32 intermediate, and per chunk of frames one
// launch per pass.  The crop alone is hm_planes_write on offset source pointers, frame by frame.  Every destination and source is
// checked before anything is queued (*failed, may be NULL: the index of the frame that was refused).  sc: n zeroed entries.
int hm_planes_view_write(hm_planes_view_item* items, int n, hipStream_t s, hm_view_scratch* sc, int* failed);

// one axis' taps of one plane (device pointers): first[m], count[m], weights[taps][m]
typedef struct hm_pv_axis { const int32_t* first; const int32_t* count; const float* weights; } hm_pv_axis;
// a SOURCE plane of the horizontal pass
typedef struct hm_pv_src_desc {
  hm_pv_axis ax;
  long long tmp_off, tmp_pitch;  // its region of a frame's intermediate (elements)
  int32_t stride, n_h, ow;       // bytes between source rows, rows of the crop (0: the plane is absent), columns written
  int32_t sample_bytes;
} hm_pv_src_desc;
typedef struct hm_pv_h_args {
  hm_pv_src_desc pl[4];
  int32_t y_end[4];              // running sums of (n_h + 3) / 4
  const void* recs;              // hm_pv_rec[frames of the chunk]
  float* tmp; long long frame_stride;
} hm_pv_h_args;
// a DESTINATION plane of the vertical pass and of the nearest kernel; pair: the interleaved CbCr plane (0 = Cb, 1 = Cr)
typedef struct hm_pv_dst_desc {
  hm_pv_axis ay;
  long long pitch;               // bytes between destination rows
  long long tmp_off0, tmp_off1, tmp_pitch;
  int32_t w, oh;                 // elements (pairs) of a row, rows (0: the plane is absent)
  int32_t pair, vec, peak, shift;
  int32_t n_w, n_h, stride0, stride1, sample_bytes; // the nearest kernel: the source crop
  float scale0, bias0, scale1, bias1;
} hm_pv_dst_desc;
typedef struct hm_pv_v_args {
  hm_pv_dst_desc pl[4];
  int32_t y_end[4];              // running sums of (oh + 3) / 4
  const void* recs;
  const float* tmp; long long frame_stride;
} hm_pv_v_args;
// both passes over `frames` frames (grid z); sample_bytes: of the image's own planes (the template instance)
int hm_launch_planes_resample(const hm_pv_h_args* h, const hm_pv_v_args* v, int sample_bytes, int dtype, int frames, hipStream_t s);
int hm_launch_planes_view_nearest(const hm_pv_v_args* v, int dtype, int frames, hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif
