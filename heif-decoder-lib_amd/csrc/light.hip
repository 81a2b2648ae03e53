// light.hip — the light step (hm_device_light) of a device destination (gfx950): transfer-encoded code values become linear light
// through a table, change primaries through a 3 x 3 matrix, and are stored as linear floats or re-encoded by a search in a
// threshold table.  No transcendental function runs here: both tables are built on the host in double (devdest.cpp), so a
// float32 restatement on the host is exact.
//   k_light_tensor   the pointwise path: pointwise_body (out_rows.h), k_to_tensor's streaming shape - a wave takes 64 consecutive pixel
//                    groups of ONE row, 16-byte stores where pointers and pitches allow, the scalar instance otherwise - with the
//                    step as its pixel.  The crop alone runs here on the offset source.
//   k_light_nearest  HM_VIEW_NEAREST: the nearest source pixel through the same per-pixel step (nearest_body's text, out_rows.h).
//   k_light_h        k_resample_h's body (resample_h_body, out_rows.h: its sums in its order) with the table lookup in place of the
//                    conversion to float (alpha: the conversion as it was).  The unstaged form, for all three filters.
//   k_light_v        vertical_sums (out_rows.h) of ONE pixel per lane - the matrix needs R, G and B together: a CHW intermediate is
//                    read at one index of three planes -, then light_out.
// The tone step (hm_device_tone) sits between matrix and finish: the max of R, G, B is searched in thr[2048] like a code in enc, and
// the pixel is scaled by sg[] at the count - a wave-uniform branch, like `encode` and `matrix`.
// The OOTF step (hm_device_ootf) sits in front of the matrix: the scene luminance Ys = y . RGB is searched in thr[1024], and the pixel is
// scaled by sg[] at the count - wave-uniform like the others (L.ootf is a kernel argument).
// LDS: lin[1 << bits] (three of them for an ICC profile with distinct curves: light_step.h, lin3), when re-encoding enc[1 << enc_bits] behind it (1 KB each at 8 bits, 16 KB each at 12), with a tone step thr
// and sg (8 KB each) behind those, with an OOTF step its thr and sg (4 KB each) behind those - at most 56 KB, and nothing more than
// before for a call without the OOTF step -, filled once per workgroup.  The lookups are data-dependent ds_read_b32: lanes
// that meet the same entry are served by one broadcast, different entries of one bank serialise - a flat image is the best case,
// noise the worst; no layout of a table changes that.
// The matrix and the scalars of the step are kernel arguments (SGPRs).  -ffp-contract=off, __fmul_rn / __fadd_rn throughout.
// What is stored is out_elem.h's: a code value is `moved`, linear light goes through `linear_out`, a resampled alpha value through
// `finish`.  The per-pixel rules - the tables' layout and fill, light_in, and light_out: OOTF step, matrix, tone step, colour_out - are
// light_step.h's, shared with alpha.hip and gain.hip; grids, the 16-byte test and the rule which instances exist are out_launch.h's.
#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"
#include "out_rows.h"

namespace {

// one pixel that is moved, not resampled: v[0 .. 2] its colour samples, v[3] its alpha sample (C == 4)
template <int C, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const LightTables& T, const unsigned (&v)[C], const Affine& a, OutT* o)
{
  float r[3];
  light_in(L, T, v, r);
  light_out(L, T, r, a, o);
  if constexpr (C == 4) o[3] = moved<OutT>(v[3], a.scale[3], a.bias[3]);
}

// pointwise_body (out_rows.h) with the step as its pixel.  SB: bytes per input sample (1 / 2, little-endian), C: channels, CHW: one plane
// per channel, VEC: 16-byte accesses allowed.  grid: x = groups of 64 pixel groups, y = groups of 4 rows; dynamic LDS: the tables.
template <int SB, int C, typename OutT, bool CHW, bool VEC>
__global__ __launch_bounds__(256) void k_light_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst,
                                                      long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_light(lds, L, true);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;
  pointwise_body<SB, C, C, OutT, VEC>(src, src_stride, w, y, dst, row_pitch, plane_pitch, CHW,
                                      [&](int, const unsigned (&v)[C], OutT* o, NoColumn::Rec) { pixel<C, OutT>(L, T, v, a, o); });
}

// HM_VIEW_NEAREST: nearest_body's text (out_rows.h) written out - through the shared body k_light_nearest<uint8_t, 4, __half> is 1 - 2 %
// slower at 4000 x 3000 (profiles/step_kernels_refactor.txt).  grid: x = groups of 64 columns, y = groups of 4 rows; dynamic LDS: the tables.
template <typename InT, int C, typename OutT>
__global__ __launch_bounds__(256) void k_light_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                       uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_light(lds, L, true);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * C;
  unsigned v[C];
#pragma unroll
  for (int c = 0; c < C; c++) v[c] = in[c];
  OutT o[C];
  pixel<C, OutT>(L, T, v, a, o);
  store_pixel<C>(dst + (long long)k * row_pitch, chw, plane_pitch, j, o);
}

// resample_h_body (out_rows.h: k_resample_h's sums in its order) with lin[min(v, peak)] in place of (float)v on the colour channels
// (LinLookup, light_step.h; lin3 - wave-uniform -: a table per channel, LinLookup3).
// grid: x = groups of 64 output columns, y = groups of 4 source rows; src points at the crop's origin; dynamic LDS: lin.
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_light_h(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                 const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                 long long pitch, long long plane, const float* __restrict__ lin, int bits, int lin3)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_tables(lds, lin, (lin3 ? 3 : 1) << bits);
  if (lin3) resample_h_body<SB, C, CHW>(src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, LinLookup3{lds, (1u << bits) - 1u, bits});
  else resample_h_body<SB, C, CHW>(src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, LinLookup{lds, (1u << bits) - 1u});
}

// The vertical pass: vertical_sums (out_rows.h) of ONE pixel per lane - the matrix needs R, G and B together -, then light_out.
// grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS: enc when re-encoding, then the tone and the OOTF tables.
template <typename OutT, bool CHW, int C>
__global__ __launch_bounds__(256) void k_light_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh,
                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                 uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_light(lds, L, false);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  float acc[C];
  vertical_sums<C, CHW>(tmp, pitch, plane, j, k, oh, first, count, wts, acc);
  OutT o[C];
  light_out(L, T, acc, a, o);
  if constexpr (C == 4) o[3] = finish<OutT>(acc[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  store_pixel<C>(dst + (long long)k * row_pitch, CHW, plane_pitch, j, o);
}

// every instance the launchers below can pick (hm_debug_kernel_regs): 48 pointwise, 12 nearest, 8 horizontal, 16 vertical
#define HM_LT_SET(SB, T) \
  (const void*)k_light_tensor<SB, 3, T, true, true>, (const void*)k_light_tensor<SB, 3, T, true, false>, (const void*)k_light_tensor<SB, 3, T, false, true>, \
  (const void*)k_light_tensor<SB, 3, T, false, false>, (const void*)k_light_tensor<SB, 4, T, true, true>, (const void*)k_light_tensor<SB, 4, T, true, false>, \
  (const void*)k_light_tensor<SB, 4, T, false, true>, (const void*)k_light_tensor<SB, 4, T, false, false>
#define HM_LN_SET(IN, T) (const void*)k_light_nearest<IN, 3, T>, (const void*)k_light_nearest<IN, 4, T>
#define HM_LV_SET(T) (const void*)k_light_v<T, true, 3>, (const void*)k_light_v<T, true, 4>, (const void*)k_light_v<T, false, 3>, (const void*)k_light_v<T, false, 4>
const void* const g_instances[] = {
  HM_LT_SET(1, uint8_t), HM_LT_SET(1, __half), HM_LT_SET(1, float), HM_LT_SET(2, uint16_t), HM_LT_SET(2, __half), HM_LT_SET(2, float),
  HM_LN_SET(uint8_t, uint8_t), HM_LN_SET(uint8_t, __half), HM_LN_SET(uint8_t, float), HM_LN_SET(uint16_t, uint16_t), HM_LN_SET(uint16_t, __half), HM_LN_SET(uint16_t, float),
  (const void*)k_light_h<1, 3, true>, (const void*)k_light_h<1, 3, false>, (const void*)k_light_h<1, 4, true>, (const void*)k_light_h<1, 4, false>,
  (const void*)k_light_h<2, 3, true>, (const void*)k_light_h<2, 3, false>, (const void*)k_light_h<2, 4, true>, (const void*)k_light_h<2, 4, false>,
  HM_LV_SET(uint8_t), HM_LV_SET(uint16_t), HM_LV_SET(__half), HM_LV_SET(float),
};
// ... and the five of the 8-bit finish from 16-bit samples (hm_device_tone.out_bits == 8): 4 pointwise, 1 nearest
const void* const g_finish8_instances[] = {
  (const void*)k_light_tensor<2, 3, uint8_t, true, true>, (const void*)k_light_tensor<2, 3, uint8_t, true, false>, (const void*)k_light_tensor<2, 3, uint8_t, false, true>,
  (const void*)k_light_tensor<2, 3, uint8_t, false, false>, (const void*)k_light_nearest<uint16_t, 3, uint8_t>,
};
#undef HM_LT_SET
#undef HM_LN_SET
#undef HM_LV_SET

// rows through the instance of k_light_tensor for the plan's dtype, layout and alignment, or NO_KERNEL_INSTANCE
template <int SB, int C>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const Light L = light_of(la);
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, C, true>()) {
      constexpr int P = 16 / (int)sizeof(OutT);
      with_flags(p->layout == HM_DEV_LAYOUT_CHW, aligned16(src, src_stride, dst, p), [&](auto chw, auto vec) {
        hipLaunchKernelGGL((k_light_tensor<SB, C, OutT, chw.value, vec.value>), grid_64x4((w + P - 1) / P, rows), dim3(256), light_tables_bytes(la), s, src, src_stride, w,
                           rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L);
      });
      return hm_check_hip(hipGetLastError(), "k_light_tensor launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, int C>
int launch_nearest(const hm_dest_plan* p, const hm_light_args* la, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh, uint8_t* dst, const Affine& a,
                   hipStream_t s)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_of(la);
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, C, true>()) {
      hipLaunchKernelGGL((k_light_nearest<InT, C, OutT>), grid_64x4(ow, oh), dim3(256), light_tables_bytes(la), s, src, src_stride, n_w, n_h, ow, oh, chw, dst,
                         (long long)p->row_pitch, (long long)p->plane_pitch, a, L);
      return hm_check_hip(hipGetLastError(), "k_light_nearest launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, int C>
void launch_h(bool chw, const hm_resample_args* r, const hm_light_args* la, hipStream_t s)
{
  const dim3 grid = grid_64x4(r->ow, r->n_h), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  const size_t lds = light_h_bytes(la);
  if (chw)
    hipLaunchKernelGGL((k_light_h<SB, C, true>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, la->lin, la->bits, la->lin3);
  else
    hipLaunchKernelGGL((k_light_h<SB, C, false>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, la->lin, la->bits, la->lin3);
}

template <typename OutT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const Light L = light_of(la);
  with_flags(p->layout == HM_DEV_LAYOUT_CHW, p->channels == 4, [&](auto chw, auto four) {
    hipLaunchKernelGGL((k_light_v<OutT, chw.value, four.value ? 4 : 3>), grid_64x4(r->ow, r->oh), dim3(256), light_v_bytes(la), s, (const float*)r->tmp, (long long)r->tmp_pitch,
                       (long long)r->tmp_plane, r->ow, r->oh, r->ay.first, r->ay.count, r->ay.weights, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L);
  });
}

} // namespace

extern "C" const void* hm_light_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

extern "C" const void* hm_light_finish8_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_finish8_instances) / sizeof(g_finish8_instances[0])) ? g_finish8_instances[index] : nullptr;
}

// what the launchers ask for as dynamic LDS (test_hooks.cpp: hm_debug_light_lds); pass 0: k_light_tensor / k_light_nearest, 1: k_light_h,
// 2: k_light_v; tone: bit 0 a tone step, bit 1 an OOTF step
extern "C" long long hm_light_lds_bytes(int bits, int enc_bits, int encode, int tone, int pass)
{
  static const float some = 0.0f;
  hm_light_args la = {};
  la.bits = bits; la.enc_bits = enc_bits; la.encode = encode; la.tone = (tone & 1) ? &some : nullptr; la.ootf = (tone & 2) ? &some : nullptr;
  return (long long)light_pass_bytes(&la, pass);
}

extern "C" int hm_light_lds_check(int bits, int enc_bits, int encode, int tone, int lin3, int pass)
{
  static const float some = 0.0f;
  hm_light_args la = {};
  la.bits = bits; la.enc_bits = enc_bits; la.encode = encode; la.tone = (tone & 1) ? &some : nullptr; la.ootf = (tone & 2) ? &some : nullptr; la.lin3 = lin3;
  return check_light_lds(&la, pass);
}

// rows [0, rows) of `src` through the light step to `dst` = the destination's first element; asynchronous on `s`
extern "C" int hm_launch_light_tensor(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int w, int rows, void* dst,
                                      const float scale[4], const float bias[4], hipStream_t s)
{
  if (w <= 0 || rows <= 0) return HM_OK;
  int rc = check_light_args("k_light", p, la);
  if (rc || (rc = check_light_lds(la, 0))) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = with_flags(la->src_bytes == 2, p->channels == 4, [&](auto wide, auto four) {
    return launch_tensor<wide.value ? 2 : 1, four.value ? 4 : 3>(p, la, in, src_stride, w, rows, out, a, s);
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_light_tensor: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return found;
}

extern "C" int hm_launch_light_nearest(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int n_w, int n_h, int ow, int oh, void* dst,
                                       const float scale[4], const float bias[4], hipStream_t s)
{
  if (ow <= 0 || oh <= 0) return HM_OK;
  int rc = check_light_args("k_light", p, la);
  if (rc || (rc = check_light_lds(la, 0))) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = with_flags(la->src_bytes == 2, p->channels == 4, [&](auto wide, auto four) {
    return launch_nearest<wide.value ? 2 : 1, four.value ? 4 : 3>(p, la, in, src_stride, n_w, n_h, ow, oh, out, a, s);
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_light_nearest: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return found;
}

// the horizontal pass of a resampled view under the light step alone (the gain step's vertical pass is gain.hip's)
extern "C" int hm_launch_light_h(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  int rc = check_light_args("k_light", p, la);
  if (rc || (rc = check_light_lds(la, 1))) return rc;
  with_flags(r->sample_bytes == 2, r->channels == 4, [&](auto wide, auto four) { launch_h<wide.value ? 2 : 1, four.value ? 4 : 3>(p->layout == HM_DEV_LAYOUT_CHW, r, la, s); });
  return hm_check_hip(hipGetLastError(), "k_light_h launch");
}

// both passes of a resampled view under the light step; the intermediate is hm_launch_resample's
extern "C" int hm_launch_light_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, void* dst, const float scale[4],
                                        const float bias[4], hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  int rc = hm_launch_light_h(p, la, r, s);
  if (rc || (rc = check_light_lds(la, 2))) return rc;
  const Affine a = affine_of(scale, bias);
  uint8_t* out = (uint8_t*)dst;
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v<typename decltype(tag)::type>(p, r, la, out, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_light_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_light_v launch");
}
