// light.hip — the light step (hm_device_light) of a device destination (gfx950): transfer-encoded code values become linear light
// through a table, change primaries through a 3 x 3 matrix, and are stored as linear floats or re-encoded by a search in a
// threshold table.  No transcendental function runs here: both tables are built on the host in double (devdest.cpp), so a
// float32 restatement on the host is exact.
//   k_light_tensor   the pointwise path, k_to_tensor's streaming shape: a wave takes 64 consecutive pixel groups of ONE row, a lane's
//                    group is 16 bytes of output per channel plane, 16-byte stores where pointers and pitches allow, the scalar
//                    instance (lane l takes pixels l, l + 64, ...) otherwise.  The crop alone runs here on the offset source.
//   k_light_nearest  HM_VIEW_NEAREST: the pixel at (j * n_w / ow, k * n_h / oh) through the same per-pixel step.
//   k_light_h        k_resample_h's body (resample_h_body, out_rows.h: its sums in its order) with the table lookup in place of the
//                    conversion to float (alpha: the conversion as it was).  The unstaged form, for all three filters.
//   k_light_v        the vertical sums of ONE pixel per lane - the matrix needs R, G and B together: a CHW intermediate is read at
//                    one index of three planes -, then matrix and finish.
// The tone step (hm_device_tone) sits between matrix and finish: the max of R, G, B is searched in thr[2048] like a code in enc, and
// the pixel is scaled by sg[] at the count - a wave-uniform branch, like `encode` and `matrix`.
// The OOTF step (hm_device_ootf) sits in front of the matrix: the scene luminance Ys = y . RGB is searched in thr[1024], and the pixel is
// scaled by sg[] at the count - wave-uniform like the others (L.ootf is a kernel argument).
// LDS: lin[1 << bits], when re-encoding enc[1 << enc_bits] behind it (1 KB each at 8 bits, 16 KB each at 12), with a tone step thr
// and sg (8 KB each) behind those, with an OOTF step its thr and sg (4 KB each) behind those - at most 56 KB, and nothing more than
// before for a call without the OOTF step -, filled once per workgroup.  The lookups are data-dependent ds_read_b32: lanes
// that meet the same entry are served by one broadcast, different entries of one bank serialise - a flat image is the best case,
// noise the worst; no layout of a table changes that.
// The matrix and the scalars of the step are kernel arguments (SGPRs).  -ffp-contract=off, __fmul_rn / __fadd_rn throughout.
// What is stored is out_elem.h's: a code value is `moved`, linear light goes through `linear_out`, a resampled alpha value through
// `finish`.  The per-pixel rules - table fill, re-encoding, matrix, tone step, colour_out - are light_step.h's, shared with alpha.hip.
#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"
#include "out_rows.h"

namespace {

// one pixel that is moved, not resampled: v0 .. v2 its colour samples, v3 its alpha sample (C == 4); lds = lin, then enc, then thr and sg
template <int C, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const float* lds, unsigned v0, unsigned v1, unsigned v2, unsigned v3, const Affine& a, OutT o[C])
{
  const unsigned peak = (1u << L.bits) - 1u;
  float r[3] = {lds[min(v0, peak)], lds[min(v1, peak)], lds[min(v2, peak)]};
  const float* enc = lds + (1 << L.bits);
  if (L.ootf) ootf_map(L, ootf_tables(L, enc), r);
  gamut(L, r);
  if (L.tone) tone_map(enc + (L.encode ? 1 << L.ebits : 0), r);
  o[0] = colour_out<OutT>(L, enc, r[0], a.scale[0], a.bias[0]);
  o[1] = colour_out<OutT>(L, enc, r[1], a.scale[1], a.bias[1]);
  o[2] = colour_out<OutT>(L, enc, r[2], a.scale[2], a.bias[2]);
  if constexpr (C == 4) o[3] = moved<OutT>(v3, a.scale[3], a.bias[3]);
}

// SB: bytes per input sample (1 / 2, little-endian), C: channels, CHW: one plane per channel, VEC: 16-byte accesses allowed (the
// launcher has checked the alignment of both sides).  grid: x = groups of 64 pixel groups, y = groups of 4 rows; dynamic LDS: the tables.
template <int SB, int C, typename OutT, bool CHW, bool VEC>
__global__ __launch_bounds__(256) void k_light_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst,
                                                      long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT); // pixels per lane
  constexpr int NB = P * C * SB;            // input bytes per lane
  fill_tables(lds, L.lin, 1 << L.bits, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS);
  const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;
  uint8_t* orow = dst + (long long)y * row_pitch;
  if (!VEC) { // one pixel per lane and step: pixels lane, lane + 64, ... of the wave's 64 * P
    const InT* irow = reinterpret_cast<const InT*>(src + (size_t)y * src_stride);
#pragma unroll 1
    for (int i = 0; i < P; i++) {
      const int x = (blockIdx.x * P + i) * 64 + lane;
      if (x >= w) break;
      const InT* ip = irow + (size_t)x * C;
      OutT o[C];
      pixel<C, OutT>(L, lds, ip[0], ip[1], ip[2], C == 4 ? ip[C - 1] : 0u, a, o);
#pragma unroll
      for (int c = 0; c < C; c++) *elem_at<OutT>(orow, CHW, plane_pitch, x, c, C) = o[c];
    }
    return;
  }
  const int x0 = (blockIdx.x * 64 + lane) * P;
  if (x0 >= w) return;
  const uint8_t* in = src + (size_t)y * src_stride + (size_t)x0 * (C * SB);
  if (x0 + P <= w) {
    typedef typename LoadWord<(NB % 16 == 0) ? 16 : (NB % 8 == 0) ? 8 : 4>::type LW;
    constexpr int NL = NB / (int)sizeof(LW);
    LW lw[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) lw[k] = reinterpret_cast<const LW*>(in)[k];
    InT smp[P * C];
    __builtin_memcpy(smp, lw, NB);
    OutT o[P * C]; // pixel-major: the row's own order
#pragma unroll
    for (int i = 0; i < P; i++) pixel<C, OutT>(L, lds, smp[i * C], smp[i * C + 1], smp[i * C + 2], C == 4 ? smp[i * C + C - 1] : 0u, a, &o[i * C]);
    if (CHW) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        OutT oc[P];
#pragma unroll
        for (int i = 0; i < P; i++) oc[i] = o[i * C + c];
        store16(elem_at<OutT>(orow, true, plane_pitch, x0, c, C), oc);
      }
    }
    else {
#pragma unroll
      for (int k = 0; k < C; k++) store16(elem_at<OutT>(orow, false, 0, x0, 0, C) + k * P, &o[k * P]); // P * C elements in a row: C stores of P elements
    }
    return;
  }
  const int n = w - x0 < P ? w - x0 : P; // the ragged last group: element by element
  const InT* ip = reinterpret_cast<const InT*>(in);
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    OutT o[C];
    pixel<C, OutT>(L, lds, ip[i * C], ip[i * C + 1], ip[i * C + 2], C == 4 ? ip[i * C + C - 1] : 0u, a, o);
#pragma unroll
    for (int c = 0; c < C; c++) *elem_at<OutT>(orow, CHW, plane_pitch, x0 + i, c, C) = o[c];
  }
}

// HM_VIEW_NEAREST: out pixel (j, k) is source pixel (j * n_w / ow, k * n_h / oh).  grid: x = groups of 64 columns, y = groups of 4 rows.
template <typename InT, int C, typename OutT>
__global__ __launch_bounds__(256) void k_light_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                       uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_tables(lds, L.lin, 1 << L.bits, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * C;
  OutT o[C];
  pixel<C, OutT>(L, lds, in[0], in[1], in[2], C == 4 ? in[C - 1] : 0u, a, o);
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < C; c++) *elem_at<OutT>(orow, chw, plane_pitch, j, c, C) = o[c];
}

// the sample-to-float step of k_light_h: the colour channels through lin (in LDS), alpha converted as it is
struct LinLookup {
  const float* lin; unsigned peak;
  __device__ __forceinline__ float operator()(unsigned v, int c) const { return c < 3 ? lin[min(v, peak)] : (float)v; }
};

// resample_h_body (out_rows.h: k_resample_h's sums in its order) with lin[min(v, peak)] in place of (float)v on the colour channels.
// grid: x = groups of 64 output columns, y = groups of 4 source rows; src points at the crop's origin; dynamic LDS: lin.
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_light_h(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                 const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                 long long pitch, long long plane, const float* __restrict__ lin, int bits)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_tables(lds, lin, 1 << bits, nullptr, 0, nullptr, 0);
  resample_h_body<SB, C, CHW>(src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, LinLookup{lds, (1u << bits) - 1u});
}

// The vertical pass: a lane is ONE output pixel, a wave 64 consecutive pixels of one output row, so the taps are wave-uniform and
// the reads of a CHW intermediate coalesce per plane (an HWC one: the wave reads 64 * C consecutive floats in C instructions).
// grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS: enc when re-encoding, then thr and sg with a tone step.
template <typename OutT, bool CHW, int C>
__global__ __launch_bounds__(256) void k_light_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh,
                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                 uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ne = L.encode ? 1 << L.ebits : 0;
  if (L.encode || L.tone || L.ootf) fill_tables(lds, L.enc, ne, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS); // (uniform: the barrier inside is met by every thread or by none)
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int y0 = first[k], n = count[k]; // (the same in every lane of the wave)
  const float* col = tmp + (long long)y0 * pitch + (CHW ? (long long)j : (long long)j * C);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; c++) acc[c] = 0.0f;
  for (int i = 0; i < n; i++) {
    const float w = wts[(size_t)i * oh + k];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = __fadd_rn(acc[c], __fmul_rn(w, CHW ? col[(long long)c * plane] : col[c]));
    col += pitch;
  }
  if (L.ootf) ootf_map(L, ootf_tables(L, lds), acc);
  gamut(L, acc);
  if (L.tone) tone_map(lds + ne, acc);
  OutT o[C];
#pragma unroll
  for (int c = 0; c < 3; c++) o[c] = colour_out<OutT>(L, lds, acc[c], a.scale[c], a.bias[c]);
  if constexpr (C == 4) o[3] = finish<OutT>(acc[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < C; c++) *elem_at<OutT>(orow, CHW, plane_pitch, j, c, C) = o[c];
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

template <int SB, int C, typename OutT, bool CHW>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool vec = ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0 && ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 &&
                   (!CHW || (p->plane_pitch % 16) == 0);
  const int groups = (w + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((rows + 3) / 4)), block(256);
  const Light L = light_of(la);
  if (vec)
    hipLaunchKernelGGL((k_light_tensor<SB, C, OutT, CHW, true>), grid, block, light_tables_bytes(la), s, src, src_stride, w, rows, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L);
  else
    hipLaunchKernelGGL((k_light_tensor<SB, C, OutT, CHW, false>), grid, block, light_tables_bytes(la), s, src, src_stride, w, rows, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L);
  return hm_check_hip(hipGetLastError(), "k_light_tensor launch");
}

// a float type, the integer type of the samples' own width, or bytes from a deeper three-channel image (the 8-bit finish); nothing else
template <int SB, int C>
int launch_tensor_dtype(const hm_dest_plan* p, const hm_light_args* la, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  const int rc = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (!std::is_integral<OutT>::value || sizeof(OutT) == SB || (SB == 2 && C == 3))
      return chw ? launch_tensor<SB, C, OutT, true>(p, la, src, src_stride, w, rows, dst, a, s) : launch_tensor<SB, C, OutT, false>(p, la, src, src_stride, w, rows, dst, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (rc != NO_KERNEL_INSTANCE) return rc;
  return hm_fail(HM_ERR_INTERNAL, "k_light_tensor: no kernel for dtype %d on %d-byte samples", p->dtype, SB);
}

template <typename InT, typename OutT>
int launch_nearest(const hm_dest_plan* p, const hm_light_args* la, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh, uint8_t* dst, const Affine& a,
                    hipStream_t s)
{
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), block(256);
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_of(la);
  constexpr bool finish8 = sizeof(InT) == 2 && sizeof(OutT) == 1; // the 8-bit finish of a deeper image: three channels only (check_args)
  if (p->channels == 3)
    hipLaunchKernelGGL((k_light_nearest<InT, 3, OutT>), grid, block, light_tables_bytes(la), s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L);
  else if constexpr (finish8) return NO_KERNEL_INSTANCE;
  else
    hipLaunchKernelGGL((k_light_nearest<InT, 4, OutT>), grid, block, light_tables_bytes(la), s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L);
  return HM_OK;
}

template <int SB, int C>
void launch_h(bool chw, const hm_resample_args* r, const hm_light_args* la, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->n_h + 3) / 4)), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  const size_t lds = light_h_bytes(la);
  if (chw)
    hipLaunchKernelGGL((k_light_h<SB, C, true>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, la->lin, la->bits);
  else
    hipLaunchKernelGGL((k_light_h<SB, C, false>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, la->lin, la->bits);
}

template <typename OutT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->oh + 3) / 4)), block(256);
  const size_t lds = light_v_bytes(la);
  const Light L = light_of(la);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
#define HM_LV_GO(CHW_, C_) \
  hipLaunchKernelGGL((k_light_v<OutT, CHW_, C_>), grid, block, lds, s, (const float*)r->tmp, (long long)r->tmp_pitch, (long long)r->tmp_plane, r->ow, r->oh, \
                     r->ay.first, r->ay.count, r->ay.weights, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L)
  if (chw) { if (p->channels == 3) HM_LV_GO(true, 3); else HM_LV_GO(true, 4); }
  else { if (p->channels == 3) HM_LV_GO(false, 3); else HM_LV_GO(false, 4); }
#undef HM_LV_GO
}

int check_args(const hm_dest_plan* p, const hm_light_args* la)
{
  if (!la->lin || (la->encode && !la->enc) || la->bits < 8 || la->bits > 12) return hm_fail(HM_ERR_INTERNAL, "k_light: tables of %d bits", la->bits);
  if (la->enc_bits != la->bits && la->enc_bits != 8) return hm_fail(HM_ERR_INTERNAL, "k_light: codes of %d bits from tables of %d", la->enc_bits, la->bits);
  if (la->src_bytes != (la->bits > 8 ? 2 : 1)) return hm_fail(HM_ERR_INTERNAL, "k_light: %d-byte samples of %d bits", la->src_bytes, la->bits);
  if (p->channels != 3 && p->channels != 4) return hm_fail(HM_ERR_INTERNAL, "k_light: %d channels", p->channels);
  // (p is the plan of the target the destination is written as: under the 8-bit finish its samples are bytes, the source's are not)
  if (p->sample_bytes != (la->enc_bits > 8 ? 2 : 1) || (p->sample_bytes != la->src_bytes && p->channels != 3))
    return hm_fail(HM_ERR_INTERNAL, "k_light: a %d-byte target of %d channels from %d-byte samples, codes of %d bits", p->sample_bytes, p->channels, la->src_bytes, la->enc_bits);
  const bool integer = p->dtype == HM_DEV_U8 || p->dtype == HM_DEV_U16;
  if (integer && (!la->encode || p->dtype != (p->sample_bytes == 1 ? HM_DEV_U8 : HM_DEV_U16)))
    return hm_fail(HM_ERR_INTERNAL, "k_light: integer dtype %d on %d-byte samples, %s", p->dtype, p->sample_bytes, la->encode ? "re-encoded" : "linear");
  return HM_OK;
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
  return (long long)(pass == 0 ? light_tables_bytes(&la) : pass == 1 ? light_h_bytes(&la) : light_v_bytes(&la));
}

// rows [0, rows) of `src` through the light step to `dst` = the destination's first element; asynchronous on `s`
extern "C" int hm_launch_light_tensor(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int w, int rows, void* dst,
                                      const float scale[4], const float bias[4], hipStream_t s)
{
  if (w <= 0 || rows <= 0) return HM_OK;
  const int rc = check_args(p, la);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  if (la->src_bytes == 1) return p->channels == 3 ? launch_tensor_dtype<1, 3>(p, la, in, src_stride, w, rows, out, a, s) : launch_tensor_dtype<1, 4>(p, la, in, src_stride, w, rows, out, a, s);
  return p->channels == 3 ? launch_tensor_dtype<2, 3>(p, la, in, src_stride, w, rows, out, a, s) : launch_tensor_dtype<2, 4>(p, la, in, src_stride, w, rows, out, a, s);
}

extern "C" int hm_launch_light_nearest(const hm_dest_plan* p, const hm_light_args* la, const void* src, int src_stride, int n_w, int n_h, int ow, int oh, void* dst,
                                       const float scale[4], const float bias[4], hipStream_t s)
{
  if (ow <= 0 || oh <= 0) return HM_OK;
  const int rc = check_args(p, la);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const bool wide = la->src_bytes == 2;
  // 16-bit elements from 16-bit samples only; bytes from either width (from 16-bit samples: the 8-bit finish); floats from either
  const int found = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if (wide) return launch_nearest<uint16_t, OutT>(p, la, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    if constexpr (!std::is_same<OutT, uint16_t>::value) return launch_nearest<uint8_t, OutT>(p, la, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_light_nearest: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return hm_check_hip(hipGetLastError(), "k_light_nearest launch");
}

// the horizontal pass of a resampled view under the light step alone (the gain step's vertical pass is gain.hip's)
extern "C" int hm_launch_light_h(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  const int rc = check_args(p, la);
  if (rc) return rc;
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  if (r->sample_bytes == 1) { if (r->channels == 3) launch_h<1, 3>(chw, r, la, s); else launch_h<1, 4>(chw, r, la, s); }
  else { if (r->channels == 3) launch_h<2, 3>(chw, r, la, s); else launch_h<2, 4>(chw, r, la, s); }
  return hm_check_hip(hipGetLastError(), "k_light_h launch");
}

// both passes of a resampled view under the light step; the intermediate is hm_launch_resample's
extern "C" int hm_launch_light_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_resample_args* r, void* dst, const float scale[4],
                                        const float bias[4], hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  int rc = hm_launch_light_h(p, la, r, s);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  uint8_t* out = (uint8_t*)dst;
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v<typename decltype(tag)::type>(p, r, la, out, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_light_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_light_v launch");
}
