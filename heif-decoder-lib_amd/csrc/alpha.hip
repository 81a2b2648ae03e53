// alpha.hip — the alpha step (hm_device_alpha) of a device destination (gfx950): colour is multiplied by alpha before a view sums it,
// and the result is straight colour (the sums' quotient), premultiplied colour, or the picture over a background colour - three
// channels.  The source is always four-channel interleaved (RGBA / RRGGBBAA_LE); OC, the channels written, is 3 exactly for
// HM_ALPHA_MATTE.  LIT: a light step runs beside it - the colour samples go through lin[] before the product, and the result takes the
// place of the resampled light (light_step.h: matrix, tone step, finish); without one the result goes through out_elem.h's `finish`.
//   k_alpha_tensor   the pointwise path, k_light_tensor's streaming shape: a wave takes 64 consecutive pixel groups of ONE row, a lane's
//                    group is 16 bytes of output per channel plane, 16-byte loads and stores where pointers and pitches allow, the
//                    scalar instance (lane l takes pixels l, l + 64, ...) otherwise.  PREMULTIPLIED (OC 4) and MATTE (OC 3) only:
//                    STRAIGHT without sums is the write without the step (devdest.cpp).
//   k_alpha_nearest  HM_VIEW_NEAREST: the pixel at (j * n_w / ow, k * n_h / oh) through the same per-pixel step.
//   k_alpha_h        the horizontal pass: per tap ONE load of the whole pixel (4 bytes at 8 bits, 8 at 16; sample by sample where the
//                    source is not aligned to its pixels), the products p_c = x_c * a, four sums (p_R, p_G, p_B, a) in k_resample_h's
//                    order.  The unstaged form, for all three filters.
//   k_alpha_v        the vertical sums of ONE pixel per lane, then the mode's rule, then `finish` or matrix, tone and colour_out;
//                    3 or 4 channels are written.
// LDS (LIT only): as light.hip has it - lin, enc, the tone and the OOTF tables in the pointwise kernels, lin in k_alpha_h, enc and the
// tone and OOTF tables in k_alpha_v; at most 56 KB.  The OOTF step (light_step.h: ootf_map) acts on r_c in front of the matrix.The mode, P and the background (as floats: lin[] of it under a light step, looked up on the host) are kernel arguments.
// -ffp-contract=off, __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn throughout: no fused multiply-add, no reciprocal.
#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"

namespace {

struct Alpha { int mode; float P; float bg[3]; };

// S[0 .. 2] the (sums of the) products, S[3] the (sum of) alpha -> r[0 .. 2] under the mode's rule
__device__ __forceinline__ void alpha_rule(const Alpha& A, const float S[4], float r[3])
{
  if (A.mode == HM_ALPHA_STRAIGHT) {
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = S[3] > 0.0f ? __fdiv_rn(S[c], S[3]) : 0.0f;
  }
  else if (A.mode == HM_ALPHA_PREMULTIPLIED) {
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = __fdiv_rn(S[c], A.P);
  }
  else {
    const float cov = fminf(fmaxf(__fdiv_rn(S[3], A.P), 0.0f), 1.0f), rest = __fsub_rn(1.0f, cov);
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = __fadd_rn(__fdiv_rn(S[c], A.P), __fmul_rn(A.bg[c], rest));
  }
}

// r[0 .. 2] to the colour elements of the destination: through matrix, tone step and the light step's finish (vl: enc, then thr and sg,
// in LDS), or through `finish` over the destination's whole range
template <bool LIT, typename OutT>
__device__ __forceinline__ void colour_elems(const Light& L, const float* vl, float r[3], const Affine& a, OutT* o)
{
  if constexpr (LIT) {
    if (L.ootf) ootf_map(L, ootf_tables(L, vl), r);
    gamut(L, r);
    if (L.tone) tone_map(vl + (L.encode ? 1 << L.ebits : 0), r);
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = colour_out<OutT>(L, vl, r[c], a.scale[c], a.bias[c]);
  }
  else {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = finish<OutT>(r[c], a.scale[c], a.bias[c], full_peak<OutT>());
  }
}

// one pixel that is moved, not summed: v0 .. v2 its colour samples, v3 its alpha sample; lds = lin, then enc, then thr and sg (LIT)
template <int OC, bool LIT, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const Alpha& A, const float* lds, unsigned v0, unsigned v1, unsigned v2, unsigned v3, const Affine& a, OutT o[OC])
{
  const float av = (float)v3;
  float x[3];
  if constexpr (LIT) {
    const unsigned peak = (1u << L.bits) - 1u;
    x[0] = lds[min(v0, peak)]; x[1] = lds[min(v1, peak)]; x[2] = lds[min(v2, peak)];
  }
  else { x[0] = (float)v0; x[1] = (float)v1; x[2] = (float)v2; }
  const float S[4] = {__fmul_rn(x[0], av), __fmul_rn(x[1], av), __fmul_rn(x[2], av), av};
  float r[3];
  alpha_rule(A, S, r);
  colour_elems<LIT, OutT>(L, LIT ? lds + (1 << L.bits) : lds, r, a, o);
  if constexpr (OC == 4) o[3] = moved<OutT>(v3, a.scale[3], a.bias[3]);
}

// SB: bytes per input sample (1 / 2, little-endian), OC: channels written, CHW: one plane per channel, VEC: 16-byte accesses allowed (the
// launcher has checked the alignment of both sides).  grid: x = groups of 64 pixel groups, y = groups of 4 rows; dynamic LDS: the tables (LIT).
template <int SB, int OC, typename OutT, bool CHW, bool VEC, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst,
                                                      long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT); // pixels per lane
  constexpr int NB = P * 4 * SB;            // input bytes per lane: a multiple of 16
  if constexpr (LIT) fill_tables(lds, L.lin, 1 << L.bits, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS);
  const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;
  uint8_t* orow = dst + (long long)y * row_pitch;
  if (!VEC) { // one pixel per lane and step: pixels lane, lane + 64, ... of the wave's 64 * P
    const InT* irow = reinterpret_cast<const InT*>(src + (size_t)y * src_stride);
#pragma unroll 1
    for (int i = 0; i < P; i++) {
      const int x = (blockIdx.x * P + i) * 64 + lane;
      if (x >= w) break;
      const InT* ip = irow + (size_t)x * 4;
      OutT o[OC];
      pixel<OC, LIT, OutT>(L, A, lds, ip[0], ip[1], ip[2], ip[3], a, o);
#pragma unroll
      for (int c = 0; c < OC; c++) *elem_at<OutT>(orow, CHW, plane_pitch, x, c, OC) = o[c];
    }
    return;
  }
  const int x0 = (blockIdx.x * 64 + lane) * P;
  if (x0 >= w) return;
  const uint8_t* in = src + (size_t)y * src_stride + (size_t)x0 * (4 * SB);
  if (x0 + P <= w) {
    constexpr int NL = NB / 16;
    uint4 lw[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) lw[k] = reinterpret_cast<const uint4*>(in)[k];
    InT smp[P * 4];
    __builtin_memcpy(smp, lw, NB);
    OutT o[P * OC]; // pixel-major: the row's own order
#pragma unroll
    for (int i = 0; i < P; i++) pixel<OC, LIT, OutT>(L, A, lds, smp[i * 4], smp[i * 4 + 1], smp[i * 4 + 2], smp[i * 4 + 3], a, &o[i * OC]);
    if (CHW) {
#pragma unroll
      for (int c = 0; c < OC; c++) {
        OutT oc[P];
#pragma unroll
        for (int i = 0; i < P; i++) oc[i] = o[i * OC + c];
        store16(elem_at<OutT>(orow, true, plane_pitch, x0, c, OC), oc);
      }
    }
    else {
#pragma unroll
      for (int k = 0; k < OC; k++) store16(elem_at<OutT>(orow, false, 0, x0, 0, OC) + k * P, &o[k * P]); // P * OC elements in a row: OC stores of P elements
    }
    return;
  }
  const int n = w - x0 < P ? w - x0 : P; // the ragged last group: element by element
  const InT* ip = reinterpret_cast<const InT*>(in);
#pragma unroll 1
  for (int i = 0; i < n; i++) {
    OutT o[OC];
    pixel<OC, LIT, OutT>(L, A, lds, ip[i * 4], ip[i * 4 + 1], ip[i * 4 + 2], ip[i * 4 + 3], a, o);
#pragma unroll
    for (int c = 0; c < OC; c++) *elem_at<OutT>(orow, CHW, plane_pitch, x0 + i, c, OC) = o[c];
  }
}

// HM_VIEW_NEAREST: out pixel (j, k) is source pixel (j * n_w / ow, k * n_h / oh).  grid: x = groups of 64 columns, y = groups of 4 rows.
template <typename InT, int OC, typename OutT, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                       uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if constexpr (LIT) fill_tables(lds, L.lin, 1 << L.bits, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * 4;
  OutT o[OC];
  pixel<OC, LIT, OutT>(L, A, lds, in[0], in[1], in[2], in[3], a, o);
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < OC; c++) *elem_at<OutT>(orow, chw, plane_pitch, j, c, OC) = o[c];
}

// The horizontal pass: rows of the crop -> float32 rows of ow x 4 sums.  k_resample_h's lane mapping, table layout and order of the
// sums (out_rows.h); a tap's pixel comes with one load when `whole` - the source address and stride are multiples of the pixel's
// 4 * SB bytes - and sample by sample otherwise.  CHW: the intermediate has one plane per sum.
// grid: x = groups of 64 output columns, y = groups of 4 source rows; src points at the crop's origin; dynamic LDS: lin (LIT).
template <int SB, bool CHW, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_h(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                 const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                 long long pitch, long long plane, const float* __restrict__ lin, int bits, int whole)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  if constexpr (LIT) fill_tables(lds, lin, 1 << bits, nullptr, 0, nullptr, 0);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || y >= n_h) return;
  const uint8_t* in = src + (size_t)y * src_stride + (size_t)first[j] * (4 * SB);
  const int n = count[j];
  const unsigned peak = (1u << bits) - 1u;
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  auto tap = [&](float w, const unsigned (&v)[4]) {
    const float av = (float)v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float x;
      if constexpr (LIT) x = lds[min(v[c], peak)];
      else x = (float)v[c];
      t[c] = __fadd_rn(t[c], __fmul_rn(w, __fmul_rn(x, av)));
    }
    t[3] = __fadd_rn(t[3], __fmul_rn(w, av));
  };
  if (whole) { // (wave-uniform)
    for (int i = 0; i < n; i++) {
      unsigned v[4];
      load_samples<SB, 4>(in + (size_t)i * (4 * SB), v);
      tap(wts[(size_t)i * ow + j], v);
    }
  }
  else {
    const InT* ip = reinterpret_cast<const InT*>(in);
    for (int i = 0; i < n; i++) {
      const unsigned v[4] = {ip[i * 4], ip[i * 4 + 1], ip[i * 4 + 2], ip[i * 4 + 3]};
      tap(wts[(size_t)i * ow + j], v);
    }
  }
  float* o = tmp + (long long)y * pitch;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (CHW) o[(long long)c * plane + j] = t[c];
    else o[(size_t)j * 4 + c] = t[c];
  }
}

// The vertical pass: a lane is ONE output pixel, a wave 64 consecutive pixels of one output row, so the taps are wave-uniform and
// the reads of a CHW intermediate coalesce per plane (an HWC one: a lane reads its four sums with one 16-byte load).
// grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS (LIT): enc when re-encoding, then thr and sg with a tone step.
template <typename OutT, bool CHW, int OC, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh,
                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                 uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if constexpr (LIT) {
    if (L.encode || L.tone || L.ootf) fill_tables(lds, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, L.tone ? 2 * TONE_STEPS : 0, L.ootf, 2 * OOTF_STEPS); // (uniform: the barrier inside is met by every thread or by none)
  }
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int y0 = first[k], n = count[k]; // (the same in every lane of the wave)
  const float* col = tmp + (long long)y0 * pitch + (CHW ? (long long)j : (long long)j * 4);
  float S[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i = 0; i < n; i++) {
    const float w = wts[(size_t)i * oh + k];
    float v[4];
    if (CHW) {
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = col[(long long)c * plane];
    }
    else { // (pitch is a multiple of 16 elements and tmp a pool block: 16-byte aligned)
      const float4 q = *reinterpret_cast<const float4*>(col);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) S[c] = __fadd_rn(S[c], __fmul_rn(w, v[c]));
    col += pitch;
  }
  float r[3];
  alpha_rule(A, S, r);
  OutT o[OC];
  colour_elems<LIT, OutT>(L, lds, r, a, o);
  if constexpr (OC == 4) o[3] = finish<OutT>(S[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < OC; c++) *elem_at<OutT>(orow, CHW, plane_pitch, j, c, OC) = o[c];
}

// every instance the launchers below can pick (hm_debug_kernel_regs): 92 pointwise, 23 nearest, 8 horizontal, 32 vertical.
// An integer dtype is the target's own, or bytes from 16-bit samples under the 8-bit finish (LIT, three channels); PREMULTIPLIED beside
// a light step stores linear light, so OC 4 with LIT has float dtypes only.
#define HM_AT_LAYOUTS(SB, OC, T, LIT) \
  (const void*)k_alpha_tensor<SB, OC, T, true, true, LIT>, (const void*)k_alpha_tensor<SB, OC, T, true, false, LIT>, \
  (const void*)k_alpha_tensor<SB, OC, T, false, true, LIT>, (const void*)k_alpha_tensor<SB, OC, T, false, false, LIT>
#define HM_AT_FLOAT(SB, T) HM_AT_LAYOUTS(SB, 3, T, false), HM_AT_LAYOUTS(SB, 4, T, false), HM_AT_LAYOUTS(SB, 3, T, true), HM_AT_LAYOUTS(SB, 4, T, true)
#define HM_AT_INT(SB, T) HM_AT_LAYOUTS(SB, 3, T, false), HM_AT_LAYOUTS(SB, 4, T, false), HM_AT_LAYOUTS(SB, 3, T, true)
#define HM_AN_FLOAT(IN, T) (const void*)k_alpha_nearest<IN, 3, T, false>, (const void*)k_alpha_nearest<IN, 4, T, false>, \
  (const void*)k_alpha_nearest<IN, 3, T, true>, (const void*)k_alpha_nearest<IN, 4, T, true>
#define HM_AN_INT(IN, T) (const void*)k_alpha_nearest<IN, 3, T, false>, (const void*)k_alpha_nearest<IN, 4, T, false>, (const void*)k_alpha_nearest<IN, 3, T, true>
#define HM_AV_SET(T, LIT) (const void*)k_alpha_v<T, true, 3, LIT>, (const void*)k_alpha_v<T, true, 4, LIT>, (const void*)k_alpha_v<T, false, 3, LIT>, \
  (const void*)k_alpha_v<T, false, 4, LIT>
const void* const g_instances[] = {
  HM_AT_INT(1, uint8_t), HM_AT_FLOAT(1, __half), HM_AT_FLOAT(1, float), HM_AT_INT(2, uint16_t), HM_AT_FLOAT(2, __half), HM_AT_FLOAT(2, float),
  HM_AT_LAYOUTS(2, 3, uint8_t, true),
  HM_AN_INT(uint8_t, uint8_t), HM_AN_FLOAT(uint8_t, __half), HM_AN_FLOAT(uint8_t, float), HM_AN_INT(uint16_t, uint16_t), HM_AN_FLOAT(uint16_t, __half),
  HM_AN_FLOAT(uint16_t, float), (const void*)k_alpha_nearest<uint16_t, 3, uint8_t, true>,
  (const void*)k_alpha_h<1, true, false>, (const void*)k_alpha_h<1, false, false>, (const void*)k_alpha_h<1, true, true>, (const void*)k_alpha_h<1, false, true>,
  (const void*)k_alpha_h<2, true, false>, (const void*)k_alpha_h<2, false, false>, (const void*)k_alpha_h<2, true, true>, (const void*)k_alpha_h<2, false, true>,
  HM_AV_SET(uint8_t, false), HM_AV_SET(uint16_t, false), HM_AV_SET(__half, false), HM_AV_SET(float, false),
  HM_AV_SET(uint8_t, true), HM_AV_SET(uint16_t, true), HM_AV_SET(__half, true), HM_AV_SET(float, true),
};
#undef HM_AT_LAYOUTS
#undef HM_AT_FLOAT
#undef HM_AT_INT
#undef HM_AN_FLOAT
#undef HM_AN_INT
#undef HM_AV_SET

// the Light a kernel gets: the light step's, or (no light step) one that names no table - the unlit instances do not look at it
Light light_or_none(const hm_light_args* la)
{
  if (la) return light_of(la);
  Light L = {};
  return L;
}

Alpha alpha_of(const hm_alpha_args* aa)
{
  Alpha A;
  A.mode = aa->mode; A.P = aa->P;
  for (int c = 0; c < 3; c++) A.bg[c] = aa->bg[c];
  return A;
}

// does an instance exist for elements of OutT from samples of SB bytes, OC channels written, with or without a light step?
template <typename OutT, int SB, int OC, bool LIT> constexpr bool has_instance()
{
  if (!std::is_integral<OutT>::value) return true;
  if (sizeof(OutT) == SB) return !(LIT && OC == 4);
  return sizeof(OutT) == 1 && SB == 2 && OC == 3 && LIT; // the 8-bit finish
}

template <int SB, int OC, typename OutT, bool CHW, bool LIT>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst,
                  const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool vec = ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0 && ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 &&
                   (!CHW || (p->plane_pitch % 16) == 0);
  const int groups = (w + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((rows + 3) / 4)), block(256);
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  const size_t lds = LIT ? light_tables_bytes(la) : 0;
  if (vec)
    hipLaunchKernelGGL((k_alpha_tensor<SB, OC, OutT, CHW, true, LIT>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L, A);
  else
    hipLaunchKernelGGL((k_alpha_tensor<SB, OC, OutT, CHW, false, LIT>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L, A);
  return hm_check_hip(hipGetLastError(), "k_alpha_tensor launch");
}

template <int SB, int OC, bool LIT>
int launch_tensor_dtype(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst,
                        const Affine& a, hipStream_t s)
{
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, OC, LIT>())
      return chw ? launch_tensor<SB, OC, OutT, true, LIT>(p, la, aa, src, src_stride, w, rows, dst, a, s)
                 : launch_tensor<SB, OC, OutT, false, LIT>(p, la, aa, src, src_stride, w, rows, dst, a, s);
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, int OC, bool LIT>
int launch_nearest_dtype(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh,
                         uint8_t* dst, const Affine& a, hipStream_t s)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), block(256);
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  const size_t lds = LIT ? light_tables_bytes(la) : 0;
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, OC, LIT>()) {
      hipLaunchKernelGGL((k_alpha_nearest<InT, OC, OutT, LIT>), grid, block, lds, s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch,
                         (long long)p->plane_pitch, a, L, A);
      return hm_check_hip(hipGetLastError(), "k_alpha_nearest launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, bool LIT>
void launch_h(bool chw, const hm_resample_args* r, const hm_light_args* la, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->n_h + 3) / 4)), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  const size_t lds = LIT ? light_h_bytes(la) : 0;
  const float* lin = LIT ? la->lin : nullptr;
  const int bits = LIT ? la->bits : 8;
  const int whole = ((uintptr_t)src % (4 * SB)) == 0 && (r->src_stride % (4 * SB)) == 0 ? 1 : 0;
  if (chw)
    hipLaunchKernelGGL((k_alpha_h<SB, true, LIT>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, lin, bits, whole);
  else
    hipLaunchKernelGGL((k_alpha_h<SB, false, LIT>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, lin, bits, whole);
}

template <typename OutT, bool LIT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, const hm_alpha_args* aa, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->oh + 3) / 4)), block(256);
  const size_t lds = LIT ? light_v_bytes(la) : 0;
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
#define HM_AV_GO(CHW_, OC_) \
  hipLaunchKernelGGL((k_alpha_v<OutT, CHW_, OC_, LIT>), grid, block, lds, s, (const float*)r->tmp, (long long)r->tmp_pitch, (long long)r->tmp_plane, r->ow, r->oh, \
                     r->ay.first, r->ay.count, r->ay.weights, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L, A)
  if (chw) { if (p->channels == 3) HM_AV_GO(true, 3); else HM_AV_GO(true, 4); }
  else { if (p->channels == 3) HM_AV_GO(false, 3); else HM_AV_GO(false, 4); }
#undef HM_AV_GO
}

// p: the plan of the target the destination is written as (three channels exactly under HM_ALPHA_MATTE)
int check_args(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, bool summed)
{
  if (aa->mode != HM_ALPHA_STRAIGHT && aa->mode != HM_ALPHA_PREMULTIPLIED && aa->mode != HM_ALPHA_MATTE) return hm_fail(HM_ERR_INTERNAL, "k_alpha: mode %d", aa->mode);
  if (aa->mode == HM_ALPHA_STRAIGHT && !summed) return hm_fail(HM_ERR_INTERNAL, "k_alpha: HM_ALPHA_STRAIGHT without sums is the write without the step");
  if (p->channels != (aa->mode == HM_ALPHA_MATTE ? 3 : 4)) return hm_fail(HM_ERR_INTERNAL, "k_alpha: %d channels in mode %d", p->channels, aa->mode);
  if (aa->src_bytes != 1 && aa->src_bytes != 2) return hm_fail(HM_ERR_INTERNAL, "k_alpha: %d-byte samples", aa->src_bytes);
  if (aa->bits < 8 || aa->bits > 16 || aa->src_bytes != (aa->bits > 8 ? 2 : 1) || aa->P != (float)((1 << aa->bits) - 1))
    return hm_fail(HM_ERR_INTERNAL, "k_alpha: %d-byte samples of %d bits, P %g", aa->src_bytes, aa->bits, (double)aa->P);
  const bool integer = p->dtype == HM_DEV_U8 || p->dtype == HM_DEV_U16;
  if (!la) {
    if (p->sample_bytes != aa->src_bytes) return hm_fail(HM_ERR_INTERNAL, "k_alpha: a %d-byte target from %d-byte samples", p->sample_bytes, aa->src_bytes);
    return HM_OK;
  }
  if (!la->lin || (la->encode && !la->enc) || la->bits != aa->bits || la->bits > HM_LIGHT_MAX_BITS || la->src_bytes != aa->src_bytes)
    return hm_fail(HM_ERR_INTERNAL, "k_alpha: light tables of %d bits beside samples of %d", la->bits, aa->bits);
  if (la->enc_bits != la->bits && la->enc_bits != 8) return hm_fail(HM_ERR_INTERNAL, "k_alpha: codes of %d bits from tables of %d", la->enc_bits, la->bits);
  if (p->sample_bytes != (la->enc_bits > 8 ? 2 : 1) || (p->sample_bytes != aa->src_bytes && p->channels != 3))
    return hm_fail(HM_ERR_INTERNAL, "k_alpha: a %d-byte target of %d channels from %d-byte samples, codes of %d bits", p->sample_bytes, p->channels, aa->src_bytes, la->enc_bits);
  if (integer && !la->encode) return hm_fail(HM_ERR_INTERNAL, "k_alpha: integer dtype %d for linear light", p->dtype);
  if (aa->mode == HM_ALPHA_PREMULTIPLIED && (la->encode || la->tone)) return hm_fail(HM_ERR_INTERNAL, "k_alpha: premultiplied light is not encoded or tone-mapped");
  return HM_OK;
}

int no_instance(const char* kernel, const hm_dest_plan* p, const hm_alpha_args* aa, bool lit)
{
  return hm_fail(HM_ERR_INTERNAL, "%s: no kernel for dtype %d, %d channels, on %d-byte samples %s a light step", kernel, p->dtype, p->channels, aa->src_bytes, lit ? "beside" : "without");
}

} // namespace

extern "C" const void* hm_alpha_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

// SB, OC and LIT become template arguments here: f<SB, OC, LIT>() for the launch at hand
#define HM_ALPHA_PICK(F, ...) \
  (aa->src_bytes == 1 ? (p->channels == 3 ? (la ? F<1, 3, true>(__VA_ARGS__) : F<1, 3, false>(__VA_ARGS__)) : (la ? F<1, 4, true>(__VA_ARGS__) : F<1, 4, false>(__VA_ARGS__))) \
                      : (p->channels == 3 ? (la ? F<2, 3, true>(__VA_ARGS__) : F<2, 3, false>(__VA_ARGS__)) : (la ? F<2, 4, true>(__VA_ARGS__) : F<2, 4, false>(__VA_ARGS__))))

// rows [0, rows) of the four-channel `src` through the alpha step to `dst` = the destination's first element; asynchronous on `s`
extern "C" int hm_launch_alpha_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const void* src, int src_stride, int w, int rows, void* dst,
                                      const float scale[4], const float bias[4], hipStream_t s)
{
  if (w <= 0 || rows <= 0) return HM_OK;
  const int rc = check_args(p, la, aa, false);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = HM_ALPHA_PICK(launch_tensor_dtype, p, la, aa, in, src_stride, w, rows, out, a, s);
  return found == NO_KERNEL_INSTANCE ? no_instance("k_alpha_tensor", p, aa, la != nullptr) : found;
}

extern "C" int hm_launch_alpha_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const void* src, int src_stride, int n_w, int n_h, int ow,
                                       int oh, void* dst, const float scale[4], const float bias[4], hipStream_t s)
{
  if (ow <= 0 || oh <= 0) return HM_OK;
  const int rc = check_args(p, la, aa, false);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = HM_ALPHA_PICK(launch_nearest_dtype, p, la, aa, in, src_stride, n_w, n_h, ow, oh, out, a, s);
  return found == NO_KERNEL_INSTANCE ? no_instance("k_alpha_nearest", p, aa, la != nullptr) : found;
}
#undef HM_ALPHA_PICK

// both passes of a resampled view under the alpha step; r describes a four-channel intermediate
extern "C" int hm_launch_alpha_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const hm_resample_args* r, void* dst,
                                        const float scale[4], const float bias[4], hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  int rc = check_args(p, la, aa, true);
  if (rc) return rc;
  if (r->channels != 4 || r->sample_bytes != aa->src_bytes) return hm_fail(HM_ERR_INTERNAL, "k_alpha_h: an intermediate of %d channels from %d-byte samples", r->channels, r->sample_bytes);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  if (aa->src_bytes == 1) { if (la) launch_h<1, true>(chw, r, la, s); else launch_h<1, false>(chw, r, la, s); }
  else { if (la) launch_h<2, true>(chw, r, la, s); else launch_h<2, false>(chw, r, la, s); }
  if ((rc = hm_check_hip(hipGetLastError(), "k_alpha_h launch"))) return rc;
  const Affine a = affine_of(scale, bias);
  uint8_t* out = (uint8_t*)dst;
  const int found = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if (la) launch_v<OutT, true>(p, r, la, aa, out, a, s); else launch_v<OutT, false>(p, r, la, aa, out, a, s);
    return HM_OK;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_alpha_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_alpha_v launch");
}
