// alpha.hip — the alpha step (hm_device_alpha) of a device destination (gfx950): colour is multiplied by alpha before a view sums it,
// and the result is straight colour (the sums' quotient), premultiplied colour, or the picture over a background colour - three
// channels.  The source is always four-channel interleaved (RGBA / RRGGBBAA_LE); OC, the channels written, is 3 exactly for
// HM_ALPHA_MATTE.  LIT: a light step runs beside it - the colour samples go through lin[] before the product, and the result takes the
// place of the resampled light (light_step.h: matrix, tone step, finish); without one the result goes through out_elem.h's `finish`.
//   k_alpha_tensor   the pointwise path: pointwise_body (out_rows.h), k_light_tensor's body, with this step as its pixel - four channels
//                    read, OC written.  PREMULTIPLIED (OC 4) and MATTE (OC 3) only: STRAIGHT without sums is the write without the
//                    step (devdest.cpp).
//   k_alpha_nearest  HM_VIEW_NEAREST: nearest_body (out_rows.h) with the same per-pixel step.
//   k_alpha_h        the horizontal pass: per tap ONE load of the whole pixel (4 bytes at 8 bits, 8 at 16; sample by sample where the
//                    source is not aligned to its pixels), the products p_c = x_c * a, four sums (p_R, p_G, p_B, a) in k_resample_h's
//                    order.  The unstaged form, for all three filters.  Not resample_h_body: the product stands between lookup and sum.
//   k_alpha_v        vertical_sums (out_rows.h) of ONE pixel per lane, then the mode's rule, then `finish` or light_out; 3 or 4
//                    channels are written.
// LDS (LIT only): as light.hip has it - lin, enc, the tone and the OOTF tables in the pointwise kernels, lin in k_alpha_h, enc and the
// tone and OOTF tables in k_alpha_v; at most 56 KB.  The OOTF step (light_step.h: light_out) acts on r_c in front of the matrix.
// The mode, P and the background (as floats: lin[] of it under a light step, looked up on the host) are kernel arguments.
// -ffp-contract=off, __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn throughout: no fused multiply-add, no reciprocal.
#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"
#include "out_rows.h"

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

// r[0 .. 2] to the colour elements of the destination: through light_out (light_step.h: OOTF step, matrix, tone step, the light step's
// finish), or through `finish` over the destination's whole range
template <bool LIT, typename OutT>
__device__ __forceinline__ void colour_elems(const Light& L, const LightTables& T, float r[3], const Affine& a, OutT* o)
{
  if constexpr (LIT) light_out(L, T, r, a, o);
  else {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = finish<OutT>(r[c], a.scale[c], a.bias[c], full_peak<OutT>());
  }
}

// one pixel that is moved, not summed: v[0 .. 2] its colour samples, v[3] its alpha sample
template <int OC, bool LIT, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const Alpha& A, const LightTables& T, const unsigned (&v)[4], const Affine& a, OutT* o)
{
  const float av = (float)v[3];
  float x[3];
  if constexpr (LIT) light_in(L, T, v, x);
  else { x[0] = (float)v[0]; x[1] = (float)v[1]; x[2] = (float)v[2]; }
  const float S[4] = {__fmul_rn(x[0], av), __fmul_rn(x[1], av), __fmul_rn(x[2], av), av};
  float r[3];
  alpha_rule(A, S, r);
  colour_elems<LIT, OutT>(L, T, r, a, o);
  if constexpr (OC == 4) o[3] = moved<OutT>(v[3], a.scale[3], a.bias[3]);
}

// the step's tables into LDS (LIT; all of them, or a vertical pass's); without a light step there are none and nothing looks at the view
template <bool LIT> __device__ __forceinline__ LightTables fill_lit(float* lds, const Light& L, bool with_lin)
{
  if constexpr (LIT) return fill_light(lds, L, with_lin);
  else return LightTables{};
}

// pointwise_body (out_rows.h) with the step as its pixel.  SB: bytes per input sample (1 / 2, little-endian), OC: channels written, CHW: one
// plane per channel, VEC: 16-byte accesses allowed.  grid: x = groups of 64 pixel groups, y = groups of 4 rows; dynamic LDS: the tables (LIT).
template <int SB, int OC, typename OutT, bool CHW, bool VEC, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst,
                                                      long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_lit<LIT>(lds, L, true);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;
  pointwise_body<SB, 4, OC, OutT, VEC>(src, src_stride, w, y, dst, row_pitch, plane_pitch, CHW,
                                       [&](int, const unsigned (&v)[4], OutT* o, NoColumn::Rec) { pixel<OC, LIT, OutT>(L, A, T, v, a, o); });
}

// nearest_body (out_rows.h) with the step as its pixel.  grid: x = groups of 64 columns, y = groups of 4 rows; dynamic LDS: the tables (LIT).
template <typename InT, int OC, typename OutT, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                       uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_lit<LIT>(lds, L, true);
  nearest_body<sizeof(InT), 4, OC, OutT>(src, src_stride, n_w, n_h, ow, oh, chw, dst, row_pitch, plane_pitch,
                                         [&](int, const unsigned (&v)[4], OutT* o, NoColumn::Rec) { pixel<OC, LIT, OutT>(L, A, T, v, a, o); });
}

// The horizontal pass: rows of the crop -> float32 rows of ow x 4 sums.  k_resample_h's lane mapping, table layout and order of the
// sums, but not resample_h_body (out_rows.h): the product with alpha stands between a sample's lookup and its sum, and a tap is loaded
// as a whole pixel - a kernel of its own.  A tap's pixel comes with one load when `whole` - the source address and stride are multiples of the pixel's
// 4 * SB bytes - and sample by sample otherwise.  CHW: the intermediate has one plane per sum.
// grid: x = groups of 64 output columns, y = groups of 4 source rows; src points at the crop's origin; dynamic LDS: lin (LIT).
template <int SB, bool CHW, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_h(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                 const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                 long long pitch, long long plane, const float* __restrict__ lin, int bits, int whole, int lin3)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  if constexpr (LIT) fill_tables(lds, lin, (lin3 ? 3 : 1) << bits);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || y >= n_h) return;
  const uint8_t* in = src + (size_t)y * src_stride + (size_t)first[j] * (4 * SB);
  const int n = count[j];
  const unsigned peak = (1u << bits) - 1u;
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  // look: a colour sample to the float that is summed (LIT: LinLookup / LinLookup3 of light_step.h)
  auto sums = [&](auto look) {
    auto tap = [&](float w, const unsigned (&v)[4]) {
      const float av = (float)v[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float x;
        if constexpr (LIT) x = look.colour(v[c], c);
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
  };
  if (LIT && lin3) sums(LinLookup3{lds, peak, bits}); // (wave-uniform: a table per channel)
  else sums(LinLookup{lds, peak});
  float* o = tmp + (long long)y * pitch;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (CHW) o[(long long)c * plane + j] = t[c];
    else o[(size_t)j * 4 + c] = t[c];
  }
}

// The vertical pass: vertical_sums (out_rows.h) of ONE pixel per lane, then the mode's rule, then `finish` or light_out.
// grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS (LIT): enc when re-encoding, then the tone and the OOTF tables.
template <typename OutT, bool CHW, int OC, bool LIT>
__global__ __launch_bounds__(256) void k_alpha_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh,
                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                 uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Alpha A)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_lit<LIT>(lds, L, false);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  float S[4];
  vertical_sums<4, CHW>(tmp, pitch, plane, j, k, oh, first, count, wts, S);
  float r[3];
  alpha_rule(A, S, r);
  OutT o[OC];
  colour_elems<LIT, OutT>(L, T, r, a, o);
  if constexpr (OC == 4) o[3] = finish<OutT>(S[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  store_pixel<OC>(dst + (long long)k * row_pitch, CHW, plane_pitch, j, o);
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

// has_instance (out_launch.h), less the integers beside a light step in four channels: PREMULTIPLIED there stores linear light
template <typename OutT, int SB, int OC, bool LIT> constexpr bool has_alpha_instance()
{
  return has_instance<OutT, SB, OC, LIT>() && !(std::is_integral<OutT>::value && LIT && OC == 4);
}

template <int SB, int OC, bool LIT>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst,
                  const Affine& a, hipStream_t s)
{
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  const size_t lds = LIT ? light_tables_bytes(la) : 0;
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_alpha_instance<OutT, SB, OC, LIT>()) {
      constexpr int P = 16 / (int)sizeof(OutT);
      with_flags(p->layout == HM_DEV_LAYOUT_CHW, aligned16(src, src_stride, dst, p), [&](auto chw, auto vec) {
        hipLaunchKernelGGL((k_alpha_tensor<SB, OC, OutT, chw.value, vec.value, LIT>), grid_64x4((w + P - 1) / P, rows), dim3(256), lds, s, src, src_stride, w, rows, dst,
                           (long long)p->row_pitch, (long long)p->plane_pitch, a, L, A);
      });
      return hm_check_hip(hipGetLastError(), "k_alpha_tensor launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, int OC, bool LIT>
int launch_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_alpha_args* aa, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh,
                   uint8_t* dst, const Affine& a, hipStream_t s)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  const size_t lds = LIT ? light_tables_bytes(la) : 0;
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_alpha_instance<OutT, SB, OC, LIT>()) {
      hipLaunchKernelGGL((k_alpha_nearest<InT, OC, OutT, LIT>), grid_64x4(ow, oh), dim3(256), lds, s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch,
                         (long long)p->plane_pitch, a, L, A);
      return hm_check_hip(hipGetLastError(), "k_alpha_nearest launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, bool LIT>
void launch_h(bool chw, const hm_resample_args* r, const hm_light_args* la, hipStream_t s)
{
  const dim3 grid = grid_64x4(r->ow, r->n_h), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  const size_t lds = LIT ? light_h_bytes(la) : 0;
  const float* lin = LIT ? la->lin : nullptr;
  const int bits = LIT ? la->bits : 8, lin3 = LIT ? la->lin3 : 0;
  const int whole = ((uintptr_t)src % (4 * SB)) == 0 && (r->src_stride % (4 * SB)) == 0 ? 1 : 0;
  if (chw)
    hipLaunchKernelGGL((k_alpha_h<SB, true, LIT>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, lin, bits, whole, lin3);
  else
    hipLaunchKernelGGL((k_alpha_h<SB, false, LIT>), grid, block, lds, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, lin, bits, whole, lin3);
}

template <typename OutT, bool LIT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, const hm_alpha_args* aa, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const Light L = light_or_none(la);
  const Alpha A = alpha_of(aa);
  with_flags(p->layout == HM_DEV_LAYOUT_CHW, p->channels == 4, [&](auto chw, auto four) {
    hipLaunchKernelGGL((k_alpha_v<OutT, chw.value, four.value ? 4 : 3, LIT>), grid_64x4(r->ow, r->oh), dim3(256), LIT ? light_v_bytes(la) : 0, s, (const float*)r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, r->ow, r->oh, r->ay.first, r->ay.count, r->ay.weights, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L, A);
  });
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
  if (integer && !la->encode) return hm_fail(HM_ERR_INTERNAL, "k_alpha: integer dtype %d for linear light", p->dtype);
  int rc = check_light_args("k_alpha", p, la); // (what is left of it: the codes' width, the target's samples, the integer dtype's width)
  if (rc || (rc = summed ? check_light_lds(la, 1) : check_light_lds(la, 0)) || (summed && (rc = check_light_lds(la, 2)))) return rc;
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
  const int found = HM_ALPHA_PICK(launch_tensor, p, la, aa, in, src_stride, w, rows, out, a, s);
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
  const int found = HM_ALPHA_PICK(launch_nearest, p, la, aa, in, src_stride, n_w, n_h, ow, oh, out, a, s);
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
