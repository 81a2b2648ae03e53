// gain.hip — the gain step (hm_device_gain) beside the light step of a device destination (gfx950): the linear light of an SDR base
// image times a factor read from its gain map (ISO 21496-1), per output pixel
//   r_c = fsub(fmul(fadd(r_c, kb_c), M_c), ka_c)
// before the gamut matrix, with M_c the view sum over tab_c[map sample] under the MAP's own taps (include/heif_mi355x.h, "Gain").  No
// transcendental function runs here: tab is built on the host in double (devdest.cpp), like the light step's tables.
//   k_gain_tensor   the pointwise path (no view, the crop alone): pointwise_body (out_rows.h), k_light_tensor's body, with this step as
//                   its pixel and a column's tap record as what it reads per column.  The map is enlarged here (n <= m: at most two taps per axis), so
//                   M_c is formed in the kernel - horizontal sums per map row first, tap 0 first, then the vertical sum over them:
//                   the sums of the two-pass form in its order - instead of a full-size float32 intermediate, which at 12 MP CHW
//                   float32 would add about half the write's traffic again.  The taps come as 16-byte records (hm_gain_tap: first,
//                   count, w0, w1): a wave is one row, so its row's record is a scalar load, and a lane loads the records of its P
//                   columns, then their 2 x 2 map samples, as independent loads - no loop whose length is read from memory.
//   k_gain_nearest  HM_VIEW_NEAREST: nearest_body (out_rows.h); base and map sample at (j * n / m) of their own crops.
//   k_gain_map_h    the map's horizontal pass of a resampled view: resample_h_body (out_rows.h) with tab_c[min(v, mpeak)] as the
//                   sample-to-float step; grid z = the table's channel.
//   k_gain_map_v    the map's vertical pass into the float32 M planes (nch planes of oh rows): vertical_sums (out_rows.h) of one channel.
//   k_gain_v        k_light_v with the update between the sums and light_out; the base's horizontal pass stays k_light_h (light.hip).
// LDS: the light step's tables (light_step.h: light_layout) and behind them nch tables of 1 << map_bits floats (1 KB each at 8 bits, 16 KB at 12).
// Where both together would pass 48 KB (12-bit samples re-encoded, or 12-bit tables beside a tone step), the gain tables are
// read from global memory instead: the same values.  Every table index is clamped to its table (min(v, peak)), every tap lies inside
// the map's crop (axis_taps, devdest.cpp).  -ffp-contract=off, __fmul_rn / __fadd_rn / __fsub_rn throughout.
#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"
#include "out_rows.h"

namespace {

enum { GAIN_LDS_MOST = 48 * 1024 }; // (what the light step's own kernels ask for at the most)

// what the kernels get beside Light (by value: SGPRs)
struct Gain {
  const float* tab;                   // nch tables of 1 << mbits entries
  const uint8_t* map; int map_stride; // at the map crop's origin
  int msb, nch, mbits, mw, mh;        // bytes per map sample, tables, the map's depth, the map's crop
  int tab_lds;                        // the tables sit in LDS behind the light step's
  float kb[3], ka[3];
  const int4* xrec; const int4* yrec; // (pointwise) the map's taps per output column and row: first, count, w0, w1 (hm_gain_tap)
};

__device__ __forceinline__ unsigned map_sample(const Gain& G, const uint8_t* row, int x)
{
  const unsigned v = G.msb == 1 ? (unsigned)row[x] : (unsigned)reinterpret_cast<const uint16_t*>(row)[x];
  return min(v, (1u << G.mbits) - 1u);
}

// the places of the light step's tables taken once: the pointwise kernels run up to 16 pixels of a lane through them
struct TablesAt {
  const float* lin_; const float* enc_; const float* tone_;
  __device__ __forceinline__ const float* lin() const { return lin_; }
  __device__ __forceinline__ const float* enc(const Light&) const { return enc_; }
  __device__ __forceinline__ const float* tone(const Light&) const { return tone_; }
  __device__ __forceinline__ const float* ootf(const Light&) const { return nullptr; } // (never beside the gain step)
};

// the light step's tables (fill_light), then the gain tables behind them, into LDS (every thread of the workgroup comes here);
// *gt: the gain tables, where they are read
__device__ __forceinline__ TablesAt fill_all(float* lds, const Light& L, const Gain& G, const float** gt)
{
  const LightTables T = fill_light(lds, L, true);
  const int nl = T.at(L).end;
  *gt = G.tab_lds ? lds + nl : G.tab; // (uniform)
  if (G.tab_lds) fill_tables(lds + nl, G.tab, G.nch << G.mbits);
  return TablesAt{T.lin(), T.enc(L), T.tone(L)};
}

// the taps of an output row or column of the pointwise path (hm_gain_tap): at most two, w1 = 0 where there is one
struct Tap2 { int first, count; float w0, w1; };
__device__ __forceinline__ Tap2 tap_of(const int4& r) { return Tap2{r.x, r.y, __int_as_float(r.z), __int_as_float(r.w)}; }

// M_c of an output pixel from its column's and its row's taps: per map row of the vertical taps the horizontal sum, tap 0 first, then
// the vertical sum over those, tap 0 first - what k_gain_map_h and k_gain_map_v form in two passes, on at most 2 x 2 samples.  The four
// loads do not depend on each other; a tap the table does not have is loaded from the first one's place and not added.
__device__ __forceinline__ void gain_M(const Gain& G, const float* gt, const Tap2& tx, const Tap2& ty, float M[3])
{
  const uint8_t* row0 = G.map + (size_t)ty.first * G.map_stride;
  const uint8_t* row1 = ty.count > 1 ? row0 + G.map_stride : row0;
  const int c0 = tx.first, c1 = tx.count > 1 ? c0 + 1 : c0;
  const unsigned v00 = map_sample(G, row0, c0), v01 = map_sample(G, row0, c1), v10 = map_sample(G, row1, c0), v11 = map_sample(G, row1, c1);
  const int n1 = 1 << G.mbits;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c && G.nch == 1) { M[c] = M[0]; continue; }
    const float* t = gt + c * n1;
    float t0 = __fadd_rn(0.0f, __fmul_rn(tx.w0, t[v00])), t1 = __fadd_rn(0.0f, __fmul_rn(tx.w0, t[v10]));
    if (tx.count > 1) { t0 = __fadd_rn(t0, __fmul_rn(tx.w1, t[v01])); t1 = __fadd_rn(t1, __fmul_rn(tx.w1, t[v11])); }
    float acc = __fadd_rn(0.0f, __fmul_rn(ty.w0, t0));
    if (ty.count > 1) acc = __fadd_rn(acc, __fmul_rn(ty.w1, t1));
    M[c] = acc;
  }
}

// the update on one pixel's linear light, then what the light step does behind its sums (light_out without the OOTF step, which
// never runs beside the gain step: refused on the host)
template <typename Tables, typename OutT>
__device__ __forceinline__ void gain_out(const Light& L, const Tables& T, const Gain& G, float r[3], const float M[3], const Affine& a, OutT* o)
{
#pragma unroll
  for (int c = 0; c < 3; c++) r[c] = __fsub_rn(__fmul_rn(__fadd_rn(r[c], G.kb[c]), M[c]), G.ka[c]);
  light_out<false>(L, T, r, a, o);
}

// one pixel that is moved, not resampled: v[0 .. 2] its colour samples, v[3] its alpha sample (C == 4)
template <int C, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const TablesAt& T, const Gain& G, const float M[3], const unsigned (&v)[C], const Affine& a, OutT* o)
{
  float r[3];
  light_in(L, T, v, r);
  gain_out(L, T, G, r, M, a, o);
  if constexpr (C == 4) o[3] = moved<OutT>(v[3], a.scale[3], a.bias[3]);
}

// pointwise_body (out_rows.h) with the step as its pixel and a column's tap record as what it reads per column.  SB: bytes per input
// sample (1 / 2, little-endian), C: channels, VEC: 16-byte accesses allowed; chw: one plane per channel.  grid: x = groups of 64 pixel
// groups, y = groups of 4 rows; dynamic LDS: the tables.
// The image is the crop itself: output pixel (x, y) is its pixel (x, y), and the map's taps are those of x and y.
template <int SB, int C, typename OutT, bool VEC>
__global__ __launch_bounds__(256) void k_gain_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst, long long row_pitch,
                                                     long long plane_pitch, int chw, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* gt;
  const TablesAt T = fill_all(lds, L, G, &gt);
  const int y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6)); // (a wave is one row: its taps are scalar loads)
  if (y >= h) return;
  const Tap2 ty = tap_of(G.yrec[y]);
  pointwise_body<SB, C, C, OutT, VEC>(
    src, src_stride, w, y, dst, row_pitch, plane_pitch, chw,
    [&](int, const unsigned (&v)[C], OutT* o, const int4& rec) {
      float M[3];
      gain_M(G, gt, tap_of(rec), ty, M);
      pixel<C, OutT>(L, T, G, M, v, a, o);
    },
    [&](int x) { return G.xrec[x]; });
}

// nearest_body (out_rows.h): the base pixel it picks, and map sample (j * mw / ow, k * mh / oh) of the map's crop.
// grid: x = groups of 64 columns, y = groups of 4 rows.
template <typename InT, int C, typename OutT>
__global__ __launch_bounds__(256) void k_gain_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                      uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* gt;
  const TablesAt T = fill_all(lds, L, G, &gt);
  nearest_body<sizeof(InT), C, C, OutT>(src, src_stride, n_w, n_h, ow, oh, chw, dst, row_pitch, plane_pitch, [&](int j, const unsigned (&v)[C], OutT* o, NoColumn::Rec) {
    const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
    const unsigned mv = map_sample(G, G.map + (size_t)(k * G.mh / oh) * G.map_stride, j * G.mw / ow);
    const int n1 = 1 << G.mbits;
    const float M[3] = {gt[mv], G.nch == 3 ? gt[n1 + mv] : gt[mv], G.nch == 3 ? gt[2 * n1 + mv] : gt[mv]};
    pixel<C, OutT>(L, T, G, M, v, a, o);
  });
}

// the sample-to-float step of k_gain_map_h: a map code through one channel's table (in LDS)
struct TabLookup {
  const float* tab; unsigned mpeak;
  __device__ __forceinline__ float operator()(unsigned v, int) const { return tab[min(v, mpeak)]; }
};

// The map's horizontal pass: resample_h_body on the one-channel map, through the table of channel blockIdx.z, into plane blockIdx.z
// of mtmp (mh rows of `pitch` floats).  grid: x = groups of 64 output columns, y = groups of 4 map rows, z = channels; dynamic LDS: one table.
template <int SB>
__global__ __launch_bounds__(256) void k_gain_map_h(const uint8_t* __restrict__ map, int map_stride, int mh, int ow, const int32_t* __restrict__ first,
                                                    const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ mtmp, long long pitch,
                                                    const float* __restrict__ tab, int mbits)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  fill_tables(lds, tab + ((size_t)blockIdx.z << mbits), 1 << mbits);
  resample_h_body<SB, 1, true>(map, map_stride, mh, ow, first, count, wts, mtmp + (long long)blockIdx.z * pitch * mh, pitch, 0, TabLookup{lds, (1u << mbits) - 1u});
}

// The map's vertical pass: plane blockIdx.z of mtmp -> plane blockIdx.z of M (oh rows), vertical_sums (out_rows.h) of one channel.
// grid: x = groups of 64 columns, y = groups of 4 output rows, z = channels.
__global__ __launch_bounds__(256) void k_gain_map_v(const float* __restrict__ mtmp, long long pitch, int mh, int ow, int oh, const int32_t* __restrict__ first,
                                                    const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ M)
{
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  float acc[1];
  vertical_sums<1, true>(mtmp + (long long)blockIdx.z * pitch * mh, pitch, 0, j, k, oh, first, count, wts, acc);
  M[(long long)blockIdx.z * pitch * oh + (long long)k * pitch + j] = acc[0];
}

// The base's vertical pass: k_light_v's sums of ONE pixel per lane (vertical_sums), then the update with M (nch planes of oh rows of
// m_pitch floats) and light_out.  grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS: enc when re-encoding, then
// the tone tables.
template <typename OutT, bool CHW, int C>
__global__ __launch_bounds__(256) void k_gain_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh, const int32_t* __restrict__ first,
                                                const int32_t* __restrict__ count, const float* __restrict__ wts, const float* __restrict__ Mp, long long m_pitch,
                                                uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LightTables T = fill_light(lds, L, false);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  float acc[C];
  vertical_sums<C, CHW>(tmp, pitch, plane, j, k, oh, first, count, wts, acc);
  const float* mp = Mp + (long long)k * m_pitch + j;
  const long long m_plane = m_pitch * oh;
  const float m0 = mp[0];
  const float M[3] = {m0, G.nch == 3 ? mp[m_plane] : m0, G.nch == 3 ? mp[2 * m_plane] : m0};
  OutT o[C];
  gain_out(L, T, G, acc, M, a, o);
  if constexpr (C == 4) o[3] = finish<OutT>(acc[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  store_pixel<C>(dst + (long long)k * row_pitch, CHW, plane_pitch, j, o);
}

// every instance the launchers below can pick (hm_debug_kernel_regs, code 12): 26 pointwise (the two of the 8-bit finish from 16-bit
// samples among them), 13 nearest, 3 of the map's two passes, 16 vertical - 58
#define HM_GT_SET(SB, T) (const void*)k_gain_tensor<SB, 3, T, true>, (const void*)k_gain_tensor<SB, 3, T, false>, (const void*)k_gain_tensor<SB, 4, T, true>, \
  (const void*)k_gain_tensor<SB, 4, T, false>
#define HM_GN_SET(IN, T) (const void*)k_gain_nearest<IN, 3, T>, (const void*)k_gain_nearest<IN, 4, T>
#define HM_GV_SET(T) (const void*)k_gain_v<T, true, 3>, (const void*)k_gain_v<T, true, 4>, (const void*)k_gain_v<T, false, 3>, (const void*)k_gain_v<T, false, 4>
const void* const g_instances[] = {
  HM_GT_SET(1, uint8_t), HM_GT_SET(1, __half), HM_GT_SET(1, float), HM_GT_SET(2, uint16_t), HM_GT_SET(2, __half), HM_GT_SET(2, float),
  (const void*)k_gain_tensor<2, 3, uint8_t, true>, (const void*)k_gain_tensor<2, 3, uint8_t, false>,
  HM_GN_SET(uint8_t, uint8_t), HM_GN_SET(uint8_t, __half), HM_GN_SET(uint8_t, float), HM_GN_SET(uint16_t, uint16_t), HM_GN_SET(uint16_t, __half), HM_GN_SET(uint16_t, float),
  (const void*)k_gain_nearest<uint16_t, 3, uint8_t>,
  (const void*)k_gain_map_h<1>, (const void*)k_gain_map_h<2>, (const void*)k_gain_map_v,
  HM_GV_SET(uint8_t), HM_GV_SET(uint16_t), HM_GV_SET(__half), HM_GV_SET(float),
};
#undef HM_GT_SET
#undef HM_GN_SET
#undef HM_GV_SET

Gain gain_of(const hm_gain_args* ga, size_t light_bytes, size_t* lds_bytes)
{
  Gain G;
  G.tab = ga->tab; G.map = (const uint8_t*)ga->map; G.map_stride = ga->map_stride;
  G.msb = ga->map_bytes; G.nch = ga->nch; G.mbits = ga->map_bits; G.mw = ga->mw; G.mh = ga->mh;
  const size_t gain_bytes = ((size_t)ga->nch << ga->map_bits) * sizeof(float);
  G.tab_lds = light_bytes + gain_bytes <= GAIN_LDS_MOST ? 1 : 0;
  for (int c = 0; c < 3; c++) { G.kb[c] = ga->kb[c]; G.ka[c] = ga->ka[c]; }
  G.xrec = reinterpret_cast<const int4*>(ga->xrec); G.yrec = reinterpret_cast<const int4*>(ga->yrec);
  if (lds_bytes) *lds_bytes = light_bytes + (G.tab_lds ? gain_bytes : 0);
  return G;
}

// rows through the instance of k_gain_tensor for the plan's dtype and alignment, or NO_KERNEL_INSTANCE
template <int SB, int C>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a,
                  hipStream_t s)
{
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_of(la);
  size_t lds = 0;
  const Gain G = gain_of(ga, light_tables_bytes(la), &lds);
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, C, true>()) {
      constexpr int P = 16 / (int)sizeof(OutT);
      const dim3 grid = grid_64x4((w + P - 1) / P, rows), block(256);
      if (aligned16(src, src_stride, dst, p))
        hipLaunchKernelGGL((k_gain_tensor<SB, C, OutT, true>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, chw, a, L, G);
      else
        hipLaunchKernelGGL((k_gain_tensor<SB, C, OutT, false>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, chw, a, L, G);
      return hm_check_hip(hipGetLastError(), "k_gain_tensor launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <int SB, int C>
int launch_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh, uint8_t* dst,
                   const Affine& a, hipStream_t s)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_of(la);
  size_t lds = 0;
  const Gain G = gain_of(ga, light_tables_bytes(la), &lds);
  return with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (has_instance<OutT, SB, C, true>()) {
      hipLaunchKernelGGL((k_gain_nearest<InT, C, OutT>), grid_64x4(ow, oh), dim3(256), lds, s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch,
                         (long long)p->plane_pitch, a, L, G);
      return hm_check_hip(hipGetLastError(), "k_gain_nearest launch");
    }
    return NO_KERNEL_INSTANCE;
  });
}

template <typename OutT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, const hm_gain_args* ga, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const Light L = light_of(la);
  const Gain G = gain_of(ga, 0, nullptr);
  with_flags(p->layout == HM_DEV_LAYOUT_CHW, p->channels == 4, [&](auto chw, auto four) {
    hipLaunchKernelGGL((k_gain_v<OutT, chw.value, four.value ? 4 : 3>), grid_64x4(r->ow, r->oh), dim3(256), light_v_bytes(la), s, (const float*)r->tmp, (long long)r->tmp_pitch,
                       (long long)r->tmp_plane, r->ow, r->oh, r->ay.first, r->ay.count, r->ay.weights, (const float*)ga->M, (long long)ga->pitch, dst, (long long)p->row_pitch,
                       (long long)p->plane_pitch, a, L, G);
  });
}

// the light step's arguments as light.hip's launchers judge them, then the gain step's
// taps: 0 none (nearest), 1 the records of the pointwise path, 2 the tables of the summed path
int check_args(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, int taps)
{
  int rc = check_light_args("k_gain", p, la);
  if (rc || (rc = taps == 2 ? check_light_lds(la, 2) : check_light_lds(la, 0))) return rc; // (the summed path's horizontal pass: hm_launch_light_h asks)
  if (!ga->tab || !ga->map || (ga->nch != 1 && ga->nch != 3) || ga->map_bits < 8 || ga->map_bits > HM_GAIN_MAX_BITS || ga->map_bytes != (ga->map_bits > 8 ? 2 : 1) ||
      ga->mw < 1 || ga->mh < 1 || (int64_t)ga->map_stride < (int64_t)ga->mw * ga->map_bytes)
    return hm_fail(HM_ERR_INTERNAL, "k_gain: a map of %d x %d samples of %d bits in %d bytes, stride %d, %d tables", ga->mw, ga->mh, ga->map_bits, ga->map_bytes, ga->map_stride, ga->nch);
  if (taps == 2 && (!ga->ax.first || !ga->ax.count || !ga->ax.weights || !ga->ay.first || !ga->ay.count || !ga->ay.weights)) return hm_fail(HM_ERR_INTERNAL, "k_gain: no tap tables for the map");
  if (taps == 1 && (!ga->xrec || !ga->yrec || (((uintptr_t)ga->xrec | (uintptr_t)ga->yrec) & 15))) return hm_fail(HM_ERR_INTERNAL, "k_gain: no 16-byte aligned tap records for the map");
  return HM_OK;
}

} // namespace

extern "C" const void* hm_gain_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

// rows [0, rows) of `src` (the crop itself: w x rows) through the light and gain steps to `dst` = the destination's first element;
// ga->ax / ga->ay: the map's taps onto w and rows.  Asynchronous on `s`.
extern "C" int hm_launch_gain_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const void* src, int src_stride, int w, int rows, void* dst,
                                     const float scale[4], const float bias[4], hipStream_t s)
{
  if (w <= 0 || rows <= 0) return HM_OK;
  const int rc = check_args(p, la, ga, 1);
  if (rc) return rc;
  if (ga->ax.m != w || ga->ay.m != rows) return hm_fail(HM_ERR_INTERNAL, "k_gain_tensor: taps for %d x %d, the image is %d x %d", ga->ax.m, ga->ay.m, w, rows);
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = with_flags(la->src_bytes == 2, p->channels == 4, [&](auto wide, auto four) {
    return launch_tensor<wide.value ? 2 : 1, four.value ? 4 : 3>(p, la, ga, in, src_stride, w, rows, out, a, s);
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_gain_tensor: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return found;
}

extern "C" int hm_launch_gain_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const void* src, int src_stride, int n_w, int n_h, int ow, int oh,
                                      void* dst, const float scale[4], const float bias[4], hipStream_t s)
{
  if (ow <= 0 || oh <= 0) return HM_OK;
  const int rc = check_args(p, la, ga, 0);
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const int found = with_flags(la->src_bytes == 2, p->channels == 4, [&](auto wide, auto four) {
    return launch_nearest<wide.value ? 2 : 1, four.value ? 4 : 3>(p, la, ga, in, src_stride, n_w, n_h, ow, oh, out, a, s);
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_gain_nearest: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return found;
}

// a resampled view under the light and gain steps: the map's two passes into M, k_light_h, k_gain_v
extern "C" int hm_launch_gain_resample(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const hm_resample_args* r, void* dst, const float scale[4],
                                       const float bias[4], hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  int rc = check_args(p, la, ga, 2);
  if (rc) return rc;
  if (!ga->mtmp || !ga->M || ga->pitch < r->ow || ga->ax.m != r->ow || ga->ay.m != r->oh)
    return hm_fail(HM_ERR_INTERNAL, "k_gain_map: taps for %d x %d, the view writes %d x %d (pitch %lld)", ga->ax.m, ga->ay.m, r->ow, r->oh, (long long)ga->pitch);
  const dim3 block(256);
  const dim3 grid_h = grid_64x4(r->ow, ga->mh, ga->nch), grid_v = grid_64x4(r->ow, r->oh, ga->nch);
  const size_t lds_h = (size_t)4 << ga->map_bits;
  const uint8_t* map = (const uint8_t*)ga->map;
  if (ga->map_bytes == 1)
    hipLaunchKernelGGL((k_gain_map_h<1>), grid_h, block, lds_h, s, map, ga->map_stride, ga->mh, r->ow, ga->ax.first, ga->ax.count, ga->ax.weights, ga->mtmp, (long long)ga->pitch, ga->tab, ga->map_bits);
  else
    hipLaunchKernelGGL((k_gain_map_h<2>), grid_h, block, lds_h, s, map, ga->map_stride, ga->mh, r->ow, ga->ax.first, ga->ax.count, ga->ax.weights, ga->mtmp, (long long)ga->pitch, ga->tab, ga->map_bits);
  if ((rc = hm_check_hip(hipGetLastError(), "k_gain_map_h launch"))) return rc;
  hipLaunchKernelGGL(k_gain_map_v, grid_v, block, 0, s, (const float*)ga->mtmp, (long long)ga->pitch, ga->mh, r->ow, r->oh, ga->ay.first, ga->ay.count, ga->ay.weights, ga->M);
  if ((rc = hm_check_hip(hipGetLastError(), "k_gain_map_v launch"))) return rc;
  if ((rc = hm_launch_light_h(p, la, r, s))) return rc;
  const Affine a = affine_of(scale, bias);
  uint8_t* out = (uint8_t*)dst;
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v<typename decltype(tag)::type>(p, r, la, ga, out, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_gain_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_gain_v launch");
}
