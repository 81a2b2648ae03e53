// gain.hip — the gain step (hm_device_gain) beside the light step of a device destination (gfx950): the linear light of an SDR base
// image times a factor read from its gain map (ISO 21496-1), per output pixel
//   r_c = fsub(fmul(fadd(r_c, kb_c), M_c), ka_c)
// before the gamut matrix, with M_c the view sum over tab_c[map sample] under the MAP's own taps (include/heif_mi355x.h, "Gain").  No
// transcendental function runs here: tab is built on the host in double (devdest.cpp), like the light step's tables.
//   k_gain_tensor   the pointwise path (no view, the crop alone), k_light_tensor's streaming shape: a wave takes 64 consecutive pixel
//                   groups of ONE row, a lane's group is 16 bytes of output per channel plane, 16-byte stores where pointers and
//                   pitches allow, the scalar instance otherwise.  The map is enlarged here (n <= m: at most two taps per axis), so
//                   M_c is formed in the kernel - horizontal sums per map row first, tap 0 first, then the vertical sum over them:
//                   the sums of the two-pass form in its order - instead of a full-size float32 intermediate, which at 12 MP CHW
//                   float32 would add about half the write's traffic again.  The taps come as 16-byte records (hm_gain_tap: first,
//                   count, w0, w1): a wave is one row, so its row's record is a scalar load, and a lane loads the records of its P
//                   columns, then their 2 x 2 map samples, as independent loads - no loop whose length is read from memory.
//   k_gain_nearest  HM_VIEW_NEAREST: base and map sample at (j * n / m) of their own crops.
//   k_gain_map_h    the map's horizontal pass of a resampled view: resample_h_body (out_rows.h) with tab_c[min(v, mpeak)] as the
//                   sample-to-float step; grid z = the table's channel.
//   k_gain_map_v    the map's vertical pass into the float32 M planes (nch planes of oh rows).
//   k_gain_v        k_light_v with the update between the sums and the matrix; the base's horizontal pass stays k_light_h (light.hip).
// LDS: the light step's tables (light_step.h) and behind them nch tables of 1 << map_bits floats (1 KB each at 8 bits, 16 KB at 12).
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

// the light step's tables, then the gain tables, into LDS (every thread of the workgroup comes here); returns the gain tables
__device__ __forceinline__ const float* fill_all(float* lds, const Light& L, const Gain& G)
{
  const int nl = (1 << L.bits) + (L.encode ? 1 << L.ebits : 0) + (L.tone ? 2 * TONE_STEPS : 0);
  fill_tables(lds, L.lin, 1 << L.bits, L.enc, L.encode ? 1 << L.ebits : 0, L.tone, 2 * TONE_STEPS);
  if (!G.tab_lds) return G.tab; // (uniform)
  fill_tables(lds + nl, G.tab, G.nch << G.mbits, nullptr, 0, nullptr, 0);
  return lds + nl;
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

// the update on one pixel's linear light, then what the light step does behind its sums: matrix, tone step, finish.  enc: the
// threshold table in LDS, the tone tables behind it
template <int C, typename OutT>
__device__ __forceinline__ void gain_out(const Light& L, const float* enc, const Gain& G, float r[3], const float M[3], const Affine& a, OutT o[C])
{
#pragma unroll
  for (int c = 0; c < 3; c++) r[c] = __fsub_rn(__fmul_rn(__fadd_rn(r[c], G.kb[c]), M[c]), G.ka[c]);
  gamut(L, r);
  if (L.tone) tone_map(enc + (L.encode ? 1 << L.ebits : 0), r);
#pragma unroll
  for (int c = 0; c < 3; c++) o[c] = colour_out<OutT>(L, enc, r[c], a.scale[c], a.bias[c]);
}

// one pixel that is moved, not resampled: v0 .. v2 its colour samples, v3 its alpha sample (C == 4); lds = lin, then enc, then thr and sg
template <int C, typename OutT>
__device__ __forceinline__ void pixel(const Light& L, const float* lds, const Gain& G, const float M[3], unsigned v0, unsigned v1, unsigned v2, unsigned v3,
                                      const Affine& a, OutT o[C])
{
  const unsigned peak = (1u << L.bits) - 1u;
  float r[3] = {lds[min(v0, peak)], lds[min(v1, peak)], lds[min(v2, peak)]};
  gain_out<C, OutT>(L, lds + (1 << L.bits), G, r, M, a, o);
  if constexpr (C == 4) o[3] = moved<OutT>(v3, a.scale[3], a.bias[3]);
}

// SB: bytes per input sample (1 / 2, little-endian), C: channels, VEC: 16-byte accesses allowed (the launcher has checked the alignment
// of both sides); chw: one plane per channel.  grid: x = groups of 64 pixel groups, y = groups of 4 rows; dynamic LDS: the tables.
// The image is the crop itself: output pixel (x, y) is its pixel (x, y), and the map's taps are those of x and y.
template <int SB, int C, typename OutT, bool VEC>
__global__ __launch_bounds__(256) void k_gain_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst, long long row_pitch,
                                                     long long plane_pitch, int chw, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT); // pixels per lane
  constexpr int NB = P * C * SB;            // input bytes per lane
  const float* gt = fill_all(lds, L, G);
  const int lane = threadIdx.x & 63, y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6)); // (a wave is one row: its taps are scalar loads)
  if (y >= h) return;
  uint8_t* orow = dst + (long long)y * row_pitch;
  const Tap2 ty = tap_of(G.yrec[y]);
  float M[3];
  if (!VEC) { // one pixel per lane and step: pixels lane, lane + 64, ... of the wave's 64 * P
    const InT* irow = reinterpret_cast<const InT*>(src + (size_t)y * src_stride);
#pragma unroll 1
    for (int i = 0; i < P; i++) {
      const int x = (blockIdx.x * P + i) * 64 + lane;
      if (x >= w) break;
      const InT* ip = irow + (size_t)x * C;
      OutT o[C];
      gain_M(G, gt, tap_of(G.xrec[x]), ty, M);
      pixel<C, OutT>(L, lds, G, M, ip[0], ip[1], ip[2], C == 4 ? ip[C - 1] : 0u, a, o);
#pragma unroll
      for (int c = 0; c < C; c++) *elem_at<OutT>(orow, chw, plane_pitch, x, c, C) = o[c];
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
    int4 rec[P]; // the columns' taps: P loads of 16 bytes, issued together
#pragma unroll
    for (int i = 0; i < P; i++) rec[i] = G.xrec[x0 + i];
    OutT o[P * C]; // pixel-major: the row's own order
#pragma unroll
    for (int i = 0; i < P; i++) {
      gain_M(G, gt, tap_of(rec[i]), ty, M);
      pixel<C, OutT>(L, lds, G, M, smp[i * C], smp[i * C + 1], smp[i * C + 2], C == 4 ? smp[i * C + C - 1] : 0u, a, &o[i * C]);
    }
    if (chw) {
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
    gain_M(G, gt, tap_of(G.xrec[x0 + i]), ty, M);
    pixel<C, OutT>(L, lds, G, M, ip[i * C], ip[i * C + 1], ip[i * C + 2], C == 4 ? ip[i * C + C - 1] : 0u, a, o);
#pragma unroll
    for (int c = 0; c < C; c++) *elem_at<OutT>(orow, chw, plane_pitch, x0 + i, c, C) = o[c];
  }
}

// HM_VIEW_NEAREST: out pixel (j, k) is base pixel (j * n_w / ow, k * n_h / oh) and map sample (j * mw / ow, k * mh / oh) of the map's crop.
// grid: x = groups of 64 columns, y = groups of 4 rows.
template <typename InT, int C, typename OutT>
__global__ __launch_bounds__(256) void k_gain_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int chw,
                                                      uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float* gt = fill_all(lds, L, G);
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * C;
  const unsigned v = map_sample(G, G.map + (size_t)(k * G.mh / oh) * G.map_stride, j * G.mw / ow);
  const int n1 = 1 << G.mbits;
  const float M[3] = {gt[v], G.nch == 3 ? gt[n1 + v] : gt[v], G.nch == 3 ? gt[2 * n1 + v] : gt[v]};
  OutT o[C];
  pixel<C, OutT>(L, lds, G, M, in[0], in[1], in[2], C == 4 ? in[C - 1] : 0u, a, o);
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < C; c++) *elem_at<OutT>(orow, chw, plane_pitch, j, c, C) = o[c];
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
  fill_tables(lds, tab + ((size_t)blockIdx.z << mbits), 1 << mbits, nullptr, 0, nullptr, 0);
  resample_h_body<SB, 1, true>(map, map_stride, mh, ow, first, count, wts, mtmp + (long long)blockIdx.z * pitch * mh, pitch, 0, TabLookup{lds, (1u << mbits) - 1u});
}

// The map's vertical pass: plane blockIdx.z of mtmp -> plane blockIdx.z of M (oh rows).  A lane is one output pixel, a wave 64
// consecutive pixels of one row: the taps are wave-uniform.  grid: x = groups of 64 columns, y = groups of 4 output rows, z = channels.
__global__ __launch_bounds__(256) void k_gain_map_v(const float* __restrict__ mtmp, long long pitch, int mh, int ow, int oh, const int32_t* __restrict__ first,
                                                    const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ M)
{
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int y0 = first[k], n = count[k];
  const float* col = mtmp + (long long)blockIdx.z * pitch * mh + (long long)y0 * pitch + j;
  float acc = 0.0f;
  for (int i = 0; i < n; i++) {
    acc = __fadd_rn(acc, __fmul_rn(wts[(size_t)i * oh + k], *col));
    col += pitch;
  }
  M[(long long)blockIdx.z * pitch * oh + (long long)k * pitch + j] = acc;
}

// The base's vertical pass: k_light_v's sums of ONE pixel per lane, then the update with M (nch planes of oh rows of m_pitch floats),
// matrix, tone step and finish.  grid: x = groups of 64 columns, y = groups of 4 output rows; dynamic LDS: enc when re-encoding, then
// thr and sg with a tone step.
template <typename OutT, bool CHW, int C>
__global__ __launch_bounds__(256) void k_gain_v(const float* __restrict__ tmp, long long pitch, long long plane, int ow, int oh, const int32_t* __restrict__ first,
                                                const int32_t* __restrict__ count, const float* __restrict__ wts, const float* __restrict__ Mp, long long m_pitch,
                                                uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a, Light L, Gain G)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ne = L.encode ? 1 << L.ebits : 0;
  if (L.encode || L.tone) fill_tables(lds, L.enc, ne, L.tone, 2 * TONE_STEPS, nullptr, 0); // (uniform: the barrier inside is met by every thread or by none)
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
  const float* mp = Mp + (long long)k * m_pitch + j;
  const long long m_plane = m_pitch * oh;
  const float m0 = mp[0];
  const float M[3] = {m0, G.nch == 3 ? mp[m_plane] : m0, G.nch == 3 ? mp[2 * m_plane] : m0};
  OutT o[C];
  gain_out<C, OutT>(L, lds, G, acc, M, a, o);
  if constexpr (C == 4) o[3] = finish<OutT>(acc[3], a.scale[3], a.bias[3], full_peak<OutT>()); // a resampled alpha value: k_resample_v's finish
  uint8_t* orow = dst + (long long)k * row_pitch;
#pragma unroll
  for (int c = 0; c < C; c++) *elem_at<OutT>(orow, CHW, plane_pitch, j, c, C) = o[c];
}

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

template <int SB, int C, typename OutT>
int launch_tensor(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a,
                  hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const bool vec = ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0 && ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 && (!chw || (p->plane_pitch % 16) == 0);
  const int groups = (w + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((rows + 3) / 4)), block(256);
  const Light L = light_of(la);
  size_t lds = 0;
  const Gain G = gain_of(ga, light_tables_bytes(la), &lds);
  if (vec)
    hipLaunchKernelGGL((k_gain_tensor<SB, C, OutT, true>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, chw, a, L, G);
  else
    hipLaunchKernelGGL((k_gain_tensor<SB, C, OutT, false>), grid, block, lds, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, chw, a, L, G);
  return hm_check_hip(hipGetLastError(), "k_gain_tensor launch");
}

// a float type, the integer type of the samples' own width, or bytes from a deeper three-channel image (the 8-bit finish); nothing else
template <int SB, int C>
int launch_tensor_dtype(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst,
                        const Affine& a, hipStream_t s)
{
  const int rc = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (!std::is_integral<OutT>::value || sizeof(OutT) == SB || (SB == 2 && C == 3)) return launch_tensor<SB, C, OutT>(p, la, ga, src, src_stride, w, rows, dst, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (rc != NO_KERNEL_INSTANCE) return rc;
  return hm_fail(HM_ERR_INTERNAL, "k_gain_tensor: no kernel for dtype %d on %d-byte samples", p->dtype, SB);
}

template <typename InT, typename OutT>
int launch_nearest(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh, uint8_t* dst,
                   const Affine& a, hipStream_t s)
{
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), block(256);
  const int chw = p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0;
  const Light L = light_of(la);
  size_t lds = 0;
  const Gain G = gain_of(ga, light_tables_bytes(la), &lds);
  constexpr bool finish8 = sizeof(InT) == 2 && sizeof(OutT) == 1; // the 8-bit finish of a deeper image: three channels only (check_args)
  if (p->channels == 3)
    hipLaunchKernelGGL((k_gain_nearest<InT, 3, OutT>), grid, block, lds, s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L, G);
  else if constexpr (finish8) return NO_KERNEL_INSTANCE;
  else
    hipLaunchKernelGGL((k_gain_nearest<InT, 4, OutT>), grid, block, lds, s, src, src_stride, n_w, n_h, ow, oh, chw, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L, G);
  return HM_OK;
}

template <typename OutT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, const hm_light_args* la, const hm_gain_args* ga, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->oh + 3) / 4)), block(256);
  const size_t lds = light_v_bytes(la);
  const Light L = light_of(la);
  const Gain G = gain_of(ga, 0, nullptr);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
#define HM_GV_GO(CHW_, C_) \
  hipLaunchKernelGGL((k_gain_v<OutT, CHW_, C_>), grid, block, lds, s, (const float*)r->tmp, (long long)r->tmp_pitch, (long long)r->tmp_plane, r->ow, r->oh, r->ay.first, \
                     r->ay.count, r->ay.weights, (const float*)ga->M, (long long)ga->pitch, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a, L, G)
  if (chw) { if (p->channels == 3) HM_GV_GO(true, 3); else HM_GV_GO(true, 4); }
  else { if (p->channels == 3) HM_GV_GO(false, 3); else HM_GV_GO(false, 4); }
#undef HM_GV_GO
}

// the light step's arguments as light.hip's launchers judge them, then the gain step's
// taps: 0 none (nearest), 1 the records of the pointwise path, 2 the tables of the summed path
int check_args(const hm_dest_plan* p, const hm_light_args* la, const hm_gain_args* ga, int taps)
{
  if (!la->lin || (la->encode && !la->enc) || la->bits < 8 || la->bits > 12) return hm_fail(HM_ERR_INTERNAL, "k_gain: tables of %d bits", la->bits);
  if (la->enc_bits != la->bits && la->enc_bits != 8) return hm_fail(HM_ERR_INTERNAL, "k_gain: codes of %d bits from tables of %d", la->enc_bits, la->bits);
  if (la->src_bytes != (la->bits > 8 ? 2 : 1)) return hm_fail(HM_ERR_INTERNAL, "k_gain: %d-byte samples of %d bits", la->src_bytes, la->bits);
  if (p->channels != 3 && p->channels != 4) return hm_fail(HM_ERR_INTERNAL, "k_gain: %d channels", p->channels);
  if (p->sample_bytes != (la->enc_bits > 8 ? 2 : 1) || (p->sample_bytes != la->src_bytes && p->channels != 3))
    return hm_fail(HM_ERR_INTERNAL, "k_gain: a %d-byte target of %d channels from %d-byte samples, codes of %d bits", p->sample_bytes, p->channels, la->src_bytes, la->enc_bits);
  const bool integer = p->dtype == HM_DEV_U8 || p->dtype == HM_DEV_U16;
  if (integer && (!la->encode || p->dtype != (p->sample_bytes == 1 ? HM_DEV_U8 : HM_DEV_U16)))
    return hm_fail(HM_ERR_INTERNAL, "k_gain: integer dtype %d on %d-byte samples, %s", p->dtype, p->sample_bytes, la->encode ? "re-encoded" : "linear");
  if (!ga->tab || !ga->map || (ga->nch != 1 && ga->nch != 3) || ga->map_bits < 8 || ga->map_bits > HM_GAIN_MAX_BITS || ga->map_bytes != (ga->map_bits > 8 ? 2 : 1) ||
      ga->mw < 1 || ga->mh < 1 || (int64_t)ga->map_stride < (int64_t)ga->mw * ga->map_bytes)
    return hm_fail(HM_ERR_INTERNAL, "k_gain: a map of %d x %d samples of %d bits in %d bytes, stride %d, %d tables", ga->mw, ga->mh, ga->map_bits, ga->map_bytes, ga->map_stride, ga->nch);
  if (taps == 2 && (!ga->ax.first || !ga->ax.count || !ga->ax.weights || !ga->ay.first || !ga->ay.count || !ga->ay.weights)) return hm_fail(HM_ERR_INTERNAL, "k_gain: no tap tables for the map");
  if (taps == 1 && (!ga->xrec || !ga->yrec || (((uintptr_t)ga->xrec | (uintptr_t)ga->yrec) & 15))) return hm_fail(HM_ERR_INTERNAL, "k_gain: no 16-byte aligned tap records for the map");
  return HM_OK;
}

} // namespace

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
  if (la->src_bytes == 1) return p->channels == 3 ? launch_tensor_dtype<1, 3>(p, la, ga, in, src_stride, w, rows, out, a, s) : launch_tensor_dtype<1, 4>(p, la, ga, in, src_stride, w, rows, out, a, s);
  return p->channels == 3 ? launch_tensor_dtype<2, 3>(p, la, ga, in, src_stride, w, rows, out, a, s) : launch_tensor_dtype<2, 4>(p, la, ga, in, src_stride, w, rows, out, a, s);
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
  const bool wide = la->src_bytes == 2;
  // 16-bit elements from 16-bit samples only; bytes from either width (from 16-bit samples: the 8-bit finish); floats from either
  const int found = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if (wide) return launch_nearest<uint16_t, OutT>(p, la, ga, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    if constexpr (!std::is_same<OutT, uint16_t>::value) return launch_nearest<uint8_t, OutT>(p, la, ga, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_gain_nearest: no kernel for dtype %d on %d-byte samples", p->dtype, la->src_bytes);
  return hm_check_hip(hipGetLastError(), "k_gain_nearest launch");
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
  const dim3 grid_h((unsigned)((r->ow + 63) / 64), (unsigned)((ga->mh + 3) / 4), (unsigned)ga->nch), grid_v((unsigned)((r->ow + 63) / 64), (unsigned)((r->oh + 3) / 4), (unsigned)ga->nch);
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
