// resample.hip — a view (hm_device_view) of the colour stage's interleaved pixels into a tensor in caller-owned device memory (gfx950):
// a rectangle of the image, resampled to the size the caller asks for, as u8 / u16 / f16 / f32 in CHW or HWC.
//   k_resample_h     the horizontal pass: rows of the crop -> float32 rows of out_w, a lane per (output column, source row) pair.  The
//                    body is resample_h_body (out_rows.h, where the mapping is described), here with the plain conversion of a sample.
//   k_resample_h_staged  the same sums in the same order for HM_VIEW_CUBIC / HM_VIEW_LANCZOS3 (2 and 3 times the taps): the contiguous run of
//                    source bytes a wave's 64 columns read goes to LDS once, in 16-byte loads, and the lanes take their taps from there.
//   k_resample_v     the vertical pass, fused with dtype, layout, scale and bias: a wave is 64 consecutive element groups of ONE output
//                    row (of one plane), so its taps are wave-uniform and the intermediate reads and the tensor stores coalesce.  A lane's
//                    group is 16 bytes of output (one 16-byte store) where pointer and pitches allow, one element otherwise.
//   k_resample_h_batch, k_resample_h_staged_batch, k_resample_v_batch  the same three passes over the frames of a sequence in one launch
//                    each (grid z): the per-frame pointers come from arrays, everything else is shared.  Same sums, same order, same bytes.
//   k_resample_h_multi, k_resample_h_staged_multi, k_resample_v_multi  the same three passes over MANY views of ONE picture in one launch
//                    each (hm_views_write): blockIdx.y is cut by running sums over the views' row groups, and a workgroup reads crop,
//                    sizes, tap tables, its region of the intermediate and its destination from its view's record.  Same bodies.
//   k_view_nearest   HM_VIEW_NEAREST: the sample at j * n / m is moved (through scale and bias for float destinations), no intermediate.
// The sums run tap by tap in float32 with separately rounded multiply and add (-ffp-contract=off, __fmul_rn / __fadd_rn): a float32
// restatement on the host is exact.  A sum becomes an element by `finish`, a sample that is only moved by `moved` (out_elem.h).
// Nothing but the out_w x out_h x C elements of the view is ever stored.
#include "hm_devdest.h"
#include "hm_view_batch.h"
#include "hm_view_multi.h"
#include "out_launch.h"
#include "out_rows.h"

namespace {

// A pointer a kernel loads from memory is a generic one to the compiler (a kernel argument is known to point to global memory):
// the batched kernels read their per-frame pointers as pointers to global memory, so that the loads and stores through them are
// the global ones of the unbatched kernels, not flat ones that might alias LDS.
typedef __attribute__((address_space(1))) uint8_t GlobalBytes;

// resample_h_body (out_rows.h) with the plain conversion of a sample
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_resample_h(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                    const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                    long long pitch, long long plane)
{
  resample_h_body<SB, C, CHW>(src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, SampleToFloat());
}

// The batched form (hm_view_write_batch: the frames of a sequence under one view): blockIdx.z is the frame within the chunk.  Its
// source origin comes from the pointer array - one read per workgroup at an address that depends on blockIdx.z alone, so a scalar
// load into SGPRs, made once, before the tap loop - and its rows of the intermediate lie frame_stride elements behind the frame
// before.  Everything else, the order of the sum included, is k_resample_h's.
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_resample_h_batch(const uint8_t* const* __restrict__ srcs, int src_stride, int n_h, int ow,
                                                          const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                          const float* __restrict__ wts, float* __restrict__ tmp, long long pitch, long long plane,
                                                          long long frame_stride)
{
  const uint8_t* src = (const uint8_t*)(const GlobalBytes*)reinterpret_cast<const uintptr_t*>(srcs)[blockIdx.z];
  resample_h_body<SB, C, CHW>(src, src_stride, n_h, ow, first, count, wts, tmp + (long long)blockIdx.z * frame_stride, pitch, plane, SampleToFloat());
}

// k_resample_h with the source run staged in LDS.  The 64 columns of a wave read the pixels first[c0] .. first[c63] + count[c63] of
// their row: one contiguous run (the windows' ends do not fall as the column rises: hm_view_write checks the table).  A workgroup is
// four waves on four consecutive rows of the same 64 columns, so the run's extent - and with it every trip count and barrier below -
// is the same in all of them.  Per chunk of at most chunk_px pixels each wave loads its row's bytes with 16-byte loads from the
// 16-byte-aligned addresses inside the chunk (the partial units at its head and tail byte by byte: nothing outside the run is
// read) into its own quarter of the LDS array, then every lane takes those of its taps that lie in the chunk, tap 0 first: chunks
// and taps both rise, so the order of a lane's sum is that of k_resample_h and the result is the same bit for bit.
// LDS image of a row: byte b of the chunk, counted from the aligned address below its first byte, sits at b + 4 * (b / 128) - one
// pad dword behind every 32 -, so lanes whose windows start 64, 128 or 256 bytes apart meet 32 different banks, not 2 or 1.
constexpr int STAGE_DATA = 3712;                          // bytes of a row's chunk, alignment head included (a multiple of 128)
constexpr int STAGE_ROW = STAGE_DATA + STAGE_DATA / 32;   // ... with the pad dwords: 3828
constexpr int STAGE_ROW_PITCH = 3840;                     // 4 rows = 15 360 B = 12 of gfx950's 1 280-byte LDS granules
static_assert(STAGE_ROW <= STAGE_ROW_PITCH && STAGE_DATA % 128 == 0 && STAGE_ROW_PITCH % 16 == 0, "LDS image of a staged row");
__device__ __forceinline__ int stage_at(int b) { return b + ((b >> 7) << 2); }

template <int SB, int C, bool CHW>
__device__ __forceinline__ void resample_h_staged_body(int by, uint8_t* lds, const uint8_t* __restrict__ src, int src_stride, int n_h, int ow,
                                                       const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                       float* __restrict__ tmp, long long pitch, long long plane, int chunk_px)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int PB = SB * C; // bytes per pixel
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64, j = j0 + lane, y = by * 4 + wv; // (by: blockIdx.y, or the row group inside its view: k_resample_h_staged_multi)
  const int jl = min(j0 + 63, ow - 1);
  const int p_end = first[jl] + count[jl]; // (the same in every lane of the workgroup, as p below)
  int p = first[j0];
  const bool row = y < n_h, col = j < ow;
  const int fj = col ? first[j] : 0, nj = col ? count[j] : 0;
  uint8_t* buf = lds + wv * STAGE_ROW_PITCH;
  const uint8_t* rowp = src + (size_t)(row ? y : 0) * src_stride;
  float t[C];
#pragma unroll
  for (int c = 0; c < C; c++) t[c] = 0.0f;
  while (p < p_end) {
    const int q = min(p_end, p + chunk_px); // pixels [p, q) of the row: (q - p) * PB + 15 <= STAGE_DATA (the launcher)
    const uint8_t* a = rowp + (size_t)p * PB;
    const int head = (int)((uintptr_t)a & 15);
    if (row) {
      const uint8_t* g = a - head;               // LDS byte b = the byte at g + b; the run is b in [head, total)
      const int total = head + (q - p) * PB;
      const int u1 = total >> 4;                 // 16-byte units [head ? 1 : 0, u1) lie inside the run
#pragma unroll 4
      for (int u = (head ? 1 : 0) + lane; u < u1; u += 64) {
        const uint4 v = *reinterpret_cast<const uint4*>(g + 16 * u);
        uint32_t* o = reinterpret_cast<uint32_t*>(buf + stage_at(16 * u)); // (a unit never straddles a pad)
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
      if (lane < 16) { // the partial unit at the head
        if (head && lane >= head && lane < total) buf[stage_at(lane)] = g[lane];
      }
      else if (lane < 32) { // ... and at the tail
        const int b = 16 * u1 + lane - 16;
        if (b >= head && b < total) buf[stage_at(b)] = g[b];
      }
    }
    __syncthreads();
    if (row && col) {
      const int i0 = max(0, p - fj), i1 = min(nj, q - fj);
      constexpr int G = C == 4 ? 2 : 4; // taps whose weights and samples are in flight together (at most 64 VGPRs), summed in the taps' order
      int i = i0;
      for (; i + G <= i1; i += G) {
        float w[G];
        InT v[G][C];
#pragma unroll
        for (int k = 0; k < G; k++) w[k] = wts[(size_t)(i + k) * ow + j];
#pragma unroll
        for (int k = 0; k < G; k++) {
          const int b = head + (fj + i + k - p) * PB;
#pragma unroll
          for (int c = 0; c < C; c++) v[k][c] = *reinterpret_cast<const InT*>(buf + stage_at(b + c * SB));
        }
#pragma unroll
        for (int k = 0; k < G; k++) {
#pragma unroll
          for (int c = 0; c < C; c++) t[c] = __fadd_rn(t[c], __fmul_rn(w[k], (float)v[k][c]));
        }
      }
      for (; i < i1; i++) {
        const float w = wts[(size_t)i * ow + j];
        const int b = head + (fj + i - p) * PB;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const InT v = *reinterpret_cast<const InT*>(buf + stage_at(b + c * SB));
          t[c] = __fadd_rn(t[c], __fmul_rn(w, (float)v));
        }
      }
    }
    __syncthreads();
    p = q;
  }
  if (!row || !col) return;
  float* o = tmp + (long long)y * pitch;
#pragma unroll
  for (int c = 0; c < C; c++) {
    if (CHW) o[(long long)c * plane + j] = t[c];
    else o[(size_t)j * C + c] = t[c];
  }
}

template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_resample_h_staged(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                           const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                           long long pitch, long long plane, int chunk_px)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * STAGE_ROW_PITCH];
  resample_h_staged_body<SB, C, CHW>((int)blockIdx.y, lds, src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, chunk_px);
}

// The batched form: blockIdx.z is the frame within the chunk, its source origin a scalar load from the pointer array before
// anything else, its intermediate frame_stride elements behind the frame before (as k_resample_h_batch).  The barriers stay
// uniform: the extent of the run, the chunks it is cut into and so every trip count depend on the workgroup's 64 columns
// (first[], count[], chunk_px) alone, which all frames share - blockIdx.z enters the addresses only, and a workgroup lies inside
// one frame.  (The alignment head of a chunk depends on the frame's source address; it moves bytes inside the LDS image, not a
// trip count: a chunk fits behind the longest head, 15 bytes, whatever the address.)
// waves_per_eu(8): without the hint the compiler schedules this form into 78-80 VGPRs (6 waves per SIMD); with it into 49-56,
// the staged kernel's own budget, still without scratch.
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_resample_h_staged_batch(const uint8_t* const* __restrict__ srcs, int src_stride, int n_h, int ow,
                                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                                 const float* __restrict__ wts, float* __restrict__ tmp, long long pitch, long long plane,
                                                                 int chunk_px, long long frame_stride)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * STAGE_ROW_PITCH];
  const uint8_t* src = (const uint8_t*)(const GlobalBytes*)reinterpret_cast<const uintptr_t*>(srcs)[blockIdx.z];
  resample_h_staged_body<SB, C, CHW>((int)blockIdx.y, lds, src, src_stride, n_h, ow, first, count, wts, tmp + (long long)blockIdx.z * frame_stride, pitch, plane, chunk_px);
}

// P: elements of one row per lane (16 bytes of output, or 1), C: channels of an interleaved row (HWC), 0 = one plane per channel
// (CHW: blockIdx.z is the channel).  E: elements per row (out_w, or out_w * C).  grid: x = groups of 64 lanes, y = groups of 4
// output rows, z = planes.  The intermediate's pitch is a multiple of 16 elements, so a ragged last group loads whole vectors
// (of padding nobody stores).
template <typename OutT, int P, int C>
__device__ __forceinline__ void resample_v_body(int by, int pl, const float* __restrict__ tmp, long long pitch, long long plane, int E, int oh,
                                                const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, const Affine& a)
{
  const int k = by * 4 + (threadIdx.x >> 6); // (by: blockIdx.y, or the row group inside its view: k_resample_v_multi)
  if (k >= oh) return;
  const int e0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * P;
  if (e0 >= E) return;
  const int y0 = first[k], n = count[k]; // (the same in every lane of the wave)
  const float* col = tmp + (long long)pl * plane + (long long)y0 * pitch + e0;
  float acc[P];
#pragma unroll
  for (int q = 0; q < P; q++) acc[q] = 0.0f;
  for (int i = 0; i < n; i++) {
    const float w = wts[(size_t)i * oh + k];
    float v[P];
    if constexpr (P == 1) v[0] = col[0];
    else {
#pragma unroll
      for (int q = 0; q < P / 4; q++) {
        const float4 f = reinterpret_cast<const float4*>(col)[q];
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
      }
    }
#pragma unroll
    for (int q = 0; q < P; q++) acc[q] = __fadd_rn(acc[q], __fmul_rn(w, v[q]));
    col += pitch;
  }
  OutT o[P];
#pragma unroll
  for (int q = 0; q < P; q++) {
    const int c = C == 0 ? pl : (e0 + q) % (C == 0 ? 1 : C);
    o[q] = finish<OutT>(acc[q], a.scale[c], a.bias[c], full_peak<OutT>());
  }
  OutT* op = reinterpret_cast<OutT*>(dst + (long long)pl * plane_pitch + (long long)k * row_pitch) + e0;
  if constexpr (P > 1)
    if (e0 + P <= E) {
      store16(op, o);
      return;
    }
  const int left = E - e0 < P ? E - e0 : P;
  for (int q = 0; q < left; q++) op[q] = o[q];
}

template <typename OutT, int P, int C>
__global__ __launch_bounds__(256) void k_resample_v(const float* __restrict__ tmp, long long pitch, long long plane, int E, int oh,
                                                    const int32_t* __restrict__ first, const int32_t* __restrict__ count, const float* __restrict__ wts,
                                                    uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a)
{
  resample_v_body<OutT, P, C>((int)blockIdx.y, (int)blockIdx.z, tmp, pitch, plane, E, oh, first, count, wts, dst, row_pitch, plane_pitch, a);
}

// The batched form: blockIdx.z = frame * planes + plane (planes: the channels of a CHW destination, 1 for HWC).  The frame's
// destination comes from the pointer array (a scalar load: the address depends on blockIdx.z alone), its intermediate lies
// frame_stride elements behind the frame before.  Pitches, scale, bias and the store width P are those of the whole launch:
// hm_view_write_batch groups frames by them.
template <typename OutT, int P, int C>
__global__ __launch_bounds__(256) void k_resample_v_batch(const float* __restrict__ tmp, long long pitch, long long plane, int E, int oh,
                                                          const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                          const float* __restrict__ wts, uint8_t* const* __restrict__ dsts, long long row_pitch,
                                                          long long plane_pitch, Affine a, int planes, long long frame_stride)
{
  int fr = blockIdx.z, pl = 0;
  if (C == 0) hm_view_z_split((int)blockIdx.z, planes, &fr, &pl);
  uint8_t* dst = (uint8_t*)(GlobalBytes*)reinterpret_cast<const uintptr_t*>(dsts)[fr];
  resample_v_body<OutT, P, C>((int)blockIdx.y, pl, tmp + (long long)fr * frame_stride, pitch, plane, E, oh, first, count, wts, dst, row_pitch, plane_pitch, a);
}

// ---- many views of one picture (hm_views_write): the multi forms ----
// A launch covers the views of one chunk.  `block` is the group's block (hm_view_multi.h): the tap tables of every view, the records,
// the running sums; recs and sums point at the chunk's first record and first sum, n is its view count.  blockIdx.y runs over the row
// groups of all the chunk's views one behind the other; hm_view_of_y finds the view by bisection over the sums.  That search, and the
// record's address, depend on blockIdx.y alone: the loads are scalar ones into SGPRs, made once per workgroup, before the tap loop
// (the reasoning of k_resample_h_batch).  The pointers inside a record are read as pointers to global memory (GlobalBytes), so the
// loads and stores through them stay global ones.  blockIdx.x is sized for the widest view of the chunk: the workgroups beyond their
// own view's width return before any load.
struct MultiView { const hm_view_rec* r; int by; };
__device__ __forceinline__ MultiView multi_view_of(const hm_view_rec* __restrict__ recs, const int32_t* __restrict__ sums, int n)
{
  int32_t local;
  const int v = hm_view_of_y(sums, n, (int32_t)blockIdx.y, &local);
  return MultiView{recs + v, (int)local};
}

template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) void k_resample_h_multi(const int32_t* __restrict__ block, const hm_view_rec* __restrict__ recs, const int32_t* __restrict__ sums, int n,
                                                          int src_stride, float* __restrict__ tmp)
{
  const MultiView m = multi_view_of(recs, sums, n);
  const hm_view_rec* r = m.r;
  const int ow = r->ow;
  if ((int)blockIdx.x * 64 >= ow) return;
  const uint8_t* src = (const uint8_t*)(const GlobalBytes*)r->src;
  resample_h_rows<SB, C, CHW>(m.by, src, src_stride, r->n_h, ow, block + r->x_first, block + r->x_count, reinterpret_cast<const float*>(block + r->x_weights),
                              tmp + r->tmp_off, r->tmp_pitch, r->tmp_plane, SampleToFloat());
}

// The staged body has barriers: its early return must be taken by the whole workgroup or by none of it.  A workgroup is four rows of
// the SAME 64 columns (blockIdx.x * 64 ..), and its view is one (blockIdx.y decides it): the condition below is workgroup-uniform.
// Behind it the trip counts depend on the workgroup's columns and its view's tables alone, as in k_resample_h_staged.
// waves_per_eu(8): as k_resample_h_staged_batch.
template <int SB, int C, bool CHW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_resample_h_staged_multi(const int32_t* __restrict__ block, const hm_view_rec* __restrict__ recs,
                                                                 const int32_t* __restrict__ sums, int n, int src_stride, float* __restrict__ tmp, int chunk_px)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * STAGE_ROW_PITCH];
  const MultiView m = multi_view_of(recs, sums, n);
  const hm_view_rec* r = m.r;
  const int ow = r->ow;
  if ((int)blockIdx.x * 64 >= ow) return;
  const uint8_t* src = (const uint8_t*)(const GlobalBytes*)r->src;
  resample_h_staged_body<SB, C, CHW>(m.by, lds, src, src_stride, r->n_h, ow, block + r->x_first, block + r->x_count, reinterpret_cast<const float*>(block + r->x_weights),
                                     tmp + r->tmp_off, r->tmp_pitch, r->tmp_plane, chunk_px);
}

// blockIdx.z is the channel for CHW destinations (C == 0), as in k_resample_v.  Scale, bias and the store width P are those of the
// whole launch: hm_views_write groups views by them.
template <typename OutT, int P, int C>
__global__ __launch_bounds__(256) void k_resample_v_multi(const int32_t* __restrict__ block, const hm_view_rec* __restrict__ recs, const int32_t* __restrict__ sums, int n,
                                                          const float* __restrict__ tmp, Affine a)
{
  const MultiView m = multi_view_of(recs, sums, n);
  const hm_view_rec* r = m.r;
  const int E = r->E;
  if ((int)blockIdx.x * 64 * P >= E) return;
  uint8_t* dst = (uint8_t*)(GlobalBytes*)r->dst;
  resample_v_body<OutT, P, C>(m.by, (int)blockIdx.z, tmp + r->tmp_off, r->tmp_pitch, r->tmp_plane, E, r->oh, block + r->y_first, block + r->y_count,
                              reinterpret_cast<const float*>(block + r->y_weights), dst, r->row_pitch, r->plane_pitch, a);
}

// HM_VIEW_NEAREST: out pixel (j, k) is source pixel (j * n_w / ow, k * n_h / oh).  grid: x = groups of 64 columns, y = groups of 4 rows.
template <typename InT, typename OutT>
__global__ __launch_bounds__(256) void k_view_nearest(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, int C, int chw,
                                                      uint8_t* __restrict__ dst, long long row_pitch, long long plane_pitch, Affine a)
{
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * C;
  uint8_t* orow = dst + (long long)k * row_pitch;
  for (int c = 0; c < C; c++) {
    const OutT o = moved<OutT>(in[c], a.scale[c], a.bias[c]);
    *elem_at<OutT>(orow, chw, plane_pitch, j, c, C) = o;
  }
}

#define HM_V_SET(T) \
  (const void*)k_resample_v<T, 16 / (int)sizeof(T), 0>, (const void*)k_resample_v<T, 16 / (int)sizeof(T), 3>, (const void*)k_resample_v<T, 16 / (int)sizeof(T), 4>, \
  (const void*)k_resample_v<T, 1, 0>, (const void*)k_resample_v<T, 1, 3>, (const void*)k_resample_v<T, 1, 4>
// every instance the launchers below can pick (hm_debug_kernel_regs)
const void* const g_instances[] = {
  (const void*)k_resample_h<1, 3, true>, (const void*)k_resample_h<1, 3, false>, (const void*)k_resample_h<1, 4, true>, (const void*)k_resample_h<1, 4, false>,
  (const void*)k_resample_h<2, 3, true>, (const void*)k_resample_h<2, 3, false>, (const void*)k_resample_h<2, 4, true>, (const void*)k_resample_h<2, 4, false>,
  HM_V_SET(uint8_t), HM_V_SET(uint16_t), HM_V_SET(__half), HM_V_SET(float),
  (const void*)k_view_nearest<uint8_t, uint8_t>, (const void*)k_view_nearest<uint8_t, __half>, (const void*)k_view_nearest<uint8_t, float>,
  (const void*)k_view_nearest<uint16_t, uint16_t>, (const void*)k_view_nearest<uint16_t, __half>, (const void*)k_view_nearest<uint16_t, float>,
};
#undef HM_V_SET
// ... and of the staged horizontal pass, a list of its own (hm_debug_kernel_regs, code 5)
const void* const g_staged_instances[] = {
  (const void*)k_resample_h_staged<1, 3, true>, (const void*)k_resample_h_staged<1, 3, false>, (const void*)k_resample_h_staged<1, 4, true>, (const void*)k_resample_h_staged<1, 4, false>,
  (const void*)k_resample_h_staged<2, 3, true>, (const void*)k_resample_h_staged<2, 3, false>, (const void*)k_resample_h_staged<2, 4, true>, (const void*)k_resample_h_staged<2, 4, false>,
};

// ... and of the batched forms (hm_view_write_batch), a list of its own (hm_debug_kernel_regs, code 6): 8 horizontal, 8 staged, 24 vertical
#define HM_VB_SET(T) \
  (const void*)k_resample_v_batch<T, 16 / (int)sizeof(T), 0>, (const void*)k_resample_v_batch<T, 16 / (int)sizeof(T), 3>, (const void*)k_resample_v_batch<T, 16 / (int)sizeof(T), 4>, \
  (const void*)k_resample_v_batch<T, 1, 0>, (const void*)k_resample_v_batch<T, 1, 3>, (const void*)k_resample_v_batch<T, 1, 4>
const void* const g_batch_instances[] = {
  (const void*)k_resample_h_batch<1, 3, true>, (const void*)k_resample_h_batch<1, 3, false>, (const void*)k_resample_h_batch<1, 4, true>, (const void*)k_resample_h_batch<1, 4, false>,
  (const void*)k_resample_h_batch<2, 3, true>, (const void*)k_resample_h_batch<2, 3, false>, (const void*)k_resample_h_batch<2, 4, true>, (const void*)k_resample_h_batch<2, 4, false>,
  (const void*)k_resample_h_staged_batch<1, 3, true>, (const void*)k_resample_h_staged_batch<1, 3, false>, (const void*)k_resample_h_staged_batch<1, 4, true>, (const void*)k_resample_h_staged_batch<1, 4, false>,
  (const void*)k_resample_h_staged_batch<2, 3, true>, (const void*)k_resample_h_staged_batch<2, 3, false>, (const void*)k_resample_h_staged_batch<2, 4, true>, (const void*)k_resample_h_staged_batch<2, 4, false>,
  HM_VB_SET(uint8_t), HM_VB_SET(uint16_t), HM_VB_SET(__half), HM_VB_SET(float),
};
#undef HM_VB_SET

// ... and of the multi forms (hm_views_write), a list of its own (hm_debug_kernel_regs, code 14): 8 horizontal, 8 staged, 24 vertical
#define HM_VM_SET(T) \
  (const void*)k_resample_v_multi<T, 16 / (int)sizeof(T), 0>, (const void*)k_resample_v_multi<T, 16 / (int)sizeof(T), 3>, (const void*)k_resample_v_multi<T, 16 / (int)sizeof(T), 4>, \
  (const void*)k_resample_v_multi<T, 1, 0>, (const void*)k_resample_v_multi<T, 1, 3>, (const void*)k_resample_v_multi<T, 1, 4>
const void* const g_multi_instances[] = {
  (const void*)k_resample_h_multi<1, 3, true>, (const void*)k_resample_h_multi<1, 3, false>, (const void*)k_resample_h_multi<1, 4, true>, (const void*)k_resample_h_multi<1, 4, false>,
  (const void*)k_resample_h_multi<2, 3, true>, (const void*)k_resample_h_multi<2, 3, false>, (const void*)k_resample_h_multi<2, 4, true>, (const void*)k_resample_h_multi<2, 4, false>,
  (const void*)k_resample_h_staged_multi<1, 3, true>, (const void*)k_resample_h_staged_multi<1, 3, false>, (const void*)k_resample_h_staged_multi<1, 4, true>, (const void*)k_resample_h_staged_multi<1, 4, false>,
  (const void*)k_resample_h_staged_multi<2, 3, true>, (const void*)k_resample_h_staged_multi<2, 3, false>, (const void*)k_resample_h_staged_multi<2, 4, true>, (const void*)k_resample_h_staged_multi<2, 4, false>,
  HM_VM_SET(uint8_t), HM_VM_SET(uint16_t), HM_VM_SET(__half), HM_VM_SET(float),
};
#undef HM_VM_SET

template <int SB, int C>
void launch_h(bool chw, const hm_resample_args* r, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->n_h + 3) / 4)), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  if (chw)
    hipLaunchKernelGGL((k_resample_h<SB, C, true>), grid, block, 0, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane);
  else
    hipLaunchKernelGGL((k_resample_h<SB, C, false>), grid, block, 0, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane);
}

template <int SB, int C>
void launch_h_staged(bool chw, const hm_resample_args* r, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->n_h + 3) / 4)), block(256);
  const uint8_t* src = (const uint8_t*)r->src;
  constexpr int most = (STAGE_DATA - 15) / (SB * C); // pixels of a chunk behind the longest alignment head
  const int chunk_px = r->stage_px > 0 && r->stage_px < most ? r->stage_px : most;
  if (chw)
    hipLaunchKernelGGL((k_resample_h_staged<SB, C, true>), grid, block, 0, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, chunk_px);
  else
    hipLaunchKernelGGL((k_resample_h_staged<SB, C, false>), grid, block, 0, s, src, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, chunk_px);
}

template <typename OutT, int P, int C>
void launch_v_inst(const hm_dest_plan* p, const hm_resample_args* r, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const int E = C == 0 ? r->ow : r->ow * C, groups = (E + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((r->oh + 3) / 4), (unsigned)(C == 0 ? p->channels : 1)), block(256);
  hipLaunchKernelGGL((k_resample_v<OutT, P, C>), grid, block, 0, s, (const float*)r->tmp, (long long)r->tmp_pitch, (long long)r->tmp_plane, E, r->oh, r->ay.first,
                     r->ay.count, r->ay.weights, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a);
}

template <typename OutT>
void launch_v(const hm_dest_plan* p, const hm_resample_args* r, uint8_t* dst, const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  const bool vec = ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 && (!chw || (p->plane_pitch % 16) == 0);
  if (chw) { if (vec) launch_v_inst<OutT, P, 0>(p, r, dst, a, s); else launch_v_inst<OutT, 1, 0>(p, r, dst, a, s); }
  else if (p->channels == 3) { if (vec) launch_v_inst<OutT, P, 3>(p, r, dst, a, s); else launch_v_inst<OutT, 1, 3>(p, r, dst, a, s); }
  else { if (vec) launch_v_inst<OutT, P, 4>(p, r, dst, a, s); else launch_v_inst<OutT, 1, 4>(p, r, dst, a, s); }
}

template <typename InT, typename OutT>
int launch_nearest(const hm_dest_plan* p, const uint8_t* src, int src_stride, int n_w, int n_h, int ow, int oh, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), block(256);
  hipLaunchKernelGGL((k_view_nearest<InT, OutT>), grid, block, 0, s, src, src_stride, n_w, n_h, ow, oh, p->channels, p->layout == HM_DEV_LAYOUT_CHW ? 1 : 0, dst,
                     (long long)p->row_pitch, (long long)p->plane_pitch, a);
  return HM_OK;
}

// the batched launches: grid z = the frames of the chunk (horizontal), frames x planes (vertical)
template <int SB, int C>
void launch_h_batch(bool chw, const hm_resample_args* r, const hm_resample_batch* b, hipStream_t s)
{
  const dim3 grid((unsigned)((r->ow + 63) / 64), (unsigned)((r->n_h + 3) / 4), (unsigned)b->frames), block(256);
  const uint8_t* const* srcs = (const uint8_t* const*)b->srcs;
  if (r->staged) {
    constexpr int most = (STAGE_DATA - 15) / (SB * C); // (as launch_h_staged)
    const int chunk_px = r->stage_px > 0 && r->stage_px < most ? r->stage_px : most;
    if (chw)
      hipLaunchKernelGGL((k_resample_h_staged_batch<SB, C, true>), grid, block, 0, s, srcs, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                         (long long)r->tmp_pitch, (long long)r->tmp_plane, chunk_px, (long long)b->frame_stride);
    else
      hipLaunchKernelGGL((k_resample_h_staged_batch<SB, C, false>), grid, block, 0, s, srcs, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                         (long long)r->tmp_pitch, (long long)r->tmp_plane, chunk_px, (long long)b->frame_stride);
  }
  else if (chw)
    hipLaunchKernelGGL((k_resample_h_batch<SB, C, true>), grid, block, 0, s, srcs, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, (long long)b->frame_stride);
  else
    hipLaunchKernelGGL((k_resample_h_batch<SB, C, false>), grid, block, 0, s, srcs, r->src_stride, r->n_h, r->ow, r->ax.first, r->ax.count, r->ax.weights, r->tmp,
                       (long long)r->tmp_pitch, (long long)r->tmp_plane, (long long)b->frame_stride);
}

template <typename OutT, int P, int C>
void launch_v_batch_inst(const hm_dest_plan* p, const hm_resample_args* r, const hm_resample_batch* b, const Affine& a, hipStream_t s)
{
  const int E = C == 0 ? r->ow : r->ow * C, groups = (E + P - 1) / P, planes = C == 0 ? p->channels : 1;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((r->oh + 3) / 4), (unsigned)(b->frames * planes)), block(256);
  hipLaunchKernelGGL((k_resample_v_batch<OutT, P, C>), grid, block, 0, s, (const float*)r->tmp, (long long)r->tmp_pitch, (long long)r->tmp_plane, E, r->oh, r->ay.first,
                     r->ay.count, r->ay.weights, (uint8_t* const*)b->dsts, (long long)p->row_pitch, (long long)p->plane_pitch, a, planes, (long long)b->frame_stride);
}

template <typename OutT>
void launch_v_batch(const hm_dest_plan* p, const hm_resample_args* r, const hm_resample_batch* b, const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW, vec = b->vec != 0;
  if (chw) { if (vec) launch_v_batch_inst<OutT, P, 0>(p, r, b, a, s); else launch_v_batch_inst<OutT, 1, 0>(p, r, b, a, s); }
  else if (p->channels == 3) { if (vec) launch_v_batch_inst<OutT, P, 3>(p, r, b, a, s); else launch_v_batch_inst<OutT, 1, 3>(p, r, b, a, s); }
  else { if (vec) launch_v_batch_inst<OutT, P, 4>(p, r, b, a, s); else launch_v_batch_inst<OutT, 1, 4>(p, r, b, a, s); }
}

// the multi launches: grid x = the widest view of the chunk, y = the row groups of all its views, z = planes (vertical, CHW)
template <int SB, int C>
void launch_h_multi(bool chw, const hm_resample_multi* m, hipStream_t s)
{
  const dim3 grid((unsigned)((m->ow_most + 63) / 64), (unsigned)m->h_groups), block(256);
  const int32_t* blk = (const int32_t*)m->block;
  const hm_view_rec* recs = (const hm_view_rec*)m->recs;
  if (m->staged) {
    constexpr int most = (STAGE_DATA - 15) / (SB * C); // (as launch_h_staged)
    const int chunk_px = m->stage_px > 0 && m->stage_px < most ? m->stage_px : most;
    if (chw) hipLaunchKernelGGL((k_resample_h_staged_multi<SB, C, true>), grid, block, 0, s, blk, recs, m->hsums, m->views, m->src_stride, m->tmp, chunk_px);
    else hipLaunchKernelGGL((k_resample_h_staged_multi<SB, C, false>), grid, block, 0, s, blk, recs, m->hsums, m->views, m->src_stride, m->tmp, chunk_px);
  }
  else if (chw) hipLaunchKernelGGL((k_resample_h_multi<SB, C, true>), grid, block, 0, s, blk, recs, m->hsums, m->views, m->src_stride, m->tmp);
  else hipLaunchKernelGGL((k_resample_h_multi<SB, C, false>), grid, block, 0, s, blk, recs, m->hsums, m->views, m->src_stride, m->tmp);
}

template <typename OutT, int P, int C>
void launch_v_multi_inst(const hm_dest_plan* p, const hm_resample_multi* m, const Affine& a, hipStream_t s)
{
  const int groups = (m->E_most + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)m->v_groups, (unsigned)(C == 0 ? p->channels : 1)), block(256);
  hipLaunchKernelGGL((k_resample_v_multi<OutT, P, C>), grid, block, 0, s, (const int32_t*)m->block, (const hm_view_rec*)m->recs, m->vsums, m->views, (const float*)m->tmp, a);
}

template <typename OutT>
void launch_v_multi(const hm_dest_plan* p, const hm_resample_multi* m, const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW, vec = m->vec != 0;
  if (chw) { if (vec) launch_v_multi_inst<OutT, P, 0>(p, m, a, s); else launch_v_multi_inst<OutT, 1, 0>(p, m, a, s); }
  else if (p->channels == 3) { if (vec) launch_v_multi_inst<OutT, P, 3>(p, m, a, s); else launch_v_multi_inst<OutT, 1, 3>(p, m, a, s); }
  else { if (vec) launch_v_multi_inst<OutT, P, 4>(p, m, a, s); else launch_v_multi_inst<OutT, 1, 4>(p, m, a, s); }
}

} // namespace

extern "C" const void* hm_resample_multi_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_multi_instances) / sizeof(g_multi_instances[0])) ? g_multi_instances[index] : nullptr;
}

extern "C" const void* hm_resample_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

extern "C" const void* hm_resample_staged_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_staged_instances) / sizeof(g_staged_instances[0])) ? g_staged_instances[index] : nullptr;
}

extern "C" const void* hm_resample_batch_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_batch_instances) / sizeof(g_batch_instances[0])) ? g_batch_instances[index] : nullptr;
}

// both passes of a resampled view; `dst` = the destination's first element.  The intermediate is laid out like the destination
// (r->tmp_plane apart per channel for CHW, interleaved rows for HWC), its pitch a multiple of 16 elements.
extern "C" int hm_launch_resample(const hm_dest_plan* p, const hm_resample_args* r, void* dst, const float scale[4], const float bias[4], hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0) return HM_OK;
  if ((r->tmp_pitch % 16) || (r->tmp_plane % 4) || ((uintptr_t)r->tmp % 16)) return hm_fail(HM_ERR_INTERNAL, "k_resample: misaligned intermediate");
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  if (r->staged) {
    if (r->sample_bytes == 1) { if (r->channels == 3) launch_h_staged<1, 3>(chw, r, s); else launch_h_staged<1, 4>(chw, r, s); }
    else { if (r->channels == 3) launch_h_staged<2, 3>(chw, r, s); else launch_h_staged<2, 4>(chw, r, s); }
  }
  else if (r->sample_bytes == 1) { if (r->channels == 3) launch_h<1, 3>(chw, r, s); else launch_h<1, 4>(chw, r, s); }
  else { if (r->channels == 3) launch_h<2, 3>(chw, r, s); else launch_h<2, 4>(chw, r, s); }
  int rc = hm_check_hip(hipGetLastError(), "k_resample_h launch");
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  uint8_t* out = (uint8_t*)dst;
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v<typename decltype(tag)::type>(p, r, out, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_resample_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_resample_v launch");
}

// both passes over the b->frames frames of one chunk (hm_view_write_batch): r->src is not looked at, r->tmp is the chunk's
// intermediate (b->frame_stride elements per frame), p the plan every frame of the group shares
extern "C" int hm_launch_resample_batch(const hm_dest_plan* p, const hm_resample_args* r, const hm_resample_batch* b, const float scale[4], const float bias[4],
                                        hipStream_t s)
{
  if (r->ow <= 0 || r->oh <= 0 || r->n_w <= 0 || r->n_h <= 0 || b->frames <= 0) return HM_OK;
  if ((r->tmp_pitch % 16) || (r->tmp_plane % 4) || (b->frame_stride % 4) || ((uintptr_t)r->tmp % 16)) return hm_fail(HM_ERR_INTERNAL, "k_resample: misaligned intermediate");
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  if ((int64_t)b->frames * (chw ? p->channels : 1) > 65535) return hm_fail(HM_ERR_INTERNAL, "k_resample: %d frames in one launch", b->frames);
  if (r->sample_bytes == 1) { if (r->channels == 3) launch_h_batch<1, 3>(chw, r, b, s); else launch_h_batch<1, 4>(chw, r, b, s); }
  else { if (r->channels == 3) launch_h_batch<2, 3>(chw, r, b, s); else launch_h_batch<2, 4>(chw, r, b, s); }
  int rc = hm_check_hip(hipGetLastError(), "k_resample_h_batch launch");
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v_batch<typename decltype(tag)::type>(p, r, b, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_resample_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_resample_v_batch launch");
}

// both passes over the m->views views of one chunk (hm_views_write): p is the plan of any view of the group - layout, dtype and channels
// are the group's, its pitches are not looked at (the records hold every view's)
extern "C" int hm_launch_resample_multi(const hm_dest_plan* p, const hm_resample_multi* m, const float scale[4], const float bias[4], hipStream_t s)
{
  if (m->views <= 0) return HM_OK;
  if (m->h_groups <= 0 || m->v_groups <= 0 || m->h_groups > HM_VIEW_MULTI_Y_MOST || m->v_groups > HM_VIEW_MULTI_Y_MOST || m->ow_most <= 0 || m->E_most <= 0)
    return hm_fail(HM_ERR_INTERNAL, "k_resample_multi: %d and %d row groups in one launch", m->h_groups, m->v_groups);
  if (((uintptr_t)m->tmp % 16) || ((uintptr_t)m->recs % 8) || ((uintptr_t)m->block % 8)) return hm_fail(HM_ERR_INTERNAL, "k_resample_multi: misaligned block or intermediate");
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  if (m->sample_bytes == 1) { if (m->channels == 3) launch_h_multi<1, 3>(chw, m, s); else launch_h_multi<1, 4>(chw, m, s); }
  else { if (m->channels == 3) launch_h_multi<2, 3>(chw, m, s); else launch_h_multi<2, 4>(chw, m, s); }
  int rc = hm_check_hip(hipGetLastError(), "k_resample_h_multi launch");
  if (rc) return rc;
  const Affine a = affine_of(scale, bias);
  const int found = with_dtype(p->dtype, [&](auto tag) -> int { launch_v_multi<typename decltype(tag)::type>(p, m, a, s); return HM_OK; });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_resample_v: no kernel for dtype %d", p->dtype);
  return hm_check_hip(hipGetLastError(), "k_resample_v_multi launch");
}

extern "C" int hm_launch_view_nearest(const hm_dest_plan* p, const void* src, int src_stride, int n_w, int n_h, int ow, int oh, void* dst, const float scale[4],
                                      const float bias[4], hipStream_t s)
{
  if (ow <= 0 || oh <= 0) return HM_OK;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  const bool wide = p->sample_bytes == 2;
  // an integer element from samples of its own width only; floats from either
  const int found = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (!std::is_same<OutT, uint8_t>::value)
      if (wide) return launch_nearest<uint16_t, OutT>(p, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    if constexpr (!std::is_same<OutT, uint16_t>::value)
      if (!wide) return launch_nearest<uint8_t, OutT>(p, in, src_stride, n_w, n_h, ow, oh, out, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_view_nearest: no kernel for dtype %d on %d-byte samples", p->dtype, p->sample_bytes);
  return hm_check_hip(hipGetLastError(), "k_view_nearest launch");
}
