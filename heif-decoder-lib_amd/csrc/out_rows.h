// out_rows.h — the row bodies more than one output kernel runs (device only; the element rules are out_elem.h's):
//   resample_h_body  the horizontal pass of a resampled view, every sample through a sample-to-float step (k_resample_h and its
//                    batched form: the conversion; k_light_h: the table lookup on the colour channels; k_gain_map_h: a gain table)
//   pointwise_body   a streamed row, every pixel through a per-pixel step (k_light_tensor, k_alpha_tensor, k_gain_tensor)
//   nearest_body     HM_VIEW_NEAREST through a per-pixel step (k_alpha_nearest, k_gain_nearest)
//   vertical_sums    the sums of a vertical pass that takes ONE output pixel per lane (k_light_v, k_alpha_v, k_gain_v, k_gain_map_v)
// k_to_tensor has pointwise_body's shape but keeps a body of its own: as one function template k_to_tensor<1, 3, __half, true, true> is
// 2 % slower (profiles/output_kernels_refactor.txt).  k_light_tensor shares its body with the alpha and gain kernels.  k_light_nearest
// keeps nearest_body's text written out: through the body k_light_nearest<uint8_t, 4, __half> is 1 - 2 % slower at 4000 x 3000 in four
// sessions out of four (profiles/step_kernels_refactor.txt).  k_resample_v takes P elements per lane and k_view_nearest a run-time
// channel count: their own.
#ifndef HM_OUT_ROWS_H
#define HM_OUT_ROWS_H

#include "out_elem.h"

// The horizontal pass: rows of the crop -> float32 rows of ow.  A lane sits on one (output column, source row) pair and walks its
// taps, tap 0 first, over contiguous source samples; a wave is 64 consecutive columns of ONE row, and the tap table is tap-major
// (wts[tap][column]), so the wave's weight reads and its stores are contiguous.  The intermediate is laid out like the
// destination: one plane per channel for CHW (plane elements apart), interleaved for HWC.
// SB: bytes per source sample (little-endian), C: channels, CHW: the intermediate has one plane per channel.  to_float(v, c): sample v
// of channel c as the float the sum takes.  grid: x = groups of 64 output columns, y = groups of 4 source rows.  src points at the
// crop's origin.
// by: the workgroup's group of 4 source rows - blockIdx.y, or its place inside its own view where a launch covers several (k_resample_h_multi).
template <int SB, int C, bool CHW, typename ToFloat>
__device__ __forceinline__ void resample_h_rows(int by, const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                long long pitch, long long plane, ToFloat to_float)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), y = by * 4 + (threadIdx.x >> 6);
  if (j >= ow || y >= n_h) return;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)y * src_stride) + (size_t)first[j] * C;
  const int n = count[j];
  float t[C];
#pragma unroll
  for (int c = 0; c < C; c++) t[c] = 0.0f;
  for (int i = 0; i < n; i++) {
    const float w = wts[(size_t)i * ow + j];
#pragma unroll
    for (int c = 0; c < C; c++) {
      const unsigned v = in[i * C + c];
      t[c] = __fadd_rn(t[c], __fmul_rn(w, to_float(v, c)));
    }
  }
  float* o = tmp + (long long)y * pitch;
#pragma unroll
  for (int c = 0; c < C; c++) {
    if (CHW) o[(long long)c * plane + j] = t[c];
    else o[(size_t)j * C + c] = t[c];
  }
}

template <int SB, int C, bool CHW, typename ToFloat>
__device__ __forceinline__ void resample_h_body(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                long long pitch, long long plane, ToFloat to_float)
{
  resample_h_rows<SB, C, CHW>((int)blockIdx.y, src, src_stride, n_h, ow, first, count, wts, tmp, pitch, plane, to_float);
}

// the plain sample-to-float step
struct SampleToFloat {
  __device__ __forceinline__ float operator()(unsigned v, int) const { return (float)v; }
};

// a step that reads nothing per column: the record pointwise_body hands to its pixels is empty
struct NoColumn {
  struct Rec {};
  __device__ __forceinline__ Rec operator()(int) const { return Rec(); }
};

// the OC elements of pixel x, one store each
template <int OC, typename OutT> __device__ __forceinline__ void store_pixel(uint8_t* orow, bool chw, long long plane_pitch, int x, const OutT* o)
{
#pragma unroll
  for (int c = 0; c < OC; c++) *elem_at<OutT>(orow, chw, plane_pitch, x, c, OC) = o[c];
}

// one pixel of a pointwise or nearest body: its C samples at ip through pixel(x, v, o, rec) to its OC elements, stored one by one
template <int C, int OC, typename OutT, typename InT, typename Pixel, typename Rec>
__device__ __forceinline__ void pixel_alone(const InT* ip, uint8_t* orow, bool chw, long long plane_pitch, int x, Pixel& pixel, const Rec& rec)
{
  unsigned v[C];
#pragma unroll
  for (int c = 0; c < C; c++) v[c] = ip[c];
  OutT o[OC];
  pixel(x, v, o, rec);
  store_pixel<OC>(orow, chw, plane_pitch, x, o);
}

// The streaming row: the wave whose row is y takes 64 consecutive pixel groups of it, a lane's group is 16 bytes of output per channel
// plane (P pixels), loaded with 16-byte loads where the group's bytes allow and stored with 16-byte stores; the ragged last group goes
// element by element.  Without VEC (the launcher has checked the alignment of both sides) lane l takes pixels l, l + 64, ... of the
// wave's 64 * P instead.  grid: x = groups of 64 pixel groups; y is the caller's (< h: checked there).
// SB: bytes per input sample (1 / 2, little-endian), C: channels read, OC: channels written; chw: one plane per channel (a constant
// folds).  pixel(x, v, o, rec): the C samples v of the pixel in column x to its OC elements o; rec = column(x), what the step reads per
// column (the gain step: a tap record) - the P records of a lane's group are fetched together, in front of its pixels, so that their
// loads are in flight at once.
template <int SB, int C, int OC, typename OutT, bool VEC, typename Pixel, typename Column = NoColumn>
__device__ __forceinline__ void pointwise_body(const uint8_t* __restrict__ src, int src_stride, int w, int y, uint8_t* __restrict__ dst, long long row_pitch,
                                               long long plane_pitch, bool chw, Pixel pixel, Column column = Column())
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT); // pixels per lane
  constexpr int NB = P * C * SB;            // input bytes per lane
  const int lane = threadIdx.x & 63;
  uint8_t* orow = dst + (long long)y * row_pitch;
  if (!VEC) { // one pixel per lane and step
    const InT* irow = reinterpret_cast<const InT*>(src + (size_t)y * src_stride);
#pragma unroll 1
    for (int i = 0; i < P; i++) {
      const int x = (blockIdx.x * P + i) * 64 + lane;
      if (x >= w) break;
      pixel_alone<C, OC, OutT>(irow + (size_t)x * C, orow, chw, plane_pitch, x, pixel, column(x));
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
    decltype(column(0)) rec[P];
#pragma unroll
    for (int i = 0; i < P; i++) rec[i] = column(x0 + i);
    OutT o[P * OC]; // pixel-major: the row's own order
#pragma unroll
    for (int i = 0; i < P; i++) {
      unsigned v[C];
#pragma unroll
      for (int c = 0; c < C; c++) v[c] = smp[i * C + c];
      pixel(x0 + i, v, &o[i * OC], rec[i]);
    }
    if (chw) {
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
  for (int i = 0; i < n; i++) pixel_alone<C, OC, OutT>(ip + i * C, orow, chw, plane_pitch, x0 + i, pixel, column(x0 + i));
}

// HM_VIEW_NEAREST: out pixel (j, k) is the source pixel (sx, sy) below, through pixel(j, v, o, rec) as above (no record).
// grid: x = groups of 64 columns, y = groups of 4 rows.
template <int SB, int C, int OC, typename OutT, typename Pixel>
__device__ __forceinline__ void nearest_body(const uint8_t* __restrict__ src, int src_stride, int n_w, int n_h, int ow, int oh, bool chw, uint8_t* __restrict__ dst,
                                             long long row_pitch, long long plane_pitch, Pixel pixel)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (j >= ow || k >= oh) return;
  const int sx = j * n_w / ow, sy = k * n_h / oh;
  pixel_alone<C, OC, OutT>(reinterpret_cast<const InT*>(src + (size_t)sy * src_stride) + (size_t)sx * C, dst + (long long)k * row_pitch, chw, plane_pitch, j, pixel,
                           NoColumn::Rec());
}

// The sums of a vertical pass whose lane is ONE output pixel (j, k), S[c] = sum over the taps of row k, tap 0 first, of
// wts[tap][k] * tmp[first[k] + tap][j][c].  A wave is 64 consecutive pixels of one output row, so first[k] and count[k] are the same in
// every lane and the reads of a CHW intermediate coalesce per plane; the four sums of an HWC pixel come with one 16-byte load (pitch is a
// multiple of 16 elements and tmp a pool block: 16-byte aligned), three with three loads.
template <int C, bool CHW>
__device__ __forceinline__ void vertical_sums(const float* __restrict__ tmp, long long pitch, long long plane, int j, int k, int oh, const int32_t* __restrict__ first,
                                              const int32_t* __restrict__ count, const float* __restrict__ wts, float S[C])
{
  const int y0 = first[k], n = count[k];
  const float* col = tmp + (long long)y0 * pitch + (CHW ? (long long)j : (long long)j * C);
#pragma unroll
  for (int c = 0; c < C; c++) S[c] = 0.0f;
  for (int i = 0; i < n; i++) {
    const float w = wts[(size_t)i * oh + k];
    float v[C];
    if constexpr (!CHW && C == 4) {
      const float4 q = *reinterpret_cast<const float4*>(col);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    else {
#pragma unroll
      for (int c = 0; c < C; c++) v[c] = CHW ? col[(long long)c * plane] : col[c];
    }
#pragma unroll
    for (int c = 0; c < C; c++) S[c] = __fadd_rn(S[c], __fmul_rn(w, v[c]));
    col += pitch;
  }
}

#endif
