// out_rows.h — the row body more than one output kernel runs (device only; the element rules are out_elem.h's):
//   resample_h_body  the horizontal pass of a resampled view, every sample through a sample-to-float step (k_resample_h and its
//                    batched form: the conversion; k_light_h: the table lookup on the colour channels)
// k_to_tensor and k_light_tensor share a shape but not a body: as one function template k_to_tensor<1, 3, __half, true, true> is 2 % slower.
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
template <int SB, int C, bool CHW, typename ToFloat>
__device__ __forceinline__ void resample_h_body(const uint8_t* __restrict__ src, int src_stride, int n_h, int ow, const int32_t* __restrict__ first,
                                                const int32_t* __restrict__ count, const float* __restrict__ wts, float* __restrict__ tmp,
                                                long long pitch, long long plane, ToFloat to_float)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
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

// the plain sample-to-float step
struct SampleToFloat {
  __device__ __forceinline__ float operator()(unsigned v, int) const { return (float)v; }
};

#endif
