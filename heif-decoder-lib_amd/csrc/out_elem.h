// out_elem.h — the element rules of every device output, stated once (included by tensor.hip, planes.hip, resample.hip and
// planes_view.hip, by out_rows.h, and through light_step.h by light.hip, alpha.hip and gain.hip; HIP only).  The tests restate these rules in float32 on the host and compare bit for bit, so
// every product and sum here is rounded on its own: -ffp-contract=off and explicit __fmul_rn / __fadd_rn, never a fused multiply-add.
//   linear_out    a float value through the destination's affine: r * scale + bias in two rounded steps, for f16 narrowed once more
//   moved         a sample that is stored, not computed: the integer itself (u16: << shift, msb_aligned planes), or linear_out of it
//   finish        a resampled sum that is stored: rounded half up and clamped to [0, peak] (u16: << shift), or linear_out of it
//   load_samples  N samples with one load of 4 / 8 / 16 bytes
//   elem_at       the address of channel c of pixel x in a CHW or HWC row
//   store16       16 bytes of elements with one global_store_dwordx4
// Behind them affine_of, which fills an Affine on the host.
#ifndef HM_OUT_ELEM_H
#define HM_OUT_ELEM_H

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <type_traits>

// a destination's scale[c] and bias[c], by value in the kernel arguments (SGPRs)
struct Affine { float scale[4], bias[4]; };

// (an integer OutT never comes here at run time - the host refuses linear light with an integer dtype -, but a branch on a run-time
// flag still names it)
template <typename OutT> __device__ __forceinline__ OutT linear_out(float r, float sc, float bi) { return (OutT)0; }
template <> __device__ __forceinline__ float linear_out<float>(float r, float sc, float bi) { return __fadd_rn(__fmul_rn(r, sc), bi); }
template <> __device__ __forceinline__ __half linear_out<__half>(float r, float sc, float bi) { return __float2half_rn(__fadd_rn(__fmul_rn(r, sc), bi)); }

template <typename OutT> __device__ __forceinline__ OutT moved(unsigned v, float sc, float bi, int shift = 0)
{
  if constexpr (std::is_same<OutT, uint8_t>::value) return (uint8_t)v;
  else if constexpr (std::is_same<OutT, uint16_t>::value) return (uint16_t)(v << shift);
  else return linear_out<OutT>((float)v, sc, bi);
}

// peak: of the plane's samples (255 / 65535 where the destination's whole range is meant); the float arms look at neither peak nor shift
template <typename OutT> __device__ __forceinline__ OutT finish(float r, float sc, float bi, int peak, int shift = 0)
{
  if constexpr (std::is_integral<OutT>::value) {
    const int v = (int)__fadd_rn(r, 0.5f);
    if constexpr (sizeof(OutT) == 1) return (uint8_t)min(max(v, 0), peak);
    else return (uint16_t)(min(max(v, 0), peak) << shift);
  }
  else return linear_out<OutT>(r, sc, bi);
}
// the whole range of an integer destination
template <typename OutT> constexpr int full_peak() { return sizeof(OutT) == 1 ? 255 : 65535; }

template <int BYTES> struct LoadWord { typedef uint32_t type; };
template <> struct LoadWord<16> { typedef uint4 type; };
template <> struct LoadWord<8> { typedef uint2 type; };

// N samples of SB bytes at `in` (aligned to their N * SB bytes) with one load
template <int SB, int N> __device__ __forceinline__ void load_samples(const uint8_t* in, unsigned (&v)[N])
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  typedef typename LoadWord<N * SB>::type LW;
  static_assert(N * SB == 4 || N * SB == 8 || N * SB == 16, "one load of 4, 8 or 16 bytes");
  const LW lw = *reinterpret_cast<const LW*>(in);
  InT smp[N];
  __builtin_memcpy(smp, &lw, N * SB);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = smp[i];
}

// channel c of pixel x of the destination row at `orow`: CHW - plane c lies c * plane_pitch bytes behind plane 0 -, or HWC with C
// elements per pixel
template <typename OutT> __device__ __forceinline__ OutT* elem_at(uint8_t* orow, bool chw, long long plane_pitch, int x, int c, int C)
{
  return chw ? reinterpret_cast<OutT*>(orow + (long long)c * plane_pitch) + x : reinterpret_cast<OutT*>(orow) + (size_t)x * C + c;
}

// 16 bytes of elements (P = 16 / sizeof(OutT) of them) at o to the 16-byte aligned dst with one global_store_dwordx4
template <typename OutT> __device__ __forceinline__ void store16(void* dst, const OutT* o)
{
  uint4 v;
  __builtin_memcpy(&v, o, 16);
  *reinterpret_cast<uint4*>(dst) = v;
}

// ---- host: the one helper every launcher needs beside the struct (the dtype dispatch is out_launch.h's) ----
static inline Affine affine_of(const float scale[4], const float bias[4])
{
  Affine a;
  for (int c = 0; c < 4; c++) { a.scale[c] = scale[c]; a.bias[c] = bias[c]; }
  return a;
}

#endif
