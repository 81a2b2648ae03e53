// tensor.hip — the interleaved pixels of the colour stage to a tensor in caller-owned device memory (gfx950):
//   k_to_tensor  rows of 3 / 4 / 6 / 8 bytes per pixel -> CHW (one plane per channel) or HWC, as u8 / u16 / f16 / f32, floats as
//                sample * scale[c] + bias[c] in two rounded steps (no fused multiply-add: a float32 restatement on the host is exact)
// A pure streaming kernel: every sample is read once and written once, no LDS.  A wave takes 64 consecutive pixel groups of ONE row;
// a lane's group is 16 bytes of output per channel plane (4 pixels as f32, 8 as f16 / u16, 16 as u8), so the lanes of a wave read one
// contiguous piece of the row (4 pixels of RGB24 are three dwords) and write 1 KiB per store instruction and plane.  The last,
// ragged group of a row is stored element by element by its one lane.  Where a pointer or a pitch is not 16-byte aligned (a tight
// CHW float32 tensor of a width that is no multiple of 4, say) the whole image takes the scalar instance: the same span of a row
// per wave, but lane l takes pixels l, l + 64, l + 128 ... of it, so every load and store instruction of the wave still covers 64
// consecutive pixels.  Nothing but the w x h x C elements of the image is ever stored.  HWC with the target's own integer type
// is a 2-D device copy and never comes here.  The rule for a moved sample, the address of an element and the 16-byte store are
// out_elem.h's.
#include "hm_devdest.h"
#include "out_elem.h"
#include "out_launch.h"

namespace {

// SB: bytes per input sample (1 / 2, little-endian), C: channels, CHW: one plane per channel, VEC: 16-byte accesses allowed
// (the launcher has checked the alignment of both sides), else the scalar instance.  grid: x = groups of 64 pixel groups, y = groups of 4 rows.
template <int SB, int C, typename OutT, bool CHW, bool VEC>
__global__ __launch_bounds__(256) void k_to_tensor(const uint8_t* __restrict__ src, int src_stride, int w, int h, uint8_t* __restrict__ dst,
                                                   long long row_pitch, long long plane_pitch, Affine a)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT); // pixels per lane
  constexpr int NB = P * C * SB;            // input bytes per lane
  const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (y >= h) return;
  uint8_t* orow = dst + (long long)y * row_pitch;
  if (!VEC) { // one element per lane and instruction: pixels lane, lane + 64, ... of the wave's 64 * P
    const InT* irow = reinterpret_cast<const InT*>(src + (size_t)y * src_stride);
#pragma unroll
    for (int i = 0; i < P; i++) {
      const int x = (blockIdx.x * P + i) * 64 + lane;
      if (x >= w) break;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const OutT o = moved<OutT>(irow[(size_t)x * C + c], a.scale[c], a.bias[c]);
        *elem_at<OutT>(orow, CHW, plane_pitch, x, c, C) = o;
      }
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
    if (CHW) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        OutT o[P];
#pragma unroll
        for (int i = 0; i < P; i++) o[i] = moved<OutT>(smp[i * C + c], a.scale[c], a.bias[c]);
        store16(elem_at<OutT>(orow, true, plane_pitch, x0, c, C), o);
      }
    }
    else {
#pragma unroll
      for (int k = 0; k < C; k++) { // P * C elements in a row: C stores of P elements
        OutT o[P];
#pragma unroll
        for (int i = 0; i < P; i++) o[i] = moved<OutT>(smp[k * P + i], a.scale[(k * P + i) % C], a.bias[(k * P + i) % C]);
        store16(elem_at<OutT>(orow, false, 0, x0, 0, C) + k * P, o);
      }
    }
    return;
  }
  const int n = w - x0 < P ? w - x0 : P;
  const InT* ip = reinterpret_cast<const InT*>(in);
  for (int i = 0; i < n; i++) {
#pragma unroll
    for (int c = 0; c < C; c++) {
      const OutT o = moved<OutT>(ip[i * C + c], a.scale[c], a.bias[c]);
      *elem_at<OutT>(orow, CHW, plane_pitch, x0 + i, c, C) = o;
    }
  }
}

template <int SB, int C, typename OutT, bool CHW>
int launch(const hm_dest_plan* p, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a, hipStream_t s)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const bool vec = ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0 && ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 &&
                   (!CHW || (p->plane_pitch % 16) == 0);
  const int groups = (w + P - 1) / P;
  const dim3 grid((unsigned)((groups + 63) / 64), (unsigned)((rows + 3) / 4)), block(256);
  if (vec)
    hipLaunchKernelGGL((k_to_tensor<SB, C, OutT, CHW, true>), grid, block, 0, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a);
  else
    hipLaunchKernelGGL((k_to_tensor<SB, C, OutT, CHW, false>), grid, block, 0, s, src, src_stride, w, rows, dst, (long long)p->row_pitch, (long long)p->plane_pitch, a);
  return hm_check_hip(hipGetLastError(), "k_to_tensor launch");
}

// float dtypes in both layouts; the integer type of the samples' own width as CHW only (HWC is the 2-D copy); nothing else
template <int SB, int C>
int launch_dtype(const hm_dest_plan* p, const uint8_t* src, int src_stride, int w, int rows, uint8_t* dst, const Affine& a, hipStream_t s)
{
  const bool chw = p->layout == HM_DEV_LAYOUT_CHW;
  const int rc = with_dtype(p->dtype, [&](auto tag) -> int {
    typedef typename decltype(tag)::type OutT;
    if constexpr (!std::is_integral<OutT>::value)
      return chw ? launch<SB, C, OutT, true>(p, src, src_stride, w, rows, dst, a, s) : launch<SB, C, OutT, false>(p, src, src_stride, w, rows, dst, a, s);
    else if constexpr (sizeof(OutT) == SB)
      if (chw) return launch<SB, C, OutT, true>(p, src, src_stride, w, rows, dst, a, s);
    return NO_KERNEL_INSTANCE;
  });
  if (rc != NO_KERNEL_INSTANCE) return rc;
  return hm_fail(HM_ERR_INTERNAL, "k_to_tensor: no kernel for dtype %d, layout %d on %d-byte samples", p->dtype, p->layout, SB);
}

} // namespace

// rows [0, rows) of `src` (interleaved, p->channels samples of p->sample_bytes bytes per pixel) to `dst` = the destination's address of the
// first of these rows (plane 0); asynchronous on `s`
extern "C" int hm_launch_to_tensor(const hm_dest_plan* p, const void* src, int src_stride, int w, int rows, void* dst, const float scale[4], const float bias[4],
                                   hipStream_t s)
{
  if (w <= 0 || rows <= 0) return HM_OK;
  const Affine a = affine_of(scale, bias);
  const uint8_t* in = (const uint8_t*)src;
  uint8_t* out = (uint8_t*)dst;
  if (p->sample_bytes == 1) return p->channels == 3 ? launch_dtype<1, 3>(p, in, src_stride, w, rows, out, a, s) : launch_dtype<1, 4>(p, in, src_stride, w, rows, out, a, s);
  return p->channels == 3 ? launch_dtype<2, 3>(p, in, src_stride, w, rows, out, a, s) : launch_dtype<2, 4>(p, in, src_stride, w, rows, out, a, s);
}
