// planes.hip — the planes of a decoded image (Y, Cb, Cr, alpha: the library's own device planes) to planar or semi-planar YCbCr in
// caller-owned device memory (hm_device_planes, gfx950):
//   k_planes_to_tensor  u8 / u16 samples -> u8 / u16 (sample << shift) / f16 / f32 (sample * scale[c] + bias[c]): `moved` of out_elem.h
//                       with the plane's shift; every plane its own pitch; HM_DEV_PLANES_SEMI interleaves Cb and Cr (Cb first) into one plane
// A pure streaming kernel in the style of k_to_tensor (tensor.hip): no LDS, every sample read once and written once.  ONE launch
// covers all planes of an image: the descriptors travel by value in the kernel arguments, and blockIdx.y - a range of 4-row
// groups per plane - decides the plane, so the plane, its sample width and its instance are wave-uniform.  A wave takes 64
// consecutive groups of ONE row; a lane's group is 16 bytes of output (16 u8, 8 u16 / f16, 4 f32 elements), read with one load of
// 16 / 8 / 4 bytes and stored with one global_store_dwordx4.  The interleaved plane: a lane's 16 bytes are n Cb / Cr pairs, read as n
// samples from each source plane (dwordx2 + dwordx2 for u8 -> u8) and interleaved in registers (v_perm_b32 on bytes, shifts / packs
// on 16-bit elements); for f32 a lane takes 4 pairs = 32 bytes = two stores, so that its loads stay whole dwords.  The ragged last
// group of a row is stored element by element by its one lane.  A plane whose destination (pointer or pitch) or source is not
// 16-byte aligned takes the element-wise path for that plane alone: the same span of a row per wave, lane l takes elements (pairs)
// l, l + 64, ... of it, so every load and store instruction of the wave covers 64 consecutive elements.
// Reads: exactly the `width` samples of every source row, never the row's pitch padding.  Writes: exactly the elements of the planes.
#include "hm_devdest.h"
#include "out_elem.h"
#include "out_launch.h"

namespace {

// one plane, one component per element.  x-group gx of 64 groups, row y
template <int SB, typename OutT, bool VEC>
__device__ __forceinline__ void plane_single(const hm_plane_desc& d, int gx, int y, int lane)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = 16 / (int)sizeof(OutT);
  const int w = d.w;
  const InT* irow = reinterpret_cast<const InT*>(d.src0 + (size_t)y * d.stride0);
  OutT* orow = reinterpret_cast<OutT*>(d.dst + (long long)y * d.pitch);
  const float sc = d.scale0, bi = d.bias0;
  if (!VEC) {
#pragma unroll
    for (int i = 0; i < P; i++) {
      const int x = (gx * P + i) * 64 + lane;
      if (x >= w) break;
      orow[x] = moved<OutT>(irow[x], sc, bi, d.shift);
    }
    return;
  }
  const int x0 = (gx * 64 + lane) * P;
  if (x0 >= w) return;
  if (x0 + P <= w) {
    unsigned v[P];
    load_samples<SB, P>(reinterpret_cast<const uint8_t*>(irow + x0), v);
    OutT o[P];
#pragma unroll
    for (int i = 0; i < P; i++) o[i] = moved<OutT>(v[i], sc, bi, d.shift);
    store16(orow + x0, o);
    return;
  }
  for (int x = x0; x < w; x++) orow[x] = moved<OutT>(irow[x], sc, bi, d.shift);
}

// the interleaved chroma plane: element 2 x of a row is Cb[x], element 2 x + 1 is Cr[x]
template <int SB, typename OutT, bool VEC>
__device__ __forceinline__ void plane_pair(const hm_plane_desc& d, int gx, int y, int lane)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int N = sizeof(OutT) == 4 ? 4 : 8 / (int)sizeof(OutT); // pairs per lane: 8 (u8), 4 (u16 / f16), 4 (f32: two stores)
  const int w = d.w;
  const InT* brow = reinterpret_cast<const InT*>(d.src0 + (size_t)y * d.stride0);
  const InT* rrow = reinterpret_cast<const InT*>(d.src1 + (size_t)y * d.stride1);
  OutT* orow = reinterpret_cast<OutT*>(d.dst + (long long)y * d.pitch);
  if (!VEC) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int x = (gx * N + i) * 64 + lane;
      if (x >= w) break;
      orow[2 * (size_t)x] = moved<OutT>(brow[x], d.scale0, d.bias0, d.shift);
      orow[2 * (size_t)x + 1] = moved<OutT>(rrow[x], d.scale1, d.bias1, d.shift);
    }
    return;
  }
  const int x0 = (gx * 64 + lane) * N;
  if (x0 >= w) return;
  if (x0 + N <= w) {
    uint4* op = reinterpret_cast<uint4*>(orow + 2 * (size_t)x0);
    if constexpr (std::is_same<OutT, uint8_t>::value) { // bytes: two dwords of Cb, two of Cr, four v_perm_b32
      const uint2 b = *reinterpret_cast<const uint2*>(brow + x0), r = *reinterpret_cast<const uint2*>(rrow + x0);
      uint4 q; // v_perm_b32 D, S0, S1, sel: selector bytes 0 - 3 pick from S1 (Cb here), 4 - 7 from S0 (Cr)
      q.x = __builtin_amdgcn_perm(r.x, b.x, 0x05010400u);
      q.y = __builtin_amdgcn_perm(r.x, b.x, 0x07030602u);
      q.z = __builtin_amdgcn_perm(r.y, b.y, 0x05010400u);
      q.w = __builtin_amdgcn_perm(r.y, b.y, 0x07030602u);
      *op = q;
    }
    else {
      unsigned vb[N], vr[N];
      load_samples<SB, N>(reinterpret_cast<const uint8_t*>(brow + x0), vb);
      load_samples<SB, N>(reinterpret_cast<const uint8_t*>(rrow + x0), vr);
      OutT o[2 * N];
#pragma unroll
      for (int i = 0; i < N; i++) {
        o[2 * i] = moved<OutT>(vb[i], d.scale0, d.bias0, d.shift);
        o[2 * i + 1] = moved<OutT>(vr[i], d.scale1, d.bias1, d.shift);
      }
      constexpr int P = 16 / (int)sizeof(OutT); // elements of one store
#pragma unroll
      for (int k = 0; k < 2 * N / P; k++) store16(op + k, o + k * P);
    }
    return;
  }
  for (int x = x0; x < w; x++) {
    orow[2 * (size_t)x] = moved<OutT>(brow[x], d.scale0, d.bias0, d.shift);
    orow[2 * (size_t)x + 1] = moved<OutT>(rrow[x], d.scale1, d.bias1, d.shift);
  }
}

template <int SB, typename OutT>
__device__ __forceinline__ void plane_any(const hm_plane_desc& d, int gx, int y, int lane)
{
  if (d.pair) {
    if (d.vec) plane_pair<SB, OutT, true>(d, gx, y, lane);
    else plane_pair<SB, OutT, false>(d, gx, y, lane);
  }
  else {
    if (d.vec) plane_single<SB, OutT, true>(d, gx, y, lane);
    else plane_single<SB, OutT, false>(d, gx, y, lane);
  }
}

// grid: x = groups of 64 lane groups of the widest plane, y = the planes' 4-row groups one plane behind the other (a.y_end)
template <typename OutT>
__global__ __launch_bounds__(256) void k_planes_to_tensor(const hm_planes_args a)
{
  const int by = blockIdx.y;
  const int p = (by >= a.y_end[0]) + (by >= a.y_end[1]) + (by >= a.y_end[2]); // wave-uniform: scalar compares, scalar loads below
  const int y_begin = p == 0 ? 0 : a.y_end[p - 1];
  const hm_plane_desc& d = a.pl[p];
  const int lane = threadIdx.x & 63, y = (by - y_begin) * 4 + (threadIdx.x >> 6);
  if (y >= d.h) return;
  // integer outputs take samples of their own width only (hm_planes_resolve); a float output may meet an alpha plane of the other width
  if (std::is_same<OutT, uint8_t>::value || (!std::is_same<OutT, uint16_t>::value && d.sample_bytes == 1)) {
    if constexpr (!std::is_same<OutT, uint16_t>::value) plane_any<1, OutT>(d, blockIdx.x, y, lane);
  }
  else {
    if constexpr (!std::is_same<OutT, uint8_t>::value) plane_any<2, OutT>(d, blockIdx.x, y, lane);
  }
}

} // namespace

extern "C" int hm_launch_planes_to_tensor(const hm_planes_args* a, int dtype, hipStream_t s)
{
  int gx = 0;
  for (int p = 0; p < 4; p++) {
    const hm_plane_desc& d = a->pl[p];
    if (d.h <= 0) continue;
    const int per_lane = d.pair ? (dtype == HM_DEV_F32 ? 4 : dtype == HM_DEV_U8 ? 8 : 4) : (dtype == HM_DEV_F32 ? 4 : dtype == HM_DEV_U8 ? 16 : 8);
    const int groups = (d.w + per_lane - 1) / per_lane;
    gx = gx > (groups + 63) / 64 ? gx : (groups + 63) / 64;
  }
  const int gy = a->y_end[3];
  if (gx <= 0 || gy <= 0) return HM_OK;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  const int found = with_dtype(dtype, [&](auto tag) -> int {
    hipLaunchKernelGGL(k_planes_to_tensor<typename decltype(tag)::type>, grid, block, 0, s, *a);
    return HM_OK;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_planes_to_tensor: no kernel for dtype %d", dtype);
  return hm_check_hip(hipGetLastError(), "k_planes_to_tensor launch");
}
