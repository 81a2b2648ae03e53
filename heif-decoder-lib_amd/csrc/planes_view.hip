// planes_view.hip — a view (hm_device_view) of the planes of a decoded image into planar or semi-planar YCbCr in caller-owned device
// memory (hm_device_planes, gfx950): every plane is an image of its own, cropped and resampled by hm_device_view's rule.
//   k_planes_resample_h   the horizontal pass of EVERY source plane (Y, Cb, Cr, alpha) in one launch: a lane sits on one (output
//                         column, source row) pair of its plane and walks its taps over contiguous samples; a wave is 64 consecutive
//                         columns of ONE row, the plane's x table is tap-major, the float32 result goes to the plane's region of the
//                         frame's intermediate.
//   k_planes_resample_v   the vertical pass of EVERY destination plane in one launch, fused with dtype, peak, shift, scale, bias and
//                         the interleaving of HM_DEV_PLANES_SEMI: a wave is 64 consecutive lane groups of ONE output row, so the row's
//                         taps are wave-uniform; a lane's group is 16 bytes of output (16 u8, 8 u16 / f16, 4 f32), summed from
//                         dwordx4 loads of the intermediate rows and stored with one global_store_dwordx4.  The interleaved plane: a
//                         lane's 16 bytes are n Cb / Cr pairs summed from the two chroma regions and interleaved in registers (f32: 4
//                         pairs = two stores, as k_planes_to_tensor's plane_pair).  The ragged last group is stored element by element
//                         by its one lane; a plane whose pointer or pitch is no multiple of 16 takes the element-wise path for that
//                         plane alone (lane l on elements or pairs l, l + 64, ... of the wave's span).
//   k_planes_view_nearest HM_VIEW_NEAREST: a lane per output element (pair) of its plane moves the sample at j * n / m.
// As k_planes_to_tensor (planes.hip), the plane descriptors travel by value in the kernel arguments and a range of blockIdx.y
// decides the plane, so plane, sample width and path are wave-uniform; blockIdx.z is the frame of the chunk, whose pointers are
// read once as scalar loads and typed as pointers to global memory (as k_resample_*_batch, resample.hip).  The sums run tap by tap
// in float32 with separately rounded multiply and add (-ffp-contract=off, __fmul_rn / __fadd_rn), tap 0 first, horizontal pass
// first: resample.hip's sums.  A sum becomes an element by `finish` with the plane's own peak and msb_aligned shift, a sample that is
// only moved by `moved` with that shift (out_elem.h).  No LDS (the staged horizontal pass of resample.hip has no sibling here), no scratch.
// Reads: the samples of the crops.  Writes: exactly the elements of the planes.
#include <algorithm>

#include "hm_devdest.h"
#include "hm_planes_view.h"
#include "out_elem.h"
#include "out_launch.h"

namespace {

typedef __attribute__((address_space(1))) uint8_t GlobalBytes; // (resample.hip: a pointer loaded from memory is typed as a global one)

__device__ __forceinline__ const uint8_t* rec_src(const void* recs, int frame, int plane)
{
  return (const uint8_t*)(const GlobalBytes*)static_cast<const hm_pv_rec*>(recs)[frame].src[plane];
}
__device__ __forceinline__ uint8_t* rec_dst(const void* recs, int frame, int plane)
{
  return (uint8_t*)(GlobalBytes*)static_cast<const hm_pv_rec*>(recs)[frame].dst[plane];
}

// ---- horizontal ----
template <int SB>
__device__ __forceinline__ void h_body(const hm_pv_src_desc& d, const uint8_t* __restrict__ src, float* __restrict__ tmp, int j, int y)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int ow = d.ow;
  const InT* in = reinterpret_cast<const InT*>(src + (size_t)y * d.stride) + d.ax.first[j];
  const int n = d.ax.count[j];
  const float* __restrict__ wts = d.ax.weights;
  float t = 0.0f;
  for (int i = 0; i < n; i++) t = __fadd_rn(t, __fmul_rn(wts[(size_t)i * ow + j], (float)in[i]));
  tmp[d.tmp_off + (long long)y * d.tmp_pitch + j] = t;
}

// grid: x = groups of 64 output columns of the widest plane, y = the source planes' 4-row groups one plane behind the other, z = frames.
// SB: the sample bytes of the image's own planes; an alpha plane of the other width (a float dtype only) is a uniform branch.
template <int SB>
__global__ __launch_bounds__(256) void k_planes_resample_h(const hm_pv_h_args a)
{
  const int by = blockIdx.y;
  const int p = hm_pv_plane_of(by, a.y_end); // wave-uniform: scalar compares, scalar loads below
  const hm_pv_src_desc& d = a.pl[p];
  const int y = hm_pv_row_of(by, p, a.y_end, threadIdx.x >> 6);
  if ((int)blockIdx.x * 64 >= d.ow) return; // a narrower plane: nothing behind its last column group
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= d.n_h || j >= d.ow) return;
  const uint8_t* src = rec_src(a.recs, blockIdx.z, p);
  float* tmp = a.tmp + (long long)blockIdx.z * a.frame_stride;
  if (d.sample_bytes == SB) h_body<SB>(d, src, tmp, j, y);
  else h_body<3 - SB>(d, src, tmp, j, y);
}

// ---- vertical ----
// one component per element.  P elements per lane.
template <typename OutT, bool VEC>
__device__ __forceinline__ void v_single(const hm_pv_dst_desc& d, const float* __restrict__ tmp, uint8_t* __restrict__ dst, int bx, int k, int lane)
{
  constexpr int P = 16 / (int)sizeof(OutT);
  const int w = d.w, oh = d.oh;
  const int y0 = d.ay.first[k], n = d.ay.count[k]; // (the same in every lane of the wave)
  const float* __restrict__ wts = d.ay.weights;
  const long long pitch = d.tmp_pitch;
  const float* col = tmp + d.tmp_off0 + (long long)y0 * pitch;
  OutT* orow = reinterpret_cast<OutT*>(dst + (long long)k * d.pitch);
  float acc[P];
#pragma unroll
  for (int q = 0; q < P; q++) acc[q] = 0.0f;
  if (VEC) {
    int x0;
    const int cnt = hm_pv_vec_span(bx, lane, P, w, &x0);
    if (cnt == 0) return;
    col += x0;
    for (int i = 0; i < n; i++) {
      const float wi = wts[(size_t)i * oh + k];
      float v[P];
#pragma unroll
      for (int q = 0; q < P / 4; q++) {
        const float4 f = reinterpret_cast<const float4*>(col)[q];
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
      }
#pragma unroll
      for (int q = 0; q < P; q++) acc[q] = __fadd_rn(acc[q], __fmul_rn(wi, v[q]));
      col += pitch;
    }
    OutT o[P];
#pragma unroll
    for (int q = 0; q < P; q++) o[q] = finish<OutT>(acc[q], d.scale0, d.bias0, d.peak, d.shift);
    if (cnt == P) {
      store16(orow + x0, o);
      return;
    }
#pragma unroll
    for (int q = 0; q < P; q++)
      if (q < cnt) orow[x0 + q] = o[q];
    return;
  }
  for (int i = 0; i < n; i++) {
    const float wi = wts[(size_t)i * oh + k];
#pragma unroll
    for (int q = 0; q < P; q++) {
      const int x = hm_pv_elem_at(bx, lane, P, q);
      const float v = x < w ? col[x] : 0.0f;
      acc[q] = __fadd_rn(acc[q], __fmul_rn(wi, v));
    }
    col += pitch;
  }
#pragma unroll
  for (int q = 0; q < P; q++) {
    const int x = hm_pv_elem_at(bx, lane, P, q);
    if (x < w) orow[x] = finish<OutT>(acc[q], d.scale0, d.bias0, d.peak, d.shift);
  }
}

// the interleaved chroma plane: element 2 x of a row is the resampled Cb, element 2 x + 1 the resampled Cr.  N pairs per lane.
template <typename OutT, bool VEC>
__device__ __forceinline__ void v_pair(const hm_pv_dst_desc& d, const float* __restrict__ tmp, uint8_t* __restrict__ dst, int bx, int k, int lane)
{
  constexpr int N = sizeof(OutT) == 4 ? 4 : 8 / (int)sizeof(OutT); // 8 (u8), 4 (u16 / f16), 4 (f32: two stores)
  const int w = d.w, oh = d.oh;
  const int y0 = d.ay.first[k], n = d.ay.count[k];
  const float* __restrict__ wts = d.ay.weights;
  const long long pitch = d.tmp_pitch;
  const float* cb = tmp + d.tmp_off0 + (long long)y0 * pitch;
  const float* cr = tmp + d.tmp_off1 + (long long)y0 * pitch;
  OutT* orow = reinterpret_cast<OutT*>(dst + (long long)k * d.pitch);
  float ab[N], ar[N];
#pragma unroll
  for (int q = 0; q < N; q++) ab[q] = ar[q] = 0.0f;
  if (VEC) {
    int x0;
    const int cnt = hm_pv_vec_span(bx, lane, N, w, &x0);
    if (cnt == 0) return;
    cb += x0; cr += x0;
    for (int i = 0; i < n; i++) {
      const float wi = wts[(size_t)i * oh + k];
      float vb[N], vr[N];
#pragma unroll
      for (int q = 0; q < N / 4; q++) {
        const float4 f = reinterpret_cast<const float4*>(cb)[q], g = reinterpret_cast<const float4*>(cr)[q];
        vb[4 * q] = f.x; vb[4 * q + 1] = f.y; vb[4 * q + 2] = f.z; vb[4 * q + 3] = f.w;
        vr[4 * q] = g.x; vr[4 * q + 1] = g.y; vr[4 * q + 2] = g.z; vr[4 * q + 3] = g.w;
      }
#pragma unroll
      for (int q = 0; q < N; q++) {
        ab[q] = __fadd_rn(ab[q], __fmul_rn(wi, vb[q]));
        ar[q] = __fadd_rn(ar[q], __fmul_rn(wi, vr[q]));
      }
      cb += pitch; cr += pitch;
    }
    OutT o[2 * N];
#pragma unroll
    for (int q = 0; q < N; q++) {
      o[2 * q] = finish<OutT>(ab[q], d.scale0, d.bias0, d.peak, d.shift);
      o[2 * q + 1] = finish<OutT>(ar[q], d.scale1, d.bias1, d.peak, d.shift);
    }
    OutT* op = orow + 2 * (size_t)x0;
    if (cnt == N) {
      constexpr int P = 16 / (int)sizeof(OutT); // elements of one store
#pragma unroll
      for (int q = 0; q < 2 * N / P; q++) store16(op + q * P, o + q * P);
      return;
    }
#pragma unroll
    for (int q = 0; q < N; q++)
      if (q < cnt) { op[2 * q] = o[2 * q]; op[2 * q + 1] = o[2 * q + 1]; }
    return;
  }
  for (int i = 0; i < n; i++) {
    const float wi = wts[(size_t)i * oh + k];
#pragma unroll
    for (int q = 0; q < N; q++) {
      const int x = hm_pv_elem_at(bx, lane, N, q);
      const float vb = x < w ? cb[x] : 0.0f, vr = x < w ? cr[x] : 0.0f;
      ab[q] = __fadd_rn(ab[q], __fmul_rn(wi, vb));
      ar[q] = __fadd_rn(ar[q], __fmul_rn(wi, vr));
    }
    cb += pitch; cr += pitch;
  }
#pragma unroll
  for (int q = 0; q < N; q++) {
    const int x = hm_pv_elem_at(bx, lane, N, q);
    if (x < w) {
      orow[2 * (size_t)x] = finish<OutT>(ab[q], d.scale0, d.bias0, d.peak, d.shift);
      orow[2 * (size_t)x + 1] = finish<OutT>(ar[q], d.scale1, d.bias1, d.peak, d.shift);
    }
  }
}

// grid: x = groups of 64 lane groups of the widest plane, y = the destination planes' 4-row groups one plane behind the other, z = frames
template <typename OutT>
__global__ __launch_bounds__(256) void k_planes_resample_v(const hm_pv_v_args a)
{
  const int by = blockIdx.y;
  const int p = hm_pv_plane_of(by, a.y_end);
  const hm_pv_dst_desc& d = a.pl[p];
  const int lane = threadIdx.x & 63, k = hm_pv_row_of(by, p, a.y_end, threadIdx.x >> 6);
  if (k >= d.oh) return;
  if ((int)blockIdx.x >= hm_pv_blocks_x(d.w, hm_pv_per_lane((int)sizeof(OutT), d.pair))) return;
  uint8_t* dst = rec_dst(a.recs, blockIdx.z, p);
  const float* tmp = a.tmp + (long long)blockIdx.z * a.frame_stride;
  if (d.pair) {
    if (d.vec) v_pair<OutT, true>(d, tmp, dst, blockIdx.x, k, lane);
    else v_pair<OutT, false>(d, tmp, dst, blockIdx.x, k, lane);
  }
  else {
    if (d.vec) v_single<OutT, true>(d, tmp, dst, blockIdx.x, k, lane);
    else v_single<OutT, false>(d, tmp, dst, blockIdx.x, k, lane);
  }
}

// ---- nearest ----
template <int SB, typename OutT>
__device__ __forceinline__ void nearest_body(const hm_pv_dst_desc& d, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1, uint8_t* __restrict__ dst, int j, int k)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  const int sx = j * d.n_w / d.w, sy = k * d.n_h / d.oh;
  OutT* orow = reinterpret_cast<OutT*>(dst + (long long)k * d.pitch);
  const unsigned v0 = reinterpret_cast<const InT*>(s0 + (size_t)sy * d.stride0)[sx];
  if (d.pair) {
    const unsigned v1 = reinterpret_cast<const InT*>(s1 + (size_t)sy * d.stride1)[sx];
    orow[2 * (size_t)j] = moved<OutT>(v0, d.scale0, d.bias0, d.shift);
    orow[2 * (size_t)j + 1] = moved<OutT>(v1, d.scale1, d.bias1, d.shift);
  }
  else orow[j] = moved<OutT>(v0, d.scale0, d.bias0, d.shift);
}

// grid: x = groups of 64 output columns (pairs) of the widest plane, y = the destination planes' 4-row groups, z = frames
template <typename OutT>
__global__ __launch_bounds__(256) void k_planes_view_nearest(const hm_pv_v_args a)
{
  const int by = blockIdx.y;
  const int p = hm_pv_plane_of(by, a.y_end);
  const hm_pv_dst_desc& d = a.pl[p];
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), k = hm_pv_row_of(by, p, a.y_end, threadIdx.x >> 6);
  if (j >= d.w || k >= d.oh) return;
  const uint8_t* s0 = rec_src(a.recs, blockIdx.z, p);
  const uint8_t* s1 = d.pair ? rec_src(a.recs, blockIdx.z, 2) : s0;
  uint8_t* dst = rec_dst(a.recs, blockIdx.z, p);
  // integer outputs take samples of their own width only (hm_planes_resolve); a float output may meet an alpha plane of the other width
  if (std::is_same<OutT, uint8_t>::value || (!std::is_same<OutT, uint16_t>::value && d.sample_bytes == 1)) {
    if constexpr (!std::is_same<OutT, uint16_t>::value) nearest_body<1, OutT>(d, s0, s1, dst, j, k);
  }
  else {
    if constexpr (!std::is_same<OutT, uint8_t>::value) nearest_body<2, OutT>(d, s0, s1, dst, j, k);
  }
}

// every instance the launchers below can pick (hm_debug_kernel_regs, code 7)
const void* const g_instances[] = {
  (const void*)k_planes_resample_h<1>, (const void*)k_planes_resample_h<2>,
  (const void*)k_planes_resample_v<uint8_t>, (const void*)k_planes_resample_v<uint16_t>, (const void*)k_planes_resample_v<__half>, (const void*)k_planes_resample_v<float>,
  (const void*)k_planes_view_nearest<uint8_t>, (const void*)k_planes_view_nearest<uint16_t>, (const void*)k_planes_view_nearest<__half>, (const void*)k_planes_view_nearest<float>,
};

int elem_of(int dtype) { return dtype == HM_DEV_U8 ? 1 : dtype == HM_DEV_F32 ? 4 : 2; }

} // namespace

extern "C" const void* hm_planes_view_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

extern "C" int hm_launch_planes_resample(const hm_pv_h_args* h, const hm_pv_v_args* v, int sample_bytes, int dtype, int frames, hipStream_t s)
{
  if (frames <= 0) return HM_OK;
  if (frames > HM_PV_Z_MOST) return hm_fail(HM_ERR_INTERNAL, "k_planes_resample: %d frames in one launch", frames);
  if (((uintptr_t)h->tmp % 16) || (h->frame_stride % 4) || h->tmp != v->tmp || h->frame_stride != v->frame_stride)
    return hm_fail(HM_ERR_INTERNAL, "k_planes_resample: misaligned intermediate");
  int hx = 0, vx = 0;
  for (int p = 0; p < 4; p++) {
    const hm_pv_src_desc& sd = h->pl[p];
    if (sd.n_h > 0) {
      if ((sd.tmp_pitch % 16) || (sd.tmp_off % 4)) return hm_fail(HM_ERR_INTERNAL, "k_planes_resample: misaligned intermediate");
      hx = std::max(hx, (sd.ow + 63) / 64);
    }
    const hm_pv_dst_desc& dd = v->pl[p];
    if (dd.oh > 0) {
      if ((dd.tmp_pitch % 16) || (dd.tmp_off0 % 4) || (dd.tmp_off1 % 4)) return hm_fail(HM_ERR_INTERNAL, "k_planes_resample: misaligned intermediate");
      vx = std::max(vx, hm_pv_blocks_x(dd.w, hm_pv_per_lane(elem_of(dtype), dd.pair)));
    }
  }
  const int hy = h->y_end[3], vy = v->y_end[3];
  if (hx <= 0 || hy <= 0 || vx <= 0 || vy <= 0) return HM_OK;
  const dim3 block(256), hgrid((unsigned)hx, (unsigned)hy, (unsigned)frames), vgrid((unsigned)vx, (unsigned)vy, (unsigned)frames);
  if (sample_bytes == 1) hipLaunchKernelGGL(k_planes_resample_h<1>, hgrid, block, 0, s, *h);
  else hipLaunchKernelGGL(k_planes_resample_h<2>, hgrid, block, 0, s, *h);
  const int rc = hm_check_hip(hipGetLastError(), "k_planes_resample_h launch");
  if (rc) return rc;
  const int found = with_dtype(dtype, [&](auto tag) -> int {
    hipLaunchKernelGGL(k_planes_resample_v<typename decltype(tag)::type>, vgrid, block, 0, s, *v);
    return HM_OK;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_planes_resample_v: no kernel for dtype %d", dtype);
  return hm_check_hip(hipGetLastError(), "k_planes_resample_v launch");
}

extern "C" int hm_launch_planes_view_nearest(const hm_pv_v_args* v, int dtype, int frames, hipStream_t s)
{
  if (frames <= 0) return HM_OK;
  if (frames > HM_PV_Z_MOST) return hm_fail(HM_ERR_INTERNAL, "k_planes_view_nearest: %d frames in one launch", frames);
  int gx = 0;
  for (int p = 0; p < 4; p++)
    if (v->pl[p].oh > 0) gx = std::max(gx, (v->pl[p].w + 63) / 64);
  const int gy = v->y_end[3];
  if (gx <= 0 || gy <= 0) return HM_OK;
  const dim3 block(256), grid((unsigned)gx, (unsigned)gy, (unsigned)frames);
  const int found = with_dtype(dtype, [&](auto tag) -> int {
    hipLaunchKernelGGL(k_planes_view_nearest<typename decltype(tag)::type>, grid, block, 0, s, *v);
    return HM_OK;
  });
  if (found == NO_KERNEL_INSTANCE) return hm_fail(HM_ERR_INTERNAL, "k_planes_view_nearest: no kernel for dtype %d", dtype);
  return hm_check_hip(hipGetLastError(), "k_planes_view_nearest launch");
}
