// planar.hip — kernels of the planar YCbCr targets (HM_OUT_YCBCR_*) for gfx950: the operations of the reference's chain that
// end in planes instead of interleaved pixels.
//   k_average_down  : Op_YCbCr444_to_YCbCr420_average / _422_average<u8|u16>   (chroma_sampling.cc:77-236, 295-434)
//   k_to_rgb_planes : Op_YCbCr_to_RGB<u8|u16> with a planar store                (yuv2rgb.cc:79-254)
//   k_to_ycbcr      : Op_RGB_to_YCbCr<u8|u16>                                    (rgb2yuv.cc:88-275)
//                     - from R, G, B planes, or
//                     - fused behind Op_YCbCr_to_RGB: the chain of 4:2:0 <-> 4:2:2 and of every GBR image.  The intermediate
//                       R, G, B samples live in registers, each rounded to the sample type exactly where the reference stores it.
// (Chroma up-sampling and the depth changes are colour.hip's k_upsample_bilinear / k_to_sdr / k_to_hdr; Op_mono_to_YCbCr420's
// neutral planes are a memset.)
//
// A lane owns 16 bytes of a luma row (16 samples of 8 bits, 8 deeper ones) - two rows of them for a 4:2:0 target so that each
// chroma sample is produced once - loads and stores are 16 B / 8 B per lane and contiguous across the wave.  Row starts are
// 16-byte aligned (hm_plane_stride); lanes on the right and bottom edges take the sample-by-sample path.
// Measured (profiles/planar_targets.txt): k_average_down is bound by memory traffic (0.66-0.70 of HBM peak); k_to_rgb_planes and
// k_to_ycbcr are bound by issue - their rate follows the float operations per pixel, not the bytes - and the fused 8-bit 4:2:0
// instantiation (16 pixels x 2 rows per lane: 197 vector registers, 2 waves per SIMD) is no faster than the two kernels it
// replaces at 16384 x 16384; the 10-bit one saves about a third.
//
// Bit-exactness as in colour.hip: individually rounded binary32 operations in the reference's order, trunc(x + 0.5f) rounding.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "colour_float.h"
#include "hm_planar.h"

namespace {

template <typename Pix> struct Lane { static constexpr int N = 16 / (int)sizeof(Pix); };

template <typename Pix>
__device__ __forceinline__ void unpack16(const uint4 q, int* v)
{
  const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < Lane<Pix>::N; i++) {
    if (sizeof(Pix) == 1) v[i] = (wd[i >> 2] >> ((i & 3) * 8)) & 0xFF;
    else v[i] = (wd[i >> 1] >> ((i & 1) * 16)) & 0xFFFF;
  }
}

template <typename Pix>
__device__ __forceinline__ void unpack8(const uint2 q, int* v) // half a lane's samples
{
  const uint32_t wd[2] = {q.x, q.y};
#pragma unroll
  for (int i = 0; i < Lane<Pix>::N / 2; i++) {
    if (sizeof(Pix) == 1) v[i] = (wd[i >> 2] >> ((i & 3) * 8)) & 0xFF;
    else v[i] = (wd[i >> 1] >> ((i & 1) * 16)) & 0xFFFF;
  }
}

template <typename Pix, int CNT>
__device__ __forceinline__ void pack(const int* v, uint32_t* wd) // CNT samples -> CNT * sizeof(Pix) / 4 words
{
  constexpr int PER = 4 / (int)sizeof(Pix);
#pragma unroll
  for (int k = 0; k < CNT / PER; k++) {
    if (sizeof(Pix) == 1)
      wd[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
    else wd[k] = (uint32_t)v[2 * k] | ((uint32_t)v[2 * k + 1] << 16);
  }
}

// one row of a lane: N samples from x0 (vector load when the lane lies inside the row, else sample by sample, clamped to the row)
template <typename Pix>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ row, int x0, int w, bool full, int* v)
{
  constexpr int N = Lane<Pix>::N;
  if (full) unpack16<Pix>(*reinterpret_cast<const uint4*>(row + (size_t)x0 * sizeof(Pix)), v);
  else {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = reinterpret_cast<const Pix*>(row)[x0 + i < w ? x0 + i : w - 1];
  }
}

// N samples to x0 of a row w samples wide
template <typename Pix>
__device__ __forceinline__ void store_row(uint8_t* __restrict__ row, int x0, int w, bool full, const int* v)
{
  constexpr int N = Lane<Pix>::N;
  if (full) {
    uint32_t wd[4];
    pack<Pix, N>(v, wd);
    *reinterpret_cast<uint4*>(row + (size_t)x0 * sizeof(Pix)) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  }
  else {
#pragma unroll
    for (int i = 0; i < N; i++)
      if (x0 + i < w) reinterpret_cast<Pix*>(row)[x0 + i] = (Pix)v[i];
  }
}

// N / 2 samples to x0 / 2 of a (sub-sampled) row cw samples wide
template <typename Pix>
__device__ __forceinline__ void store_half_row(uint8_t* __restrict__ row, int cx0, int cw, bool full, const int* v)
{
  constexpr int NC = Lane<Pix>::N / 2;
  if (full) {
    uint32_t wd[2];
    pack<Pix, NC>(v, wd);
    *reinterpret_cast<uint2*>(row + (size_t)cx0 * sizeof(Pix)) = make_uint2(wd[0], wd[1]);
  }
  else {
#pragma unroll
    for (int i = 0; i < NC; i++)
      if (cx0 + i < cw) reinterpret_cast<Pix*>(row)[cx0 + i] = (Pix)v[i];
  }
}

// ---------------------------------------------------------------------------------------
// 4:4:4 chroma -> 4:2:0 / 4:2:2 by averaging.  One lane: 8 output samples of one plane (blockIdx.y: Cb / Cr).
//   4:2:0 (chroma_sampling.cc:172-221): (a + b + c + d + 2) / 4; odd height: the last row averages horizontal pairs
//         (a + b + 1) / 2; odd width: the last column averages vertical pairs; both: the corner is copied
//   4:2:2 (chroma_sampling.cc:396-420): (a + b + 1) / 2; odd width: the last column is copied - the reference's border loop stops
//         one row early, its last sample stays whatever the allocation held; the copied sample is written there
// ---------------------------------------------------------------------------------------
template <typename Pix, bool V420>
__global__ __launch_bounds__(256) void k_average_down(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr, int is_cb, int is_cr,
                                                      uint8_t* __restrict__ ocb, uint8_t* __restrict__ ocr, int os_cb, int os_cr,
                                                      int w, int h, int cw, int groups_per_row, int total_groups)
{
  constexpr int NO = 8; // output samples per lane
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= total_groups) return;
  const uint8_t* __restrict__ in = blockIdx.y ? cr : cb;
  uint8_t* __restrict__ out = blockIdx.y ? ocr : ocb;
  const int is = blockIdx.y ? is_cr : is_cb, os = blockIdx.y ? os_cr : os_cb;
  const int cy = gid / groups_per_row;
  const int cx0 = (gid - cy * groups_per_row) * NO;
  const int y0 = V420 ? 2 * cy : cy;
  const bool two_rows = V420 && y0 + 1 < h;
  const uint8_t* __restrict__ ra = in + (size_t)y0 * is;
  const uint8_t* __restrict__ rb = in + (size_t)(two_rows ? y0 + 1 : y0) * is;
  uint8_t* __restrict__ ro = out + (size_t)cy * os;
  if (2 * (cx0 + NO) <= w && (!V420 || two_rows)) {
    int a[2 * NO], b[2 * NO], o[NO];
    constexpr int HALF = Lane<Pix>::N; // samples per 16-byte load
#pragma unroll
    for (int k = 0; k < 2 * NO / HALF; k++) {
      unpack16<Pix>(*reinterpret_cast<const uint4*>(ra + (size_t)(2 * cx0 + k * HALF) * sizeof(Pix)), a + k * HALF);
      if (V420) unpack16<Pix>(*reinterpret_cast<const uint4*>(rb + (size_t)(2 * cx0 + k * HALF) * sizeof(Pix)), b + k * HALF);
    }
#pragma unroll
    for (int i = 0; i < NO; i++) o[i] = V420 ? (a[2 * i] + a[2 * i + 1] + b[2 * i] + b[2 * i + 1] + 2) >> 2 : (a[2 * i] + a[2 * i + 1] + 1) >> 1;
    uint32_t wd[NO * sizeof(Pix) / 4];
    pack<Pix, NO>(o, wd);
    if constexpr (sizeof(Pix) == 1) *reinterpret_cast<uint2*>(ro + cx0) = make_uint2(wd[0], wd[1]);
    else *reinterpret_cast<uint4*>(ro + (size_t)cx0 * 2) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    return;
  }
  const Pix* pa = reinterpret_cast<const Pix*>(ra);
  const Pix* pb = reinterpret_cast<const Pix*>(rb);
  for (int i = 0; i < NO && cx0 + i < cw; i++) {
    const int x = 2 * (cx0 + i);
    const bool pair = x + 1 < w;
    int v;
    if (two_rows) v = pair ? ((int)pa[x] + pa[x + 1] + pb[x] + pb[x + 1] + 2) >> 2 : ((int)pa[x] + pb[x] + 1) >> 1;
    else v = pair ? ((int)pa[x] + pa[x + 1] + 1) >> 1 : (int)pa[x];
    reinterpret_cast<Pix*>(ro)[cx0 + i] = (Pix)v;
  }
}

// ---------------------------------------------------------------------------------------
// The R, G, B samples of one lane-row: read from planes, or produced by Op_YCbCr_to_RGB (px_float, colour_float.h) from the
// Y / Cb / Cr planes with nearest-neighbour chroma (cx = x >> shiftH, cy = y >> shiftV: yuv2rgb.cc:200-203).  Coordinates
// beyond the image are clamped to its last column / row: that is the pixel x2 / y2 of Op_RGB_to_YCbCr's 2x2 box falls back to
// (rgb2yuv.cc:237-238).
// ---------------------------------------------------------------------------------------
template <typename Pix, bool FROM_YCBCR>
__device__ __forceinline__ void rgb_row(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ p1, const uint8_t* __restrict__ p2, int s0, int s1, int s2,
                                        const FloatParams& fp, int x0, int py, int w, bool full, int* r, int* g, int* b)
{
  constexpr int N = Lane<Pix>::N;
  if (!FROM_YCBCR) {
    load_row<Pix>(p0 + (size_t)py * s0, x0, w, full, r);
    load_row<Pix>(p1 + (size_t)py * s1, x0, w, full, g);
    load_row<Pix>(p2 + (size_t)py * s2, x0, w, full, b);
    return;
  }
  int yv[N], uu[N], vv[N];
  load_row<Pix>(p0 + (size_t)py * s0, x0, w, full, yv);
  const int cy = py >> fp.shiftV;
  const uint8_t* __restrict__ ru = p1 + (size_t)cy * s1;
  const uint8_t* __restrict__ rv = p2 + (size_t)cy * s2;
  if (!fp.shiftH) {
    load_row<Pix>(ru, x0, w, full, uu);
    load_row<Pix>(rv, x0, w, full, vv);
  }
  else if (full) {
    int hu[N / 2], hv[N / 2];
    unpack8<Pix>(*reinterpret_cast<const uint2*>(ru + (size_t)(x0 >> 1) * sizeof(Pix)), hu);
    unpack8<Pix>(*reinterpret_cast<const uint2*>(rv + (size_t)(x0 >> 1) * sizeof(Pix)), hv);
#pragma unroll
    for (int i = 0; i < N; i++) { uu[i] = hu[i >> 1]; vv[i] = hv[i >> 1]; }
  }
  else {
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int px = x0 + i < w ? x0 + i : w - 1;
      uu[i] = reinterpret_cast<const Pix*>(ru)[px >> 1];
      vv[i] = reinterpret_cast<const Pix*>(rv)[px >> 1];
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) px_float(fp, yv[i], uu[i], vv[i], r[i], g[i], b[i]);
}

// Op_YCbCr_to_RGB to three planes of one stride
template <typename Pix>
__global__ __launch_bounds__(256) void k_to_rgb_planes(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ Cb, const uint8_t* __restrict__ Cr, int ys, int cbs, int crs,
                                                       uint8_t* __restrict__ R, uint8_t* __restrict__ G, uint8_t* __restrict__ B, int os, int w, int h,
                                                       FloatParams fp, int groups_per_row, int total_groups)
{
  constexpr int N = Lane<Pix>::N;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= total_groups) return;
  const int py = gid / groups_per_row;
  const int x0 = (gid - py * groups_per_row) * N;
  const bool full = x0 + N <= w;
  int r[N], g[N], b[N];
  rgb_row<Pix, true>(Y, Cb, Cr, ys, cbs, crs, fp, x0, py, w, full, r, g, b);
  store_row<Pix>(R + (size_t)py * os, x0, w, full, r);
  store_row<Pix>(G + (size_t)py * os, x0, w, full, g);
  store_row<Pix>(B + (size_t)py * os, x0, w, full, b);
}

// Op_RGB_to_YCbCr's own parameters: RGB_to_YCbCr_coefficients row by row, the target's range and matrix class
struct ToYCbCrParams {
  float c[9];
  float lim_off;  // 16 << (bpp - 8)
  float half;     // halfRange as the float the reference adds
  int maxv;
  int mode;       // 0 matrix, 1 GBR full range (copies), 2 GBR limited range
  int limited;    // !full_range (mode 0)
  int subH;       // the target's horizontal sub-sampling (1 / 2); the vertical one is the ROWS template argument
};

__device__ __forceinline__ float scale_256(float v, float num) { return __fmul_rn(__fmul_rn(v, num), 0.00390625f); } // (v * num) / 256: the division is exact

__device__ __forceinline__ int luma_of(const ToYCbCrParams& t, int r, int g, int b) // rgb2yuv.cc:194-218
{
  if (t.mode == 1) return g;
  if (t.mode == 2) return clip_f(__fadd_rn(scale_256((float)g, 219.0f), t.lim_off), t.maxv);
  float v = __fadd_rn(__fadd_rn(__fmul_rn((float)r, t.c[0]), __fmul_rn((float)g, t.c[1])), __fmul_rn((float)b, t.c[2]));
  if (t.limited) v = __fadd_rn(scale_256(v, 219.0f), t.lim_off);
  return clip_f(v, t.maxv);
}

// r, g, b: the (box-averaged) values as floats (rgb2yuv.cc:231-266)
__device__ __forceinline__ void chroma_of(const ToYCbCrParams& t, float r, float g, float b, int& cb, int& cr)
{
  float fcb = __fadd_rn(__fadd_rn(__fmul_rn(r, t.c[3]), __fmul_rn(g, t.c[4])), __fmul_rn(b, t.c[5]));
  float fcr = __fadd_rn(__fadd_rn(__fmul_rn(r, t.c[6]), __fmul_rn(g, t.c[7])), __fmul_rn(b, t.c[8]));
  if (t.limited) { fcb = scale_256(fcb, 224.0f); fcr = scale_256(fcr, 224.0f); }
  cb = clip_f(__fadd_rn(fcb, t.half), t.maxv);
  cr = clip_f(__fadd_rn(fcr, t.half), t.maxv);
}

// GBR targets take the top-left sample of the box (rgb2yuv.cc:222-230)
__device__ __forceinline__ void chroma_gbr(const ToYCbCrParams& t, int r, int b, int& cb, int& cr)
{
  if (t.mode == 1) { cb = b; cr = r; return; }
  cb = clip_f(__fadd_rn(scale_256((float)b, 224.0f), t.lim_off), t.maxv);
  cr = clip_f(__fadd_rn(scale_256((float)r, 224.0f), t.lim_off), t.maxv);
}

// One lane: N pixels x ROWS rows (ROWS = 2: a 4:2:0 target).  Luma of every pixel; chroma: one sample per pixel (4:4:4), per
// pixel pair of the row taken from its left pixel (4:2:2: the reference's box degenerates to x2 = x, y2 = y there, and
// (4 r) * 0.25f is r), or per 2x2 box averaged (4:2:0: the four samples summed - exact in binary32 - times 0.25f).
template <typename Pix, bool FROM_YCBCR, int ROWS>
__global__ __launch_bounds__(256) void k_to_ycbcr(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ p1, const uint8_t* __restrict__ p2, int s0, int s1, int s2,
                                                  FloatParams fp, uint8_t* __restrict__ oy, uint8_t* __restrict__ ocb, uint8_t* __restrict__ ocr, int oys, int ocbs, int ocrs,
                                                  int w, int h, ToYCbCrParams t, int groups_per_row, int total_groups)
{
  constexpr int N = Lane<Pix>::N;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= total_groups) return;
  const int gy = gid / groups_per_row;
  const int x0 = (gid - gy * groups_per_row) * N;
  const int y0 = gy * ROWS;
  const bool full = x0 + N <= w;
  int sr[N], sg[N], sb[N]; // per chroma sample: sums over the box (mode 0), the top-left sample (GBR)
#pragma unroll
  for (int j = 0; j < ROWS; j++) {
    const int py = y0 + j < h ? y0 + j : h - 1;
    int r[N], g[N], b[N], yv[N];
    rgb_row<Pix, FROM_YCBCR>(p0, p1, p2, s0, s1, s2, fp, x0, py, w, full, r, g, b);
    if (y0 + j < h) {
#pragma unroll
      for (int i = 0; i < N; i++) yv[i] = luma_of(t, r[i], g[i], b[i]);
      store_row<Pix>(oy + (size_t)py * oys, x0, w, full, yv);
    }
    if (ROWS == 2) {
#pragma unroll
      for (int i = 0; i < N / 2; i++) {
        if (j == 0) { sr[i] = r[2 * i]; sg[i] = g[2 * i]; sb[i] = b[2 * i]; if (t.mode == 0) { sr[i] += r[2 * i + 1]; sg[i] += g[2 * i + 1]; sb[i] += b[2 * i + 1]; } }
        else if (t.mode == 0) { sr[i] += r[2 * i] + r[2 * i + 1]; sg[i] += g[2 * i] + g[2 * i + 1]; sb[i] += b[2 * i] + b[2 * i + 1]; }
      }
    }
    else {
#pragma unroll
      for (int i = 0; i < N; i++) { sr[i] = r[i]; sg[i] = g[i]; sb[i] = b[i]; }
    }
  }
  int cb[N], cr[N];
  if (ROWS == 2) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      if (t.mode == 0) chroma_of(t, __fmul_rn((float)sr[i], 0.25f), __fmul_rn((float)sg[i], 0.25f), __fmul_rn((float)sb[i], 0.25f), cb[i], cr[i]);
      else chroma_gbr(t, sr[i], sb[i], cb[i], cr[i]);
    }
    const int cw = (w + 1) >> 1;
    store_half_row<Pix>(ocb + (size_t)gy * ocbs, x0 >> 1, cw, full, cb);
    store_half_row<Pix>(ocr + (size_t)gy * ocrs, x0 >> 1, cw, full, cr);
  }
  else if (t.subH == 2) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      if (t.mode == 0) chroma_of(t, (float)sr[2 * i], (float)sg[2 * i], (float)sb[2 * i], cb[i], cr[i]);
      else chroma_gbr(t, sr[2 * i], sb[2 * i], cb[i], cr[i]);
    }
    const int cw = (w + 1) >> 1;
    store_half_row<Pix>(ocb + (size_t)gy * ocbs, x0 >> 1, cw, full, cb);
    store_half_row<Pix>(ocr + (size_t)gy * ocrs, x0 >> 1, cw, full, cr);
  }
  else {
#pragma unroll
    for (int i = 0; i < N; i++) {
      if (t.mode == 0) chroma_of(t, (float)sr[i], (float)sg[i], (float)sb[i], cb[i], cr[i]);
      else chroma_gbr(t, sr[i], sb[i], cb[i], cr[i]);
    }
    store_row<Pix>(ocb + (size_t)gy * ocbs, x0, w, full, cb);
    store_row<Pix>(ocr + (size_t)gy * ocrs, x0, w, full, cr);
  }
}

bool aligned16(const void* p, int stride) { return ((uintptr_t)p % 16) == 0 && (stride % 16) == 0; }

// Op_YCbCr_to_RGB's parameters for planes as its output: no depth change behind it
void float_params_planes(const hm_colour_desc* img, const float coef[4], int mode, FloatParams* fp)
{
  hm_float_params(img, coef, mode, fp);
  fp->post = 0; fp->s1 = fp->s2 = 0;
}

template <typename Pix, bool V420>
int launch_average(const void* cb, int is_cb, const void* cr, int is_cr, void* ocb, int os_cb, void* ocr, int os_cr, int w, int h, hipStream_t s)
{
  const int cw = (w + 1) / 2, ch = V420 ? (h + 1) / 2 : h;
  const int gpr = (cw + 7) / 8;
  const long total = (long)gpr * ch;
  if (total <= 0) return HM_OK;
  hipLaunchKernelGGL((k_average_down<Pix, V420>), dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, s, (const uint8_t*)cb, (const uint8_t*)cr, is_cb, is_cr,
                     (uint8_t*)ocb, (uint8_t*)ocr, os_cb, os_cr, w, h, cw, gpr, (int)total);
  return hm_check_hip(hipGetLastError(), "k_average_down launch");
}

template <typename Pix, bool FROM_YCBCR, int ROWS>
int launch_to_ycbcr(const hm_to_ycbcr* a, const FloatParams& fp, const ToYCbCrParams& t, hipStream_t s)
{
  constexpr int N = Lane<Pix>::N;
  const int gpr = (a->w + N - 1) / N;
  const long total = (long)gpr * ((a->h + ROWS - 1) / ROWS);
  if (total <= 0) return HM_OK;
  hipLaunchKernelGGL((k_to_ycbcr<Pix, FROM_YCBCR, ROWS>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint8_t*)a->src[0], (const uint8_t*)a->src[1],
                     (const uint8_t*)a->src[2], a->src_stride[0], a->src_stride[1], a->src_stride[2], fp, (uint8_t*)a->dst[0], (uint8_t*)a->dst[1], (uint8_t*)a->dst[2],
                     a->dst_stride[0], a->dst_stride[1], a->dst_stride[2], a->w, a->h, t, gpr, (int)total);
  return hm_check_hip(hipGetLastError(), "k_to_ycbcr launch");
}

template <typename Pix, bool FROM_YCBCR>
int launch_to_ycbcr_rows(const hm_to_ycbcr* a, const FloatParams& fp, const ToYCbCrParams& t, hipStream_t s)
{
  return a->chroma == HM_CHROMA_420 ? launch_to_ycbcr<Pix, FROM_YCBCR, 2>(a, fp, t, s) : launch_to_ycbcr<Pix, FROM_YCBCR, 1>(a, fp, t, s);
}

} // namespace

int hm_launch_average_down(int bits, int v420, const void* cb, int cb_stride, const void* cr, int cr_stride, void* ocb, int ocb_stride,
                           void* ocr, int ocr_stride, int w, int h, hipStream_t s)
{
  if (!aligned16(cb, cb_stride) || !aligned16(cr, cr_stride) || !aligned16(ocb, ocb_stride) || !aligned16(ocr, ocr_stride))
    return hm_fail(HM_ERR_INVALID_ARG, "planes must be 16-byte aligned with 16-byte multiple strides");
  if (bits == 8) return v420 ? launch_average<uint8_t, true>(cb, cb_stride, cr, cr_stride, ocb, ocb_stride, ocr, ocr_stride, w, h, s)
                             : launch_average<uint8_t, false>(cb, cb_stride, cr, cr_stride, ocb, ocb_stride, ocr, ocr_stride, w, h, s);
  return v420 ? launch_average<uint16_t, true>(cb, cb_stride, cr, cr_stride, ocb, ocb_stride, ocr, ocr_stride, w, h, s)
              : launch_average<uint16_t, false>(cb, cb_stride, cr, cr_stride, ocb, ocb_stride, ocr, ocr_stride, w, h, s);
}

int hm_launch_ycbcr_to_rgb_planes(const hm_colour_desc* img, const float coef[4], int mode, const void* y, const void* cb, const void* cr,
                                  void* const rgb[3], int rgb_stride, hipStream_t s)
{
  if (!aligned16(y, img->y_stride) || !aligned16(cb, img->cb_stride) || !aligned16(cr, img->cr_stride) || !aligned16(rgb[0], rgb_stride) ||
      !aligned16(rgb[1], rgb_stride) || !aligned16(rgb[2], rgb_stride))
    return hm_fail(HM_ERR_INVALID_ARG, "planes must be 16-byte aligned with 16-byte multiple strides");
  FloatParams fp;
  float_params_planes(img, coef, mode, &fp);
  const int N = img->bit_depth == 8 ? 16 : 8;
  const int gpr = (img->width + N - 1) / N;
  const long total = (long)gpr * img->height;
  if (total <= 0) return HM_OK;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (img->bit_depth == 8)
    hipLaunchKernelGGL((k_to_rgb_planes<uint8_t>), grid, dim3(256), 0, s, (const uint8_t*)y, (const uint8_t*)cb, (const uint8_t*)cr, img->y_stride, img->cb_stride,
                       img->cr_stride, (uint8_t*)rgb[0], (uint8_t*)rgb[1], (uint8_t*)rgb[2], rgb_stride, img->width, img->height, fp, gpr, (int)total);
  else
    hipLaunchKernelGGL((k_to_rgb_planes<uint16_t>), grid, dim3(256), 0, s, (const uint8_t*)y, (const uint8_t*)cb, (const uint8_t*)cr, img->y_stride, img->cb_stride,
                       img->cr_stride, (uint8_t*)rgb[0], (uint8_t*)rgb[1], (uint8_t*)rgb[2], rgb_stride, img->width, img->height, fp, gpr, (int)total);
  return hm_check_hip(hipGetLastError(), "k_to_rgb_planes launch");
}

int hm_launch_to_ycbcr(const hm_to_ycbcr* a, hipStream_t s)
{
  for (int c = 0; c < 3; c++)
    if (!aligned16(a->src[c], a->src_stride[c]) || !aligned16(a->dst[c], a->dst_stride[c]))
      return hm_fail(HM_ERR_INVALID_ARG, "planes must be 16-byte aligned with 16-byte multiple strides");
  ToYCbCrParams t;
  hm_rgb_to_ycbcr_coefficients(a->matrix, a->primaries, t.c);
  t.lim_off = (float)(16 << (a->bits - 8));
  t.half = (float)(1 << (a->bits - 1));
  t.maxv = (1 << a->bits) - 1;
  t.mode = a->matrix == 0 ? (a->full_range ? 1 : 2) : 0;
  t.limited = !a->full_range;
  t.subH = a->chroma == HM_CHROMA_444 ? 1 : 2;
  FloatParams fp;
  if (a->ycbcr_src) {
    float_params_planes(a->ycbcr_src, a->src_coef, a->src_mode, &fp);
    return a->bits == 8 ? launch_to_ycbcr_rows<uint8_t, true>(a, fp, t, s) : launch_to_ycbcr_rows<uint16_t, true>(a, fp, t, s);
  }
  std::memset(&fp, 0, sizeof(fp));
  return a->bits == 8 ? launch_to_ycbcr_rows<uint8_t, false>(a, fp, t, s) : launch_to_ycbcr_rows<uint16_t, false>(a, fp, t, s);
}
