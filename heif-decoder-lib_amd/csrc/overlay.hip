// overlay.hip — k_overlay: the composition of an 'iovl' item on the device (gfx950).
//
// The reference composes on the host, one pass over the canvas per layer and channel (HeifContext::decode_overlay_image,
// context.cc:2579-2675; HeifPixelImage::overlay, pixelimage.cc:1022-1153), after converting every layer to R, G, B planes
// (Op_YCbCr_to_RGB<uint8_t>, yuv2rgb.cc:79-254).  Here the layers sit in HBM as their decoded 8-bit Y / Cb / Cr (+ alpha) planes
// and ONE streaming kernel produces the canvas: per canvas pixel the background, then every layer that covers it from the bottom
// up - converted with the op's own arithmetic (px_float, colour_float.h: the device function of k_ycbcr_float and
// k_to_rgb_planes) and either copied (no alpha plane: the reference's memcpy) or blended,
//   out = (in * a + out * (255 - a)) / 255   in integers, truncating (pixelimage.cc:1146; hm_div255),
// and one store of the result: interleaved RGB24 / RGBA32 (alpha 255: Op_RGB_to_RGB24_32) or R, G, B planes.
//
// Mapping: wave64, no LDS.  A lane owns 4 consecutive canvas pixels of one row (one 16-byte store for RGBA32, 12 bytes for RGB24,
// 4 bytes per plane), a wave 256 consecutive pixels (HM_OVL_SPAN), a workgroup of four waves four rows.  The row and the span are
// the same in every lane of a wave, so the layer table is read with wave-uniform loads and the row / span tests of a layer are
// scalar branches; only the lanes inside a layer's rectangle load its samples.  The loop starts at the span's start layer
// (hm_ovl_start_layer, hm_overlay_plan.h): the highest layer without alpha that covers the whole span - nothing below it is read.
// The last group of a row is stored element by element: nothing but w x h x C bytes is written.
// Loads: a layer's samples are not aligned to the lane's group (dx is arbitrary), so they are byte loads - per covered pixel
// 1 (Y) + 2 (Cb, Cr; none for a monochrome layer) + 1 (alpha, if any), neighbouring lanes reading neighbouring bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "colour_float.h"
#include "hm_overlay.h"

namespace {

// device image of one layer (behind the table's hm_ovl_rect array)
struct OvlLayer {
  const uint8_t* p[4];
  int32_t pitch[4];
  FloatParams fp;
  int32_t mono, has_alpha;
};

template <int OUT>
__global__ __launch_bounds__(256) void k_overlay(const hm_ovl_rect* __restrict__ rects, const OvlLayer* __restrict__ layers, int n, int use_start,
                                                 int bg_r, int bg_g, int bg_b, uint8_t* __restrict__ o0, uint8_t* __restrict__ o1, uint8_t* __restrict__ o2,
                                                 int opitch, int W, int H)
{
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.y * 4 + wave;
  if (y >= H) return;
  const int sx0 = blockIdx.x * HM_OVL_SPAN;
  const int sx1 = sx0 + HM_OVL_SPAN < W ? sx0 + HM_OVL_SPAN : W;
  const int x = sx0 + lane * 4;
  int r[4], g[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; i++) { r[i] = bg_r; g[i] = bg_g; b[i] = bg_b; }
  const int start = use_start ? hm_ovl_start_layer(rects, n, sx0, sx1, y) : 0;
  for (int l = start; l < n; l++) {
    const hm_ovl_rect R = rects[l];
    if (y < R.y0 || y >= R.y1 || R.x1 <= sx0 || R.x0 >= sx1) continue; // (wave-uniform)
    const OvlLayer& L = layers[l];
    const int sy = y - R.y0 + R.sy;
    const int shiftH = L.fp.shiftH;
    const uint8_t* __restrict__ ry = L.p[0] + (size_t)sy * L.pitch[0];
    const uint8_t* __restrict__ ru = L.mono ? ry : L.p[1] + (size_t)(sy >> L.fp.shiftV) * L.pitch[1];
    const uint8_t* __restrict__ rv = L.mono ? ry : L.p[2] + (size_t)(sy >> L.fp.shiftV) * L.pitch[2];
    const uint8_t* __restrict__ ra = L.has_alpha ? L.p[3] + (size_t)sy * L.pitch[3] : ry;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int px = x + i;
      if (px < R.x0 || px >= R.x1) continue;
      const int sx = px - R.x0 + R.sx;
      const int Yv = ry[sx];
      int U = 128, V = 128;
      if (!L.mono) { U = ru[sx >> shiftH]; V = rv[sx >> shiftH]; }
      int lr, lg, lb;
      px_float(L.fp, Yv, U, V, lr, lg, lb);
      if (L.has_alpha) {
        const uint32_t a = ra[sx];
        r[i] = (int)hm_div255((uint32_t)lr * a + (uint32_t)r[i] * (255u - a));
        g[i] = (int)hm_div255((uint32_t)lg * a + (uint32_t)g[i] * (255u - a));
        b[i] = (int)hm_div255((uint32_t)lb * a + (uint32_t)b[i] * (255u - a));
      }
      else { r[i] = lr; g[i] = lg; b[i] = lb; }
    }
  }
  if (x >= W) return;
  const bool full = x + 4 <= W;
  if (OUT == HM_OVL_OUT_RGBA32) {
    uint8_t* __restrict__ o = o0 + (size_t)y * opitch + (size_t)x * 4;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)r[i] | ((uint32_t)g[i] << 8) | ((uint32_t)b[i] << 16) | 0xFF000000u;
    if (full) *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (x + i < W) reinterpret_cast<uint32_t*>(o)[i] = w[i];
    }
  }
  else if (OUT == HM_OVL_OUT_RGB24) {
    uint8_t* __restrict__ o = o0 + (size_t)y * opitch + (size_t)x * 3;
    if (full) {
      struct W3 { uint32_t a, b, c; };
      W3 w;
      w.a = (uint32_t)r[0] | ((uint32_t)g[0] << 8) | ((uint32_t)b[0] << 16) | ((uint32_t)r[1] << 24);
      w.b = (uint32_t)g[1] | ((uint32_t)b[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)g[2] << 24);
      w.c = (uint32_t)b[2] | ((uint32_t)r[3] << 8) | ((uint32_t)g[3] << 16) | ((uint32_t)b[3] << 24);
      *reinterpret_cast<W3*>(o) = w;
    }
    else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (x + i < W) { o[3 * i] = (uint8_t)r[i]; o[3 * i + 1] = (uint8_t)g[i]; o[3 * i + 2] = (uint8_t)b[i]; }
    }
  }
  else {
    const size_t off = (size_t)y * opitch + (size_t)x;
    if (full) {
      *reinterpret_cast<uint32_t*>(o0 + off) = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
      *reinterpret_cast<uint32_t*>(o1 + off) = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16) | ((uint32_t)g[3] << 24);
      *reinterpret_cast<uint32_t*>(o2 + off) = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (x + i < W) { o0[off + i] = (uint8_t)r[i]; o1[off + i] = (uint8_t)g[i]; o2[off + i] = (uint8_t)b[i]; }
    }
  }
}

size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// every sample the kernel can read of this layer lies inside its planes, and its rectangle inside the canvas
bool layer_in_bounds(const hm_overlay_job* job, const hm_overlay_layer& L)
{
  const hm_ovl_rect& R = L.rect;
  if (R.x0 < 0 || R.y0 < 0 || R.x0 >= R.x1 || R.y0 >= R.y1 || R.x1 > job->width || R.y1 > job->height || R.sx < 0 || R.sy < 0) return false;
  const int64_t last_x = (int64_t)R.sx + (R.x1 - R.x0) - 1, last_y = (int64_t)R.sy + (R.y1 - R.y0) - 1;
  if (last_x >= L.width || last_y >= L.height) return false;
  if (!L.plane[0] || L.pitch[0] < L.width || L.plane_w[0] < L.width || L.plane_h[0] < L.height) return false;
  if (L.plane[3] && (L.pitch[3] < L.width || L.plane_w[3] < L.width || L.plane_h[3] < L.height)) return false;
  if (L.chroma != 0) {
    if (L.chroma < 1 || L.chroma > 3 || !L.plane[1] || !L.plane[2]) return false;
    const int cw = L.chroma == HM_CHROMA_444 ? L.width : (L.width + 1) / 2;
    const int ch = L.chroma == HM_CHROMA_420 ? (L.height + 1) / 2 : L.height;
    for (int c = 1; c <= 2; c++)
      if (L.pitch[c] < cw || L.plane_w[c] < cw || L.plane_h[c] < ch) return false;
  }
  return true;
}

} // namespace

int hm_launch_overlay(const hm_overlay_job* job, const hm_overlay_layer* layers, int n, void** pinned, void** device, hipStream_t s)
{
  if (!job || !pinned || !device || n < 0 || (n > 0 && !layers)) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  *pinned = *device = nullptr;
  const int W = job->width, H = job->height;
  if (W <= 0 || H <= 0) return hm_fail(HM_ERR_INVALID_ARG, "overlay canvas %d x %d", W, H);
  const int bpp = job->out_kind == HM_OVL_OUT_RGB24 ? 3 : (job->out_kind == HM_OVL_OUT_RGBA32 ? 4 : 1);
  if (job->out_kind < 0 || job->out_kind > HM_OVL_OUT_PLANES) return hm_fail(HM_ERR_INVALID_ARG, "overlay output kind %d", job->out_kind);
  if (!job->out[0] || (job->out_kind == HM_OVL_OUT_PLANES && (!job->out[1] || !job->out[2]))) return hm_fail(HM_ERR_INVALID_ARG, "overlay output: null pointer");
  if ((int64_t)job->out_pitch < (int64_t)W * bpp || (job->out_pitch & 3)) return hm_fail(HM_ERR_INVALID_ARG, "overlay output pitch %d", job->out_pitch);
  for (int c = 0; c < (job->out_kind == HM_OVL_OUT_PLANES ? 3 : 1); c++)
    if ((uintptr_t)job->out[c] & 15) return hm_fail(HM_ERR_INVALID_ARG, "overlay output must be 16-byte aligned");
  for (int l = 0; l < n; l++)
    if (!layer_in_bounds(job, layers[l])) return hm_fail(HM_ERR_INTERNAL, "overlay layer %d reaches outside its planes or the canvas", l);

  // the table: the rectangles (what the start-layer search walks), then the layers; one pinned block, one upload
  const size_t rect_bytes = round16(sizeof(hm_ovl_rect) * (size_t)(n > 0 ? n : 1));
  const size_t bytes = rect_bytes + sizeof(OvlLayer) * (size_t)(n > 0 ? n : 1);
  uint8_t* host = (uint8_t*)hm_pool_pinned_alloc(bytes);
  uint8_t* dev = (uint8_t*)hm_pool_device_alloc(bytes);
  *pinned = host; *device = dev;
  if (!host || !dev) return hm_fail(HM_ERR_NOMEM, "overlay layer table: out of memory");
  std::memset(host, 0, bytes);
  hm_ovl_rect* hr = reinterpret_cast<hm_ovl_rect*>(host);
  OvlLayer* hl = reinterpret_cast<OvlLayer*>(host + rect_bytes);
  for (int l = 0; l < n; l++) {
    const hm_overlay_layer& L = layers[l];
    hr[l] = L.rect;
    hr[l].opaque = L.plane[3] ? 0 : 1;
    for (int c = 0; c < 4; c++) { hl[l].p[c] = (const uint8_t*)L.plane[c]; hl[l].pitch[c] = L.pitch[c]; }
    hl[l].mono = L.chroma == 0;
    hl[l].has_alpha = L.plane[3] != nullptr;
    // Op_YCbCr_to_RGB's parameters for the image it is handed (the last lines of hm_colour_float_chain): 8-bit samples, planes out
    hm_colour_desc cd;
    std::memset(&cd, 0, sizeof(cd));
    cd.width = L.width; cd.height = L.height; cd.bit_depth = 8; cd.chroma = L.chroma == 0 ? HM_CHROMA_444 : L.chroma;
    cd.has_nclx = L.has_nclx; cd.matrix = L.matrix; cd.primaries = L.primaries; cd.full_range = L.full_range;
    cd.out_format = HM_OUT_RGB;
    float cf[4];
    hm_ycbcr_coefficients(cd.has_nclx, cd.matrix, cd.primaries, cf);
    const int m = cd.has_nclx ? cd.matrix : 2;
    const bool full = cd.has_nclx ? cd.full_range != 0 : true;
    hm_float_params(&cd, cf, m == 0 ? (full ? 1 : 2) : (m == 8 ? 3 : 0), &hl[l].fp);
  }
  hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hm_check_hip(e, "overlay layer table upload");
  const dim3 grid((unsigned)((W + HM_OVL_SPAN - 1) / HM_OVL_SPAN), (unsigned)((H + 3) / 4));
  if (grid.y > 65535u) return hm_fail(HM_ERR_UNSUPPORTED, "overlay canvas of %d rows", H);
  const hm_ovl_rect* dr = reinterpret_cast<const hm_ovl_rect*>(dev);
  const OvlLayer* dl = reinterpret_cast<const OvlLayer*>(dev + rect_bytes);
  const int use_start = hm_knob(HM_KNOB_OVERLAY_START) != 0;
  const int br = job->background[0], bg = job->background[1], bb = job->background[2];
  uint8_t* o0 = (uint8_t*)job->out[0];
  uint8_t* o1 = (uint8_t*)job->out[1];
  uint8_t* o2 = (uint8_t*)job->out[2];
  if (job->out_kind == HM_OVL_OUT_RGB24)
    hipLaunchKernelGGL((k_overlay<HM_OVL_OUT_RGB24>), grid, dim3(256), 0, s, dr, dl, n, use_start, br, bg, bb, o0, o1, o2, job->out_pitch, W, H);
  else if (job->out_kind == HM_OVL_OUT_RGBA32)
    hipLaunchKernelGGL((k_overlay<HM_OVL_OUT_RGBA32>), grid, dim3(256), 0, s, dr, dl, n, use_start, br, bg, bb, o0, o1, o2, job->out_pitch, W, H);
  else
    hipLaunchKernelGGL((k_overlay<HM_OVL_OUT_PLANES>), grid, dim3(256), 0, s, dr, dl, n, use_start, br, bg, bb, o0, o1, o2, job->out_pitch, W, H);
  return hm_check_hip(hipGetLastError(), "k_overlay launch");
}

// (test hook, test_hooks.cpp) the instances of k_overlay: 0 RGB24, 1 RGBA32, 2 planes; NULL behind the last
extern "C" const void* hm_overlay_kernel_of(int index)
{
  if (index == 0) return reinterpret_cast<const void*>(&k_overlay<HM_OVL_OUT_RGB24>);
  if (index == 1) return reinterpret_cast<const void*>(&k_overlay<HM_OVL_OUT_RGBA32>);
  if (index == 2) return reinterpret_cast<const void*>(&k_overlay<HM_OVL_OUT_PLANES>);
  return nullptr;
}
