// unci.hip - the samples of an ISO/IEC 23001-17 uncompressed ('unci') item, gathered from its payload on the device (gfx950):
//   k_unci_unpack   payload bytes -> planes (each mapped component at its own depth: bytes up to 8 bits, 16-bit words above) and / or
//                   interleaved R G B [A] pixels of 8 or 16 bits
// A memory-bound gather with no LDS: where a sample lies follows from the closed form of hm_unci_layout.h - eleven numbers per
// component in the kernel arguments, one division per lane for the tile column and one for the tile row; no lane ever walks bits.
// ONE launch covers every plane and the interleaved pixels: blockIdx.z is the job (a plane, or the pixels), so the component, its
// depth and its path are wave-uniform.  A wave takes 64 consecutive groups of ONE row; a lane's group is one dword of a plane (4
// samples up to 8 bits, 2 above) - four dwords and one 16-byte store where the samples are runs of consecutive bytes - or 12 / 16 bytes of
// pixels (4 pixels of 8 bits, 2 of 16), so neighbouring lanes take neighbouring output samples and every store of a full group is a dword or wider.
// Loads are aligned dwords of the payload:
//   generic path   the dword that holds the sample's most significant bit and, when the sample reaches into it, the next one; both
//                  byte-swapped (the packing is MSB-first) and funnel-shifted: (w0:w1 << phase) >> (64 - depth).  depth <= 16 and
//                  phase <= 31, so two dwords always hold a sample.
//   byte path      every mapped component 8 bits deep at byte positions (all 8-bit modes without bit padding): nothing is
//                  swapped or masked across dwords - a run of 4 samples that lie in 4 consecutive bytes (component, row and
//                  tile-component modes) is two dwords and one funnel shift by the byte phase, any other sample one dword and a byte
//                  extract.
// Nothing behind the payload is read: the last, partial dword is assembled from its own bytes by the lanes that need it, and a dword
// behind it reads as 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hm_internal.h"
#include "hm_unci_layout.h"

namespace {

struct UnciComp {
  uint64_t base, tile_stride, row_stride; // hm_unci_comp_layout's, bytes
  uint32_t first_len, stride, off0, off1; // bits
  uint32_t tw, th, depth;
  uint32_t present;
};

enum { JOB_PIXELS = 4 };

struct UnciArgs {
  const uint32_t* src;
  uint64_t n_full;       // whole dwords of the payload
  uint32_t tail_bytes;   // bytes of the partial dword behind them (0..3)
  uint32_t tile_cols;
  UnciComp c[4];         // by output plane: 0..2 colour, 3 alpha
  uint8_t* plane[4];
  int32_t  stride[4];
  uint32_t plane_vec[4]; // pointer and stride are 16-byte aligned: a lane's 4 dwords go out in one store
  uint32_t pw[4], ph[4]; // the planes' sizes in samples
  uint32_t byte_path;    // every present component: 8 bits at byte positions
  uint32_t n_jobs;
  uint32_t job[5];       // 0..3: plane, JOB_PIXELS
  // the interleaved pixels
  uint8_t* px;
  int64_t  px_pitch;
  uint32_t px_channels, px_wide, px_dwords_ok; // 3 / 4; 16-bit elements; pointer and pitch allow dword stores
  uint32_t w, h;
};

__device__ __forceinline__ uint32_t load_dword(const UnciArgs& a, uint64_t i)
{
  if (i < a.n_full) return a.src[i];
  uint32_t v = 0;
  if (i == a.n_full) { // (the payload's last bytes: only the lanes that reach them come here)
    const uint8_t* p = reinterpret_cast<const uint8_t*>(a.src + i);
    for (uint32_t k = 0; k < a.tail_bytes; k++) v |= (uint32_t)p[k] << (8 * k);
  }
  return v;
}

// where a lane's run of samples starts: one division per axis, then the run steps along the row
struct Cursor {
  uint64_t row;   // bit position of the tile row's start
  uint32_t lx;    // column inside the tile
  __device__ __forceinline__ Cursor(const UnciArgs& a, const UnciComp& c, uint32_t x, uint32_t y)
  {
    const uint32_t tx = x / c.tw, ty = y / c.th;
    lx = x - tx * c.tw;
    row = (c.base + ((uint64_t)ty * a.tile_cols + tx) * c.tile_stride + (uint64_t)(y - ty * c.th) * c.row_stride) * 8;
  }
  __device__ __forceinline__ uint64_t bit(const UnciComp& c) const
  {
    return row + (lx == 0 ? (uint64_t)c.off0 : (uint64_t)c.first_len + (uint64_t)(lx - 1) * c.stride + c.off1);
  }
  __device__ __forceinline__ void step(const UnciComp& c)
  {
    if (++lx == c.tw) { lx = 0; row += c.tile_stride * 8; }
  }
};

template <bool BYTES>
__device__ __forceinline__ uint32_t fetch(const UnciArgs& a, const UnciComp& c, uint64_t bit)
{
  if (BYTES) {
    const uint64_t at = bit >> 3;
    return (load_dword(a, at >> 2) >> (8 * (uint32_t)(at & 3))) & 0xFFu;
  }
  const uint64_t i = bit >> 5;
  const uint32_t phase = (uint32_t)bit & 31;
  const uint32_t w0 = __builtin_bswap32(load_dword(a, i));
  const uint32_t w1 = phase + c.depth > 32 ? __builtin_bswap32(load_dword(a, i + 1)) : 0;
  const uint64_t v = ((uint64_t)w0 << 32) | w1;
  return (uint32_t)((v << phase) >> (64 - c.depth));
}

// one or four dwords of plane p, each 4 samples of up to 8 bits or 2 deeper ones; samples behind the row's end are 0, dwords behind it are not written
template <bool BYTES>
__device__ __forceinline__ void plane_group(const UnciArgs& a, int p, uint32_t g, uint32_t y)
{
  const UnciComp& c = a.c[p];
  const uint32_t n = c.depth > 8 ? 2 : 4, w = a.pw[p];
  const uint32_t dwords = (w + n - 1) / n; // of the row
  // runs of consecutive bytes: four dwords per lane; strided samples (a load or two each): one dword per lane, measured faster there
  const uint32_t per = BYTES && c.stride == 8 && c.first_len == 8 ? 4 : 1;
  const uint32_t d0 = g * per;
  if (d0 >= dwords) return;
  Cursor k(a, c, d0 * n, y);
  uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const uint32_t x0 = (d0 + d) * n;
    if ((uint32_t)d >= per || x0 >= w) break;
    if (BYTES && c.stride == 8 && c.first_len == 8 && k.lx + 4 <= c.tw) { // 4 consecutive bytes (the row's padding is the payload's own bytes or 0)
      const uint64_t at = k.bit(c) >> 3;
      const uint32_t lo = load_dword(a, at >> 2), sh = 8 * (uint32_t)(at & 3);
      const uint32_t hi = sh ? load_dword(a, (at >> 2) + 1) : 0;
      uint32_t o = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
      if (x0 + 4 > w) o &= 0xFFFFFFFFu >> (8 * (x0 + 4 - w));
      out[d] = o;
      k.lx += 4;
      if (k.lx == c.tw) { k.lx = 0; k.row += c.tile_stride * 8; }
    }
    else {
      const uint32_t shift = c.depth > 8 ? 16 : 8;
      uint32_t o = 0;
      for (uint32_t i = 0; i < n && x0 + i < w; i++) {
        o |= fetch<BYTES>(a, c, k.bit(c)) << (shift * i);
        k.step(c);
      }
      out[d] = o;
    }
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.plane[p] + (size_t)y * a.stride[p]) + d0;
  if (per == 4 && d0 + 4 <= dwords && a.plane_vec[p]) { *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]); return; }
#pragma unroll
  for (int d = 0; d < 4; d++)
    if ((uint32_t)d < per && d0 + d < dwords) dst[d] = out[d];
}

// 4 pixels of 8 bits or 2 of 16: R G B [A] interleaved, 12 or 16 bytes
template <bool BYTES>
__device__ __forceinline__ void pixel_group(const UnciArgs& a, uint32_t g, uint32_t y)
{
  const uint32_t n = a.px_wide ? 2 : 4, ch = a.px_channels, w = a.w;
  const uint32_t x0 = g * n;
  if (x0 >= w) return;
  const uint32_t npx = x0 + n <= w ? n : w - x0;
  Cursor k(a, a.c[0], x0, y); // (R, G, B and A share the tile geometry; their rows may start elsewhere)
  Cursor kg(a, a.c[1], x0, y), kb(a, a.c[2], x0, y);
  const bool has_a = a.c[3].present != 0;
  Cursor ka(a, a.c[has_a ? 3 : 0], x0, y);
  uint32_t o[4] = {0, 0, 0, 0}; // the group's bytes, little-endian
  uint32_t e = 0;               // elements so far
  const uint32_t ebits = a.px_wide ? 16 : 8;
  auto put = [&](uint32_t v) {
    const uint32_t at = e * ebits;
    o[at >> 5] |= v << (at & 31);
    e++;
  };
  for (uint32_t i = 0; i < npx; i++) {
    put(fetch<BYTES>(a, a.c[0], k.bit(a.c[0])));
    put(fetch<BYTES>(a, a.c[1], kg.bit(a.c[1])));
    put(fetch<BYTES>(a, a.c[2], kb.bit(a.c[2])));
    if (ch == 4) put(has_a ? fetch<BYTES>(a, a.c[3], ka.bit(a.c[3])) : (a.px_wide ? 0xFFFFu : 0xFFu));
    k.step(a.c[0]); kg.step(a.c[1]); kb.step(a.c[2]);
    if (has_a) ka.step(a.c[3]);
  }
  const uint32_t group_bytes = n * ch * (ebits / 8); // 12 or 16
  uint8_t* dst = a.px + (int64_t)y * a.px_pitch + (size_t)g * group_bytes;
  if (npx == n && a.px_dwords_ok) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    if (group_bytes == 16) d[3] = o[3];
    return;
  }
  const uint32_t bytes = npx * ch * (ebits / 8); // the row's ragged end, or a destination that is not dword-aligned
  for (uint32_t b = 0; b < bytes; b++) dst[b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
}

template <bool BYTES>
__global__ void __launch_bounds__(256) k_unci_unpack(const UnciArgs a)
{
  const uint32_t job = a.job[blockIdx.z];
  const uint32_t g = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (job == JOB_PIXELS) { if (y < a.h) pixel_group<BYTES>(a, g, y); }
  else if (y < a.ph[job]) plane_group<BYTES>(a, (int)job, g, y);
}

int bad_detail(const char* m) { return hm_fail_detail(HM_ERR_UNSUPPORTED, HM_DETAIL_NO_COLOUR_CHAIN, m); }

// R, G, B [, A] planes of one sample width (after an irot / imir / clap on the planes) to interleaved pixels: the groups of pixel_group
struct InterleaveArgs {
  const uint8_t* plane[4]; // [3] NULL: opaque
  int32_t stride[4];
  uint8_t* dst;
  int32_t dst_stride;
  uint32_t w, h, channels, wide;
};

__global__ void __launch_bounds__(256) k_unci_interleave(const InterleaveArgs a)
{
  const uint32_t n = a.wide ? 2 : 4, ebits = a.wide ? 16 : 8;
  const uint32_t g = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, x0 = g * n;
  if (y >= a.h || x0 >= a.w) return;
  const uint32_t npx = x0 + n <= a.w ? n : a.w - x0;
  uint32_t o[4] = {0, 0, 0, 0}, e = 0;
  for (uint32_t i = 0; i < npx; i++)
    for (uint32_t c = 0; c < a.channels; c++) {
      uint32_t v = a.wide ? 0xFFFFu : 0xFFu;
      if (a.plane[c]) {
        const uint8_t* p = a.plane[c] + (size_t)y * a.stride[c];
        v = a.wide ? reinterpret_cast<const uint16_t*>(p)[x0 + i] : p[x0 + i];
      }
      const uint32_t at = e++ * ebits;
      o[at >> 5] |= v << (at & 31);
    }
  const uint32_t group_bytes = n * a.channels * (ebits / 8);
  uint8_t* dst = a.dst + (size_t)y * a.dst_stride + (size_t)g * group_bytes;
  if (npx == n) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    if (group_bytes == 16) d[3] = o[3];
    return;
  }
  const uint32_t bytes = npx * a.channels * (ebits / 8);
  for (uint32_t b = 0; b < bytes; b++) dst[b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
}

} // namespace

// dst: 4-byte aligned, dst_stride a multiple of 4 (the library's own buffers)
extern "C" int hm_launch_unci_interleave(const void* const plane[4], const int32_t stride[4], int wide, int w, int h, int channels, void* dst, int dst_stride,
                                         hipStream_t s)
{
  if (w <= 0 || h <= 0 || ((uintptr_t)dst & 3) || (dst_stride & 3)) return hm_fail(HM_ERR_INTERNAL, "unci interleave: bad destination");
  InterleaveArgs a;
  for (int c = 0; c < 4; c++) { a.plane[c] = static_cast<const uint8_t*>(plane[c]); a.stride[c] = stride[c]; }
  a.dst = static_cast<uint8_t*>(dst); a.dst_stride = dst_stride;
  a.w = (uint32_t)w; a.h = (uint32_t)h; a.channels = (uint32_t)channels; a.wide = wide ? 1 : 0;
  const uint32_t n = wide ? 2 : 4, groups = ((uint32_t)w + n - 1) / n;
  const dim3 grid((groups + 63) / 64, ((uint32_t)h + 3) / 4, 1), block(64, 4, 1);
  if (grid.y > 65535u) return hm_fail(HM_ERR_UNSUPPORTED, "unci: %d rows are more than one launch takes", h);
  hipLaunchKernelGGL(k_unci_interleave, grid, block, 0, s, a);
  return hm_check_hip(hipGetLastError(), "k_unci_interleave");
}

extern "C" int hm_unci_unpack(const hm_unci_info* info, const void* d_bytes, size_t n_bytes, const int32_t tiles[4], const hm_planes* out, int out_format,
                              const hm_device_dest* il, void* stream)
{
  if (!info || !d_bytes || (!out && !il)) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_unci_info sub;
  hm_unci_layout L;
  int rc;
  if ((rc = hm_unci_subgrid(info, tiles, &sub)) || (rc = hm_unci_layout_compute(&sub, &L))) return rc;
  if ((uint64_t)n_bytes < L.total_bytes)
    return hm_fail(HM_ERR_BITSTREAM, "unci: the payload has %zu bytes, the layout needs %llu", n_bytes, (unsigned long long)L.total_bytes);
  if ((uintptr_t)d_bytes & 3) return hm_fail(HM_ERR_INVALID_ARG, "unci: the payload pointer is not 4-byte aligned");
  UnciArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src = static_cast<const uint32_t*>(d_bytes);
  a.n_full = L.total_bytes / 4; a.tail_bytes = (uint32_t)(L.total_bytes & 3); // (what the layout needs: bytes behind it are never looked at)
  a.tile_cols = L.tile_cols;
  a.w = (uint32_t)sub.width; a.h = (uint32_t)sub.height;
  a.byte_path = 1;
  for (int c = 0; c < L.n; c++) {
    const hm_unci_comp_layout& k = L.c[c];
    if (k.plane < 0) continue;
    UnciComp& o = a.c[k.plane];
    o.base = k.base; o.tile_stride = k.tile_stride; o.row_stride = k.row_stride;
    o.first_len = k.first_len; o.stride = k.stride; o.off0 = k.off0; o.off1 = k.off1;
    o.tw = k.tw; o.th = k.th; o.depth = k.depth; o.present = 1;
    a.pw[k.plane] = k.tw * L.tile_cols; a.ph[k.plane] = k.th * L.tile_rows;
    if (k.depth != 8 || ((k.first_len | k.stride | k.off0 | k.off1) & 7)) a.byte_path = 0;
  }
  uint32_t max_groups = 0, max_rows = 0;
  if (out) {
    for (int p = 0; p < 4; p++) {
      if (!a.c[p].present || !out->plane[p]) continue; // (a plane the caller does not want, or alpha of an item without)
      const uint32_t bps = a.c[p].depth > 8 ? 2 : 1;
      const uint64_t row = ((uint64_t)a.pw[p] * bps + 3) & ~(uint64_t)3;
      if (((uintptr_t)out->plane[p] & 3) || (out->stride[p] & 3) || out->stride[p] <= 0 || (uint64_t)out->stride[p] < row)
        return hm_fail(HM_ERR_INVALID_ARG, "unci: plane %d needs a 4-byte aligned pointer and a stride that is a multiple of 4 of at least %llu bytes", p, (unsigned long long)row);
      a.plane[p] = static_cast<uint8_t*>(out->plane[p]); a.stride[p] = out->stride[p];
      a.plane_vec[p] = !((uintptr_t)out->plane[p] & 15) && !(out->stride[p] & 15);
      a.job[a.n_jobs++] = (uint32_t)p;
      const bool runs = a.byte_path && a.c[p].stride == 8 && a.c[p].first_len == 8; // (plane_group's `per`)
      max_groups = std::max<uint32_t>(max_groups, (uint32_t)(runs ? (row / 4 + 3) / 4 : row / 4)); max_rows = std::max(max_rows, a.ph[p]);
    }
  }
  if (il) {
    if (sub.colour_space != HM_UNCI_RGB) return bad_detail("unci: interleaved pixels are written for R G B items only");
    const bool wide = out_format == HM_OUT_RRGGBB_LE || out_format == HM_OUT_RRGGBBAA_LE;
    const bool four = out_format == HM_OUT_RGBA || out_format == HM_OUT_RRGGBBAA_LE;
    if (!wide && out_format != HM_OUT_RGB && out_format != HM_OUT_RGBA) return bad_detail("unci: interleaved pixels are HM_OUT_RGB / _RGBA / _RRGGBB_LE / _RRGGBBAA_LE");
    for (int p = 0; p < 4; p++)
      if (a.c[p].present && (p < 3 || four) && a.c[p].depth != (wide ? 16u : 8u))
        return bad_detail(wide ? "unci: a 16-bit interleaved target takes components of 16 bits only" : "unci: an 8-bit interleaved target takes components of 8 bits only");
    if (il->layout != HM_DEV_LAYOUT_HWC || il->dtype != (wide ? HM_DEV_U16 : HM_DEV_U8))
      return hm_fail(HM_ERR_UNSUPPORTED, "unci: the interleaved pixels are written as HWC in the target's own integer type");
    const int64_t need = hm_device_dest_bytes(out_format, sub.width, sub.height, il);
    if (need < 0) return (int)need;
    if (!il->ptr || il->len < (uint64_t)need) return hm_fail(HM_ERR_INVALID_ARG, "unci: the destination holds %llu bytes, %lld are needed", (unsigned long long)il->len, (long long)need);
    a.px = static_cast<uint8_t*>(il->ptr);
    a.px_channels = four ? 4 : 3; a.px_wide = wide;
    a.px_pitch = il->row_pitch ? il->row_pitch : (int64_t)sub.width * a.px_channels * (wide ? 2 : 1);
    a.px_dwords_ok = !((uintptr_t)il->ptr & 3) && !(a.px_pitch & 3);
    a.job[a.n_jobs++] = JOB_PIXELS;
    const uint32_t n = wide ? 2 : 4;
    max_groups = std::max(max_groups, (a.w + n - 1) / n); max_rows = std::max(max_rows, a.h);
  }
  if (!a.n_jobs) return HM_OK;
  const dim3 grid((max_groups + 63) / 64, (max_rows + 3) / 4, a.n_jobs), block(64, 4, 1);
  if (grid.y > 65535u) return hm_fail(HM_ERR_UNSUPPORTED, "unci: %u rows are more than one launch takes", max_rows);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.byte_path) hipLaunchKernelGGL(k_unci_unpack<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_unci_unpack<false>, grid, block, 0, s, a);
  return hm_check_hip(hipGetLastError(), "k_unci_unpack");
}
