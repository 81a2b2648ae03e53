// regions.hip - the regions of 'rgan' region items rasterised to mask planes on the device (gfx950), under the membership rules that
// include/heif_mi355x.h states once ("Regions and masks"):
//   k_regions   ONE launch: every region of a request over the view's rectangle of the canvas, to one plane per region
//               (HM_REGIONS_STACK, blockIdx.z the region) or to one plane of labels (HM_REGIONS_LABELS)
// A lane owns one dword of an output row - 4 pixels -, a wave 256 consecutive pixels of ONE row (block 64 x 4: threadIdx.y is the wave),
// so the row is the same in every lane of a wave and is held in a scalar register.  With it the tests that decide whether a region, or
// an edge of a polygon, can touch the wave at all - the region's bounding box against the wave's span, an edge's row-crossing test, an
// edge's bounding box for the on-segment rule - are wave-uniform branches: most waves of a large canvas pass every region by and
// store zeros, and a polygon edge that crosses no row of the rectangle costs the row test and nothing else.
// Edge delivery: uniform-address loads.  The loop over a polygon's vertices runs on a scalar counter, the vertex array is read-only and
// nothing the kernel stores can alias it before the loop ends, so every vertex is fetched once per wave through the scalar cache - no
// LDS, no barrier, no chunk size and so no limit on the point count but the payload's length.  Staging chunks in LDS would pay a
// barrier per chunk in every wave of a block to feed waves of which most reject the region by its bounding box.
// STACK and LABELS share one row body: the loop over a range of regions with a writer - LABELS keeps 1 + the index of the last region
// whose value is >= 128, STACK is that loop over the one-region range blockIdx.z with the writer that keeps the value.
// Device data: ONE block, uploaded once from a pooled pinned staging buffer: the fixed-size descriptors, then the point arrays (int32
// pairs), the inline bit strings and the referenced masks' bytes, each padded with zeros to a dword - nothing behind the block is read.
// Stores: a lane's 4 elements go out in one store where pointer and pitches allow; a row's last partial group and unaligned
// destinations fall back to element stores.  Nothing outside width x height of a plane is written.
// An output size that differs from the crop's: the planes go to a temporary of bytes and from there through the grouped planes-view
// writer (hm_planes_view_write: the regions are its "frames" - monochrome 8-bit planes that share tap tables and one launch per pass).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hm_devdest.h"
#include "out_elem.h"

namespace {

struct RegionDesc {            // 48 bytes
  int32_t  type, x, y;
  uint32_t w, h, n_points;
  int32_t  bx0, by0, bx1, by1; // the closed bounding box on the canvas; bx1 < bx0: nothing
  uint64_t off;                // its points / bits / mask bytes: bytes from the block's start (points 8-byte, the others 4-byte aligned)
};

struct RasterArgs {
  const uint8_t* block;        // descriptors first
  int32_t  crop_x, crop_y, w, h; // the rectangle of the canvas that is generated
  uint8_t* dst;
  long long row_pitch, plane_pitch;
  uint32_t n;                  // LABELS: the regions; STACK: planes (grid z)
  uint32_t wide_ok;            // pointer and pitches take a lane's 4 elements in one store
  float scale, bias;
};

enum { ROWS_PER_WAVE = 8 };

__device__ __forceinline__ long long abs64(long long v) { return v < 0 ? -v : v; }

// the values of region d at the lane's pixels (px0 .. px0 + 3, py); [sx0, sx1]: the wave's span of the row.  Everything int64.
__device__ __forceinline__ void region_values(const RasterArgs& a, const RegionDesc& d, int px0, int py, int sx0, int sx1, uint32_t (&v)[4])
{
  const long long x = d.x, y = d.y, w = d.w, h = d.h;
  switch (d.type) {
    case HM_REGION_POINT:
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = (px0 + i == x && py == y) ? 255u : 0u;
      return;
    case HM_REGION_RECTANGLE:
#pragma unroll
      for (int i = 0; i < 4; i++) { const long long px = px0 + i; v[i] = (px >= x && px < x + w && py >= y && py < y + h) ? 255u : 0u; }
      return;
    case HM_REGION_ELLIPSE: {
      const long long dy = py - y, ry2 = h * h, rx2 = w * w;
      const bool row_in = abs64(dy) <= h; // (the bounding box has let the row through: always true; kept as the rule states it)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const long long dx = (long long)(px0 + i) - x;
        const bool box = row_in && abs64(dx) <= w;
        const long long cx = box ? dx : 0, cy = box ? dy : 0; // (products stay below 2^61 inside the box only)
        v[i] = (box && cx * cx * ry2 + cy * cy * rx2 <= rx2 * ry2) ? 255u : 0u;
      }
      return;
    }
    case HM_REGION_POLYGON:
    case HM_REGION_POLYLINE: {
      const bool closed = d.type == HM_REGION_POLYGON;
      const uint32_t n = d.n_points;
      const int2* P = reinterpret_cast<const int2*>(a.block + d.off);
      const uint32_t segs = closed || n == 1 ? n : n - 1; // (n == 1: the segment A -> A is the point; n == 0: nothing)
      uint32_t on = 0, par = 0;
      if (n == 0) { v[0] = v[1] = v[2] = v[3] = 0; return; }
      int2 A = P[0];
      for (uint32_t k = 0; k < segs; k++) { // (k, and with it every address, is the same in all lanes)
        const int2 B = P[k + 1 == n ? 0 : k + 1];
        const int minx = min(A.x, B.x), maxx = max(A.x, B.x), miny = min(A.y, B.y), maxy = max(A.y, B.y);
        if (py >= miny && py <= maxy && sx1 >= minx && sx0 <= maxx) { // the segment rule, for the waves its bounding box touches
          const long long dx = (long long)B.x - A.x, dy = (long long)B.y - A.y, m = max(abs64(dx), abs64(dy));
          const long long t0 = dx * ((long long)py - A.y);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int px = px0 + i;
            if (px >= minx && px <= maxx && 2 * abs64(t0 - dy * ((long long)px - A.x)) <= m) on |= 1u << i;
          }
        }
        if (closed && ((A.y <= py) != (B.y <= py))) { // the edge crosses the row: even-odd
          const int2 L = A.y < B.y ? A : B, U = A.y < B.y ? B : A;
          const long long ey = (long long)U.y - L.y, t = ((long long)U.x - L.x) * ((long long)py - L.y);
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (((long long)(px0 + i) - L.x) * ey < t) par ^= 1u << i;
        }
        A = B;
      }
      const uint32_t in = on | par;
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = (in >> i) & 1u ? 255u : 0u;
      return;
    }
    case HM_REGION_INLINE_MASK: {
      const uint32_t* bits = reinterpret_cast<const uint32_t*>(a.block + d.off);
      const long long ly = py - y;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const long long lx = (long long)(px0 + i) - x;
        uint32_t s = 0;
        if (lx >= 0 && lx < w && ly >= 0 && ly < h) {
          const unsigned long long bit = (unsigned long long)(ly * w + lx); // most significant bit of a byte first; the dword is little-endian
          s = (bits[bit >> 5] >> (8 * ((uint32_t)(bit >> 3) & 3) + (7 - ((uint32_t)bit & 7)))) & 1u;
        }
        v[i] = s ? 255u : 0u;
      }
      return;
    }
    case HM_REGION_REFERENCED_MASK: {
      const uint8_t* M = a.block + d.off;
      const long long ly = py - y;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const long long lx = (long long)(px0 + i) - x;
        v[i] = (lx >= 0 && lx < w && ly >= 0 && ly < h) ? (uint32_t)M[ly * w + lx] : 0u;
      }
      return;
    }
    default:
      v[0] = v[1] = v[2] = v[3] = 0;
  }
}

// the row body: regions [r0, r1) at the lane's 4 pixels of row Y; the writer keeps a label (LABELS) or the value (STACK)
template <bool LABELS>
__device__ __forceinline__ void row_body(const RasterArgs& a, uint32_t r0, uint32_t r1, int X, int Y, int span, uint32_t (&out)[4])
{
  const RegionDesc* D = reinterpret_cast<const RegionDesc*>(a.block);
  const int py = a.crop_y + Y, px0 = a.crop_x + X;
  const int sx0 = a.crop_x + span, sx1 = a.crop_x + min(span + 255, a.w - 1);
  for (uint32_t r = r0; r < r1; r++) {
    const RegionDesc d = D[r];
    if (py < d.by0 || py > d.by1 || sx1 < d.bx0 || sx0 > d.bx1) continue; // the whole wave passes the region by
    uint32_t v[4];
    region_values(a, d, px0, py, sx0, sx1, v);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (LABELS) { if (v[i] >= 128) out[i] = r + 1; }
      else out[i] = v[i];
    }
  }
}

template <typename OutT, bool LABELS>
__global__ void __launch_bounds__(256) k_regions(const RasterArgs a)
{
  // (block 64 x 4: a wave is one threadIdx.y, so the first lane's row is every lane's)
  const int span = (int)(blockIdx.x * 256), X = span + (int)threadIdx.x * 4;
  const uint32_t z = blockIdx.z;
  // a wave takes up to ROWS_PER_WAVE rows, one after the other, 4 * gridDim.y rows apart (the waves in flight write neighbouring rows): a
  // wave that stores one dword per lane and ends costs more to start than to run
  int Y = (int)(blockIdx.y * 4) + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  for (int j = 0; j < ROWS_PER_WAVE && Y < a.h; j++, Y += 4 * (int)gridDim.y) {
    uint32_t out[4] = {0, 0, 0, 0};
    row_body<LABELS>(a, LABELS ? 0u : z, LABELS ? a.n : z + 1, X, Y, span, out);
    if (X >= a.w) continue;
    uint8_t* row = a.dst + (LABELS ? 0ll : (long long)z * a.plane_pitch) + (long long)Y * a.row_pitch;
    OutT* p = reinterpret_cast<OutT*>(row) + X;
    OutT o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = moved<OutT>(out[i], a.scale, a.bias);
    if (X + 4 <= a.w && a.wide_ok) {
      typedef typename LoadWord<4 * sizeof(OutT)>::type W;
      W word;
      __builtin_memcpy(&word, o, sizeof(W));
      *reinterpret_cast<W*>(p) = word;
      continue;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (X + i < a.w) p[i] = o[i];
  }
}

int elem_of(int dtype) { return dtype == HM_DEV_U8 ? 1 : dtype == HM_DEV_F32 ? 4 : 2; }

struct DestPlan { int64_t row_pitch, plane_pitch, bytes; int elem, planes; };

// the destination against planes x (w x h): everything but ptr and len
int dest_resolve(int mode, int n, int w, int h, const hm_regions_dest* d, DestPlan* p)
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (mode != HM_REGIONS_STACK && mode != HM_REGIONS_LABELS) return hm_fail(HM_ERR_INVALID_ARG, "regions: unknown mode %d", mode);
  if (n < 0) return hm_fail(HM_ERR_INVALID_ARG, "regions: %d regions", n);
  if (mode == HM_REGIONS_LABELS && n > 255) return hm_fail(HM_ERR_INVALID_ARG, "regions: %d regions, HM_REGIONS_LABELS numbers at most 255 in a byte", n);
  if (n > 65535) return hm_fail(HM_ERR_INVALID_ARG, "regions: %d regions are more than one launch takes (65535)", n);
  if (d->dtype != HM_DEV_U8 && d->dtype != HM_DEV_F16 && d->dtype != HM_DEV_F32) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: dtype %d (HM_DEV_U8, HM_DEV_F16 and HM_DEV_F32 are taken)", d->dtype);
  if (mode == HM_REGIONS_LABELS && d->dtype != HM_DEV_U8) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: HM_REGIONS_LABELS is written as HM_DEV_U8 only");
  if (d->reserved) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: reserved is %d, not 0", d->reserved);
  if (w < 1 || h < 1 || w > 32768 || h > 32768) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: plane size %d x %d", w, h);
  p->elem = elem_of(d->dtype);
  p->planes = mode == HM_REGIONS_LABELS ? 1 : n;
  const int64_t tight = (int64_t)w * p->elem;
  if (d->row_pitch < 0 || d->plane_pitch < 0) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: a negative pitch");
  p->row_pitch = d->row_pitch ? d->row_pitch : tight;
  if (p->row_pitch < tight) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: row_pitch %lld below the %lld bytes of a row", (long long)p->row_pitch, (long long)tight);
  if (p->row_pitch > ((int64_t)1 << 40)) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: row_pitch %lld", (long long)p->row_pitch);
  const int64_t plane = p->row_pitch * (h - 1) + tight;
  p->plane_pitch = d->plane_pitch ? d->plane_pitch : p->row_pitch * h;
  if (p->planes > 1 && p->plane_pitch < plane) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: plane_pitch %lld below the %lld bytes of a plane", (long long)p->plane_pitch, (long long)plane);
  if (p->plane_pitch > ((int64_t)1 << 44)) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: plane_pitch %lld", (long long)p->plane_pitch);
  if ((p->row_pitch % p->elem) || (p->plane_pitch % p->elem)) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: a pitch is not a multiple of the element size %d", p->elem);
  p->bytes = p->planes ? p->plane_pitch * (p->planes - 1) + plane : 0;
  return HM_OK;
}

template <bool LABELS>
int launch(int dtype, const RasterArgs& a, dim3 grid, hipStream_t s)
{
  const dim3 block(64, 4, 1);
  if (dtype == HM_DEV_U8) hipLaunchKernelGGL((k_regions<uint8_t, LABELS>), grid, block, 0, s, a);
  else if (dtype == HM_DEV_F16) hipLaunchKernelGGL((k_regions<__half, LABELS>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_regions<float, LABELS>), grid, block, 0, s, a);
  return hm_check_hip(hipGetLastError(), "k_regions");
}

// one region against the limits and its data pointer; *bytes: what its data adds to the block
int region_check(const hm_region& g, const void* data, int i, uint64_t* bytes)
{
  const int64_t lim = HM_REGION_COORD_LIMIT;
  *bytes = 0;
  if (g.type < HM_REGION_POINT || g.type > HM_REGION_POLYLINE) return hm_fail(HM_ERR_UNSUPPORTED, "region %d has the unknown geometry type %d (0..6 are defined)", i, g.type);
  const bool poly = g.type == HM_REGION_POLYGON || g.type == HM_REGION_POLYLINE;
  if (!poly && (g.x < -lim || g.x >= lim || g.y < -lim || g.y >= lim || g.w >= (uint64_t)lim || g.h >= (uint64_t)lim))
    return hm_fail(HM_ERR_UNSUPPORTED, "region %d: a coordinate outside -2^28 <= v < 2^28 or a size of 2^28 or more (the limits of the rasteriser's exact arithmetic)", i);
  if (g.type == HM_REGION_ELLIPSE && (g.w > HM_REGION_MAX_RADIUS || g.h > HM_REGION_MAX_RADIUS))
    return hm_fail(HM_ERR_UNSUPPORTED, "region %d: an ellipse radius above 32767 (the limit of the rasteriser's exact arithmetic)", i);
  if (poly) {
    if (g.n_points && !data) return hm_fail(HM_ERR_INVALID_ARG, "region %d: no points given", i);
    const int32_t* p = static_cast<const int32_t*>(data);
    for (uint64_t k = 0; k < 2 * (uint64_t)g.n_points; k++)
      if (p[k] < -lim || p[k] >= lim) return hm_fail(HM_ERR_UNSUPPORTED, "region %d: a point coordinate outside -2^28 <= v < 2^28 (the limit of the rasteriser's exact arithmetic)", i);
    *bytes = 8 * (uint64_t)g.n_points;
  }
  else if (g.type == HM_REGION_INLINE_MASK || g.type == HM_REGION_REFERENCED_MASK) {
    const uint64_t need = g.type == HM_REGION_INLINE_MASK ? ((uint64_t)g.w * g.h + 7) / 8 : (uint64_t)g.w * g.h;
    if (need && !data) return hm_fail(HM_ERR_INVALID_ARG, "region %d: no mask data given", i);
    if (g.mask_bytes < need) return hm_fail(HM_ERR_BITSTREAM, "region %d: a mask of %u x %u with %llu bytes of data, %llu are needed", i, g.w, g.h, (unsigned long long)g.mask_bytes, (unsigned long long)need);
    *bytes = need;
  }
  return HM_OK;
}

int clamp_i32(int64_t v) { return (int)std::min<int64_t>(std::max<int64_t>(v, INT32_MIN), INT32_MAX); }

} // namespace

extern "C" int64_t hm_regions_dest_bytes(int mode, int n_regions, int width, int height, const hm_regions_dest* d)
{
  DestPlan p;
  const int rc = dest_resolve(mode, n_regions, width, height, d, &p);
  return rc ? rc : p.bytes;
}

extern "C" int hm_rasterise_regions(const hm_region* regions, const void* const* data, int n, int canvas_w, int canvas_h, const hm_device_view* view,
                                    int mode, const hm_regions_dest* dest, void* stream)
{
  if (!dest || (n > 0 && (!regions || !data))) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (canvas_w < 1 || canvas_h < 1 || canvas_w >= HM_REGION_COORD_LIMIT || canvas_h >= HM_REGION_COORD_LIMIT)
    return hm_fail(HM_ERR_UNSUPPORTED, "regions: a canvas of %d x %d (each side must be in 1 .. 2^28 - 1)", canvas_w, canvas_h);
  // ---- every refusal, before anything is queued ----
  hm_device_view whole;
  std::memset(&whole, 0, sizeof(whole));
  hm_view_plan vp;
  int rc = hm_view_resolve(0, canvas_w, canvas_h, view ? view : &whole, &vp);
  if (rc) return rc;
  const bool resize = vp.ow != vp.w || vp.oh != vp.h;
  if (resize && mode == HM_REGIONS_LABELS && vp.filter != HM_VIEW_NEAREST)
    return hm_fail(HM_ERR_INVALID_ARG, "regions: HM_REGIONS_LABELS at a size other than the crop's takes HM_VIEW_NEAREST only (averaged labels mean nothing)");
  DestPlan dp;
  if ((rc = dest_resolve(mode, n, vp.ow, vp.oh, dest, &dp))) return rc;
  if (dp.planes == 0) return HM_OK; // (a stack of no regions)
  if (!dest->ptr) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: null ptr");
  if ((uintptr_t)dest->ptr % (unsigned)dp.elem) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: ptr is not a multiple of the element size %d", dp.elem);
  if (dest->len < (uint64_t)dp.bytes) return hm_fail(HM_ERR_INVALID_ARG, "regions destination: len %llu below the %lld bytes the planes need", (unsigned long long)dest->len, (long long)dp.bytes);
  std::vector<uint64_t> sizes((size_t)n);
  uint64_t block_bytes = (uint64_t)n * sizeof(RegionDesc);
  for (int i = 0; i < n; i++) {
    if ((rc = region_check(regions[i], data[i], i, &sizes[(size_t)i]))) return rc;
    block_bytes += (sizes[(size_t)i] + 7) & ~(uint64_t)7; // (every array starts 8-byte aligned and ends padded with zeros)
  }
  if (block_bytes > ((uint64_t)1 << 40)) return hm_fail(HM_ERR_UNSUPPORTED, "regions: %llu bytes of region data", (unsigned long long)block_bytes);
  hm_planes_view_plan pv;
  hm_device_view tmp_view;
  std::memset(&tmp_view, 0, sizeof(tmp_view));
  if (resize) { // the temporary is the crop: the writer takes all of it to ow x oh
    tmp_view.out_w = vp.ow; tmp_view.out_h = vp.oh; tmp_view.filter = vp.filter;
    if ((rc = hm_planes_view_resolve(HM_CHROMA_MONO, vp.w, vp.h, &tmp_view, &pv))) return rc;
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  hm_device_dest probe;
  std::memset(&probe, 0, sizeof(probe));
  probe.ptr = dest->ptr;
  if ((rc = hm_dest_check_pointer(&probe))) return rc;
  const uint32_t row_blocks = ((uint32_t)vp.h + 3) / 4;
  const dim3 grid(((uint32_t)vp.w + 255) / 256, (row_blocks + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE, (uint32_t)dp.planes);

  // ---- the block: descriptors, then every region's data; one upload ----
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<hm_view_scratch> sc((size_t)dp.planes + 1); // [0]: the block, its staging and the temporary; [1 ..]: the writer's, per plane
  std::memset(sc.data(), 0, sc.size() * sizeof(hm_view_scratch));
  hm_view_scratch& own = sc[0];
  struct Retire { hipStream_t s; std::vector<hm_view_scratch>& sc; ~Retire() { hm_view_scratch_retire(s, sc.data(), (int)sc.size()); } } retire{s, sc};
  const size_t upload = (size_t)std::max<uint64_t>(block_bytes, 8);
  uint8_t* host = static_cast<uint8_t*>(own.pinned = hm_pool_pinned_alloc(upload));
  if (!host) return hm_fail(HM_ERR_NOMEM, "out of memory");
  if (!(own.dev[0] = hm_pool_device_alloc(upload))) return HM_ERR_NO_DEVICE;
  RegionDesc* D = reinterpret_cast<RegionDesc*>(host);
  uint64_t at = (uint64_t)n * sizeof(RegionDesc);
  for (int i = 0; i < n; i++) {
    const hm_region& g = regions[i];
    RegionDesc& d = D[i];
    std::memset(&d, 0, sizeof(d));
    d.type = g.type; d.x = g.x; d.y = g.y; d.w = g.w; d.h = g.h; d.n_points = g.n_points; d.off = at;
    int64_t x0 = g.x, y0 = g.y, x1 = g.x, y1 = g.y; // the closed bounding box
    switch (g.type) {
      case HM_REGION_ELLIPSE: x0 -= g.w; x1 += g.w; y0 -= g.h; y1 += g.h; break;
      case HM_REGION_RECTANGLE: case HM_REGION_INLINE_MASK: case HM_REGION_REFERENCED_MASK:
        x1 = x0 + (int64_t)g.w - 1; y1 = y0 + (int64_t)g.h - 1; break; // (a zero size: empty)
      case HM_REGION_POLYGON: case HM_REGION_POLYLINE: {
        const int32_t* p = static_cast<const int32_t*>(data[i]);
        x0 = y0 = INT32_MAX; x1 = y1 = INT32_MIN;
        for (uint32_t k = 0; k < g.n_points; k++) {
          x0 = std::min<int64_t>(x0, p[2 * k]); x1 = std::max<int64_t>(x1, p[2 * k]);
          y0 = std::min<int64_t>(y0, p[2 * k + 1]); y1 = std::max<int64_t>(y1, p[2 * k + 1]);
        }
        break;
      }
      default: break;
    }
    if (y1 < y0) { x0 = 0; x1 = -1; } // (an empty box in y is an empty box)
    d.bx0 = clamp_i32(x0); d.by0 = clamp_i32(y0); d.bx1 = clamp_i32(x1); d.by1 = clamp_i32(y1);
    const uint64_t padded = (sizes[(size_t)i] + 7) & ~(uint64_t)7;
    if (sizes[(size_t)i]) std::memcpy(host + at, data[i], (size_t)sizes[(size_t)i]);
    std::memset(host + at + sizes[(size_t)i], 0, (size_t)(padded - sizes[(size_t)i]));
    at += padded;
  }
  if ((rc = hm_check_hip(hipMemcpyAsync(own.dev[0], host, upload, hipMemcpyHostToDevice, s), "upload of the region data"))) return rc;

  RasterArgs a;
  std::memset(&a, 0, sizeof(a));
  a.block = static_cast<const uint8_t*>(own.dev[0]);
  a.crop_x = vp.x; a.crop_y = vp.y; a.w = vp.w; a.h = vp.h;
  a.n = (uint32_t)n;
  if (!resize) {
    a.dst = static_cast<uint8_t*>(dest->ptr); a.row_pitch = dp.row_pitch; a.plane_pitch = dp.plane_pitch;
    a.wide_ok = (((uintptr_t)dest->ptr | (uint64_t)dp.row_pitch | (uint64_t)dp.plane_pitch) % (4u * (unsigned)dp.elem)) == 0;
    a.scale = dest->scale; a.bias = dest->bias;
    return mode == HM_REGIONS_LABELS ? launch<true>(dest->dtype, a, grid, s) : launch<false>(dest->dtype, a, grid, s);
  }
  // ---- resized: bytes to a temporary, then the grouped planes-view writer, every plane a frame ----
  const int64_t tpitch = ((int64_t)vp.w + 15) & ~(int64_t)15, tplane = tpitch * vp.h;
  if (tpitch > INT32_MAX) return hm_fail(HM_ERR_UNSUPPORTED, "regions: a crop of %d columns", vp.w);
  if (!(own.dev[1] = hm_pool_device_alloc((size_t)(tplane * dp.planes)))) return HM_ERR_NO_DEVICE;
  a.dst = static_cast<uint8_t*>(own.dev[1]); a.row_pitch = tpitch; a.plane_pitch = tplane; a.wide_ok = 1;
  a.scale = 1.0f; a.bias = 0.0f;
  if ((rc = mode == HM_REGIONS_LABELS ? launch<true>(HM_DEV_U8, a, grid, s) : launch<false>(HM_DEV_U8, a, grid, s))) return rc;
  std::vector<hm_device_planes> planes((size_t)dp.planes);
  std::vector<hm_planes_view_item> items((size_t)dp.planes);
  std::memset(planes.data(), 0, planes.size() * sizeof(hm_device_planes));
  std::memset(items.data(), 0, items.size() * sizeof(hm_planes_view_item));
  const int64_t plane_bytes = dp.row_pitch * (vp.oh - 1) + (int64_t)vp.ow * dp.elem;
  for (int r = 0; r < dp.planes; r++) {
    hm_device_planes& P = planes[(size_t)r];
    P.plane[0].ptr = static_cast<uint8_t*>(dest->ptr) + (int64_t)r * dp.plane_pitch;
    P.plane[0].len = (uint64_t)plane_bytes; P.plane[0].row_pitch = dp.row_pitch;
    P.layout = HM_DEV_PLANES_SEPARATE; P.dtype = dest->dtype;
    P.scale[0] = dest->scale; P.bias[0] = dest->bias;
    hm_planes_view_item& it = items[(size_t)r];
    it.planes = &P; it.pv = pv; it.chroma = HM_CHROMA_MONO; it.bits = 8; it.alpha_bits = 0;
    it.src[0] = a.dst + (int64_t)r * tplane; it.stride[0] = (int32_t)tpitch;
  }
  return hm_planes_view_write(items.data(), dp.planes, s, sc.data() + 1, nullptr);
}
