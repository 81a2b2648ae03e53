// hm_planes_view.h — the index arithmetic of a planar view (a view, hm_device_view, into planar YCbCr, hm_device_planes:
// hm_planes_view_write, devdest.cpp; kernels: planes_view.hip): the geometry per plane, the split of a launch's blockIdx.y into
// plane and row group, the map from a lane to the elements (or Cb / Cr pairs) it stores, the key frames are grouped by, the cut of
// a group into chunks and the layout of the one block that goes up per group.  Nothing but integers: no HIP, no allocation - a
// stand-alone host program can hold it to its rules (tests/host/planes_view_check.cpp).
#ifndef HM_PLANES_VIEW_H
#define HM_PLANES_VIEW_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HM_PV_FN __host__ __device__ inline
#else
#define HM_PV_FN inline
#endif

// ---- geometry: every plane is an image of its own ----
// chroma: HM_CHROMA_* (0 4:0:0, 1 4:2:0, 2 4:2:2, 3 4:4:4)
HM_PV_FN int hm_pv_sub_x(int chroma) { return chroma == 1 || chroma == 2 ? 2 : 1; }
HM_PV_FN int hm_pv_sub_y(int chroma) { return chroma == 1 ? 2 : 1; }

// The crop (x, y, w, h) of the luma plane, inside a W x H image, at ow x oh: crop[c] = x, y, w, h and out[c] = w, h of plane c
// (0 Y, 1 Cb, 2 Cr, 3 alpha; all zero for Cb / Cr of 4:0:0).  Returns 0, or 1 / 2 where x / y is no multiple of the sub-sampling.
// Cb / Cr take (x / sx, y / sy, (w + sx - 1) / sx, (h + sy - 1) / sy) to ((ow + sx - 1) / sx, (oh + sy - 1) / sy): the plane size
// hm_planes_resolve computes for an ow x oh result.  The chroma crop lies inside the chroma plane: with sx = 2, x is even and
// x + w <= W, so x / 2 + (w + 1) / 2 = (x + w + 1) / 2 <= (W + 1) / 2, the chroma plane's width (the same vertically with sy = 2;
// with a factor of 1 the chroma crop is the luma crop).
inline int hm_pv_geometry(int chroma, int x, int y, int w, int h, int ow, int oh, int32_t crop[4][4], int32_t out[4][2])
{
  const int sx = hm_pv_sub_x(chroma), sy = hm_pv_sub_y(chroma);
  memset(crop, 0, sizeof(int32_t) * 16);
  memset(out, 0, sizeof(int32_t) * 8);
  if (x % sx) return 1;
  if (y % sy) return 2;
  for (int c = 0; c < 4; c += 3) { crop[c][0] = x; crop[c][1] = y; crop[c][2] = w; crop[c][3] = h; out[c][0] = ow; out[c][1] = oh; }
  if (chroma != 0)
    for (int c = 1; c <= 2; c++) {
      crop[c][0] = x / sx; crop[c][1] = y / sy; crop[c][2] = (w + sx - 1) / sx; crop[c][3] = (h + sy - 1) / sy;
      out[c][0] = (ow + sx - 1) / sx; out[c][1] = (oh + sy - 1) / sy;
    }
  return 0;
}

// ---- a launch: blockIdx.y = the planes' groups of 4 rows one plane behind the other, blockIdx.x = groups of 64 lanes ----
// y_end[p]: the running sum of (rows + 3) / 4 over planes 0 .. p (an absent plane adds nothing)
HM_PV_FN int hm_pv_plane_of(int by, const int32_t y_end[4]) { return (by >= y_end[0]) + (by >= y_end[1]) + (by >= y_end[2]); }
HM_PV_FN int hm_pv_row_of(int by, int plane, const int32_t y_end[4], int wave) { return (by - (plane == 0 ? 0 : y_end[plane - 1])) * 4 + wave; }
// elements (pair = 0) or Cb / Cr pairs (pair = 1) of a row a lane stores: 16 bytes of output, the interleaved float32 plane 32
HM_PV_FN int hm_pv_per_lane(int elem_bytes, int pair) { return pair ? (elem_bytes == 1 ? 8 : 4) : 16 / elem_bytes; }
// blocks along x of a plane of w elements (pairs) per row
HM_PV_FN int hm_pv_blocks_x(int w, int per_lane) { return ((w + per_lane - 1) / per_lane + 63) / 64; }
// the 16-byte path: lane `lane` of block bx stores elements [*x0, *x0 + n) of its row, n (returned) = per_lane, less in the ragged
// last group, 0 behind the row's end
HM_PV_FN int hm_pv_vec_span(int bx, int lane, int per_lane, int w, int* x0)
{
  *x0 = (bx * 64 + lane) * per_lane;
  if (*x0 >= w) return 0;
  return w - *x0 < per_lane ? w - *x0 : per_lane;
}
// the element-wise path covers the same span of a row per wave: lane `lane` takes elements l, l + 64, ... of it (i = 0 .. per_lane - 1;
// an index at or behind w is not stored)
HM_PV_FN int hm_pv_elem_at(int bx, int lane, int per_lane, int i) { return (bx * per_lane + i) * 64 + lane; }

// ---- what a launch has ONE of: frames that agree in all of it share tap tables and launches.  Zeroed, filled, compared as bytes ----
typedef struct hm_pv_key {
  int32_t chroma, bits, alpha_bits, filter;
  int32_t layout, dtype, msb_aligned, crop_only;
  int32_t crop[4][4], out[4][2];  // per plane
  int32_t stride[4];              // of the source planes
  int32_t vec[4];                 // the destination plane's pointer and pitch are multiples of 16
  int64_t pitch[4];               // as resolved (0: the plane is not written)
  uint32_t scale[4], bias[4];     // the floats' bits
} hm_pv_key;
inline int hm_pv_key_equal(const hm_pv_key* a, const hm_pv_key* b) { return memcmp(a, b, sizeof(*a)) == 0; }
inline int hm_pv_vec_class(uintptr_t ptr, int64_t pitch) { return (ptr % 16) == 0 && (pitch % 16) == 0; }

// the intermediate of one frame: one region per source plane, a row pitch of a multiple of 16 float32 elements (so a ragged last
// group loads whole vectors), regions one behind the other.  off[c] / pitch[c] in elements; returns the frame's elements.
inline int64_t hm_pv_tmp_layout(const int32_t crop[4][4], const int32_t out[4][2], const int present[4], int64_t off[4], int64_t pitch[4])
{
  int64_t at = 0;
  for (int c = 0; c < 4; c++) {
    off[c] = pitch[c] = 0;
    if (!present[c]) continue;
    pitch[c] = ((int64_t)out[c][0] + 15) / 16 * 16;
    off[c] = at;
    at += pitch[c] * crop[c][3];
  }
  return at;
}

// frames per chunk: frame_elems x 4 x frames <= bound (hm_view_batch.h's default where bound <= 0), frames <= gridDim.z's limit, at least one
enum { HM_PV_Z_MOST = 65535 };
inline int64_t hm_pv_chunk_frames(int64_t frame_elems, int64_t bound)
{
  if (bound <= 0) bound = (int64_t)64 << 20;
  const int64_t per = frame_elems * 4;
  int64_t n = per > 0 ? bound / per : 1;
  if (n > HM_PV_Z_MOST) n = HM_PV_Z_MOST;
  return n < 1 ? 1 : n;
}

// per frame: the source planes at their crop's origin and the destination planes (device addresses)
typedef struct hm_pv_rec { uint64_t src[4], dst[4]; } hm_pv_rec;
// the block of a group: `words` 32-bit words of tap tables, then, 8-byte aligned, rec[frames]
typedef struct hm_pv_block { int64_t rec_off, bytes; } hm_pv_block;
inline hm_pv_block hm_pv_block_layout(int64_t words, int64_t frames)
{
  hm_pv_block b;
  b.rec_off = (words * 4 + 7) / 8 * 8;
  b.bytes = b.rec_off + frames * (int64_t)sizeof(hm_pv_rec);
  return b;
}

#endif
