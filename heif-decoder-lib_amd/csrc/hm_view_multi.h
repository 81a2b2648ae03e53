// hm_view_multi.h — the index arithmetic of a multi-view write (hm_views_write, devdest.cpp; kernels: resample.hip): MANY views of ONE
// picture, one launch per pass.  The key views are grouped by, the record a workgroup reads about its view, the layout of the one
// block that goes up per group, the cut of blockIdx.y by running sums over the views, and the cut of a group into chunks.  Nothing but
// integers: no HIP, no allocation - a stand-alone host program can hold it to its rules (tests/host/view_multi_check.cpp).
#ifndef HM_VIEW_MULTI_H
#define HM_VIEW_MULTI_H

#include <stdint.h>
#include <string.h>

#include "hm_view_batch.h"

// what a launch of the multi kernels has ONE of - the template instance and the kernel arguments that are no record: views that
// agree in all of it share launches.  Crop, size written, filter, pointer and pitches are the record's.  Zeroed first, compared as bytes.
typedef struct hm_view_multi_key {
  int32_t staged;                 // the horizontal pass stages its source run in LDS (HM_VIEW_CUBIC / HM_VIEW_LANCZOS3)
  int32_t sample_bytes, channels;
  int32_t layout, dtype;
  int32_t vec;                    // pointer and pitches are all multiples of 16: the 16-byte store instance (hm_view_batch_key_make's rule)
  uint32_t scale[4], bias[4];     // the floats' bits
} hm_view_multi_key;

inline void hm_view_multi_key_make(hm_view_multi_key* k, int staged, int32_t sample_bytes, int32_t channels, int32_t layout, int32_t dtype, int64_t row_pitch,
                                   int64_t plane_pitch, uintptr_t ptr, int chw, const float scale[4], const float bias[4])
{
  memset(k, 0, sizeof(*k));
  k->staged = staged ? 1 : 0;
  k->sample_bytes = sample_bytes; k->channels = channels;
  k->layout = layout; k->dtype = dtype;
  k->vec = (ptr % 16) == 0 && (row_pitch % 16) == 0 && (!chw || (plane_pitch % 16) == 0);
  memcpy(k->scale, scale, 16);
  memcpy(k->bias, bias, 16);
}
inline int hm_view_multi_key_equal(const hm_view_multi_key* a, const hm_view_multi_key* b) { return memcmp(a, b, sizeof(*a)) == 0; }

// What a workgroup reads about its view: one record in device memory, at an address that depends on the block index alone.
// Offsets of tap tables are 32-bit words from the start of the block; the intermediate's are float32 elements from the start of the
// chunk's intermediate.  96 bytes, 8-byte aligned.
typedef struct hm_view_rec {
  uint64_t src;                          // the crop's first sample (device address)
  uint64_t dst;                          // the destination's first element
  int64_t row_pitch, plane_pitch;        // of the destination, bytes
  int64_t tmp_off, tmp_pitch, tmp_plane; // the view's region of the intermediate; pitch a multiple of 16 elements
  int32_t n_h, ow, oh, E;                // rows of the crop, the size written, elements of a destination row (ow, or ow * C for HWC)
  int32_t x_first, x_count, x_weights;   // the horizontal axis: first[ow], count[ow], weights[taps][ow]
  int32_t y_first, y_count, y_weights;   // the vertical axis: first[oh], count[oh], weights[taps][oh]
} hm_view_rec;

// the block of a group of `views` views: the tap tables (table_words 32-bit words), then, 8-byte aligned, the records rec[views], then the
// running sums of row groups of the horizontal pass hsum[views] and of the vertical pass vsum[views] (they restart with every chunk)
typedef struct hm_view_multi_block { int64_t rec_off, hsum_off, vsum_off, bytes; } hm_view_multi_block;
inline hm_view_multi_block hm_view_multi_layout(int64_t table_words, int64_t views)
{
  hm_view_multi_block b;
  b.rec_off = (table_words * 4 + 7) / 8 * 8;
  b.hsum_off = b.rec_off + views * (int64_t)sizeof(hm_view_rec);
  b.vsum_off = b.hsum_off + views * 4;
  b.bytes = b.vsum_off + views * 4;
  return b;
}

// row groups (four rows per workgroup) of a view in a pass over `rows` rows
HM_VB_FN int32_t hm_view_row_groups(int32_t rows) { return (rows + 3) / 4; }

// blockIdx.y -> the view of a chunk: sums[i] = row groups of views 0 .. i of the chunk (rising, every view has at least one group), y <
// sums[n - 1].  The smallest i with y < sums[i], by bisection; *local = y's row group inside that view.  It reads nothing but the
// sums and depends on y alone: in a kernel it is uniform over the workgroup.
HM_VB_FN int hm_view_of_y(const int32_t* sums, int n, int32_t y, int32_t* local)
{
  int lo = 0, hi = n - 1; // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (y < sums[mid]) hi = mid;
    else lo = mid + 1;
  }
  *local = y - (lo ? sums[lo - 1] : 0);
  return lo;
}

// The cut of a group into chunks: views [first, first + n) of the group form the next chunk, where n is the most for which the sum of
// out_w x crop_h x C x 4 bytes stays within the bound (hm_view_chunk_frames': `bound` <= 0 is HM_VIEW_BATCH_BYTES) and the row groups of
// either pass sum to at most 65535 (gridDim.y's limit) - and at least one: a view beyond the bound is a chunk of its own.
// bytes[i], hgroups[i], vgroups[i]: of view i of the group.
enum { HM_VIEW_MULTI_Y_MOST = 65535 };
inline int32_t hm_view_multi_chunk(const int64_t* bytes, const int32_t* hgroups, const int32_t* vgroups, int32_t first, int32_t views, int64_t bound)
{
  if (bound <= 0) bound = HM_VIEW_BATCH_BYTES;
  int64_t b = 0, h = 0, v = 0;
  int32_t n = 0;
  while (first + n < views) {
    const int32_t i = first + n;
    if (n && (b + bytes[i] > bound || h + hgroups[i] > HM_VIEW_MULTI_Y_MOST || v + vgroups[i] > HM_VIEW_MULTI_Y_MOST)) break;
    b += bytes[i]; h += hgroups[i]; v += vgroups[i];
    n++;
  }
  return n;
}

#endif
