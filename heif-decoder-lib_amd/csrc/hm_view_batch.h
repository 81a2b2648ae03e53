// hm_view_batch.h — the index arithmetic of a batched view write (hm_view_write_batch, devdest.cpp; kernels: resample.hip): the key
// frames are grouped by, the cut of a group into chunks, the layout of the one block that goes up per group, and the split of a
// launch's z index.  Nothing but integers: no HIP, no allocation - a stand-alone host program can hold it to its rules
// (tests/host/view_batch_check.cpp).
#ifndef HM_VIEW_BATCH_H
#define HM_VIEW_BATCH_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HM_VB_FN __host__ __device__ inline
#else
#define HM_VB_FN inline
#endif

// what a launch of the batched kernels has ONE of: frames that agree in all of it share tap tables and launches.  Filled through
// hm_view_batch_key_make (zeroed first), compared as bytes.
typedef struct hm_view_batch_key {
  int32_t x, y, w, h;            // the crop
  int32_t ow, oh;                // the size written
  int32_t filter;
  int32_t sample_bytes, channels;
  int32_t layout, dtype;
  int32_t src_stride;            // (the kernels take one: frames of one picture size have one)
  int32_t vec;                   // pointer and pitches are all multiples of 16: the 16-byte store instance
  int32_t pad_;
  int64_t row_pitch, plane_pitch; // as resolved (never 0)
  uint32_t scale[4], bias[4];    // the floats' bits
} hm_view_batch_key;

inline void hm_view_batch_key_make(hm_view_batch_key* k, const int32_t crop[4], int32_t ow, int32_t oh, int32_t filter, int32_t sample_bytes, int32_t channels,
                                   int32_t layout, int32_t dtype, int32_t src_stride, int64_t row_pitch, int64_t plane_pitch, uintptr_t ptr, int chw,
                                   const float scale[4], const float bias[4])
{
  memset(k, 0, sizeof(*k));
  k->x = crop[0]; k->y = crop[1]; k->w = crop[2]; k->h = crop[3];
  k->ow = ow; k->oh = oh; k->filter = filter;
  k->sample_bytes = sample_bytes; k->channels = channels;
  k->layout = layout; k->dtype = dtype; k->src_stride = src_stride;
  k->row_pitch = row_pitch; k->plane_pitch = chw ? plane_pitch : 0;
  k->vec = (ptr % 16) == 0 && (row_pitch % 16) == 0 && (!chw || (plane_pitch % 16) == 0); // (launch_v's rule, resample.hip)
  memcpy(k->scale, scale, 16);
  memcpy(k->bias, bias, 16);
}
inline int hm_view_batch_key_equal(const hm_view_batch_key* a, const hm_view_batch_key* b) { return memcmp(a, b, sizeof(*a)) == 0; }

// The default bound of a chunk's intermediate: 64 MiB, a quarter of the 256 MB last-level cache, so that what the horizontal pass
// writes can still be there when the vertical pass reads it.  The figure rests on no measurement.
enum { HM_VIEW_BATCH_Z_MOST = 65535 };
static const int64_t HM_VIEW_BATCH_BYTES = (int64_t)64 << 20;

// frames per chunk: out_w x crop_h x C x 4 x frames <= bound, frames x planes <= gridDim.z's limit, at least one frame
inline int64_t hm_view_chunk_frames(int64_t ow, int64_t crop_h, int64_t channels, int64_t planes, int64_t bound)
{
  if (bound <= 0) bound = HM_VIEW_BATCH_BYTES;
  const int64_t per = ow * crop_h * channels * 4;
  int64_t n = per > 0 ? bound / per : 1;
  const int64_t z = HM_VIEW_BATCH_Z_MOST / (planes > 0 ? planes : 1);
  if (n > z) n = z;
  return n < 1 ? 1 : n;
}

// the block of a group of `frames` frames: the tap tables of both axes (words_x + words_y 32-bit words), then, 8-byte aligned,
// the source origins src[frames] and the destinations dst[frames]
typedef struct hm_view_block { int64_t src_off, dst_off, bytes; } hm_view_block;
inline hm_view_block hm_view_block_layout(int64_t words_x, int64_t words_y, int64_t frames)
{
  hm_view_block b;
  b.src_off = ((words_x + words_y) * 4 + 7) / 8 * 8;
  b.dst_off = b.src_off + frames * 8;
  b.bytes = b.dst_off + frames * 8;
  return b;
}

// k_resample_v_batch: z = frame * planes + plane
HM_VB_FN void hm_view_z_split(int z, int planes, int* frame, int* plane)
{
  *frame = z / planes;
  *plane = z - *frame * planes;
}

#endif
