// view_batch_check.cpp - a stand-alone host program over the index arithmetic of a batched view write (csrc/hm_view_batch.h): the
// grouping key, the cut of a group into chunks, the layout of a group's block, and the z -> (frame, plane) split of the vertical
// launch.  Built with -fsanitize=address,undefined by tests/test_view_batch_host.py: the block is really allocated at the size
// the layout gives and every table word and pointer slot is written, the chunks are walked the way view_write_group walks them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hm_view_batch.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static hm_view_batch_key key_of(int x, int ow, int64_t row_pitch, int64_t plane_pitch, uintptr_t ptr, int chw, float s0)
{
  const int32_t crop[4] = {x, 5, 191, 127};
  const float scale[4] = {s0, 1.0f, 1.0f, 1.0f}, bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  hm_view_batch_key k;
  hm_view_batch_key_make(&k, crop, ow, 50, 0, 1, 3, chw, 3, 640, row_pitch, plane_pitch, ptr, chw, scale, bias);
  return k;
}

int main()
{
  // ---- the key: equal where everything a launch has one of is equal, whatever the pointer (inside an alignment class) ----
  const hm_view_batch_key a = key_of(3, 96, 384, 384 * 50, 0x1000, 1, 1.0f);
  const hm_view_batch_key b = key_of(3, 96, 384, 384 * 50, 0x1000 + 384 * 50 * 3, 1, 1.0f);
  CHECK(hm_view_batch_key_equal(&a, &b) && a.vec == 1);
  const hm_view_batch_key off = key_of(3, 96, 384, 384 * 50, 0x1004, 1, 1.0f);       // a pointer off 16 bytes: the element-store class
  const hm_view_batch_key pitch = key_of(3, 96, 448, 448 * 50, 0x1000, 1, 1.0f);     // a padded row pitch
  const hm_view_batch_key plane = key_of(3, 96, 384, 384 * 53, 0x1000, 1, 1.0f);     // a padded plane pitch
  const hm_view_batch_key odd = key_of(3, 97, 388, 388 * 50, 0x1000, 1, 1.0f);       // rows that are no multiple of 16 bytes
  const hm_view_batch_key crop = key_of(4, 96, 384, 384 * 50, 0x1000, 1, 1.0f);
  const hm_view_batch_key scale = key_of(3, 96, 384, 384 * 50, 0x1000, 1, 0.5f);
  const hm_view_batch_key hwc = key_of(3, 96, 384 * 3, 0, 0x1000, 0, 1.0f);
  const hm_view_batch_key hwc2 = key_of(3, 96, 384 * 3, 12345, 0x1000, 0, 1.0f);     // (HWC: the plane pitch is not looked at)
  CHECK(!hm_view_batch_key_equal(&a, &off) && off.vec == 0);
  CHECK(!hm_view_batch_key_equal(&a, &pitch) && !hm_view_batch_key_equal(&a, &plane) && !hm_view_batch_key_equal(&a, &odd) && odd.vec == 0);
  CHECK(!hm_view_batch_key_equal(&a, &crop) && !hm_view_batch_key_equal(&a, &scale) && !hm_view_batch_key_equal(&a, &hwc));
  CHECK(hm_view_batch_key_equal(&hwc, &hwc2) && hwc.vec == 1);

  // ---- the chunk cut: out_w x crop_h x C x 4 x frames <= bound, frames x planes <= 65535, at least one ----
  const int64_t per = 97 * 127 * 3 * 4;
  CHECK(hm_view_chunk_frames(97, 127, 3, 3, 2 * per) == 2 && hm_view_chunk_frames(97, 127, 3, 3, 3 * per - 1) == 2 && hm_view_chunk_frames(97, 127, 3, 3, 3 * per) == 3);
  CHECK(hm_view_chunk_frames(97, 127, 3, 3, 1) == 1 && hm_view_chunk_frames(97, 127, 3, 3, per - 1) == 1);
  CHECK(hm_view_chunk_frames(224, 1080, 3, 3, 0) == HM_VIEW_BATCH_BYTES / (224 * 1080 * 3 * 4)); // the default: 23 frames of 1080 rows
  CHECK(hm_view_chunk_frames(1, 1, 3, 3, 0) == 65535 / 3 && hm_view_chunk_frames(1, 1, 4, 4, 0) == 65535 / 4 && hm_view_chunk_frames(1, 1, 3, 1, 0) == 65535);
  CHECK(hm_view_chunk_frames(32768, 32768, 4, 4, 0) == 1); // (no overflow: 2^34 bytes per frame)
  for (int frames : {1, 2, 5, 64, 1000}) {
    for (int64_t bound : {(int64_t)1, per, 2 * per + 7, 64 * per}) {
      const int64_t n = hm_view_chunk_frames(97, 127, 3, 3, bound);
      std::vector<int> seen((size_t)frames, 0); // every frame in exactly one chunk, chunks in order
      int chunks = 0;
      for (int c0 = 0; c0 < frames; c0 += (int)(n < frames ? n : frames), chunks++) {
        const int m = (int)(n < frames - c0 ? n : frames - c0);
        CHECK(m >= 1 && (m == 1 || m * per <= bound) && (int64_t)m * 3 <= HM_VIEW_BATCH_Z_MOST);
        for (int i = 0; i < m; i++) seen[(size_t)(c0 + i)]++;
      }
      for (int v : seen) CHECK(v == 1);
      CHECK(chunks == (frames + (n < frames ? n : frames) - 1) / (n < frames ? n : frames));
    }
  }

  // ---- the block: tables, then the pointer arrays, 8-byte aligned, nothing overlapping, nothing past the end ----
  for (int frames : {1, 3, 5, 128}) {
    for (int64_t wx : {(int64_t)97 * 4, (int64_t)224 * 5, (int64_t)1 * 3}) {
      const int64_t wy = 50 * 4 + 1; // (an odd word count: the pad in front of the pointers)
      const hm_view_block l = hm_view_block_layout(wx, wy, frames);
      CHECK(l.src_off % 8 == 0 && l.src_off >= (wx + wy) * 4 && l.src_off < (wx + wy) * 4 + 8);
      CHECK(l.dst_off == l.src_off + 8 * frames && l.bytes == l.dst_off + 8 * frames);
      unsigned char* block = (unsigned char*)std::malloc((size_t)l.bytes);
      CHECK(block);
      int32_t* words = (int32_t*)block;
      for (int64_t i = 0; i < wx + wy; i++) words[i] = (int32_t)i;
      const void** src = (const void**)(block + l.src_off);
      void** dst = (void**)(block + l.dst_off);
      for (int i = 0; i < frames; i++) { src[i] = block + i; dst[i] = block + 2 * i; }
      for (int64_t i = 0; i < wx + wy; i++) CHECK(words[i] == (int32_t)i);
      for (int i = 0; i < frames; i++) CHECK(src[i] == block + i && dst[i] == block + 2 * i);
      std::free(block);
    }
  }

  // ---- z = frame * planes + plane ----
  for (int planes : {1, 3, 4}) {
    const int frames = HM_VIEW_BATCH_Z_MOST / planes;
    int z = 0;
    for (int f = 0; f < frames; f++)
      for (int p = 0; p < planes; p++, z++) {
        int fr = -1, pl = -1;
        hm_view_z_split(z, planes, &fr, &pl);
        CHECK(fr == f && pl == p);
      }
    CHECK(z <= HM_VIEW_BATCH_Z_MOST);
  }
  std::puts("view batch arithmetic: ok");
  return 0;
}
