// view_multi_check.cpp - a stand-alone host program over the index arithmetic of a multi-view write (csrc/hm_view_multi.h): the
// grouping key, the layout of a group's block, the cut of blockIdx.y by running sums, and the cut of a group into chunks.  Built
// with -fsanitize=address,undefined by tests/test_view_multi_host.py: the block is really allocated at the size the layout gives and
// every table word, record and sum is written, the chunks are walked the way views_write_group walks them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hm_view_multi.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static hm_view_multi_key key_of(int staged, int dtype, int64_t row_pitch, int64_t plane_pitch, uintptr_t ptr, int chw, float s0)
{
  const float scale[4] = {s0, 1.0f, 1.0f, 1.0f}, bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  hm_view_multi_key k;
  hm_view_multi_key_make(&k, staged, 1, 3, chw, dtype, row_pitch, plane_pitch, ptr, chw, scale, bias);
  return k;
}

// the chunks of a group, walked as the writer walks them: every view in exactly one chunk, in order, both bounds kept
static int walk_chunks(const std::vector<int64_t>& bytes, const std::vector<int32_t>& hg, const std::vector<int32_t>& vg, int64_t bound, int* chunks_out)
{
  const int32_t m = (int32_t)bytes.size();
  const int64_t limit = bound > 0 ? bound : HM_VIEW_BATCH_BYTES;
  int chunks = 0;
  for (int32_t c0 = 0; c0 < m; chunks++) {
    const int32_t n = hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), c0, m, bound);
    CHECK(n >= 1 && c0 + n <= m); // never empty, never past the end
    int64_t b = 0, h = 0, v = 0;
    for (int32_t i = c0; i < c0 + n; i++) { b += bytes[(size_t)i]; h += hg[(size_t)i]; v += vg[(size_t)i]; }
    CHECK(n == 1 || (b <= limit && h <= HM_VIEW_MULTI_Y_MOST && v <= HM_VIEW_MULTI_Y_MOST)); // a view beyond a bound: a chunk of its own
    if (c0 + n < m) { // greedy: the next view did not fit
      const size_t x = (size_t)(c0 + n);
      CHECK(b + bytes[x] > limit || h + hg[x] > HM_VIEW_MULTI_Y_MOST || v + vg[x] > HM_VIEW_MULTI_Y_MOST);
    }
    c0 += n;
  }
  *chunks_out = chunks;
  return 0;
}

int main()
{
  // ---- the key: what a launch has one of; crop, sizes, pitches and the pointer (inside an alignment class) are the record's ----
  const hm_view_multi_key a = key_of(0, 3, 384, 384 * 50, 0x1000, 1, 1.0f);
  const hm_view_multi_key other_pitch = key_of(0, 3, 896, 896 * 224, 0x1000 + 384 * 50 * 3 + 16, 1, 1.0f); // another size, 16-byte aligned all the same
  CHECK(hm_view_multi_key_equal(&a, &other_pitch) && a.vec == 1);
  const hm_view_multi_key off = key_of(0, 3, 384, 384 * 50, 0x1004, 1, 1.0f);   // a pointer off 16 bytes: the element-store class
  const hm_view_multi_key odd = key_of(0, 3, 308, 308 * 77, 0x1000, 1, 1.0f);   // rows of 308 bytes: no multiple of 16
  const hm_view_multi_key plane = key_of(0, 3, 384, 384 * 50 + 4, 0x1000, 1, 1.0f);
  const hm_view_multi_key staged = key_of(1, 3, 384, 384 * 50, 0x1000, 1, 1.0f);
  const hm_view_multi_key dtype = key_of(0, 0, 384, 384 * 50, 0x1000, 1, 1.0f);
  const hm_view_multi_key scale = key_of(0, 3, 384, 384 * 50, 0x1000, 1, 0.5f);
  const hm_view_multi_key hwc = key_of(0, 3, 384 * 3, 0, 0x1000, 0, 1.0f);
  const hm_view_multi_key hwc2 = key_of(0, 3, 384 * 3, 12345, 0x1000, 0, 1.0f);  // (HWC: the plane pitch is not looked at)
  CHECK(!hm_view_multi_key_equal(&a, &off) && off.vec == 0 && !hm_view_multi_key_equal(&a, &odd) && odd.vec == 0 && hm_view_multi_key_equal(&off, &odd));
  CHECK(!hm_view_multi_key_equal(&a, &plane) && plane.vec == 0);
  CHECK(!hm_view_multi_key_equal(&a, &staged) && !hm_view_multi_key_equal(&a, &dtype) && !hm_view_multi_key_equal(&a, &scale) && !hm_view_multi_key_equal(&a, &hwc));
  CHECK(hm_view_multi_key_equal(&hwc, &hwc2) && hwc.vec == 1);

  // ---- the block: tables, then the records 8-byte aligned, then the two arrays of sums; nothing overlaps, nothing past the end ----
  CHECK(sizeof(hm_view_rec) == 96 && sizeof(hm_view_rec) % 8 == 0);
  for (int views : {1, 3, 10, (int)4096}) {
    for (int64_t words : {(int64_t)1, (int64_t)97 * 4 + 50 * 4 + 1, (int64_t)224 * 9}) {
      const hm_view_multi_block l = hm_view_multi_layout(words, views);
      CHECK(l.rec_off % 8 == 0 && l.rec_off >= words * 4 && l.rec_off < words * 4 + 8);
      CHECK(l.hsum_off == l.rec_off + (int64_t)views * 96 && l.hsum_off % 4 == 0);
      CHECK(l.vsum_off == l.hsum_off + 4 * (int64_t)views && l.bytes == l.vsum_off + 4 * (int64_t)views);
      unsigned char* block = (unsigned char*)std::malloc((size_t)l.bytes);
      CHECK(block);
      int32_t* w = (int32_t*)block;
      hm_view_rec* rec = (hm_view_rec*)(block + l.rec_off);
      int32_t* hs = (int32_t*)(block + l.hsum_off);
      int32_t* vs = (int32_t*)(block + l.vsum_off);
      for (int64_t i = 0; i < words; i++) w[i] = (int32_t)i;
      for (int i = 0; i < views; i++) { memset(&rec[i], 0, sizeof(rec[i])); rec[i].src = (uint64_t)i; rec[i].y_weights = -i; hs[i] = 3 * i; vs[i] = 5 * i; }
      for (int64_t i = 0; i < words; i++) CHECK(w[i] == (int32_t)i);
      for (int i = 0; i < views; i++) CHECK(rec[i].src == (uint64_t)i && rec[i].y_weights == -i && hs[i] == 3 * i && vs[i] == 5 * i);
      std::free(block);
    }
  }

  // ---- blockIdx.y -> view: every y of every view, first and last included, views of one row group, one view, HM_VIEWS_MOST (4096) views ----
  for (int n : {1, 2, 3, 7, 64, 4096}) {
    std::vector<int32_t> rows((size_t)n), sums((size_t)n);
    int32_t total = 0;
    for (int i = 0; i < n; i++) {
      rows[(size_t)i] = n == 4096 ? 1 + (i % 3 == 0 ? 0 : i % 61) : (i % 2 ? 1 : 4 * i + 130); // (views of ONE row: one group)
      total += hm_view_row_groups(rows[(size_t)i]);
      sums[(size_t)i] = total;
    }
    CHECK(total <= HM_VIEW_MULTI_Y_MOST);
    int32_t y = 0;
    for (int i = 0; i < n; i++)
      for (int32_t g = 0; g < hm_view_row_groups(rows[(size_t)i]); g++, y++) {
        int32_t local = -1;
        CHECK(hm_view_of_y(sums.data(), n, y, &local) == i && local == g);
      }
    CHECK(y == total);
  }
  CHECK(hm_view_row_groups(1) == 1 && hm_view_row_groups(4) == 1 && hm_view_row_groups(5) == 2);

  // ---- the chunk cut ----
  {
    // the multi-crop set: 2 x 224^2 from large crops, 8 x 96^2 from small ones (C = 3): under the default bound one chunk
    std::vector<int64_t> bytes;
    std::vector<int32_t> hg, vg;
    for (int i = 0; i < 10; i++) {
      const int ow = i < 2 ? 224 : 96, crop_h = i < 2 ? 2400 : 700;
      bytes.push_back((int64_t)ow * crop_h * 3 * 4); hg.push_back(hm_view_row_groups(crop_h)); vg.push_back(hm_view_row_groups(ow));
    }
    int chunks = 0;
    CHECK(walk_chunks(bytes, hg, vg, 0, &chunks) == 0 && chunks == 1);
    CHECK(walk_chunks(bytes, hg, vg, 1, &chunks) == 0 && chunks == 10);               // a bound below every view: a view per chunk
    CHECK(walk_chunks(bytes, hg, vg, bytes[2] * 3, &chunks) == 0 && chunks == 2 + 3); // the two large ones alone, the small ones by threes (3, 3, 2)
    CHECK(hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), 0, 10, bytes[0] + bytes[1]) == 2);
    CHECK(hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), 0, 10, bytes[0] + bytes[1] - 1) == 1);
    CHECK(hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), 9, 10, 1) == 1);
    // one view larger than the bound between small ones: a chunk of its own
    std::vector<int64_t> b2 = {100, 100, 5000, 100, 100};
    std::vector<int32_t> g2 = {1, 1, 1, 1, 1};
    CHECK(hm_view_multi_chunk(b2.data(), g2.data(), g2.data(), 0, 5, 250) == 2 && hm_view_multi_chunk(b2.data(), g2.data(), g2.data(), 2, 5, 250) == 1 &&
          hm_view_multi_chunk(b2.data(), g2.data(), g2.data(), 3, 5, 250) == 2);
    CHECK(walk_chunks(b2, g2, g2, 250, &chunks) == 0 && chunks == 3);
  }
  {
    // the row-group bound: 4096 views of 100 rows (25 groups each: 102400 in all) cut at 65535 / 25 = 2621 views, whichever pass is the longer
    std::vector<int64_t> bytes(4096, 16);
    std::vector<int32_t> tall(4096, 25), flat(4096, 1);
    int chunks = 0;
    CHECK(hm_view_multi_chunk(bytes.data(), tall.data(), flat.data(), 0, 4096, 0) == 2621 && hm_view_multi_chunk(bytes.data(), flat.data(), tall.data(), 0, 4096, 0) == 2621);
    CHECK(walk_chunks(bytes, tall, flat, 0, &chunks) == 0 && chunks == 2);
    CHECK(walk_chunks(bytes, flat, flat, 0, &chunks) == 0 && chunks == 1);   // count = HM_VIEWS_MOST in one chunk
    CHECK(walk_chunks(bytes, flat, tall, 16 * 100, &chunks) == 0 && chunks == 41); // 100 views per chunk by bytes: 40 full ones and one of 96
    // a single view with more row groups than a launch takes is still a chunk (the launcher refuses it, the cut does not loop)
    std::vector<int64_t> one_b = {1};
    std::vector<int32_t> huge = {70000}, small = {1};
    CHECK(hm_view_multi_chunk(one_b.data(), huge.data(), small.data(), 0, 1, 0) == 1);
    // count = 1
    CHECK(walk_chunks(one_b, small, small, 0, &chunks) == 0 && chunks == 1);
  }
  // (no overflow: 4096 views of 2^34 bytes each)
  {
    std::vector<int64_t> bytes(4096, (int64_t)1 << 34);
    std::vector<int32_t> g(4096, 8192);
    int chunks = 0;
    CHECK(walk_chunks(bytes, g, g, 0, &chunks) == 0 && chunks == 4096);
  }
  std::puts("view multi arithmetic: ok");
  return 0;
}
