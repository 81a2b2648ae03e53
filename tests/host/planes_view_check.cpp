// planes_view_check.cpp - a stand-alone host program over the index arithmetic of a planar view write (csrc/hm_planes_view.h): the
// geometry, the blockIdx.y plane ranges, the lane-group to element and pair maps of the vertical pass (ragged tails, the 16-byte
// and the element-wise path), the columns of the horizontal pass in the intermediate, the grouping key, the chunk cut and the
// block layout.  Built with -fsanitize=address,undefined by tests/test_planes_view_host.py: every plane and every intermediate is
// really allocated at its exact size, the launches are walked block by block, wave by wave and lane by lane the way the kernels
// of planes_view.hip walk them, and every element must be covered exactly once and nothing else.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hm_planes_view.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// the vertical launch over the destination planes of an ow x oh result: w[p] elements (pairs) per row, rows[p], pair[p], vec[p]
static int walk_vertical(const int w[4], const int rows[4], const int pair[4], const int vec[4], int elem_bytes)
{
  int32_t y_end[4];
  int at = 0, gx = 0;
  for (int p = 0; p < 4; p++) {
    if (rows[p] > 0) {
      at += (rows[p] + 3) / 4;
      const int bx = hm_pv_blocks_x(w[p], hm_pv_per_lane(elem_bytes, pair[p]));
      gx = gx > bx ? gx : bx;
    }
    y_end[p] = at;
  }
  std::vector<std::vector<int>> seen(4);
  for (int p = 0; p < 4; p++) seen[(size_t)p].assign((size_t)(rows[p] > 0 ? w[p] * (pair[p] ? 2 : 1) * rows[p] : 0), 0);
  for (int by = 0; by < y_end[3]; by++)
    for (int bx = 0; bx < gx; bx++)
      for (int wave = 0; wave < 4; wave++) {
        const int p = hm_pv_plane_of(by, y_end), k = hm_pv_row_of(by, p, y_end, wave);
        CHECK(p >= 0 && p < 4 && rows[p] > 0 && k >= 0); // (a block never lands on an absent plane)
        if (k >= rows[p]) continue;
        const int per = hm_pv_per_lane(elem_bytes, pair[p]), mult = pair[p] ? 2 : 1;
        if (bx >= hm_pv_blocks_x(w[p], per)) continue;
        std::vector<int>& s = seen[(size_t)p];
        const size_t row = (size_t)k * w[p] * mult;
        for (int lane = 0; lane < 64; lane++) {
          if (vec[p]) {
            int x0 = -1;
            const int n = hm_pv_vec_span(bx, lane, per, w[p], &x0);
            CHECK(n >= 0 && n <= per && x0 % per == 0);
            CHECK(n == 0 || ((size_t)x0 * mult * elem_bytes) % 16 == 0); // a 16-byte store at a 16-byte offset of the row
            for (int q = 0; q < n * mult; q++) s.at(row + (size_t)x0 * mult + q)++;
          }
          else
            for (int i = 0; i < per; i++) {
              const int x = hm_pv_elem_at(bx, lane, per, i);
              CHECK(x >= 0);
              if (x >= w[p]) continue;
              for (int q = 0; q < mult; q++) s.at(row + (size_t)x * mult + q)++;
            }
        }
      }
  for (int p = 0; p < 4; p++)
    for (int v : seen[(size_t)p]) CHECK(v == 1);
  return 0;
}

// the horizontal launch over the source planes: every (row, column) of every plane's region once, the pitch padding never
static int walk_horizontal(const int32_t crop[4][4], const int32_t out[4][2], const int present[4])
{
  int64_t off[4], pitch[4];
  const int64_t total = hm_pv_tmp_layout(crop, out, present, off, pitch);
  std::vector<int> tmp((size_t)total, 0);
  int32_t y_end[4];
  int at = 0, gx = 0;
  for (int p = 0; p < 4; p++) {
    if (present[p]) {
      CHECK(pitch[p] % 16 == 0 && pitch[p] >= out[p][0] && pitch[p] < out[p][0] + 16 && off[p] % 4 == 0);
      at += (crop[p][3] + 3) / 4;
      gx = gx > (out[p][0] + 63) / 64 ? gx : (out[p][0] + 63) / 64;
    }
    y_end[p] = at;
  }
  for (int by = 0; by < y_end[3]; by++)
    for (int bx = 0; bx < gx; bx++)
      for (int wave = 0; wave < 4; wave++) {
        const int p = hm_pv_plane_of(by, y_end), y = hm_pv_row_of(by, p, y_end, wave);
        CHECK(present[p]);
        if (bx * 64 >= out[p][0] || y >= crop[p][3]) continue;
        for (int lane = 0; lane < 64; lane++) {
          const int j = bx * 64 + lane;
          if (j < out[p][0]) tmp.at((size_t)(off[p] + (int64_t)y * pitch[p] + j))++;
        }
      }
  for (int p = 0; p < 4; p++) {
    if (!present[p]) continue;
    for (int y = 0; y < crop[p][3]; y++)
      for (int64_t j = 0; j < pitch[p]; j++) CHECK(tmp[(size_t)(off[p] + y * pitch[p] + j)] == (j < out[p][0] ? 1 : 0));
    // the vertical pass loads whole vectors of up to 16 elements from a row: they end inside the row's pitch
    for (int per : {4, 8, 16}) CHECK((out[p][0] + per - 1) / per * per <= pitch[p]);
  }
  int64_t covered = 0;
  for (int v : tmp) covered += v;
  int64_t want = 0;
  for (int p = 0; p < 4; p++) want += present[p] ? (int64_t)out[p][0] * crop[p][3] : 0;
  CHECK(covered == want);
  return 0;
}

static hm_pv_key key_of(int chroma, int x, int ow, int64_t pitch1, uintptr_t ptr1, float s0, int stride0)
{
  hm_pv_key k;
  memset(&k, 0, sizeof(k));
  k.chroma = chroma; k.bits = 8; k.filter = 0; k.layout = 1; k.dtype = 0;
  hm_pv_geometry(chroma, x, 2, 191, 127, ow, 50, k.crop, k.out);
  for (int c = 0; c < 3; c++) k.stride[c] = c == 0 ? stride0 : 128;
  k.pitch[0] = 96; k.pitch[1] = pitch1;
  k.vec[0] = hm_pv_vec_class(0x1000, 96); k.vec[1] = hm_pv_vec_class(ptr1, pitch1);
  const float scale[4] = {s0, 1.0f, 1.0f, 1.0f}, bias[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  memcpy(k.scale, scale, 16);
  memcpy(k.bias, bias, 16);
  return k;
}

int main()
{
  // ---- geometry: chroma crops inside the chroma plane, the output the plane size of an ow x oh result ----
  for (int chroma = 0; chroma < 4; chroma++) {
    const int sx = hm_pv_sub_x(chroma), sy = hm_pv_sub_y(chroma);
    for (int W = 1; W <= 20; W++)
      for (int x = 0; x < W; x++)
        for (int w = 1; x + w <= W; w++) {
          int32_t crop[4][4], out[4][2];
          const int bad = hm_pv_geometry(chroma, x, 0, w, 3, 2 * w + 1, 5, crop, out);
          CHECK((bad != 0) == (x % sx != 0));
          if (bad) continue;
          CHECK(crop[0][0] == x && crop[0][2] == w && crop[3][2] == w && out[0][0] == 2 * w + 1 && out[3][1] == 5);
          if (chroma == 0) { CHECK(crop[1][2] == 0 && out[2][0] == 0); continue; }
          CHECK(crop[1][0] + crop[1][2] <= (W + sx - 1) / sx && crop[1][2] >= 1 && crop[2][0] == crop[1][0]);
          CHECK(out[1][0] == (2 * w + 1 + sx - 1) / sx && out[1][1] == (5 + sy - 1) / sy && crop[1][3] == (3 + sy - 1) / sy);
        }
    int32_t crop[4][4], out[4][2];
    CHECK((hm_pv_geometry(chroma, 0, 1, 4, 4, 4, 4, crop, out) != 0) == (sy == 2));
  }

  // ---- the vertical and the nearest launch: plane ranges, lane maps, ragged tails; every element exactly once ----
  for (int chroma = 0; chroma < 4; chroma++)
    for (int semi = 0; semi < 2; semi++)
      for (int elem : {1, 2, 4})
        for (int alpha = 0; alpha < 2; alpha++)
          for (int ow : {1, 7, 16, 77, 128, 129, 1030})
            for (int oh : {1, 3, 4, 51}) {
              int32_t crop[4][4], out[4][2];
              CHECK(hm_pv_geometry(chroma, 0, 0, ow, oh, ow, oh, crop, out) == 0);
              const int pair[4] = {0, semi && chroma != 0, 0, 0};
              int w[4], rows[4];
              for (int p = 0; p < 4; p++) {
                const bool there = p == 0 || (p == 3 ? alpha != 0 : chroma != 0 && !(semi && p == 2));
                w[p] = there ? out[p][0] : 0; rows[p] = there ? out[p][1] : 0;
              }
              for (int mask = 0; mask < 16; mask += 5) { // all vector, all element-wise, and two mixtures: one plane alone off the 16-byte path
                const int vec[4] = {!(mask & 1), !(mask & 2), !(mask & 4), !(mask & 8)};
                if (walk_vertical(w, rows, pair, vec, elem)) return 1;
              }
              // k_planes_view_nearest: one lane per element (pair) = the element-wise map with one element per lane
              int gx = 0;
              for (int p = 0; p < 4; p++) gx = rows[p] > 0 && (w[p] + 63) / 64 > gx ? (w[p] + 63) / 64 : gx;
              for (int p = 0; p < 4; p++) {
                if (rows[p] <= 0) continue;
                std::vector<int> s((size_t)w[p], 0);
                for (int bx = 0; bx < gx; bx++)
                  for (int lane = 0; lane < 64; lane++)
                    if (bx * 64 + lane < w[p]) s.at((size_t)(bx * 64 + lane))++;
                for (int v : s) CHECK(v == 1);
              }
            }

  // ---- the horizontal launch: every column of every source row of every plane's region, the padding never ----
  for (int chroma = 0; chroma < 4; chroma++)
    for (int alpha = 0; alpha < 2; alpha++)
      for (int ow : {1, 16, 77, 200})
        for (int h : {1, 5, 136}) {
          int32_t crop[4][4], out[4][2];
          CHECK(hm_pv_geometry(chroma, 2, 2, 150, h, ow, 9, crop, out) == 0);
          const int present[4] = {1, chroma != 0, chroma != 0, alpha};
          if (walk_horizontal(crop, out, present)) return 1;
        }

  // ---- the key: equal where everything a launch has one of is equal, whatever the pointer (inside an alignment class) ----
  const hm_pv_key a = key_of(1, 2, 96, 96, 0x2000, 1.0f, 256), b = key_of(1, 2, 96, 96, 0x2000 + 96 * 25, 1.0f, 256);
  CHECK(hm_pv_key_equal(&a, &b) && a.vec[0] == 1 && a.vec[1] == 1);
  const hm_pv_key off = key_of(1, 2, 96, 96, 0x2002, 1.0f, 256), pitch = key_of(1, 2, 96, 100, 0x2000, 1.0f, 256);
  const hm_pv_key crop = key_of(1, 4, 96, 96, 0x2000, 1.0f, 256), size = key_of(1, 2, 98, 98, 0x2000, 1.0f, 256);
  const hm_pv_key scale = key_of(1, 2, 96, 96, 0x2000, 0.5f, 256), stride = key_of(1, 2, 96, 96, 0x2000, 1.0f, 320), fmt = key_of(2, 2, 96, 96, 0x2000, 1.0f, 256);
  CHECK(!hm_pv_key_equal(&a, &off) && off.vec[1] == 0 && off.vec[0] == 1);
  CHECK(!hm_pv_key_equal(&a, &pitch) && pitch.vec[1] == 0);
  CHECK(!hm_pv_key_equal(&a, &crop) && !hm_pv_key_equal(&a, &size) && !hm_pv_key_equal(&a, &scale) && !hm_pv_key_equal(&a, &stride) && !hm_pv_key_equal(&a, &fmt));

  // ---- the chunk cut: frame_elems x 4 x frames <= bound, frames <= 65535, at least one; every frame in exactly one chunk ----
  const int64_t fe = 80 * 136 + 2 * 48 * 68, per = fe * 4;
  CHECK(hm_pv_chunk_frames(fe, 3 * per) == 3 && hm_pv_chunk_frames(fe, 3 * per + per - 1) == 3 && hm_pv_chunk_frames(fe, 4 * per) == 4);
  CHECK(hm_pv_chunk_frames(fe, 1) == 1 && hm_pv_chunk_frames(fe, per - 1) == 1);
  CHECK(hm_pv_chunk_frames(16, 0) == HM_PV_Z_MOST && hm_pv_chunk_frames(fe, 0) == ((int64_t)64 << 20) / per);
  CHECK(hm_pv_chunk_frames((int64_t)32768 * 32768 * 3, 0) == 1); // (no overflow)
  for (int frames : {1, 2, 8, 1000})
    for (int64_t bound : {(int64_t)1, per, 3 * per + 7, 64 * per}) {
      const int64_t n = hm_pv_chunk_frames(fe, bound);
      const int step = (int)(n < frames ? n : frames);
      std::vector<int> seen((size_t)frames, 0);
      for (int c0 = 0; c0 < frames; c0 += step) {
        const int m = step < frames - c0 ? step : frames - c0;
        CHECK(m >= 1 && (m == 1 || m * per <= bound) && m <= HM_PV_Z_MOST);
        for (int i = 0; i < m; i++) seen.at((size_t)(c0 + i))++;
      }
      for (int v : seen) CHECK(v == 1);
    }

  // ---- the block: tables, then the records, 8-byte aligned, nothing overlapping, nothing past the end ----
  CHECK(sizeof(hm_pv_rec) == 64);
  for (int frames : {1, 3, 8, 128})
    for (int64_t words : {(int64_t)0, (int64_t)77 * 5 + 51 * 4 + 39 * 5 + 26 * 4, (int64_t)224 * 9 + 1}) {
      const hm_pv_block l = hm_pv_block_layout(words, frames);
      CHECK(l.rec_off % 8 == 0 && l.rec_off >= words * 4 && l.rec_off < words * 4 + 8 && l.bytes == l.rec_off + 64 * frames);
      unsigned char* block = (unsigned char*)std::malloc((size_t)l.bytes);
      CHECK(block);
      int32_t* tab = (int32_t*)block;
      for (int64_t i = 0; i < words; i++) tab[i] = (int32_t)i;
      hm_pv_rec* rec = (hm_pv_rec*)(block + l.rec_off);
      for (int i = 0; i < frames; i++)
        for (int c = 0; c < 4; c++) { rec[i].src[c] = (uint64_t)(i * 8 + c); rec[i].dst[c] = (uint64_t)(i * 8 + 4 + c); }
      for (int64_t i = 0; i < words; i++) CHECK(tab[i] == (int32_t)i);
      for (int i = 0; i < frames; i++)
        for (int c = 0; c < 4; c++) CHECK(rec[i].src[c] == (uint64_t)(i * 8 + c) && rec[i].dst[c] == (uint64_t)(i * 8 + 4 + c));
      std::free(block);
    }
  std::puts("planes view arithmetic: ok");
  return 0;
}
