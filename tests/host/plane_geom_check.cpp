// plane_geom_check.cpp - a stand-alone host program over the plane geometry of the library (csrc/hm_plane_geom.h): every function
// of the header beside the rule it stands for, stated here a second time in plain expressions and by hand-computed values - the plane
// layout of HeifPixelImage::ImagePlane::alloc (pixelimage.cc:139-218), the conformance window the decoder plugin hands over
// (decoder_libde265.cc:88-157) and the channel-by-channel paste of a tile (context.cc:2466-2497).  Built with
// -fsanitize=address,undefined by tests/test_plane_geom_host.py; exhaustive over chroma 0..3, channel 0..2, sizes 1..130 and
// 32767 / 32768, origins 0..130 and depths 8..16.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hm_plane_geom.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// What the paste of a 64 x 64 tile plane (the tiles of the suite) must come to in channel c: the rule of context.cc:2466-2497 in this
// project's words.  Halved is a direction a Cb / Cr channel is subsampled in (x under 4:2:0 and 4:2:2, y under 4:2:0); there the canvas
// extent AND the origin are halved rounding up, elsewhere both stay.  The origin must lie inside; the copy ends at the tile's or the
// channel's end, whichever comes first.
static int check_paste(int chroma, int c, int w, int h, int x0, int y0, long* inside, long* edge)
{
  const int tile = 64;
  const bool half_x = c > 0 && (chroma == 1 || chroma == 2), half_y = c > 0 && chroma == 1;
  const int want_w = half_x ? (w + 1) / 2 : w, want_h = half_y ? (h + 1) / 2 : h;
  const int want_x = half_x ? (x0 + 1) / 2 : x0, want_y = half_y ? (y0 + 1) / 2 : y0;
  const hm_tile_place p = hm_place_tile(chroma, c, w, h, x0, y0);
  CHECK(p.chan_w == want_w && p.chan_h == want_h && p.x0 == want_x && p.y0 == want_y && p.inside == (want_x < want_w && want_y < want_h));
  CHECK(p.chan_w == hm_plane_w(chroma, c, w) && p.chan_h == hm_plane_h(chroma, c, h));
  if (!p.inside) return 0;
  ++*inside;
  const int cw = hm_copy_extent(tile, p.chan_w, p.x0), ch = hm_copy_extent(tile, p.chan_h, p.y0);
  CHECK(cw == (want_w - want_x < tile ? want_w - want_x : tile) && ch == (want_h - want_y < tile ? want_h - want_y : tile));
  CHECK(cw >= 1 && ch >= 1 && p.x0 + cw <= p.chan_w && p.y0 + ch <= p.chan_h); // (what the paste writes lies inside the channel)
  if (p.x0 == p.chan_w - 1) { CHECK(cw == 1); ++*edge; }
  if (p.y0 == p.chan_h - 1) { CHECK(ch == 1); ++*edge; }
  return 0;
}

int main()
{
  std::vector<int> sizes;
  for (int v = 1; v <= 130; v++) sizes.push_back(v);
  sizes.push_back(32767); sizes.push_back(32768);

  // ---- bytes of a sample (pixelimage.cc:195): as many whole bytes as hold its bits - one up to 8 bits, two from 9 to 16 ----
  for (int bits = 8; bits <= 16; bits++) CHECK(hm_sample_bytes(bits) == (bits + 7) / 8 && hm_sample_bytes(bits) == (bits == 8 ? 1 : 2));

  // ---- rows of a plane (pixelimage.cc:139-148, 179): the height rounded up to an even count, and never fewer than 64 ----
  for (int h : sizes) {
    const int even = h % 2 ? h + 1 : h;
    CHECK(hm_padded_rows(h) == (even > 64 ? even : 64));
  }
  CHECK(hm_padded_rows(1) == 64 && hm_padded_rows(63) == 64 && hm_padded_rows(64) == 64 && hm_padded_rows(65) == 66);
  CHECK(hm_padded_rows(32767) == 32768 && hm_padded_rows(32768) == 32768);

  // ---- the size of a plane: luma / alpha / mono as the image, Cb / Cr (w + 1) / 2 under 4:2:0 and 4:2:2, (h + 1) / 2 under 4:2:0
  //      (context.cc:2469-2479; 4:0:0 has no chroma planes: c > 0 is not asked) ----
  for (int chroma = 0; chroma <= 3; chroma++)
    for (int c = 0; c < (chroma == 0 ? 1 : 3); c++)
      for (int v : sizes) {
        const bool cbcr = c > 0;
        CHECK(hm_plane_w(chroma, c, v) == (cbcr && (chroma == 1 || chroma == 2) ? (v + 1) / 2 : v));
        CHECK(hm_plane_h(chroma, c, v) == (cbcr && chroma == 1 ? (v + 1) / 2 : v));
      }

  // ---- the conformance window (decoder_libde265.cc:88-157: de265_get_image_width / height) and the header of a command stream ----
  for (int w : {8, 64, 130, 8192})
    for (int l : {0, 1, 7})
      for (int r : {0, 2, 5})
        for (int t : {0, 3})
          for (int b : {0, 4, 6}) {
            std::vector<unsigned char> blob(sizeof(hm_pic) + 16, 0);
            hm_pic h;
            std::memset(&h, 0, sizeof(h));
            h.width = (uint16_t)w; h.height = (uint16_t)(w + 8);
            h.crop_left = (uint16_t)l; h.crop_right = (uint16_t)r; h.crop_top = (uint16_t)t; h.crop_bottom = (uint16_t)b;
            std::memcpy(blob.data(), &h, sizeof(h));
            const hm_pic* p = hm_pic_of(blob.data());
            CHECK((const void*)p == (const void*)blob.data() && p->width == w && p->crop_bottom == b);
            CHECK(hm_window_w(*p) == w - l - r && hm_window_h(*p) == w + 8 - t - b);
          }
  { // (a window can be empty or negative in a damaged stream: the arithmetic is plain int, its callers refuse such a picture)
    hm_pic h;
    std::memset(&h, 0, sizeof(h));
    h.width = 8; h.height = 8; h.crop_left = 65535; h.crop_right = 65535; h.crop_top = 4; h.crop_bottom = 4;
    CHECK(hm_window_w(h) == 8 - 65535 - 65535 && hm_window_h(h) == 0);
  }

  // ---- the paste of a tile, channel by channel: every canvas width against every origin x (odd and even) over a few (height, y)
  //      pairs, then every canvas height against every origin y over a few (width, x) pairs ----
  const int other[][2] = {{1, 0}, {1, 1}, {64, 0}, {64, 63}, {65, 64}, {65, 65}, {127, 126}, {128, 127}, {129, 65}, {130, 129}, {130, 130}, {32767, 129}, {32768, 130}};
  long inside = 0, edge = 0;
  for (int chroma = 0; chroma <= 3; chroma++)
    for (int c = 0; c < (chroma == 0 ? 1 : 3); c++)
      for (int v : sizes)
        for (int o = 0; o <= 130; o++)
          for (const int (&q)[2] : other) {
            if (check_paste(chroma, c, v, q[0], o, q[1], &inside, &edge)) return 1;
            if (check_paste(chroma, c, q[0], v, q[1], o, &inside, &edge)) return 1;
          }
  CHECK(inside > 1000000 && edge > 10000);

  // ---- the cases that can go wrong, by name ----
  // odd origins under 4:2:0 and 4:2:2: the chroma origin rounds UP (context.cc:2471, 2474)
  CHECK(hm_place_tile(1, 1, 120, 100, 63, 63).x0 == 32 && hm_place_tile(1, 2, 120, 100, 63, 63).y0 == 32);
  CHECK(hm_place_tile(2, 1, 120, 100, 63, 63).x0 == 32 && hm_place_tile(2, 1, 120, 100, 63, 63).y0 == 63);
  CHECK(hm_place_tile(3, 1, 120, 100, 63, 63).x0 == 63 && hm_place_tile(1, 0, 120, 100, 63, 63).x0 == 63);
  // origin equal to the channel size: outside; one less: inside, one sample copied
  CHECK(!hm_place_tile(1, 1, 127, 100, 127, 0).inside);                                                        // chroma: 64 wide, origin 64
  CHECK(hm_place_tile(1, 0, 127, 100, 126, 0).inside && hm_place_tile(1, 1, 127, 100, 126, 0).inside);         // luma 126 of 127, chroma 63 of 64
  CHECK(hm_copy_extent(64, 127, 126) == 1 && hm_copy_extent(32, 64, 63) == 1);
  CHECK(hm_place_tile(1, 0, 128, 100, 127, 0).inside && !hm_place_tile(1, 1, 128, 100, 127, 0).inside);        // luma inside, chroma (64 of 64) outside
  CHECK(!hm_place_tile(1, 0, 64, 100, 64, 0).inside && !hm_place_tile(0, 0, 64, 64, 0, 64).inside);
  std::puts("plane geometry: ok");
  return 0;
}
