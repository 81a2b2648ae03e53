// overlay_plan_check.cpp - stand-alone host program over csrc/hm_overlay_plan.h (built by tests/test_overlay_plan_host.py under
// AddressSanitizer and UndefinedBehaviorSanitizer): the 'iovl' payload parser at every truncated length and with offsets at
// INT32_MIN / INT32_MAX, the clipping and the start-layer search against a brute-force pixel walk on small canvases, and the
// multiply-shift that replaces the division by 255 over its whole range.
//   overlay_plan_check                      runs the checks, prints "overlay plan: ok"
//   overlay_plan_check defined cw ch w h a  prints hm::reference_defined for dx = -(w+1) .. cw+1 (columns), dy = -(h+1) .. ch+1 (rows)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hm_overlay_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); failures++; } } while (0)

static void put(std::vector<uint8_t>& v, uint32_t x, int n) { for (int i = n - 1; i >= 0; i--) v.push_back((uint8_t)(x >> (8 * i))); }

static std::vector<uint8_t> payload(bool wide, uint32_t w, uint32_t h, const std::vector<int32_t>& offs, int version = 0)
{
  std::vector<uint8_t> v;
  v.push_back((uint8_t)version); v.push_back(wide ? 1 : 0);
  put(v, 0x1234, 2); put(v, 0x8000, 2); put(v, 0xFFFF, 2); put(v, 0x00FF, 2);
  put(v, w, wide ? 4 : 2); put(v, h, wide ? 4 : 2);
  for (int32_t o : offs) put(v, (uint32_t)o, wide ? 4 : 2);
  return v;
}

static void check_parser()
{
  for (int wide = 0; wide < 2; wide++) {
    const std::vector<int32_t> offs = wide ? std::vector<int32_t>{INT32_MIN, INT32_MAX, -1, 0, 7, -70000}
                                           : std::vector<int32_t>{-32768, 32767, -1, 0, 7, -300};
    const std::vector<uint8_t> full = payload(wide != 0, wide ? 70000u : 96u, 80u, offs);
    for (size_t n = 0; n <= full.size(); n++) { // every truncated length, in a buffer of exactly that size
      std::vector<uint8_t> cut(full.begin(), full.begin() + n);
      hm::OverlayPayload o;
      std::string err;
      const int rc = hm::parse_overlay_payload(cut.data(), cut.size(), 3, o, err);
      if (n < full.size()) CHECK(rc == 1 && err == "Overlay image data incomplete", "truncated at %zu of %zu: rc %d '%s'", n, full.size(), rc, err.c_str());
      else {
        CHECK(rc == 0, "full payload: rc %d '%s'", rc, err.c_str());
        CHECK(o.width == (wide ? 70000u : 96u) && o.height == 80u, "canvas %u x %u", o.width, o.height);
        CHECK(o.background[0] == 0x1234 && o.background[1] == 0x8000 && o.background[2] == 0xFFFF && o.background[3] == 0x00FF, "background");
        CHECK(o.dx.size() == 3 && o.dy.size() == 3, "offset count");
        for (int i = 0; i < 3 && o.dx.size() == 3; i++) CHECK(o.dx[i] == offs[2 * i] && o.dy[i] == offs[2 * i + 1], "offset %d: %d %d", i, o.dx[i], o.dy[i]);
      }
    }
    // fewer references than the payload holds offsets for: the tail is ignored; none: the header alone
    hm::OverlayPayload o;
    std::string err;
    CHECK(hm::parse_overlay_payload(full.data(), full.size(), 1, o, err) == 0 && o.dx.size() == 1, "one reference");
    CHECK(hm::parse_overlay_payload(full.data(), full.size(), 0, o, err) == 0 && o.dx.empty(), "no reference");
    CHECK(hm::parse_overlay_payload(full.data(), full.size(), 4, o, err) == 1, "more references than offsets");
    CHECK(hm::parse_overlay_payload(full.data(), full.size(), 65535, o, err) == 1, "65535 references");
    std::vector<uint8_t> v1 = payload(wide != 0, 96, 80, offs, 1);
    CHECK(hm::parse_overlay_payload(v1.data(), v1.size(), 3, o, err) == 2 && err == "Overlay image data version 1 is not implemented yet", "version 1: '%s'", err.c_str());
    std::vector<uint8_t> zw = payload(wide != 0, 0, 80, offs), zh = payload(wide != 0, 96, 0, offs);
    CHECK(hm::parse_overlay_payload(zw.data(), zw.size(), 3, o, err) == 1 && err == "Overlay image with zero width or height.", "zero width");
    CHECK(hm::parse_overlay_payload(zh.data(), zh.size(), 3, o, err) == 1, "zero height");
  }
}

static void check_div255()
{
  for (uint32_t v = 0; v <= 65025u; v++) CHECK(hm_div255(v) == v / 255u, "hm_div255(%u) = %u", v, hm_div255(v));
}

struct Layer { int w, h; int32_t dx, dy; bool opaque; };

// brute force: which layers cover canvas pixel (x, y), and the lowest layer a composition has to start at
static void check_plan(int cw, int ch, const std::vector<Layer>& layers)
{
  std::vector<hm_ovl_rect> rects;
  for (const Layer& l : layers) rects.push_back(hm::overlay_clip(cw, ch, l.w, l.h, l.dx, l.dy, l.opaque));
  const int n = (int)layers.size();
  for (int l = 0; l < n; l++) {
    const hm_ovl_rect& r = rects[l];
    bool any = false;
    for (int y = 0; y < ch; y++)
      for (int x = 0; x < cw; x++) {
        const int64_t sx = (int64_t)x - layers[l].dx, sy = (int64_t)y - layers[l].dy;
        const bool covered = sx >= 0 && sx < layers[l].w && sy >= 0 && sy < layers[l].h;
        const bool in_rect = x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1;
        CHECK(covered == in_rect, "layer %d pixel (%d, %d): covered %d, rectangle %d", l, x, y, (int)covered, (int)in_rect);
        if (in_rect) CHECK((int64_t)x - r.x0 + r.sx == sx && (int64_t)y - r.y0 + r.sy == sy, "layer %d pixel (%d, %d): source", l, x, y);
        any = any || covered;
      }
    CHECK(any == hm::overlay_touches(r), "layer %d: touches", l);
  }
  // spans of a few widths (the kernel's is HM_OVL_SPAN; the search does not depend on it)
  for (int span : {1, 3, 4, 256})
    for (int y = 0; y < ch; y++)
      for (int sx0 = 0; sx0 < cw; sx0 += span) {
        const int sx1 = sx0 + span < cw ? sx0 + span : cw;
        int expect = 0;
        for (int l = n - 1; l > 0 && !expect; l--) {
          if (!layers[l].opaque) continue;
          bool all = true;
          for (int x = sx0; x < sx1; x++) {
            const int64_t px = (int64_t)x - layers[l].dx, py = (int64_t)y - layers[l].dy;
            all = all && px >= 0 && px < layers[l].w && py >= 0 && py < layers[l].h;
          }
          if (all) expect = l;
        }
        const int got = hm_ovl_start_layer(rects.data(), n, sx0, sx1, y);
        CHECK(got == expect, "start layer of span [%d, %d) row %d: %d, brute force %d", sx0, sx1, y, got, expect);
      }
}

static void check_plans()
{
  check_plan(7, 6, {});
  check_plan(7, 6, {{5, 3, 0, 0, true}});
  for (int dx = -9; dx <= 8; dx++)
    for (int dy = -9; dy <= 7; dy++) {
      check_plan(7, 6, {{5, 3, dx, dy, true}, {8, 8, dy, dx, false}});
      check_plan(7, 6, {{8, 8, 0, 0, false}, {8, 8, dx, dy, true}, {5, 3, 1, 1, (dx & 1) != 0}, {20, 20, -3, dy, true}});
    }
  // offsets at the ends of int32: no overflow (UndefinedBehaviorSanitizer would stop the program), nothing touches
  for (int32_t d : {INT32_MIN, INT32_MIN + 1, INT32_MAX, INT32_MAX - 1}) {
    check_plan(7, 6, {{5, 3, d, 0, true}, {5, 3, 0, d, false}, {5, 3, d, d, true}});
    const hm_ovl_rect r = hm::overlay_clip(32768, 32768, 32768, 32768, d, d, true);
    CHECK(!hm::overlay_touches(r), "a layer at %d touches", d);
    CHECK(hm::reference_defined(7, 6, 5, 3, d, d, false), "a layer at %d: the reference skips it", d);
  }
  const hm_ovl_rect big = hm::overlay_clip(32768, 32768, 0x7FFFFFFF, 0x7FFFFFFF, INT32_MIN + 5, -1, true);
  CHECK(big.x0 == 0 && big.x1 == 4 && big.y0 == 0 && big.y1 == 32768, "huge layer: %d %d %d %d", big.x0, big.y0, big.x1, big.y1);
  // the crop of a view
  const hm_ovl_rect r = hm::overlay_clip(96, 80, 24, 24, 70, 60, true);
  CHECK(hm::overlay_touches(r, 60, 50, 20, 20) && !hm::overlay_touches(r, 0, 0, 70, 80) && !hm::overlay_touches(r, 0, 0, 96, 60) && hm::overlay_touches(r, 93, 79, 1, 1), "crop");
}

int main(int argc, char** argv)
{
  if (argc == 7 && !std::strcmp(argv[1], "defined")) {
    const int cw = std::atoi(argv[2]), ch = std::atoi(argv[3]), w = std::atoi(argv[4]), h = std::atoi(argv[5]), a = std::atoi(argv[6]);
    for (int dy = -(h + 1); dy <= ch + 1; dy++) {
      for (int dx = -(w + 1); dx <= cw + 1; dx++) std::putchar(hm::reference_defined(cw, ch, w, h, dx, dy, a != 0) ? '1' : '0');
      std::putchar('\n');
    }
    return 0;
  }
  check_parser();
  check_div255();
  check_plans();
  if (failures) { std::printf("overlay plan: %d failures\n", failures); return 1; }
  std::printf("overlay plan: ok\n");
  return 0;
}
