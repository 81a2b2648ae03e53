// hm_overlay_plan.h — derived image items ('iovl'): the payload parser and the placement plan of the layers, pure host code
// (no HIP, no allocation beyond std::vector) so that a stand-alone program can run it under sanitizers
// (tests/host/overlay_plan_check.cpp).  The two functions the kernel needs per span - hm_ovl_start_layer, hm_div255 - are the
// same definitions on both sides (HM_OVL_HD), so what the host test proves holds for the device code.
//
// Reference: ImageOverlay::parse (context.cc:318-369), HeifPixelImage::overlay (pixelimage.cc:1022-1153).
#ifndef HM_OVERLAY_PLAN_H
#define HM_OVERLAY_PLAN_H

#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define HM_OVL_HD __host__ __device__ inline
#else
#define HM_OVL_HD inline
#endif

#define HM_OVL_SPAN 256     // canvas pixels of one row a wave covers
#define HM_OVL_MAX_DEPTH 8  // derived items nested deeper are refused (the reference recurses without a bound)

// the rectangle of one layer on the canvas after clipping, and where its first pixel lies in the layer image.  x1 / y1 exclusive;
// an empty rectangle (x0 >= x1) does not touch the canvas.
struct hm_ovl_rect {
  int32_t x0, y0, x1, y1;
  int32_t sx, sy;   // layer-image coordinate of canvas pixel (x0, y0)
  int32_t opaque;   // the layer has no alpha plane: it replaces what lies below
};

// (in * a + out * (255 - a)) / 255 for in, out, a in 0..255: the numerator is at most 255 * 255 = 65 025.  The truncating quotient
// by multiply and shift; tests/host/overlay_plan_check.cpp compares it with the division over 0 .. 65 025.
HM_OVL_HD uint32_t hm_div255(uint32_t v) { return (v * 0x8081u) >> 23; }

// the highest opaque layer that covers the whole span [sx0, sx1) of row y: nothing below it reaches the result.  0 when there is none.
HM_OVL_HD int hm_ovl_start_layer(const hm_ovl_rect* r, int n, int sx0, int sx1, int y)
{
  for (int l = n - 1; l > 0; l--)
    if (r[l].opaque && r[l].y0 <= y && y < r[l].y1 && r[l].x0 <= sx0 && sx1 <= r[l].x1) return l;
  return 0;
}

namespace hm {

struct OverlayPayload {
  uint16_t background[4] = {0, 0, 0, 0}; // R G B A, 16 bit
  uint32_t width = 0, height = 0;
  std::vector<int32_t> dx, dy;           // one offset per 'dimg' reference
};

// ImageOverlay::parse.  -> 0, 1 = data incomplete / zero size (invalid overlay data), 2 = unsupported version; message in err
inline int parse_overlay_payload(const uint8_t* d, size_t n, size_t num_images, OverlayPayload& o, std::string& err)
{
  if (n < 2 + 4 * 2) { err = "Overlay image data incomplete"; return 1; }
  if (d[0] != 0) { err = "Overlay image data version " + std::to_string((int)d[0]) + " is not implemented yet"; return 2; }
  const size_t field = (d[1] & 1) ? 4 : 2;
  // (num_images comes from the file's iref box: at most 65535 references of 32-bit IDs - no overflow in 64 bits)
  if ((uint64_t)2 + 4 * 2 + 2 * field + (uint64_t)num_images * 2 * field > (uint64_t)n) { err = "Overlay image data incomplete"; return 1; }
  size_t p = 2;
  auto rd = [&](size_t len) { uint32_t v = 0; for (size_t i = 0; i < len; i++) v = (v << 8) | d[p++]; return v; };
  auto rds = [&](size_t len) { const uint32_t v = rd(len); return len == 2 ? (int32_t)(int16_t)(uint16_t)v : (int32_t)v; };
  for (int i = 0; i < 4; i++) o.background[i] = (uint16_t)rd(2);
  o.width = rd(field);
  o.height = rd(field);
  if (o.width == 0 || o.height == 0) { err = "Overlay image with zero width or height."; return 1; }
  o.dx.resize(num_images); o.dy.resize(num_images);
  for (size_t i = 0; i < num_images; i++) { o.dx[i] = rds(field); o.dy[i] = rds(field); }
  return 0;
}

// The layer of size w x h (after its transformations) placed at (dx, dy) on a cw x ch canvas, clipped to the canvas as
// ISO/IEC 23008-12 6.6.2.3 says.  64-bit arithmetic: offsets may be INT32_MIN / INT32_MAX.
inline hm_ovl_rect overlay_clip(int64_t cw, int64_t ch, int64_t w, int64_t h, int32_t dx, int32_t dy, bool opaque)
{
  int64_t x0 = dx, y0 = dy, x1 = (int64_t)dx + w, y1 = (int64_t)dy + h;
  if (x0 < 0) x0 = 0;
  if (y0 < 0) y0 = 0;
  if (x1 > cw) x1 = cw;
  if (y1 > ch) y1 = ch;
  hm_ovl_rect r;
  if (x0 >= x1 || y0 >= y1) { r.x0 = r.y0 = r.x1 = r.y1 = r.sx = r.sy = 0; r.opaque = opaque; return r; }
  r.x0 = (int32_t)x0; r.y0 = (int32_t)y0; r.x1 = (int32_t)x1; r.y1 = (int32_t)y1;
  r.sx = (int32_t)(x0 - dx); r.sy = (int32_t)(y0 - dy);
  r.opaque = opaque ? 1 : 0;
  return r;
}

inline bool overlay_touches(const hm_ovl_rect& r) { return r.x0 < r.x1 && r.y0 < r.y1; }

// ... and whether it touches the rectangle [vx, vx + vw) x [vy, vy + vh) of the canvas (a view's crop)
inline bool overlay_touches(const hm_ovl_rect& r, int64_t vx, int64_t vy, int64_t vw, int64_t vh)
{
  return overlay_touches(r) && r.x0 < vx + vw && vx < r.x1 && r.y0 < vy + vh && vy < r.y1;
}

// Q20: whether HeifPixelImage::overlay (pixelimage.cc:1072-1149) stays inside the planes of both images for this placement.
// Where it does, its result is the clipped composition; where it does not, the reference reads or writes outside and is not
// reproduced.
//   - a layer wholly off the canvas is skipped before any access
//   - dx < 0: the row copy takes canvas-width bytes from column |dx| (the right-border test is always true after in_w -= in_x0):
//     inside exactly when w - |dx| >= cw; with an alpha plane the loop writes out_p[.. + x] for x up to cw + |dx| - 1: never inside
//   - dy < 0: rows |dy| .. ch + |dy| - 1 of the layer are read: inside exactly when h - |dy| >= ch
inline bool reference_defined(int64_t cw, int64_t ch, int64_t w, int64_t h, int32_t dx, int32_t dy, bool has_alpha)
{
  if (dx > 0 && dx >= cw) return true;
  if (dx < 0 && w <= -(int64_t)dx) return true;
  if (dy > 0 && dy >= ch) return true;
  if (dy < 0 && h <= -(int64_t)dy) return true;
  if (dx < 0 && (has_alpha || w + dx < cw)) return false;
  if (dy < 0 && h + dy < ch) return false;
  return true;
}

} // namespace hm
#endif
