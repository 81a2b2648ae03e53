// hm_plane_geom.h — the plane geometry of this library, stated once: libheif's plane layout, the conformance window of a coded
// picture and the placement of a tile on a grid canvas.  Pure host arithmetic on ints: no HIP header, no allocation, no
// hm_fail - a stand-alone program can include it (tests/host/plane_geom_check.cpp compares every function with the reference's
// formulas written out).  hm_window_w / hm_window_h / hm_pic_of live here, not beside hm_pic: hm_stream.h is the public C description of
// the command stream and stays free of helpers; it is the only header this one needs.
#ifndef HM_PLANE_GEOM_H
#define HM_PLANE_GEOM_H

#include "hm_stream.h"

// ---- the plane layout of HeifPixelImage::ImagePlane::alloc (pixelimage.cc:139-218) ----
// bytes of one sample of `bits` bits
static inline int hm_sample_bytes(int bits) { return bits > 8 ? 2 : 1; }
// the rows a plane of h rows is allocated with: an even count of at least 64
static inline int hm_padded_rows(int h) { const int r = (h + 1) & ~1; return r < 64 ? 64 : r; }
// Size of plane c of a w x h image of `chroma` (0 4:0:0, 1 4:2:0, 2 4:2:2, 3 4:4:4): c == 0 is luma / alpha / mono, c 1 or 2 Cb / Cr.
// A 4:0:0 image has no chroma planes: callers do not ask for c > 0 of chroma 0 (the answer would be that of 4:2:2 / 4:4:4).
static inline int hm_plane_w(int chroma, int c, int w) { return c == 0 || chroma == 3 ? w : (w + 1) / 2; }
static inline int hm_plane_h(int chroma, int c, int h) { return c == 0 || chroma != 1 ? h : (h + 1) / 2; }

// ---- a coded picture: the header at the front of its command stream, and the conformance window the decoder plugin hands
//      libheif as the image (de265_get_image_width / height, decoder_libde265.cc:88-157) ----
static inline const hm_pic* hm_pic_of(const void* blob) { return reinterpret_cast<const hm_pic*>(blob); }
static inline int hm_window_w(const hm_pic& h) { return h.width - h.crop_left - h.crop_right; }
static inline int hm_window_h(const hm_pic& h) { return h.height - h.crop_top - h.crop_bottom; }

// ---- the paste of a tile image at luma position (x0, y0) of a canvas_w x canvas_h canvas, channel by channel
//      (decode_and_paste_tile_image, context.cc:2466-2483): a subsampled channel's canvas size AND its origin round up - the
//      reference's quirk, origin (x0 + 1) / 2 - and a channel whose origin is not inside its canvas refuses the whole tile
//      (the refusal is worded once: hm_tile_origin_refused, batch.cpp) ----
struct hm_tile_place { int chan_w, chan_h, x0, y0; bool inside; }; // the channel's canvas size, the tile's origin in it, whether that lies inside
static inline hm_tile_place hm_place_tile(int chroma, int c, int canvas_w, int canvas_h, int x0, int y0)
{
  hm_tile_place p = {hm_plane_w(chroma, c, canvas_w), hm_plane_h(chroma, c, canvas_h), hm_plane_w(chroma, c, x0), hm_plane_h(chroma, c, y0), false};
  p.inside = p.chan_w > p.x0 && p.chan_h > p.y0;
  return p;
}
// what of a picture extent (a width or a height) is copied from `origin` on into a channel of `chan` samples (origin inside)
static inline int hm_copy_extent(int extent, int chan, int origin) { return extent < chan - origin ? extent : chan - origin; }

#endif
