// hm_overlay.h — internal: the launcher of k_overlay (overlay.hip), the composition of an 'iovl' item's layers on the device.
// Not part of the C ABI.
#ifndef HM_OVERLAY_H
#define HM_OVERLAY_H

#include "hm_internal.h"
#include "hm_overlay_plan.h"

enum { HM_OVL_OUT_RGB24 = 0, HM_OVL_OUT_RGBA32 = 1, HM_OVL_OUT_PLANES = 2 };

// one layer that touches the canvas: 8-bit planes on the device, the image Op_YCbCr_to_RGB<uint8_t> is handed (yuv2rgb.cc:79-254)
struct hm_overlay_layer {
  hm_ovl_rect rect;         // clipped placement (hm_overlay_plan.h)
  const void* plane[4];     // Y, Cb, Cr, alpha; Cb = Cr = NULL: monochrome (Cb = Cr = 128); alpha = NULL: opaque.
                            // A composed overlay enters as G, B, R with matrix 0 at full range (the op's copy arm)
  int32_t pitch[4];
  int32_t plane_w[4], plane_h[4]; // samples each plane holds: every read is checked against them before the launch
  int32_t width, height;    // of the layer image
  int32_t chroma;           // HM_CHROMA_*, 0 = monochrome
  int32_t has_nclx, matrix, primaries, full_range;
};

struct hm_overlay_job {
  int32_t width, height;    // canvas
  uint8_t background[3];    // R G B (the 16-bit values of the payload >> 8)
  int32_t out_kind;         // HM_OVL_OUT_*
  void* out[3];             // interleaved pixels in out[0], or R, G, B planes
  int32_t out_pitch;        // bytes; a multiple of 4
};

// Queues the upload of the layer table and k_overlay on `s`.  *pinned / *device: the table's two blocks (pools), the caller's to
// release once the stream has drained.  layers may be NULL with n = 0: the background alone.
int hm_launch_overlay(const hm_overlay_job* job, const hm_overlay_layer* layers, int n, void** pinned, void** device, hipStream_t s);

#endif
