// hm_planar.h — planar YCbCr targets (HM_OUT_YCBCR_*): the executor that runs the reference's chain operation by operation
// over device planes (colour_planar.cpp) and the launchers of its kernels (planar.hip).  Internal.
#ifndef HM_PLANAR_H
#define HM_PLANAR_H

#include <vector>

#include "hm_colour_plan.h"
#include "hm_internal.h"

// an image on the device: [0..2] Y / Cb / Cr (R / G / B between Op_YCbCr_to_RGB and Op_RGB_to_YCbCr), [3] alpha or NULL
struct hm_planar_image {
  const void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  int stride[4] = {0, 0, 0, 0};
  int w = 0, h = 0, chroma = 0, bits = 8, alpha_bits = 0;
};

// Runs the chain of d (d->out_format: a planar code; width, height, depth, chroma, nclx, options: the image's) on `src`.
// dst != NULL: the caller's planes of the target's geometry - every plane of the result is written there.  dst == NULL: *res
// names the result's planes wherever they are - planes the chain passes through untouched stay the caller's own (src), the
// others are pool blocks.  Every pool block taken is appended to `temps`: the caller returns them (hm_pool_device_free) once
// the stream has drained.  flags: HM_PLANAR_UNFUSED.
int hm_planar_convert(const hm_colour_desc* d, const hm_planar_image* src, const hm_planar_image* dst, hm_planar_image* res,
                      std::vector<void*>& temps, int flags, hipStream_t s);

// ---- planar.hip ----
// Op_YCbCr444_to_YCbCr420/422_average on both chroma planes (chroma_sampling.cc:77-236, 295-434); w, h: luma size
int hm_launch_average_down(int bits, int v420, const void* cb, int cb_stride, const void* cr, int cr_stride, void* ocb, int ocb_stride,
                           void* ocr, int ocr_stride, int w, int h, hipStream_t s);
// Op_YCbCr_to_RGB ending in planes (yuv2rgb.cc:79-254).  img: the image the op is handed (size, depth, chroma format, nclx,
// strides); coef / mode as hm_launch_colour_float
int hm_launch_ycbcr_to_rgb_planes(const hm_colour_desc* img, const float coef[4], int mode, const void* y, const void* cb, const void* cr,
                                  void* const rgb[3], int rgb_stride, hipStream_t s);
// Op_RGB_to_YCbCr (rgb2yuv.cc:88-275) to target chroma format `chroma` with the target profile (matrix, primaries, full_range).
// ycbcr_src == NULL: src = R, G, B planes of w x h at `bits`.  ycbcr_src != NULL: the fused round trip - src = Y, Cb, Cr of the
// image *ycbcr_src describes, each intermediate R, G, B sample produced by Op_YCbCr_to_RGB in registers (src_coef / src_mode)
struct hm_to_ycbcr {
  int w, h, bits, chroma, matrix, primaries, full_range;
  const void* src[3]; int src_stride[3];
  void* dst[3]; int dst_stride[3];
  const hm_colour_desc* ycbcr_src; float src_coef[4]; int src_mode;
};
int hm_launch_to_ycbcr(const hm_to_ycbcr* a, hipStream_t s);

#endif
