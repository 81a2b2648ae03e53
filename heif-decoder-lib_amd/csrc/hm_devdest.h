// hm_devdest.h — internal: a caller's device destination (hm_device_dest, include/heif_mi355x.h) resolved for one image.
// devdest.cpp holds the host arithmetic and the checks (no device needed except hm_dest_check_pointer), tensor.hip the kernel.
#ifndef HM_DEVDEST_H
#define HM_DEVDEST_H

#include "hm_internal.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hm_dest_plan {
  int32_t layout, dtype;
  int32_t channels;      // 3 / 4
  int32_t sample_bytes;  // of the out_format: 1 / 2
  int32_t elem;          // bytes per element of the destination
  int32_t raw;           // HWC with the target's own integer type: the bytes as they are (a 2-D device copy, no kernel)
  int64_t row_pitch, plane_pitch, tight_row, bytes;
} hm_dest_plan;

// what does not depend on the image size: the target, layout / dtype combination, alignment of ptr and pitches
int hm_dest_check_static(int out_format, const hm_device_dest* d);
// ... and what does: pitches against the tight values, the byte count (d->len is NOT compared: hm_dest_check_len)
int hm_dest_resolve(int out_format, int w, int h, const hm_device_dest* d, hm_dest_plan* p);
int hm_dest_check_len(const hm_device_dest* d, const hm_dest_plan* p);
// d->ptr is device memory of the current device
int hm_dest_check_pointer(const hm_device_dest* d);
// rows [y0, y0 + rows) of a w x h image from `src` (row 0 of src = image row y0) into the destination; asynchronous on `s`.
// The destination has been checked against w x h.
int hm_dest_write(const hm_device_dest* d, int out_format, int w, int h, int y0, int rows, const void* src, int src_stride, hipStream_t s);

int hm_launch_to_tensor(const hm_dest_plan* p, const void* src, int src_stride, int w, int rows, void* dst, const float scale[4], const float bias[4],
                        hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif
