// devdest.cpp — device-resident output: the arithmetic and the refusals of hm_device_dest, and the step that writes the colour
// stage's interleaved pixels into it (a 2-D device copy for HWC with the target's own integer type, k_to_tensor otherwise).
#include <cstring>

#include "hm_colour_plan.h"
#include "hm_devdest.h"

extern "C" {

int hm_dest_check_static(int out_format, const hm_device_dest* d)
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null device destination");
  if (out_format == 0 || hm_out_is_planar(out_format)) return hm_fail(HM_ERR_UNSUPPORTED, "planar YCbCr output (format %d) is not supported with a device destination", out_format);
  const int obpp = hm_out_bytes_per_pixel(out_format);
  if (obpp < 0) return obpp;
  const int sb = obpp >= 6 ? 2 : 1;
  if (d->layout != HM_DEV_LAYOUT_HWC && d->layout != HM_DEV_LAYOUT_CHW) return hm_fail(HM_ERR_INVALID_ARG, "device destination: unknown layout %d", d->layout);
  if (d->dtype < HM_DEV_U8 || d->dtype > HM_DEV_F32) return hm_fail(HM_ERR_INVALID_ARG, "device destination: unknown dtype %d", d->dtype);
  const bool integer = d->dtype == HM_DEV_U8 || d->dtype == HM_DEV_U16;
  if (integer && d->dtype != (sb == 1 ? HM_DEV_U8 : HM_DEV_U16))
    return hm_fail(HM_ERR_INVALID_ARG, "device destination: integer dtype %d does not match the %d-bit samples of output format %d", d->dtype, sb * 8, out_format);
  const bool raw = integer && d->layout == HM_DEV_LAYOUT_HWC;
  if (!raw && (out_format == HM_OUT_RRGGBB_BE || out_format == HM_OUT_RRGGBBAA_BE))
    return hm_fail(HM_ERR_INVALID_ARG, "device destination: a big-endian target has no sample values for CHW or float output: ask for the _LE format");
  const int elem = d->dtype == HM_DEV_U8 ? 1 : d->dtype == HM_DEV_F32 ? 4 : 2;
  if (d->row_pitch < 0 || d->plane_pitch < 0) return hm_fail(HM_ERR_INVALID_ARG, "device destination: negative pitch");
  if ((uintptr_t)d->ptr % (unsigned)elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: ptr is not a multiple of the element size %d", elem);
  if (d->row_pitch % elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: row_pitch %lld is not a multiple of the element size %d", (long long)d->row_pitch, elem);
  if (d->plane_pitch % elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: plane_pitch %lld is not a multiple of the element size %d", (long long)d->plane_pitch, elem);
  return HM_OK;
}

int hm_dest_resolve(int out_format, int w, int h, const hm_device_dest* d, hm_dest_plan* p)
{
  const int rc = hm_dest_check_static(out_format, d);
  if (rc) return rc;
  if (w <= 0 || h <= 0 || w > 32768 || h > 32768) return hm_fail(HM_ERR_INVALID_ARG, "device destination: image size %d x %d", w, h);
  std::memset(p, 0, sizeof(*p));
  const int obpp = hm_out_bytes_per_pixel(out_format);
  p->layout = d->layout; p->dtype = d->dtype;
  p->sample_bytes = obpp >= 6 ? 2 : 1;
  p->channels = obpp / p->sample_bytes;
  p->elem = d->dtype == HM_DEV_U8 ? 1 : d->dtype == HM_DEV_F32 ? 4 : 2;
  p->raw = d->layout == HM_DEV_LAYOUT_HWC && (d->dtype == HM_DEV_U8 || d->dtype == HM_DEV_U16);
  const bool chw = d->layout == HM_DEV_LAYOUT_CHW;
  p->tight_row = (int64_t)w * p->elem * (chw ? 1 : p->channels);
  p->row_pitch = d->row_pitch ? d->row_pitch : p->tight_row;
  if (p->row_pitch < p->tight_row) return hm_fail(HM_ERR_INVALID_ARG, "device destination: row_pitch %lld below the %lld bytes of a row", (long long)p->row_pitch, (long long)p->tight_row);
  if (p->row_pitch > ((int64_t)1 << 40)) return hm_fail(HM_ERR_INVALID_ARG, "device destination: row_pitch %lld", (long long)p->row_pitch);
  if (chw) {
    const int64_t tight_plane = p->row_pitch * h;
    p->plane_pitch = d->plane_pitch ? d->plane_pitch : tight_plane;
    if (p->plane_pitch < tight_plane) return hm_fail(HM_ERR_INVALID_ARG, "device destination: plane_pitch %lld below the %lld bytes of a plane", (long long)p->plane_pitch, (long long)tight_plane);
    if (p->plane_pitch > ((int64_t)1 << 56)) return hm_fail(HM_ERR_INVALID_ARG, "device destination: plane_pitch %lld", (long long)p->plane_pitch);
    p->bytes = p->plane_pitch * (p->channels - 1) + p->row_pitch * (h - 1) + p->tight_row;
  }
  else p->bytes = p->row_pitch * (h - 1) + p->tight_row;
  return HM_OK;
}

int hm_dest_check_len(const hm_device_dest* d, const hm_dest_plan* p)
{
  if (!d->ptr) return hm_fail(HM_ERR_INVALID_ARG, "device destination: null ptr");
  if (d->len < (uint64_t)p->bytes) return hm_fail(HM_ERR_INVALID_ARG, "device destination: len %llu below the %lld bytes the image needs", (unsigned long long)d->len, (long long)p->bytes);
  return HM_OK;
}

int hm_dest_check_pointer(const hm_device_dest* d)
{
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return hm_fail(HM_ERR_NO_DEVICE, "no current HIP device");
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, d->ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError(); // (an unknown pointer is an answer, not a sticky error)
    return hm_fail(HM_ERR_INVALID_ARG, "device destination: ptr is not memory the HIP runtime knows (host memory?)");
  }
  if (at.type != hipMemoryTypeDevice) return hm_fail(HM_ERR_INVALID_ARG, "device destination: ptr is not device memory (memory type %d)", (int)at.type);
  if (at.device != cur) return hm_fail(HM_ERR_INVALID_ARG, "device destination: ptr belongs to device %d, the decode runs on device %d", at.device, cur);
  return HM_OK;
}

int64_t hm_device_dest_bytes(int out_format, int width, int height, const hm_device_dest* d)
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_device_dest probe = *d;
  probe.ptr = nullptr; // (ptr and len are not looked at)
  hm_dest_plan p;
  const int rc = hm_dest_resolve(out_format, width, height, &probe, &p);
  return rc ? rc : p.bytes;
}

int hm_to_tensor(int out_format, int width, int height, const void* d_src, int src_stride, const hm_device_dest* dest, void* stream)
{
  if (!d_src || !dest) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_dest_plan p;
  int rc = hm_dest_resolve(out_format, width, height, dest, &p);
  if (!rc) rc = hm_dest_check_len(dest, &p);
  if (rc) return rc;
  if (src_stride < width * hm_out_bytes_per_pixel(out_format)) return hm_fail(HM_ERR_INVALID_ARG, "src_stride %d below the bytes of a row", src_stride);
  if (p.sample_bytes == 2 && (((uintptr_t)d_src | (unsigned)src_stride) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  if ((rc = hm_dest_check_pointer(dest))) return rc;
  return hm_dest_write(dest, out_format, width, height, 0, height, d_src, src_stride, (hipStream_t)stream);
}

int hm_dest_write(const hm_device_dest* d, int out_format, int w, int h, int y0, int rows, const void* src, int src_stride, hipStream_t s)
{
  hm_dest_plan p;
  int rc = hm_dest_resolve(out_format, w, h, d, &p);
  if (!rc) rc = hm_dest_check_len(d, &p);
  if (rc) return rc;
  if (y0 < 0 || rows < 0 || y0 + rows > h) return hm_fail(HM_ERR_INTERNAL, "device destination: rows %d..%d of %d", y0, y0 + rows, h);
  uint8_t* dst = (uint8_t*)d->ptr + (int64_t)y0 * p.row_pitch;
  if (p.raw) {
    const hipError_t e = hipMemcpy2DAsync(dst, (size_t)p.row_pitch, src, (size_t)src_stride, (size_t)p.tight_row, (size_t)rows, hipMemcpyDeviceToDevice, s);
    return hm_check_hip(e, "copy to the device destination");
  }
  return hm_launch_to_tensor(&p, src, src_stride, w, rows, dst, d->scale, d->bias, s);
}

} // extern "C"
