// devdest.cpp — device-resident output: the arithmetic and the refusals of hm_device_dest, and the step that writes the colour
// stage's interleaved pixels into it (a 2-D device copy for HWC with the target's own integer type, k_to_tensor otherwise).
// Planar YCbCr (hm_device_planes): the arithmetic and the refusals, and the step that writes the decoded planes (kernel: planes.hip).
// Views (hm_device_view): the refusals, the tap tables and the step that writes a resampled rectangle (kernels: resample.hip).
// Planar views (a view into hm_device_planes): the geometry per plane, the refusals and the write step (kernels: planes_view.hip).
// Light (hm_device_light): the transfer tables and the gamut matrix in double, the refusals and the write step (kernels: light.hip).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "hm_colour_plan.h"
#include "hm_devdest.h"
#include "hm_entry_steps.h"
#include "hm_icc.h"
#include "hm_plane_geom.h"
#include "hm_planes_view.h"
#include "hm_primaries.h"
#include "hm_view_batch.h"
#include "hm_view_multi.h"

extern "C" {

static int dtype_elem(int dtype) { return dtype == HM_DEV_U8 ? 1 : dtype == HM_DEV_F32 ? 4 : 2; }

// w and h in 1 .. 32768; prefix: whose message it is ("device destination: ", "" for the stand-alone entries)
static int check_image_size(const char* prefix, int w, int h)
{
  return w <= 0 || h <= 0 || w > 32768 || h > 32768 ? hm_fail(HM_ERR_INVALID_ARG, "%simage size %d x %d", prefix, w, h) : (int)HM_OK;
}

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
  const int elem = dtype_elem(d->dtype);
  if (d->row_pitch < 0 || d->plane_pitch < 0) return hm_fail(HM_ERR_INVALID_ARG, "device destination: negative pitch");
  if ((uintptr_t)d->ptr % (unsigned)elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: ptr is not a multiple of the element size %d", elem);
  if (d->row_pitch % elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: row_pitch %lld is not a multiple of the element size %d", (long long)d->row_pitch, elem);
  if (d->plane_pitch % elem) return hm_fail(HM_ERR_INVALID_ARG, "device destination: plane_pitch %lld is not a multiple of the element size %d", (long long)d->plane_pitch, elem);
  return HM_OK;
}

int hm_dest_resolve(int out_format, int w, int h, const hm_device_dest* d, hm_dest_plan* p)
{
  int rc = hm_dest_check_static(out_format, d);
  if (rc || (rc = check_image_size("device destination: ", w, h))) return rc;
  std::memset(p, 0, sizeof(*p));
  const int obpp = hm_out_bytes_per_pixel(out_format);
  p->layout = d->layout; p->dtype = d->dtype;
  p->sample_bytes = obpp >= 6 ? 2 : 1;
  p->channels = obpp / p->sample_bytes;
  p->elem = dtype_elem(d->dtype);
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

// `ptr` is device memory of the current device; what: "device destination: ptr", "device planes: plane[1].ptr"
static int check_device_pointer(const void* ptr, const char* what)
{
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return hm_fail(HM_ERR_NO_DEVICE, "no current HIP device");
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError(); // (an unknown pointer is an answer, not a sticky error)
    return hm_fail(HM_ERR_INVALID_ARG, "%s is not memory the HIP runtime knows (host memory?)", what);
  }
  if (at.type != hipMemoryTypeDevice) return hm_fail(HM_ERR_INVALID_ARG, "%s is not device memory (memory type %d)", what, (int)at.type);
  if (at.device != cur) return hm_fail(HM_ERR_INVALID_ARG, "%s belongs to device %d, the decode runs on device %d", what, at.device, cur);
  return HM_OK;
}

int hm_dest_check_pointer(const hm_device_dest* d) { return check_device_pointer(d->ptr, "device destination: ptr"); }

int64_t hm_device_dest_bytes(int out_format, int width, int height, const hm_device_dest* d)
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_device_dest probe = *d;
  probe.ptr = nullptr; // (ptr and len are not looked at)
  hm_dest_plan p;
  const int rc = hm_dest_resolve(out_format, width, height, &probe, &p);
  return rc ? rc : p.bytes;
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

// ---- planar YCbCr (hm_device_planes) --------------------------------------------------------------------------------------------

int hm_planes_check_static(const hm_device_planes* d)
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null device planes");
  if (d->layout != HM_DEV_PLANES_SEPARATE && d->layout != HM_DEV_PLANES_SEMI) return hm_fail(HM_ERR_INVALID_ARG, "device planes: unknown layout %d", d->layout);
  if (d->dtype < HM_DEV_U8 || d->dtype > HM_DEV_F32) return hm_fail(HM_ERR_INVALID_ARG, "device planes: unknown dtype %d", d->dtype);
  if (d->reserved) return hm_fail(HM_ERR_INVALID_ARG, "device planes: reserved is %d, not 0", d->reserved);
  if (d->msb_aligned != 0 && d->msb_aligned != 1) return hm_fail(HM_ERR_INVALID_ARG, "device planes: msb_aligned is %d, not 0 or 1", d->msb_aligned);
  if (d->msb_aligned && d->dtype != HM_DEV_U16) return hm_fail(HM_ERR_INVALID_ARG, "device planes: msb_aligned with dtype %d (HM_DEV_U16 only)", d->dtype);
  if (d->layout == HM_DEV_PLANES_SEMI && (d->plane[2].ptr || d->plane[2].len || d->plane[2].row_pitch))
    return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[2] must be all zero with HM_DEV_PLANES_SEMI (Cb and Cr share plane[1])");
  const int elem = dtype_elem(d->dtype);
  for (int c = 0; c < 4; c++) {
    const hm_device_plane& pl = d->plane[c];
    if (pl.row_pitch < 0) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].row_pitch is negative", c);
    if ((uintptr_t)pl.ptr % (unsigned)elem) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].ptr is not a multiple of the element size %d", c, elem);
    if (pl.row_pitch % elem) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].row_pitch %lld is not a multiple of the element size %d", c, (long long)pl.row_pitch, elem);
  }
  return HM_OK;
}

int hm_planes_resolve(int chroma, int bits, int w, int h, int alpha_bits, const hm_device_planes* d, hm_planes_plan* p)
{
  int rc = hm_planes_check_static(d);
  if (rc) return rc;
  if (chroma < HM_CHROMA_MONO || chroma > HM_CHROMA_444) return hm_fail(HM_ERR_INVALID_ARG, "device planes: chroma format %d", chroma);
  if (bits < 8 || bits > 16) return hm_fail(HM_ERR_INVALID_ARG, "device planes: bit depth %d", bits);
  if (alpha_bits > 0 && (alpha_bits < 8 || alpha_bits > 16)) return hm_fail(HM_ERR_INVALID_ARG, "device planes: alpha bit depth %d", alpha_bits);
  if ((rc = check_image_size("device planes: ", w, h))) return rc;
  std::memset(p, 0, sizeof(*p));
  p->layout = d->layout; p->dtype = d->dtype; p->elem = dtype_elem(d->dtype);
  p->chroma = chroma; p->bits = bits;
  if (d->dtype == HM_DEV_U8 && bits != 8) return hm_fail(HM_ERR_INVALID_ARG, "device planes: dtype HM_DEV_U8 does not hold the %d-bit samples of the result", bits);
  if (d->dtype == HM_DEV_U16 && bits == 8) return hm_fail(HM_ERR_INVALID_ARG, "device planes: dtype HM_DEV_U16 with the 8-bit samples of the result (HM_DEV_U8 holds them)");
  p->shift = d->msb_aligned ? 16 - bits : 0;
  const bool semi = d->layout == HM_DEV_PLANES_SEMI;
  if (chroma == HM_CHROMA_MONO)
    for (int c = 1; c <= 2; c++)
      if (d->plane[c].ptr || d->plane[c].len || d->plane[c].row_pitch) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d] must be all zero for a 4:0:0 result (Y only)", c);
  const bool want_alpha = d->plane[3].ptr != nullptr;
  if (want_alpha && alpha_bits == 0) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[3] is given, but the image has no alpha plane");
  if (want_alpha && alpha_bits > 0 && (d->dtype == HM_DEV_U8 || d->dtype == HM_DEV_U16) && (alpha_bits > 8) != (d->dtype == HM_DEV_U16))
    return hm_fail(HM_ERR_UNSUPPORTED, "device planes: alpha plane of %d bits with integer dtype %d", alpha_bits, d->dtype);
  p->alpha_bits = want_alpha && alpha_bits > 0 ? alpha_bits : 0;
  for (int c = 0; c < 4; c++) {
    auto& pl = p->pl[c];
    // (the alpha plane is sized whether it is written or not: hm_device_planes_bytes reports it)
    pl.present = c == 0 || (c == 3 ? want_alpha : chroma != HM_CHROMA_MONO && !(semi && c == 2));
    if (c != 3 && !pl.present) continue;
    pl.width = hm_plane_w(chroma, c == 3 ? 0 : c, w);
    pl.height = hm_plane_h(chroma, c == 3 ? 0 : c, h);
    pl.elems = semi && c == 1 ? 2 * pl.width : pl.width;
    pl.tight = (int64_t)pl.elems * p->elem;
    pl.pitch = d->plane[c].row_pitch ? d->plane[c].row_pitch : pl.tight;
    if (pl.pitch < pl.tight) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].row_pitch %lld below the %lld bytes of a row", c, (long long)pl.pitch, (long long)pl.tight);
    if (pl.pitch > ((int64_t)1 << 40)) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].row_pitch %lld", c, (long long)pl.pitch);
    pl.bytes = pl.pitch * (pl.height - 1) + pl.tight;
    pl.vec = ((uintptr_t)d->plane[c].ptr % 16) == 0 && (pl.pitch % 16) == 0;
    if (pl.present) p->bytes += pl.bytes;
  }
  return HM_OK;
}

int hm_planes_check_len(const hm_device_planes* d, const hm_planes_plan* p)
{
  for (int c = 0; c < 4; c++) {
    if (!p->pl[c].present) continue;
    if (!d->plane[c].ptr) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].ptr is null", c);
    if (d->plane[c].len < (uint64_t)p->pl[c].bytes)
      return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[%d].len %llu below the %lld bytes the plane needs", c, (unsigned long long)d->plane[c].len, (long long)p->pl[c].bytes);
  }
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++) {
      if (!p->pl[a].present || !p->pl[b].present) continue;
      const uintptr_t a0 = (uintptr_t)d->plane[a].ptr, b0 = (uintptr_t)d->plane[b].ptr;
      if (a0 < b0 + (uint64_t)p->pl[b].bytes && b0 < a0 + (uint64_t)p->pl[a].bytes)
        return hm_fail(HM_ERR_INVALID_ARG, "device planes: the bytes of plane[%d] and plane[%d] overlap", a, b);
    }
  return HM_OK;
}

int hm_planes_check_pointer(const hm_device_planes* d, const hm_planes_plan* p)
{
  for (int c = 0; c < 4; c++) {
    if (!p->pl[c].present) continue;
    char what[48];
    std::snprintf(what, sizeof(what), "device planes: plane[%d].ptr", c);
    const int rc = check_device_pointer(d->plane[c].ptr, what);
    if (rc) return rc;
  }
  return HM_OK;
}

int64_t hm_device_planes_bytes(int chroma, int bits, int width, int height, const hm_device_planes* d, int64_t need[4])
{
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_planes_plan p;
  const int rc = hm_planes_resolve(chroma, bits, width, height, -1, d, &p);
  if (rc) return rc;
  for (int c = 0; c < 4 && need; c++) need[c] = p.pl[c].bytes;
  return p.bytes;
}

int hm_planes_write(const hm_device_planes* d, int chroma, int bits, int w, int h, int alpha_bits, const void* const src[4], const int32_t stride[4],
                    hipStream_t s, int64_t pitches[4])
{
  hm_planes_plan p;
  int rc = hm_planes_resolve(chroma, bits, w, h, alpha_bits, d, &p);
  if (!rc) rc = hm_planes_check_len(d, &p);
  if (!rc) rc = hm_planes_check_pointer(d, &p); // (an entry point may not have known the result's format: the launch relies on none of them)
  if (rc) return rc;
  const bool semi = p.layout == HM_DEV_PLANES_SEMI;
  hm_planes_args a;
  std::memset(&a, 0, sizeof(a));
  int y_end = 0;
  for (int c = 0; c < 4; c++) {
    if (pitches) pitches[c] = p.pl[c].present ? p.pl[c].pitch : 0;
    if (p.pl[c].present) {
      hm_plane_desc& pd = a.pl[c];
      const int sbits = c == 3 ? p.alpha_bits : bits, sb = hm_sample_bytes(sbits);
      const bool pair = semi && c == 1;
      for (int k = c; k <= (pair ? 2 : c); k++) {
        if (!src[k]) return hm_fail(HM_ERR_INVALID_ARG, "device planes: source plane %d is null", k);
        if (stride[k] < p.pl[c].width * sb) return hm_fail(HM_ERR_INVALID_ARG, "device planes: source stride %d of plane %d below the bytes of a row", stride[k], k);
        if (sb == 2 && (((uintptr_t)src[k] | (unsigned)stride[k]) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
      }
      pd.src0 = (const uint8_t*)src[c]; pd.stride0 = stride[c];
      pd.scale0 = d->scale[c]; pd.bias0 = d->bias[c];
      bool vec = p.pl[c].vec && ((uintptr_t)src[c] % 16) == 0 && (stride[c] % 16) == 0;
      if (pair) {
        pd.src1 = (const uint8_t*)src[2]; pd.stride1 = stride[2];
        pd.scale1 = d->scale[2]; pd.bias1 = d->bias[2];
        vec = vec && ((uintptr_t)src[2] % 16) == 0 && (stride[2] % 16) == 0;
      }
      pd.dst = (uint8_t*)d->plane[c].ptr; pd.pitch = p.pl[c].pitch;
      pd.w = p.pl[c].width; pd.h = p.pl[c].height;
      pd.sample_bytes = sb; pd.pair = pair ? 1 : 0; pd.vec = vec ? 1 : 0;
      pd.shift = d->msb_aligned ? 16 - sbits : 0;
      y_end += (pd.h + 3) / 4;
    }
    a.y_end[c] = y_end;
  }
  return hm_launch_planes_to_tensor(&a, p.dtype, s);
}

int hm_planes_to_tensor(int chroma, int bits, int width, int height, int alpha_bits, const void* const d_src[4], const int32_t src_stride[4],
                        const hm_device_planes* planes, void* stream)
{
  if (!d_src || !src_stride || !planes) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (alpha_bits < 0) return hm_fail(HM_ERR_INVALID_ARG, "device planes: alpha bit depth %d", alpha_bits);
  hm_planes_plan p;
  int rc = hm_planes_resolve(chroma, bits, width, height, alpha_bits, planes, &p);
  if (!rc) rc = hm_planes_check_len(planes, &p);
  if (rc) return rc;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  return hm_planes_write(planes, chroma, bits, width, height, alpha_bits, d_src, src_stride, (hipStream_t)stream, nullptr);
}

// ---- views ----------------------------------------------------------------------------------------------------------------------

// the kernel function k of a resampling filter at x (include/heif_mi355x.h), in double, every operation rounded on its own
static double filter_k(int filter, double x)
{
  if (x < 0) x = -x;
  if (filter == HM_VIEW_CUBIC) { // Keys, a = -0.5
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
  }
  if (filter == HM_VIEW_LANCZOS3) {
    if (x == 0.0) return 1.0;
    if (x >= 3.0) return 0.0;
    const double p = 3.14159265358979323846 * x, q = p / 3.0;
    return (std::sin(p) / p) * (std::sin(q) / q);
  }
  const double wi = 1.0 - x; // HM_VIEW_TRIANGLE
  return wi > 0.0 ? wi : 0.0;
}

// the support a of a filter and the strongest reduction n / m it takes: (2 a fs + 1) taps must fit HM_VIEW_MAX_TAPS
enum { HM_VIEW_MAX_TAPS = 2 * 256 + 2 };
static double filter_support(int filter) { return filter == HM_VIEW_CUBIC ? 2.0 : filter == HM_VIEW_LANCZOS3 ? 3.0 : 1.0; }
static int filter_max_reduction(int filter) { return filter == HM_VIEW_CUBIC ? 128 : filter == HM_VIEW_LANCZOS3 ? 85 : 256; }
static const char* filter_name(int filter) { return filter == HM_VIEW_CUBIC ? "HM_VIEW_CUBIC" : filter == HM_VIEW_LANCZOS3 ? "HM_VIEW_LANCZOS3" : "HM_VIEW_TRIANGLE"; }
static bool filter_known(int filter) { return filter == HM_VIEW_TRIANGLE || filter == HM_VIEW_NEAREST || filter == HM_VIEW_CUBIC || filter == HM_VIEW_LANCZOS3; }
static bool filter_resamples(int filter) { return filter != HM_VIEW_NEAREST; }

// the taps of output index j on an axis of n -> m, all in double (the contract of include/heif_mi355x.h): returns their count,
// *first the first source index, w[0 .. count) the normalised weights when w is given (count <= HM_VIEW_MAX_TAPS: check_axis has
// bounded n / m for the filter; a count beyond it is reported, never written)
static int axis_taps(int n, int m, int filter, int j, int* first, float* w)
{
  const double s = (double)n / (double)m, fs = s > 1.0 ? s : 1.0, c = ((double)j + 0.5) * s, r = filter_support(filter) * fs;
  int lo = (int)(c - r + 0.5), hi = (int)(c + r + 0.5);
  if (lo < 0) lo = 0;
  if (hi > n) hi = n;
  *first = lo;
  if (hi - lo > HM_VIEW_MAX_TAPS) return hm_fail(HM_ERR_INTERNAL, "view: %d taps on an axis of %d -> %d (%s)", hi - lo, n, m, filter_name(filter));
  if (!w) return hi - lo;
  double W = 0.0;
  for (int i = lo; i < hi; i++) W += filter_k(filter, ((double)i + 0.5 - c) / fs);
  for (int i = lo; i < hi; i++) w[i - lo] = (float)(filter_k(filter, ((double)i + 0.5 - c) / fs) / W);
  return hi - lo;
}

static int check_axis(int n, int m, int filter, const char* what)
{
  if (n < 1 || n > 32768) return hm_fail(HM_ERR_INVALID_ARG, "view: source %s %d", what, n);
  if (m < 1 || m > 32768) return hm_fail(HM_ERR_INVALID_ARG, "view: output %s %d is not in 1 .. 32768", what, m);
  const int most = filter_max_reduction(filter);
  if ((int64_t)n > (int64_t)most * m) {
    if (most == 256) return hm_fail(HM_ERR_INVALID_ARG, "view: %s %d -> %d is a reduction by more than 256", what, n, m);
    return hm_fail(HM_ERR_INVALID_ARG, "view: %s %d -> %d is a reduction by more than %d, the most %s takes", what, n, m, most, filter_name(filter));
  }
  return HM_OK;
}

int hm_view_filter_taps(int n_in, int n_out, int filter, int j, int32_t* first, float* weights, int cap)
{
  if (!first || (cap > 0 && !weights)) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!filter_known(filter)) return hm_fail(HM_ERR_INVALID_ARG, "view: unknown filter %d", filter);
  const int rc = check_axis(n_in, n_out, filter, "extent");
  if (rc) return rc;
  if (j < 0 || j >= n_out) return hm_fail(HM_ERR_INVALID_ARG, "view: output index %d of %d", j, n_out);
  if (filter == HM_VIEW_NEAREST) {
    *first = j * n_in / n_out;
    if (cap > 0) weights[0] = 1.0f;
    return 1;
  }
  float w[HM_VIEW_MAX_TAPS + 2];
  int f0 = 0;
  const int n = axis_taps(n_in, n_out, filter, j, &f0, w);
  *first = f0;
  for (int i = 0; i < n && i < cap; i++) weights[i] = w[i];
  return n;
}

int hm_view_resolve(int out_format, int src_w, int src_h, const hm_device_view* v, hm_view_plan* vp)
{
  if (!v || !vp) return hm_fail(HM_ERR_INVALID_ARG, "null view");
  std::memset(vp, 0, sizeof(*vp));
  if (!filter_known(v->filter)) return hm_fail(HM_ERR_INVALID_ARG, "view: unknown filter %d", v->filter);
  if (v->crop_w == 0 && v->crop_h == 0) {
    if (v->crop_x || v->crop_y) return hm_fail(HM_ERR_INVALID_ARG, "view: crop origin %d, %d with an empty crop", v->crop_x, v->crop_y);
    vp->x = vp->y = 0; vp->w = src_w; vp->h = src_h;
  }
  else {
    if (v->crop_w <= 0 || v->crop_h <= 0) return hm_fail(HM_ERR_INVALID_ARG, "view: crop extent %d x %d is not positive", v->crop_w, v->crop_h);
    if (v->crop_x < 0 || v->crop_y < 0 || (int64_t)v->crop_x + v->crop_w > src_w || (int64_t)v->crop_y + v->crop_h > src_h)
      return hm_fail(HM_ERR_INVALID_ARG, "view: crop %d x %d at %d, %d is not inside the %d x %d image", v->crop_w, v->crop_h, v->crop_x, v->crop_y, src_w, src_h);
    vp->x = v->crop_x; vp->y = v->crop_y; vp->w = v->crop_w; vp->h = v->crop_h;
  }
  vp->filter = v->filter;
  vp->crop_only = v->out_w == 0 && v->out_h == 0;
  vp->ow = vp->crop_only ? vp->w : v->out_w;
  vp->oh = vp->crop_only ? vp->h : v->out_h;
  int rc;
  if ((rc = check_axis(vp->w, vp->ow, vp->filter, "width")) || (rc = check_axis(vp->h, vp->oh, vp->filter, "height"))) return rc;
  const bool be = out_format == HM_OUT_RRGGBB_BE || out_format == HM_OUT_RRGGBBAA_BE;
  if (be && !vp->crop_only && filter_resamples(vp->filter))
    return hm_fail(HM_ERR_INVALID_ARG, "view: a big-endian target has no sample values to resample: ask for the _LE format");
  return HM_OK;
}

void hm_view_scratch_free(hm_view_scratch* sc)
{
  for (int i = 0; i < 2; i++) { if (sc->dev[i]) hm_pool_device_free(sc->dev[i]); sc->dev[i] = nullptr; }
  if (sc->pinned) hm_pool_pinned_free(sc->pinned);
  sc->pinned = nullptr;
}

// the most taps an output index of an axis of n -> m has (or a negative status)
static int axis_most_taps(int n, int m, int filt)
{
  int most = 0, f0;
  for (int j = 0; j < m; j++) { const int cnt = axis_taps(n, m, filt, j, &f0, nullptr); if (cnt < 0) return cnt; most = std::max(most, cnt); }
  return most;
}
// one axis' table as the kernels read it, m * (2 + taps) words at base: first[m], count[m], weights[taps][m], tap-major
static void fill_axis(int32_t* base, int n, int m, int filt, int taps)
{
  float w[HM_VIEW_MAX_TAPS + 2];
  float* wt = reinterpret_cast<float*>(base + 2 * (size_t)m);
  for (int j = 0; j < m; j++) {
    const int cnt = axis_taps(n, m, filt, j, &base[j], w);
    base[m + j] = cnt;
    for (int i = 0; i < taps; i++) wt[(size_t)i * m + j] = i < cnt ? w[i] : 0.0f;
  }
}

// one axis of n -> m, n <= m, as 16-byte records (hm_gain_tap): the tap rule gives such an axis at most two taps per output index
static int fill_axis_records(hm_gain_tap* rec, int n, int m, int filt)
{
  float w[HM_VIEW_MAX_TAPS + 2];
  for (int j = 0; j < m; j++) {
    int first = 0;
    const int cnt = axis_taps(n, m, filt, j, &first, w);
    if (cnt < 1 || cnt > 2) return hm_fail(HM_ERR_INTERNAL, "gain: %d taps at index %d of a map axis of %d -> %d", cnt, j, n, m);
    rec[j].first = first; rec[j].count = cnt; rec[j].w0 = w[0]; rec[j].w1 = cnt > 1 ? w[1] : 0.0f;
  }
  return HM_OK;
}

// the tap tables of both axes of a resampled view in one pinned block (sc->pinned, `extra` bytes more behind them): first[m],
// count[m], weights[taps][m] per axis, tap-major.  *staged: the horizontal pass may stage its source run in LDS.
static int view_tables(const hm_view_plan* vp, size_t extra, hm_view_scratch* sc, size_t* words_x_out, size_t* words_y_out, int* tx_out, int* ty_out, bool* staged_out)
{
  const int filt = vp->filter;
  const int tx = axis_most_taps(vp->w, vp->ow, filt), ty = axis_most_taps(vp->h, vp->oh, filt);
  if (tx < 0 || ty < 0) return tx < 0 ? tx : ty;
  const size_t words_x = (size_t)vp->ow * (2 + tx), words_y = (size_t)vp->oh * (2 + ty), bytes = (words_x + words_y) * 4;
  int32_t* host = (int32_t*)hm_pool_pinned_alloc(bytes + extra);
  if (!host) return hm_fail(HM_ERR_NOMEM, "out of memory");
  sc->pinned = host;
  fill_axis(host, vp->w, vp->ow, filt, tx);
  fill_axis(host + words_x, vp->h, vp->oh, filt, ty);
  // the staged horizontal pass (k_resample_h_staged) loads the run first[j0] .. first[j63] + count[j63] of a wave's 64 columns: both
  // ends must not fall as j rises, and every window must lie inside the crop
  const bool staged = (filt == HM_VIEW_CUBIC || filt == HM_VIEW_LANCZOS3) && hm_knob(HM_KNOB_VIEW_H_STAGED) != 0;
  if (staged)
    for (int j = 0; j < vp->ow; j++) {
      const int lo = host[j], hi = lo + host[vp->ow + j];
      if (lo < 0 || hi > vp->w || hi <= lo || (j && (lo < host[j - 1] || hi < host[j - 1] + host[vp->ow + j - 1])))
        return hm_fail(HM_ERR_INTERNAL, "view: the windows of columns %d and %d are not in order", j - 1, j);
    }
  *words_x_out = words_x; *words_y_out = words_y; *tx_out = tx; *ty_out = ty; *staged_out = staged;
  return HM_OK;
}

// The arguments of both passes of a resampled view: the view vp of samples of `sample_bytes` bytes (origin: the crop's first sample,
// NULL for a batch), the device tap block `taps` as view_tables lays it out (words_x words of the x axis, then the y axis; tx and ty
// taps) and the destination plan p, which also decides the float32 intermediate: laid out like the destination, its pitch a
// multiple of 16 elements, one plane of vp->h rows per channel for CHW.  tmp stays NULL: the caller sizes it by tmp_plane.
static hm_resample_args resample_args_of(const hm_view_plan* vp, int sample_bytes, const void* origin, int src_stride, const void* taps, size_t words_x, int tx,
                                         int ty, const hm_dest_plan& p)
{
  hm_resample_args a;
  std::memset(&a, 0, sizeof(a));
  a.sample_bytes = sample_bytes; a.channels = p.channels;
  a.src = origin; a.src_stride = src_stride;
  a.n_w = vp->w; a.n_h = vp->h; a.ow = vp->ow; a.oh = vp->oh;
  const int32_t* dx = (const int32_t*)taps;
  const int32_t* dy = dx + words_x;
  a.ax.first = dx; a.ax.count = dx + vp->ow; a.ax.weights = reinterpret_cast<const float*>(dx + 2 * (size_t)vp->ow); a.ax.m = vp->ow; a.ax.taps = tx;
  a.ay.first = dy; a.ay.count = dy + vp->oh; a.ay.weights = reinterpret_cast<const float*>(dy + 2 * (size_t)vp->oh); a.ay.m = vp->oh; a.ay.taps = ty;
  const int64_t E = p.layout == HM_DEV_LAYOUT_CHW ? vp->ow : (int64_t)vp->ow * p.channels;
  a.tmp_pitch = (E + 15) / 16 * 16; a.tmp_plane = a.tmp_pitch * vp->h;
  return a;
}
// ... and the floats of that intermediate for one frame
static size_t resample_tmp_floats(const hm_resample_args& a, const hm_dest_plan& p) { return (size_t)a.tmp_plane * (p.layout == HM_DEV_LAYOUT_CHW ? p.channels : 1); }

// one group of a batched view write: frames idx[0 .. m) of `it` share the plan p, the view and everything else of the key
static int view_write_group(const hm_view_item* it, const int* idx, int m, const hm_dest_plan& p, hipStream_t s, hm_view_scratch* sc)
{
  const hm_view_plan* vp = &it[idx[0]].vp;
  const hm_device_dest* d0 = it[idx[0]].dest;
  const int obpp = p.channels * p.sample_bytes;
  const bool chw = p.layout == HM_DEV_LAYOUT_CHW;
  const int planes = chw ? p.channels : 1;
  size_t words_x = 0, words_y = 0;
  int tx = 0, ty = 0, rc;
  bool staged = false;
  // ONE pinned block and one upload: the tap tables, then the frames' source origins and destinations
  if ((rc = view_tables(vp, 16 + 16 * (size_t)m, sc, &words_x, &words_y, &tx, &ty, &staged))) return rc;
  const hm_view_block lay = hm_view_block_layout((int64_t)words_x, (int64_t)words_y, m);
  uint8_t* host = (uint8_t*)sc->pinned;
  const void** hsrc = reinterpret_cast<const void**>(host + lay.src_off);
  void** hdst = reinterpret_cast<void**>(host + lay.dst_off);
  bool vec = true;
  for (int i = 0; i < m; i++) {
    const hm_view_item& f = it[idx[i]];
    hsrc[i] = (const uint8_t*)f.src + (size_t)vp->y * f.src_stride + (size_t)vp->x * obpp;
    hdst[i] = f.dest->ptr;
    vec = vec && ((uintptr_t)f.dest->ptr % 16) == 0;
  }
  vec = vec && (p.row_pitch % 16) == 0 && (!chw || (p.plane_pitch % 16) == 0);
  if (!(sc->dev[0] = hm_pool_device_alloc((size_t)lay.bytes))) return HM_ERR_NO_DEVICE;
  hm_resample_args a = resample_args_of(vp, p.sample_bytes, nullptr, it[idx[0]].src_stride, sc->dev[0], words_x, tx, ty, p);
  // the intermediate of one chunk of frames, reused chunk after chunk in stream order
  const int64_t frame_stride = (int64_t)resample_tmp_floats(a, p);
  const int64_t bound = hm_knob(HM_KNOB_VIEW_BATCH_BYTES);
  const int per_chunk = (int)std::min<int64_t>(m, hm_view_chunk_frames(vp->ow, vp->h, p.channels, planes, bound));
  if (!(sc->dev[1] = hm_pool_device_alloc((size_t)frame_stride * per_chunk * sizeof(float)))) return HM_ERR_NO_DEVICE;
  if ((rc = hm_check_hip(hipMemcpyAsync(sc->dev[0], host, (size_t)lay.bytes, hipMemcpyHostToDevice, s), "upload of the tap tables"))) return rc;
  a.tmp = (float*)sc->dev[1];
  a.staged = staged ? 1 : 0; a.stage_px = hm_knob(HM_KNOB_VIEW_STAGE_PX);
  const void* const* dsrc = reinterpret_cast<const void* const*>((const uint8_t*)sc->dev[0] + lay.src_off);
  void* const* ddst = reinterpret_cast<void* const*>((uint8_t*)sc->dev[0] + lay.dst_off);
  for (int c0 = 0; c0 < m; c0 += per_chunk) {
    hm_resample_batch b;
    b.srcs = dsrc + c0; b.dsts = ddst + c0;
    b.frames = std::min(per_chunk, m - c0);
    b.vec = vec ? 1 : 0;
    b.frame_stride = frame_stride;
    if ((rc = hm_launch_resample_batch(&p, &a, &b, d0->scale, d0->bias, s))) return rc;
  }
  return HM_OK;
}

int hm_view_write_batch(int out_format, const hm_view_item* it, int n, hipStream_t s, hm_view_scratch* sc)
{
  if (n <= 0) return HM_OK;
  std::vector<hm_dest_plan> plans((size_t)n);
  for (int k = 0; k < n; k++) { // every destination, before anything is queued
    int rc = hm_dest_resolve(out_format, it[k].vp.ow, it[k].vp.oh, it[k].dest, &plans[k]);
    if (!rc) rc = hm_dest_check_len(it[k].dest, &plans[k]);
    if (rc) return rc;
  }
  const bool batched = hm_knob(HM_KNOB_VIEW_BATCH) != 0;
  std::vector<hm_view_batch_key> keys;
  std::vector<std::vector<int>> members;
  for (int k = 0; k < n; k++) {
    const hm_view_plan& vp = it[k].vp;
    if (!batched || vp.crop_only || vp.filter == HM_VIEW_NEAREST) { // what exists, frame by frame
      hm_out_plan one; // the view alone
      std::memset(&one, 0, sizeof(one));
      one.out_format = one.dest_format = out_format; one.has_view = 1; one.vp = vp; one.dp = plans[k];
      const int rc = hm_out_write(it[k].dest, &one, it[k].src, it[k].src_stride, nullptr, s, &sc[k]);
      if (rc) return rc;
      continue;
    }
    const hm_dest_plan& p = plans[k];
    const int32_t crop[4] = {vp.x, vp.y, vp.w, vp.h};
    hm_view_batch_key key;
    hm_view_batch_key_make(&key, crop, vp.ow, vp.oh, vp.filter, p.sample_bytes, p.channels, p.layout, p.dtype, it[k].src_stride, p.row_pitch, p.plane_pitch,
                           (uintptr_t)it[k].dest->ptr, p.layout == HM_DEV_LAYOUT_CHW, it[k].dest->scale, it[k].dest->bias);
    size_t g = 0;
    while (g < keys.size() && !hm_view_batch_key_equal(&keys[g], &key)) g++;
    if (g == keys.size()) { keys.push_back(key); members.emplace_back(); }
    members[g].push_back(k);
  }
  for (const std::vector<int>& m : members) { // (a group's blocks hang on the scratch entry of its first frame: unused otherwise)
    const int rc = view_write_group(it, m.data(), (int)m.size(), plans[(size_t)m[0]], s, &sc[m[0]]);
    if (rc) return rc;
  }
  return HM_OK;
}

// The stand-alone entries return before their kernels have run: the blocks they work on go back to the pools once the stream has
// passed them.  The stream's host function only hands them to this list (no HIP call there); the next call releases them.
namespace {
std::mutex g_done_mu;
std::vector<hm_view_scratch> g_done;
void scratch_done(void* arg)
{
  hm_view_scratch* sc = static_cast<hm_view_scratch*>(arg);
  { std::lock_guard<std::mutex> g(g_done_mu); g_done.push_back(*sc); }
  delete sc;
}
void release_done()
{
  std::vector<hm_view_scratch> v;
  { std::lock_guard<std::mutex> g(g_done_mu); v.swap(g_done); }
  for (hm_view_scratch& sc : v) hm_view_scratch_free(&sc);
}
// `write` on a scratch entry of its own, which follows the stream to release_done
int with_scratch(hipStream_t s, const std::function<int(hm_view_scratch*)>& write)
{
  release_done();
  hm_view_scratch* sc = new (std::nothrow) hm_view_scratch();
  if (!sc) return hm_fail(HM_ERR_NOMEM, "out of memory");
  const int rc = write(sc);
  if (!sc->dev[0] && !sc->dev[1] && !sc->pinned) { delete sc; return rc; }
  if (hipLaunchHostFunc(s, scratch_done, sc) != hipSuccess) { // (never on a healthy runtime: wait, then release here)
    (void)hipGetLastError();
    hipStreamSynchronize(s);
    hm_view_scratch_free(sc);
    delete sc;
  }
  return rc;
}
struct Retired { std::vector<hm_view_scratch> v; };
void retired_done(void* arg)
{
  Retired* r = static_cast<Retired*>(arg);
  { std::lock_guard<std::mutex> g(g_done_mu); g_done.insert(g_done.end(), r->v.begin(), r->v.end()); }
  delete r;
}
} // namespace

// with_scratch for a stand-alone entry outside this file (regions.hip) that works on several entries: the blocks of sc[0 .. n) follow
// the stream to release_done, which this call runs first; the entries are emptied
void hm_view_scratch_retire(hipStream_t s, hm_view_scratch* sc, int n)
{
  release_done();
  Retired* r = new (std::nothrow) Retired();
  for (int i = 0; i < n; i++)
    if (r && (sc[i].dev[0] || sc[i].dev[1] || sc[i].pinned)) r->v.push_back(sc[i]);
  if (r && r->v.empty()) { delete r; return; }
  if (!r || hipLaunchHostFunc(s, retired_done, r) != hipSuccess) { // (never on a healthy runtime: wait, then release here)
    (void)hipGetLastError();
    hipStreamSynchronize(s);
    for (int i = 0; i < n; i++) hm_view_scratch_free(&sc[i]);
    delete r;
    return;
  }
  for (int i = 0; i < n; i++) sc[i] = hm_view_scratch{{nullptr, nullptr}, nullptr};
}

// ---- the light step (hm_device_light) -------------------------------------------------------------------------------------------

namespace {

using hm_light::transfer_known; using hm_light::primaries_known; using hm_light::primaries_to_xyz; using hm_light::invert3; // (hm_primaries.h)

// F_t: the code-to-light function of transfer t at e in [0, 1] (include/heif_mi355x.h), in double
double light_of_code(int t, double e)
{
  switch (t) {
    case 1: case 6: case 14: case 15: { // BT.709, with the constants that make the two pieces meet
      const double alpha = 1.09929682680944, beta = 0.018053968510807;
      return e < 4.5 * beta ? e / 4.5 : std::pow((e + (alpha - 1.0)) / alpha, 1.0 / 0.45);
    }
    case 4: return std::pow(e, 2.2);
    case 5: return std::pow(e, 2.8);
    case 13: return e <= 0.04045 ? e / 12.92 : std::pow((e + 0.055) / 1.055, 2.4);
    case 16: { // SMPTE ST 2084 EOTF, 1.0 = 10000 cd/m2
      const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
      const double p = std::pow(e, 1.0 / m2), num = p - c1 > 0.0 ? p - c1 : 0.0;
      return std::pow(num / (c2 - c3 * p), 1.0 / m1);
    }
    case 18: { // BT.2100 HLG: the inverse OETF (scene light, no OOTF)
      const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * std::log(4.0 * a);
      return e <= 0.5 ? e * e / 3.0 : (std::exp((e - c) / a) + b) / 12.0;
    }
    default: return e; // 8: linear
  }
}

void fill_light_table(int transfer, int bits, double g, bool encode, float* out)
{
  const int n = 1 << bits;
  const double peak = (double)(n - 1);
  if (!encode) { for (int c = 0; c < n; c++) out[c] = (float)(g * light_of_code(transfer, (double)c / peak)); return; }
  out[0] = 0.0f; // (never looked at: the count runs over c = 1 .. peak)
  for (int c = 1; c < n; c++) out[c] = (float)(g * light_of_code(transfer, ((double)c - 0.5) / peak));
}

} // namespace

int hm_light_table(int transfer, int bits, float gain, int encode, float* out)
{
  if (!out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!transfer_known(transfer)) return hm_fail(HM_ERR_UNSUPPORTED, "light: transfer characteristics %d are not supported", transfer);
  if (bits < 8 || bits > HM_LIGHT_MAX_BITS) return hm_fail(HM_ERR_UNSUPPORTED, "light: samples of %d bits (8 .. %d are supported)", bits, (int)HM_LIGHT_MAX_BITS);
  if (!std::isfinite(gain) || !(gain > 0.0f)) return hm_fail(HM_ERR_INVALID_ARG, "light: gain %g is not finite and above 0", (double)gain);
  fill_light_table(transfer, bits, (double)gain, encode != 0, out);
  return 1 << bits;
}

int hm_light_matrix(int from_primaries, int to_primaries, float m[9])
{
  if (!m) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!primaries_known(from_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", from_primaries);
  if (!primaries_known(to_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", to_primaries);
  if (from_primaries == to_primaries) {
    for (int i = 0; i < 9; i++) m[i] = i % 4 == 0 ? 1.0f : 0.0f;
    return HM_OK;
  }
  double A[9], B[9], Bi[9];
  primaries_to_xyz(from_primaries, A);
  primaries_to_xyz(to_primaries, B);
  invert3(B, Bi);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) m[3 * r + c] = (float)(Bi[3 * r] * A[c] + Bi[3 * r + 1] * A[3 + c] + Bi[3 * r + 2] * A[6 + c]);
  return HM_OK;
}

// dest_format: the target the destination is judged by (hm_out_dest_format)
static int light_check(int out_format, int dest_format, const hm_device_dest* d, const hm_out_steps* st, int explicit_from)
{
  const hm_device_light* l = st->light;
  if (!l) return hm_fail(HM_ERR_INVALID_ARG, "null light step");
  int rc = hm_dest_check_static(dest_format, d);
  if (rc) return rc;
  if (l->reserved[0] || l->reserved[1] || l->reserved[2]) return hm_fail(HM_ERR_INVALID_ARG, "light: reserved is not 0");
  if (!std::isfinite(l->gain) || !(l->gain > 0.0f)) return hm_fail(HM_ERR_INVALID_ARG, "light: gain %g is not finite and above 0", (double)l->gain);
  if (explicit_from && (l->from_transfer == 0 || l->from_primaries == 0))
    return hm_fail(HM_ERR_INVALID_ARG, "light: from_transfer and from_primaries must be given: the pixels carry no profile");
  const bool from_icc = hm_light_from_icc(l);
  if (const int rc = hm_entry_icc(*st, nullptr)) return rc; // (the sentinel in one field only)
  if (from_icc && !st->icc) return hm_fail(HM_ERR_UNSUPPORTED, "light: HM_LIGHT_FROM_ICC without a profile to read");
  if (!from_icc && l->from_transfer != 0 && !transfer_known(l->from_transfer)) return hm_fail(HM_ERR_UNSUPPORTED, "light: transfer characteristics %d are not supported", l->from_transfer);
  if (!transfer_known(l->to_transfer)) return hm_fail(HM_ERR_UNSUPPORTED, "light: transfer characteristics %d are not supported", l->to_transfer);
  if (!from_icc && l->from_primaries != 0 && !primaries_known(l->from_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", l->from_primaries);
  if (l->to_primaries != 0 && !primaries_known(l->to_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", l->to_primaries);
  if (out_format == HM_OUT_RRGGBB_BE || out_format == HM_OUT_RRGGBBAA_BE)
    return hm_fail(HM_ERR_INVALID_ARG, "light: a big-endian target has no sample values to look up: ask for the _LE format");
  if (l->to_transfer == HM_LIGHT_LINEAR && (d->dtype == HM_DEV_U8 || d->dtype == HM_DEV_U16))
    return hm_fail(HM_ERR_INVALID_ARG, "light: linear light needs a float dtype (integer dtype %d)", d->dtype);
  return HM_OK;
}

// the plan of a light step whose static checks have passed (light_check)
// icc, icc_size: the request's profile (hm_out_steps), read when l carries HM_LIGHT_FROM_ICC
static int light_plan_of(int out_format, int bits, int img_transfer, int img_primaries, const hm_device_light* l, const uint8_t* icc, size_t icc_size, hm_light_plan* lp)
{
  std::memset(lp, 0, sizeof(*lp));
  lp->from_transfer = l->from_transfer ? l->from_transfer : img_transfer;
  lp->from_primaries = l->from_primaries ? l->from_primaries : img_primaries;
  hm_icc::Profile prof;
  if (hm_light_from_icc(l)) {
    if (!icc) return hm_fail(HM_ERR_UNSUPPORTED, "light: HM_LIGHT_FROM_ICC without a profile to read");
    const int rc = hm_icc::parse(icc, icc_size, &prof);
    if (rc) return rc;
    if (prof.cicp_known) { lp->from_primaries = prof.cicp[0]; lp->from_transfer = prof.cicp[1]; } // the cicp tag stands for the profile: the path of the codes, unchanged
    else { lp->icc = 1; lp->icc_data = icc; lp->icc_size = icc_size; }
  }
  if (lp->icc) {
    lp->to_transfer = l->to_transfer;
    lp->to_primaries = l->to_primaries; // (0: the profile's own primaries, which have no code)
    const int sb = hm_out_bytes_per_pixel(out_format) >= 6 ? 2 : 1;
    if (sb == 1) bits = 8;
    if (bits < 8 || bits > HM_LIGHT_MAX_BITS) return hm_fail(HM_ERR_UNSUPPORTED, "light: samples of %d bits (8 .. %d are supported)", bits, (int)HM_LIGHT_MAX_BITS);
    lp->bits = bits; lp->enc_bits = bits;
    lp->encode = lp->to_transfer != HM_LIGHT_LINEAR;
    lp->gain = l->gain;
    if (!prof.same_curves) { // three tables only where they differ at this depth
      std::vector<float> t((size_t)3 << bits);
      for (int c = 0; c < 3; c++) hm_icc::fill_table(prof.curve[c], bits, (double)l->gain, t.data() + ((size_t)c << bits));
      const size_t n = (size_t)sizeof(float) << bits;
      lp->lin3 = std::memcmp(t.data(), t.data() + ((size_t)1 << bits), n) != 0 || std::memcmp(t.data(), t.data() + ((size_t)2 << bits), n) != 0;
    }
    lp->matrix = lp->to_primaries != 0;
    if (lp->matrix) hm_icc::matrix_to(prof, lp->to_primaries, lp->m);
    return HM_OK;
  }
  if (!transfer_known(lp->from_transfer)) return hm_fail(HM_ERR_UNSUPPORTED, "light: the image's transfer characteristics %d are not supported", lp->from_transfer);
  if (!primaries_known(lp->from_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: the image's colour primaries %d are not supported", lp->from_primaries);
  lp->to_transfer = l->to_transfer;
  lp->to_primaries = l->to_primaries ? l->to_primaries : lp->from_primaries;
  const int sb = hm_out_bytes_per_pixel(out_format) >= 6 ? 2 : 1;
  if (sb == 1) bits = 8;
  if (bits < 8 || bits > HM_LIGHT_MAX_BITS) return hm_fail(HM_ERR_UNSUPPORTED, "light: samples of %d bits (8 .. %d are supported)", bits, (int)HM_LIGHT_MAX_BITS);
  lp->bits = bits;
  lp->enc_bits = bits;
  lp->encode = lp->to_transfer != HM_LIGHT_LINEAR;
  lp->matrix = lp->to_primaries != lp->from_primaries;
  lp->gain = l->gain;
  return hm_light_matrix(lp->from_primaries, lp->to_primaries, lp->m);
}

// ---- the tone step (hm_device_tone) ----------------------------------------------------------------------------------------------

namespace {

// the inverse of light_of_code(16, .): ST 2084, y = 1.0 at 10000 cd/m2
double pq_of_light(double y)
{
  const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
  const double p = std::pow(y, m1);
  return std::pow((c1 + c2 * p) / (1.0 + c3 * p), m2);
}

bool nits_ok(float v) { return std::isfinite(v) && v > 0.0f && v <= 10000.0f; }

// KS of the curve src -> dst (cd/m2): the knee start in units of the source's PQ peak
double tone_knee(double src_peak, double dst_peak) { return 1.5 * (pq_of_light(dst_peak / 10000.0) / pq_of_light(src_peak / 10000.0)) - 0.5; }

// thr[HM_TONE_STEPS], then sg[HM_TONE_STEPS] (include/heif_mi355x.h); every argument resolved
void fill_tone_tables(double g, double src_peak, double dst_peak, double U, double Uo, float* thr, float* sg)
{
  const int n = HM_TONE_STEPS;
  const double top = (double)(n - 1);
  if (thr) {
    thr[0] = 0.0f;
    for (int i = 1; i < n; i++) thr[i] = (float)(g * (10000.0 / U) * light_of_code(16, ((double)i - 0.5) / top));
  }
  if (!sg) return;
  const double Pw = pq_of_light(src_peak / 10000.0), maxLum = pq_of_light(dst_peak / 10000.0) / Pw, KS = 1.5 * maxLum - 0.5;
  for (int k = 0; k < n; k++) {
    const double e = (double)k / top, E1 = std::min(e / Pw, 1.0);
    double ratio = 1.0;
    if (!(maxLum >= 1.0 || E1 < KS || k == 0)) {
      const double T = (E1 - KS) / (1.0 - KS), T2 = T * T, T3 = T2 * T;
      const double E2 = (2.0 * T3 - 3.0 * T2 + 1.0) * KS + (T3 - 2.0 * T2 + T) * (1.0 - KS) + (-2.0 * T3 + 3.0 * T2) * maxLum;
      ratio = light_of_code(16, E2 * Pw) / light_of_code(16, e);
    }
    sg[k] = (float)(ratio * U / Uo);
  }
}

// the tone step's own refusals; defaults: src_peak and unit_nits may be 0 (resolved against the image later)
int tone_check(const hm_device_tone* t, bool defaults)
{
  if (t->curve != HM_TONE_BT2390) return hm_fail(HM_ERR_INVALID_ARG, "tone: unknown curve %d", t->curve);
  if (t->reserved[0] || t->reserved[1]) return hm_fail(HM_ERR_INVALID_ARG, "tone: reserved is not 0");
  if (!(defaults && t->src_peak == 0.0f) && !nits_ok(t->src_peak))
    return hm_fail(HM_ERR_INVALID_ARG, "tone: src_peak %g is not finite, above 0 and at most 10000", (double)t->src_peak);
  if (!nits_ok(t->dst_peak)) return hm_fail(HM_ERR_INVALID_ARG, "tone: dst_peak %g is not finite, above 0 and at most 10000", (double)t->dst_peak);
  if (!(defaults && t->unit_nits == 0.0f) && !nits_ok(t->unit_nits))
    return hm_fail(HM_ERR_INVALID_ARG, "tone: unit_nits %g is not finite, above 0 and at most 10000", (double)t->unit_nits);
  if (t->out_unit_nits != 0.0f && !nits_ok(t->out_unit_nits))
    return hm_fail(HM_ERR_INVALID_ARG, "tone: out_unit_nits %g is not finite, above 0 and at most 10000", (double)t->out_unit_nits);
  if (t->src_peak != 0.0f && tone_knee(t->src_peak, t->dst_peak) < 0.0)
    return hm_fail(HM_ERR_INVALID_ARG, "tone: the knee of %g -> %g cd/m2 lies below black (KS < 0)", (double)t->src_peak, (double)t->dst_peak);
  if (t->out_bits != 0 && t->out_bits != 8) return hm_fail(HM_ERR_INVALID_ARG, "tone: out_bits %d is not 0 or 8", t->out_bits);
  return HM_OK;
}

} // namespace

// the target the destination is judged by under a tone step (may be NULL): the 8-bit finish writes the 8-bit sibling
static int tone_dest_format(int out_format, const hm_device_tone* tone)
{
  if (tone && tone->out_bits == 8 && (out_format == HM_OUT_RRGGBB_LE || out_format == HM_OUT_RRGGBB_BE)) return HM_OUT_RGB;
  return out_format;
}

float hm_tone_peak_of(int has_clli, unsigned max_cll, int has_mdcv, unsigned mdcv_max)
{
  if (has_clli && max_cll != 0) return (float)std::min(max_cll, 10000u); // (the field is 16 bits wide; PQ codes no light above 10000 cd/m2)
  if (has_mdcv && mdcv_max >= 50000u && mdcv_max <= 100000000u) return (float)((double)mdcv_max * 0.0001);
  return 1000.0f;
}

// what light value 1.0 (before gain) stands for under the plan lp, cd/m2: as given, or what 0 stands for - behind an OOTF step (resolved
// into lp already) light value g stands for display_peak; PQ says 10000 - or the refusal; who: the step that asks, for the message
static int unit_nits_of(const char* who, const hm_light_plan* lp, float given, float* U)
{
  const float unit_nits = given != 0.0f ? given : lp->ootf ? lp->ootf_peak : 0.0f;
  if (unit_nits == 0.0f && lp->icc) return hm_fail(HM_ERR_INVALID_ARG, "%s: unit_nits must be given for an ICC profile as the source (no profile says what 1.0 stands for)", who);
  if (unit_nits == 0.0f && lp->from_transfer != 16)
    return hm_fail(HM_ERR_INVALID_ARG, "%s: unit_nits must be given for transfer characteristics %d (only PQ says what 1.0 stands for)", who, lp->from_transfer);
  *U = unit_nits != 0.0f ? unit_nits : 10000.0f;
  return HM_OK;
}

// the tone step into the plan of its light step (light_plan_of); the static checks have passed
static int tone_plan_of(const hm_device_tone* tone, hm_light_plan* lp)
{
  // behind an OOTF step nothing brighter than display_peak comes out of it
  const float src_peak = tone->src_peak != 0.0f ? tone->src_peak : lp->ootf ? lp->ootf_peak : 0.0f;
  float unit_nits;
  const int rc = unit_nits_of("tone", lp, tone->unit_nits, &unit_nits);
  if (rc) return rc;
  if (src_peak == 0.0f) return hm_fail(HM_ERR_INVALID_ARG, "tone: src_peak must be given: the pixels carry no light levels"); // (else the knee has been judged)
  lp->tone = 1;
  if (tone->out_bits == 8) lp->enc_bits = 8;
  lp->src_peak = src_peak; lp->dst_peak = tone->dst_peak;
  lp->unit_nits = unit_nits;
  lp->out_unit_nits = tone->out_unit_nits != 0.0f ? tone->out_unit_nits : tone->dst_peak;
  return HM_OK;
}

int hm_tone_table(const hm_device_tone* tone, float gain, int which, float* out)
{
  if (!tone || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (which != 0 && which != 1) return hm_fail(HM_ERR_INVALID_ARG, "tone: table %d is not 0 (thr) or 1 (sg)", which);
  if (!std::isfinite(gain) || !(gain > 0.0f)) return hm_fail(HM_ERR_INVALID_ARG, "light: gain %g is not finite and above 0", (double)gain);
  const int rc = tone_check(tone, false);
  if (rc) return rc;
  if (tone->out_unit_nits == 0.0f) return hm_fail(HM_ERR_INVALID_ARG, "tone: out_unit_nits must be given");
  fill_tone_tables((double)gain, tone->src_peak, tone->dst_peak, tone->unit_nits, tone->out_unit_nits, which ? nullptr : out, which ? out : nullptr);
  return HM_TONE_STEPS;
}

// ---- the OOTF step (hm_device_ootf) ----------------------------------------------------------------------------------------------

namespace {

// the system gamma of BT.2100 Table 5 for a display peak L (cd/m2): note 5e inside 400 .. 2000, note 5f outside; gamma != 0: as given
double ootf_gamma_of(double L, double gamma)
{
  if (gamma != 0.0) return gamma;
  if (L >= 400.0 && L <= 2000.0) return 1.2 + 0.42 * std::log10(L / 1000.0);
  return 1.2 * std::pow(1.111, std::log2(L / 1000.0));
}

// thr[HM_OOTF_STEPS], then sg[HM_OOTF_STEPS] (include/heif_mi355x.h); gamma resolved
void fill_ootf_tables(double g, double gamma, float* thr, float* sg)
{
  const int n = HM_OOTF_STEPS;
  const double top = (double)(n - 1);
  if (thr) {
    thr[0] = 0.0f;
    for (int i = 1; i < n; i++) thr[i] = (float)(g * light_of_code(18, ((double)i - 0.5) / top));
  }
  if (!sg) return;
  for (int k = 1; k < n; k++) sg[k] = (float)std::pow(light_of_code(18, (double)k / top), gamma - 1.0);
  sg[0] = sg[1];
}

// the step's own refusals
int ootf_check(const hm_device_ootf* o)
{
  if (o->kind != HM_OOTF_HLG) return hm_fail(HM_ERR_INVALID_ARG, "ootf: unknown kind %d", o->kind);
  for (int i = 0; i < 5; i++)
    if (o->reserved[i]) return hm_fail(HM_ERR_INVALID_ARG, "ootf: reserved is not 0");
  if (!nits_ok(o->display_peak)) return hm_fail(HM_ERR_INVALID_ARG, "ootf: display_peak %g is not finite, above 0 and at most 10000", (double)o->display_peak);
  if (!std::isfinite(o->gamma) || o->gamma < 0.0f) return hm_fail(HM_ERR_INVALID_ARG, "ootf: gamma %g is not finite and 0 or above", (double)o->gamma);
  return HM_OK;
}

// ... and those of the request around it
int ootf_check_request(const hm_out_steps* st)
{
  const hm_device_ootf* o = st->ootf;
  const hm_device_light* l = st->light;
  if (!l) return hm_fail(HM_ERR_INVALID_ARG, "ootf: null light step");
  const int rc = ootf_check(o);
  if (rc) return rc;
  if (l->from_transfer == HM_LIGHT_FROM_ICC || l->from_primaries == HM_LIGHT_FROM_ICC)
    return hm_fail(HM_ERR_UNSUPPORTED, "ootf: HM_LIGHT_FROM_ICC beside the OOTF step (it renders HLG scene light, which no matrix/TRC profile describes)");
  if (st->gain) return hm_fail(HM_ERR_UNSUPPORTED, "ootf: a gain step beside the OOTF step is not supported (a gain map's base is SDR)");
  if (st->alpha && st->alpha->mode == HM_ALPHA_PREMULTIPLIED)
    return hm_fail(HM_ERR_INVALID_ARG, "ootf: HM_ALPHA_PREMULTIPLIED beside the OOTF step (the luminance of premultiplied light is not the scene's)");
  if (l->from_transfer != 0 && l->from_transfer != 18)
    return hm_fail(HM_ERR_INVALID_ARG, "ootf: from_transfer %d is not 18 (the OOTF of BT.2100 renders HLG scene light)", l->from_transfer);
  if (l->to_transfer == 18)
    return hm_fail(HM_ERR_INVALID_ARG, "ootf: to_transfer 18 (display light through the OETF alone is no HLG signal; the inverse OOTF is out of scope)");
  if (st->tone && st->tone->src_peak == 0.0f && nits_ok(st->tone->dst_peak) && tone_knee(o->display_peak, st->tone->dst_peak) < 0.0) // (src_peak 0: display_peak)
    return hm_fail(HM_ERR_INVALID_ARG, "tone: the knee of %g -> %g cd/m2 lies below black (KS < 0)", (double)o->display_peak, (double)st->tone->dst_peak);
  return HM_OK;
}

} // namespace

int hm_ootf_gamma(const hm_device_ootf* ootf, double* gamma)
{
  if (!ootf || !gamma) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const int rc = ootf_check(ootf);
  if (rc) return rc;
  *gamma = ootf_gamma_of((double)ootf->display_peak, (double)ootf->gamma);
  return HM_OK;
}

int hm_ootf_table(const hm_device_ootf* ootf, float gain, int which, float* out)
{
  if (!ootf || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (which != 0 && which != 1) return hm_fail(HM_ERR_INVALID_ARG, "ootf: table %d is not 0 (thr) or 1 (sg)", which);
  if (!std::isfinite(gain) || !(gain > 0.0f)) return hm_fail(HM_ERR_INVALID_ARG, "light: gain %g is not finite and above 0", (double)gain);
  const int rc = ootf_check(ootf);
  if (rc) return rc;
  fill_ootf_tables((double)gain, ootf_gamma_of((double)ootf->display_peak, (double)ootf->gamma), which ? nullptr : out, which ? out : nullptr);
  return HM_OOTF_STEPS;
}

int hm_ootf_luma(int primaries, float out[3])
{
  if (!out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  double M[9];
  if (!primaries_to_xyz(primaries, M)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", primaries);
  for (int c = 0; c < 3; c++) out[c] = (float)M[3 + c];
  return HM_OK;
}

// the OOTF step into the plan of its light step (light_plan_of); the static checks have passed
static int ootf_plan_of(const hm_device_ootf* o, hm_light_plan* lp)
{
  if (lp->from_transfer != 18)
    return hm_fail(HM_ERR_INVALID_ARG, "ootf: the image's from_transfer %d is not 18 (the OOTF of BT.2100 renders HLG scene light)", lp->from_transfer);
  lp->ootf = 1;
  lp->ootf_peak = o->display_peak; lp->ootf_gamma = o->gamma;
  return hm_ootf_luma(lp->from_primaries, lp->y);
}

namespace {

// the tables a light plan's kernels read, one behind the other: lin (three of them under lp->lin3), then enc, then thr and sg of the tone step, then thr and sg of
// the OOTF step (hm_out_write; the plan may be NULL - no light step, no tables)
struct LightTables {
  const hm_light_plan* lp;
  size_t n, ne, nt, no;
  explicit LightTables(const hm_light_plan* plan)
    : lp(plan), n(plan ? (size_t)(plan->lin3 ? 3 : 1) << plan->bits : 0), ne(plan && plan->encode ? (size_t)1 << plan->enc_bits : 0), nt(plan && plan->tone ? 2 * (size_t)HM_TONE_STEPS : 0),
      no(plan && plan->ootf ? 2 * (size_t)HM_OOTF_STEPS : 0) {}
  size_t bytes() const { return (n + ne + nt + no) * sizeof(float); }
  void fill(float* host) const
  {
    if (!lp) return;
    if (lp->icc) { // (parsed when the plan was made: it parses again)
      hm_icc::Profile prof;
      if (hm_icc::parse(lp->icc_data, lp->icc_size, &prof)) return;
      for (int c = 0; c < (lp->lin3 ? 3 : 1); c++) hm_icc::fill_table(prof.curve[c], lp->bits, (double)lp->gain, host + ((size_t)c << lp->bits));
    }
    else fill_light_table(lp->from_transfer, lp->bits, (double)lp->gain, false, host);
    if (lp->encode) fill_light_table(lp->to_transfer, lp->enc_bits, (double)lp->gain, true, host + n);
    if (lp->tone) fill_tone_tables((double)lp->gain, lp->src_peak, lp->dst_peak, lp->unit_nits, lp->out_unit_nits, host + n + ne, host + n + ne + HM_TONE_STEPS);
    if (lp->ootf) fill_ootf_tables((double)lp->gain, ootf_gamma_of((double)lp->ootf_peak, (double)lp->ootf_gamma), host + n + ne + nt, host + n + ne + nt + HM_OOTF_STEPS);
  }
  // the kernels' arguments, the table pointers still NULL ...
  hm_light_args args(int src_bytes) const
  {
    hm_light_args la;
    std::memset(&la, 0, sizeof(la));
    la.src_bytes = src_bytes;
    if (!lp) return la;
    la.bits = lp->bits; la.enc_bits = lp->enc_bits; la.src_bytes = src_bytes; la.encode = lp->encode; la.matrix = lp->matrix; la.lin3 = lp->lin3;
    std::memcpy(la.m, lp->m, sizeof(la.m));
    std::memcpy(la.y, lp->y, sizeof(la.y));
    return la;
  }
  // ... and pointed at the device copy of what fill wrote
  void point(hm_light_args* la, const float* dev) const
  {
    if (!lp) return;
    la->lin = dev; la->enc = lp->encode ? dev + n : nullptr; la->tone = lp->tone ? dev + n + ne : nullptr; la->ootf = lp->ootf ? dev + n + ne + nt : nullptr;
  }
};

} // namespace

// ---- the alpha step (hm_device_alpha) --------------------------------------------------------------------------------------------

int hm_alpha_dest_format(int out_format, const hm_device_alpha* a, const hm_device_tone* tone)
{
  if (!a) return hm_fail(HM_ERR_INVALID_ARG, "null alpha step");
  if (a->mode != HM_ALPHA_STRAIGHT && a->mode != HM_ALPHA_PREMULTIPLIED && a->mode != HM_ALPHA_MATTE) return hm_fail(HM_ERR_INVALID_ARG, "alpha: unknown mode %d", a->mode);
  if (a->reserved[0] || a->reserved[1] || a->reserved[2]) return hm_fail(HM_ERR_INVALID_ARG, "alpha: reserved is not 0");
  const bool matte = a->mode == HM_ALPHA_MATTE;
  if (!matte && (a->background[0] || a->background[1] || a->background[2])) return hm_fail(HM_ERR_INVALID_ARG, "alpha: a background outside HM_ALPHA_MATTE");
  if (a->background[3]) return hm_fail(HM_ERR_INVALID_ARG, "alpha: background[3] is %d, not 0", (int)a->background[3]);
  if (out_format == 0 || hm_out_is_planar(out_format)) return hm_fail(HM_ERR_UNSUPPORTED, "planar YCbCr output (format %d) is not supported with a device destination", out_format);
  const int obpp = hm_out_bytes_per_pixel(out_format);
  if (obpp < 0) return obpp;
  if (out_format == HM_OUT_RRGGBB_BE || out_format == HM_OUT_RRGGBBAA_BE)
    return hm_fail(HM_ERR_INVALID_ARG, "alpha: a big-endian target has no sample values to multiply: ask for the _LE format");
  if (out_format != HM_OUT_RGBA && out_format != HM_OUT_RRGGBBAA_LE) return hm_fail(HM_ERR_INVALID_ARG, "alpha: the three-channel output format %d carries no alpha", out_format);
  if (out_format == HM_OUT_RGBA)
    for (int c = 0; c < 3; c++)
      if (a->background[c] > 255) return hm_fail(HM_ERR_INVALID_ARG, "alpha: background[%d] = %d above the peak 255", c, (int)a->background[c]);
  if (a->mode == HM_ALPHA_PREMULTIPLIED && tone) return hm_fail(HM_ERR_INVALID_ARG, "alpha: HM_ALPHA_PREMULTIPLIED beside a tone step (tone-mapped premultiplied light is not a defined result)");
  if (!matte) return out_format;
  if (tone && tone->out_bits == 8) return HM_OUT_RGB;
  return out_format == HM_OUT_RGBA ? HM_OUT_RGB : HM_OUT_RRGGBB_LE;
}

// ---- the gain step (hm_device_gain) ------------------------------------------------------------------------------------------------

int hm_gain_check(const hm_gain_params* g, float headroom, int bad)
{
  if (!g) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (std::isnan(headroom) || headroom < 0.0f) return hm_fail(HM_ERR_INVALID_ARG, "gain: headroom %g is NaN or negative", (double)headroom);
  if (g->reserved) return hm_fail(bad, "gain: reserved is not 0");
  bool finite = std::isfinite(g->base_headroom) && std::isfinite(g->alternate_headroom);
  for (int c = 0; c < 3; c++) finite = finite && std::isfinite(g->map_min[c]) && std::isfinite(g->map_max[c]) && std::isfinite(g->base_offset[c]) && std::isfinite(g->alternate_offset[c]);
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(g->gamma[c]) || !(g->gamma[c] > 0.0)) return hm_fail(bad, "gain: gamma[%d] = %g is not finite and above 0", c, g->gamma[c]);
  if (!finite) return hm_fail(bad, "gain: a parameter is not finite");
  if (g->alternate_headroom == g->base_headroom) return hm_fail(bad, "gain: alternate_headroom == base_headroom (%g): the map has no weight", g->base_headroom);
  return HM_OK;
}

double hm_gain_weight(const hm_gain_params* g, float headroom)
{
  const double w = ((double)headroom - g->base_headroom) / (g->alternate_headroom - g->base_headroom);
  return std::min(std::max(w, 0.0), 1.0);
}

// one table and one M serve the three colour channels
static bool gain_one_channel(const hm_gain_params* g)
{
  for (int c = 1; c < 3; c++)
    if (g->map_min[c] != g->map_min[0] || g->map_max[c] != g->map_max[0] || g->gamma[c] != g->gamma[0] || g->base_offset[c] != g->base_offset[0] ||
        g->alternate_offset[c] != g->alternate_offset[0]) return false;
  return true;
}

// tab_c of include/heif_mi355x.h: 1 << bits entries
static void fill_gain_table(const hm_gain_params* g, double wgt, int c, int bits, float* out)
{
  const int n = 1 << bits;
  const double mpeak = (double)(n - 1), lo = g->map_min[c], span = g->map_max[c] - g->map_min[c], gamma = g->gamma[c];
  for (int v = 0; v < n; v++) {
    double u = (double)v / mpeak;
    if (gamma != 1.0) u = std::pow(u, 1.0 / gamma);
    out[v] = (float)std::exp2(wgt * (lo + span * u));
  }
}

int hm_gain_table(const hm_gain_params* params, float headroom, int channel, int map_bits, float* out)
{
  if (!params || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (channel < 0 || channel > 2) return hm_fail(HM_ERR_INVALID_ARG, "gain: channel %d is not 0 .. 2", channel);
  if (map_bits < 8 || map_bits > HM_GAIN_MAX_BITS) return hm_fail(HM_ERR_UNSUPPORTED, "gain: a map of %d bits (8 .. %d are supported)", map_bits, (int)HM_GAIN_MAX_BITS);
  const int rc = hm_gain_check(params, headroom, HM_ERR_INVALID_ARG);
  if (rc) return rc;
  fill_gain_table(params, hm_gain_weight(params, headroom), channel, map_bits, out);
  return 1 << map_bits;
}

// the step's own refusals that need nothing but the request
static int gain_check(const hm_out_steps* st)
{
  const hm_device_gain* g = st->gain;
  if (!st->light) return hm_fail(HM_ERR_INVALID_ARG, "gain: null light step");
  if (g->reserved[0] || g->reserved[1] || g->reserved[2] || g->reserved[3]) return hm_fail(HM_ERR_INVALID_ARG, "gain: reserved is not 0");
  const int rc = hm_gain_check(&g->params, g->headroom, HM_ERR_INVALID_ARG);
  if (rc) return rc;
  if (st->alpha) return hm_fail(HM_ERR_UNSUPPORTED, "gain: an alpha step beside the gain step is not supported (the open step)");
  return HM_OK;
}

// the gain step into the plan: the weight and the offsets (lp: the light plan beside it), and - once the map's size is known - the geometry
static int gain_plan_of(const hm_device_gain* g, const hm_out_image* img, const hm_view_plan* vp, const hm_light_plan* lp, hm_gain_plan* gp)
{
  std::memset(gp, 0, sizeof(*gp));
  gp->params = g->params; gp->headroom = g->headroom;
  gp->active = hm_gain_weight(&g->params, g->headroom) != 0.0;
  gp->nch = gain_one_channel(&g->params) ? 1 : 3;
  for (int c = 0; c < 3; c++) { gp->kb[c] = (float)((double)lp->gain * g->params.base_offset[c]); gp->ka[c] = (float)((double)lp->gain * g->params.alternate_offset[c]); }
  if (img->map_w == 0 && img->map_h == 0) return HM_OK;
  return hm_gain_geometry(img->w, img->h, img->map_w, img->map_h, img->map_bits, vp, gp);
}

int hm_gain_geometry(int W, int H, int MW, int MH, int map_bits, const hm_view_plan* vp, hm_gain_plan* gp)
{
  gp->filter = !vp->crop_only && vp->filter == HM_VIEW_NEAREST ? HM_VIEW_NEAREST : HM_VIEW_TRIANGLE;
  if (MW < 1 || MH < 1 || MW > W || MH > H) return hm_fail(HM_ERR_UNSUPPORTED, "gain: a %d x %d map for a %d x %d base image is not supported", MW, MH, W, H);
  const int sx = (int)(((int64_t)W + MW - 1) / MW), sy = (int)(((int64_t)H + MH - 1) / MH); // (sizes as a file declares them: up to 2^31 - 1)
  if (MW != ((int64_t)W + sx - 1) / sx || MH != ((int64_t)H + sy - 1) / sy)
    return hm_fail(HM_ERR_UNSUPPORTED, "gain: a %d x %d map for a %d x %d base image is not supported (no whole factor per axis gives that size)", MW, MH, W, H);
  if (map_bits < 8 || map_bits > HM_GAIN_MAX_BITS)
    return hm_fail(HM_ERR_UNSUPPORTED, "gain: a map of %d bits is not supported (8 .. %d are; deeper maps are the open step)", map_bits, (int)HM_GAIN_MAX_BITS);
  if (vp->x % sx) return hm_fail(HM_ERR_INVALID_ARG, "gain: crop_x %d is no multiple of %d, the map has one column for %d of the base", vp->x, sx, sx);
  if (vp->y % sy) return hm_fail(HM_ERR_INVALID_ARG, "gain: crop_y %d is no multiple of %d, the map has one row for %d of the base", vp->y, sy, sy);
  gp->map_w = MW; gp->map_h = MH; gp->map_bits = map_bits; gp->sx = sx; gp->sy = sy;
  gp->mx = vp->x / sx; gp->my = vp->y / sy; gp->mw = (int)(((int64_t)vp->w + sx - 1) / sx); gp->mh = (int)(((int64_t)vp->h + sy - 1) / sy);
  int rc;
  if ((rc = check_axis(gp->mw, vp->ow, gp->filter, "map width")) || (rc = check_axis(gp->mh, vp->oh, gp->filter, "map height"))) return rc;
  return HM_OK;
}

// ---- the device write: one request (hm_out_steps), one plan (hm_out_plan), one writer --------------------------------------------

int hm_out_dest_format(int out_format, const hm_out_steps* st)
{
  return st->alpha ? hm_alpha_dest_format(out_format, st->alpha, st->tone) : tone_dest_format(out_format, st->tone);
}

int hm_out_check_static(int out_format, const hm_device_dest* d, const hm_out_steps* st, int explicit_from)
{
  const hm_device_light* l = st->light;
  const hm_device_tone* tone = st->tone;
  const hm_device_alpha* a = st->alpha;
  const int dest_format = hm_out_dest_format(out_format, st); // (the alpha step's own refusals)
  if (dest_format < 0) return dest_format;
  if (!d) return hm_fail(HM_ERR_INVALID_ARG, "null device destination");
  if (tone && !l) return hm_fail(HM_ERR_INVALID_ARG, "tone: null light step");
  if (st->gain) { const int rc = gain_check(st); if (rc) return rc; }
  if (a && a->mode == HM_ALPHA_PREMULTIPLIED && l && l->to_transfer != HM_LIGHT_LINEAR)
    return hm_fail(HM_ERR_INVALID_ARG, "alpha: HM_ALPHA_PREMULTIPLIED beside a light step that re-encodes (transfer %d; encoded premultiplied light is not a defined result)", l->to_transfer);
  if (st->ootf) { const int rc = ootf_check_request(st); if (rc) return rc; }
  if (tone) {
    const int rc = tone_check(tone, !explicit_from || st->ootf); // (beside an OOTF step src_peak and unit_nits have a default of their own: display_peak)
    if (rc) return rc;
    if (tone->out_bits == 8) {
      if (d->dtype == HM_DEV_U16) return hm_fail(HM_ERR_INVALID_ARG, "tone: out_bits 8 with HM_DEV_U16 (HM_DEV_U8 holds the codes)");
      const int obpp = hm_out_bytes_per_pixel(out_format);
      if (a ? a->mode != HM_ALPHA_MATTE : obpp == 4 || obpp == 8) // (a matte has three channels: the 8-bit finish takes it)
        return hm_fail(HM_ERR_UNSUPPORTED, "tone: out_bits 8 with the four-channel output format %d is not supported", out_format);
    }
  }
  return l ? light_check(out_format, dest_format, d, st, explicit_from) : hm_dest_check_static(dest_format, d);
}

// the part of hm_out_resolve that needs the image's profile and depth
static int out_resolve_profile(int out_format, const hm_out_image* img, const hm_device_dest* d, const hm_out_steps* st, hm_out_plan* p)
{
  if (!st->light && !st->alpha) return HM_OK;
  int rc = hm_out_check_static(out_format, d, st, 0);
  if (rc) return rc;
  int bits = img->bits;
  if (const hm_device_alpha* a = st->alpha) {
    p->ap.mode = a->mode;
    if (out_format == HM_OUT_RGBA) bits = 8;
    if (bits < 8 || bits > 16 || (bits == 8) != (out_format == HM_OUT_RGBA)) return hm_fail(HM_ERR_UNSUPPORTED, "alpha: samples of %d bits in output format %d", bits, out_format);
    p->ap.bits = bits;
    for (int c = 0; c < 3; c++) {
      if (a->background[c] > (1 << bits) - 1) return hm_fail(HM_ERR_INVALID_ARG, "alpha: background[%d] = %d above the peak %d", c, (int)a->background[c], (1 << bits) - 1);
      p->ap.background[c] = a->background[c];
    }
  }
  if (!st->light) return HM_OK;
  if ((rc = light_plan_of(out_format, bits, img->transfer, img->primaries, st->light, st->icc, st->icc_size, &p->lp))) return rc;
  if (st->ootf && (rc = ootf_plan_of(st->ootf, &p->lp))) return rc;
  if (st->tone && (rc = tone_plan_of(st->tone, &p->lp))) return rc;
  { // no launch of the write asks for more local memory than a workgroup gets (light_step.h: check_light_lds) - only three tables get there
    const hm_light_plan& lp = p->lp;
    const bool summed = !p->vp.crop_only && p->vp.filter != HM_VIEW_NEAREST;
    const int steps = (lp.tone ? 1 : 0) | (lp.ootf ? 2 : 0);
    if (st->measure && (rc = hm_light_lds_check(lp.bits, lp.enc_bits, lp.encode, steps, lp.lin3, 3))) return rc; // the statistics pass
    if (st->measure == HM_MEASURE_STATS) return HM_OK; // (nothing is written: no other launch)
    if ((rc = hm_light_lds_check(lp.bits, lp.enc_bits, lp.encode, steps, lp.lin3, summed ? 1 : 0)) || (summed && (rc = hm_light_lds_check(lp.bits, lp.enc_bits, lp.encode, steps, lp.lin3, 2)))) return rc;
  }
  return st->gain ? gain_plan_of(st->gain, img, &p->vp, &p->lp, &p->gp) : (int)HM_OK;
}

int hm_out_resolve(int out_format, const hm_out_image* img, int know_profile, const hm_device_dest* d, const hm_out_steps* st, hm_out_plan* p)
{
  int rc;
  std::memset(p, 0, sizeof(*p));
  p->out_format = out_format; p->w = img->w; p->h = img->h;
  p->has_view = st->view != nullptr; p->has_light = st->light != nullptr; p->has_alpha = st->alpha != nullptr; p->has_gain = st->gain != nullptr;
  if (st->view) { if ((rc = hm_view_resolve(out_format, img->w, img->h, st->view, &p->vp))) return rc; }
  else { p->vp.w = p->vp.ow = img->w; p->vp.h = p->vp.oh = img->h; p->vp.crop_only = 1; }
  if (know_profile == HM_OUT_PROFILE_FIRST && (rc = out_resolve_profile(out_format, img, d, st, p))) return rc;
  if ((p->dest_format = hm_out_dest_format(out_format, st)) < 0) return p->dest_format;
  if ((rc = hm_dest_resolve(p->dest_format, p->vp.ow, p->vp.oh, d, &p->dp)) || (rc = hm_dest_check_len(d, &p->dp))) return rc;
  if (know_profile == HM_OUT_PROFILE_LAST && (rc = out_resolve_profile(out_format, img, d, st, p))) return rc;
  return HM_OK;
}

// The write under an active gain step (light beside it, no alpha): ONE pinned block and one upload - the base's tap tables (summed),
// the light tables, the gain tables, the map's tap tables (pointwise, summed) -, one device block for the intermediates of a summed
// view: the base's horizontal pass, the map's, and the M planes.
static int gain_write(const hm_device_dest* d, const hm_out_plan* p, const uint8_t* origin, int src_stride, int src_bytes, const hm_out_map* map, hipStream_t s,
                      hm_view_scratch* sc)
{
  const hm_view_plan* vp = &p->vp;
  const hm_dest_plan& dp = p->dp;
  const hm_gain_plan& gp = p->gp;
  const bool summed = !vp->crop_only && vp->filter != HM_VIEW_NEAREST, nearest = !vp->crop_only && !summed;
  if (!map || !map->plane || gp.map_w <= 0) return hm_fail(HM_ERR_INTERNAL, "gain: no map for the write");
  if (!p->has_light || p->has_alpha) return hm_fail(HM_ERR_INTERNAL, "gain: light%s alpha%s", p->has_light ? "+" : "-", p->has_alpha ? "+" : "-");
  const int map_bytes = hm_sample_bytes(gp.map_bits);
  if ((int64_t)map->stride < (int64_t)gp.map_w * map_bytes) return hm_fail(HM_ERR_INVALID_ARG, "gain: map_stride %d below the bytes of a row", map->stride);
  const LightTables T(&p->lp);
  const size_t table_bytes = T.bytes(), gain_floats = (size_t)gp.nch << gp.map_bits;
  int mtx = 0, mty = 0, rc;
  if (summed && ((mtx = axis_most_taps(gp.mw, vp->ow, gp.filter)) < 0 || (mty = axis_most_taps(gp.mh, vp->oh, gp.filter)) < 0)) return mtx < 0 ? mtx : mty;
  // the map's taps: tables like the base's (summed), 16-byte records per output index (pointwise: the map is enlarged), none (nearest)
  const size_t mwords_x = nearest ? 0 : summed ? (size_t)vp->ow * (2 + mtx) : (size_t)vp->ow * 4, mwords_y = nearest ? 0 : summed ? (size_t)vp->oh * (2 + mty) : (size_t)vp->oh * 4;
  const size_t extra = table_bytes + (gain_floats + mwords_x + mwords_y) * 4;
  size_t words_x = 0, words_y = 0;
  int tx = 0, ty = 0;
  bool staged = false;
  if (!sc || sc->pinned || sc->dev[0] || sc->dev[1]) return hm_fail(HM_ERR_INTERNAL, "device write: no free scratch for the tables");
  if (summed) { if ((rc = view_tables(vp, extra, sc, &words_x, &words_y, &tx, &ty, &staged))) return rc; }
  else if (!(sc->pinned = hm_pool_pinned_alloc(extra))) return hm_fail(HM_ERR_NOMEM, "out of memory");
  const size_t tap_bytes = (words_x + words_y) * 4, bytes = tap_bytes + extra;
  float* host_tables = reinterpret_cast<float*>((uint8_t*)sc->pinned + tap_bytes);
  float* host_gain = host_tables + table_bytes / 4;
  int32_t* host_mx = reinterpret_cast<int32_t*>(host_gain + gain_floats);
  T.fill(host_tables);
  const double wgt = hm_gain_weight(&gp.params, gp.headroom);
  for (int c = 0; c < gp.nch; c++) fill_gain_table(&gp.params, wgt, c, gp.map_bits, host_gain + ((size_t)c << gp.map_bits));
  if (summed) { fill_axis(host_mx, gp.mw, vp->ow, gp.filter, mtx); fill_axis(host_mx + mwords_x, gp.mh, vp->oh, gp.filter, mty); }
  else if (!nearest && ((rc = fill_axis_records(reinterpret_cast<hm_gain_tap*>(host_mx), gp.mw, vp->ow, gp.filter)) ||
                        (rc = fill_axis_records(reinterpret_cast<hm_gain_tap*>(host_mx + mwords_x), gp.mh, vp->oh, gp.filter)))) return rc;
  if (!(sc->dev[0] = hm_pool_device_alloc(bytes))) return HM_ERR_NO_DEVICE;
  hm_light_args la = T.args(src_bytes);
  hm_gain_args ga;
  hm_resample_args r;
  std::memset(&ga, 0, sizeof(ga));
  std::memset(&r, 0, sizeof(r));
  ga.pitch = ((int64_t)vp->ow + 15) / 16 * 16;
  if (summed) {
    r = resample_args_of(vp, src_bytes, origin, src_stride, sc->dev[0], words_x, tx, ty, dp);
    const size_t base_floats = resample_tmp_floats(r, dp), mtmp_floats = (size_t)ga.pitch * gp.mh * gp.nch, M_floats = (size_t)ga.pitch * vp->oh * gp.nch;
    if (!(sc->dev[1] = hm_pool_device_alloc((base_floats + mtmp_floats + M_floats) * sizeof(float)))) return HM_ERR_NO_DEVICE;
    r.tmp = (float*)sc->dev[1];
    ga.mtmp = r.tmp + base_floats; ga.M = ga.mtmp + mtmp_floats;
  }
  if ((rc = hm_check_hip(hipMemcpyAsync(sc->dev[0], sc->pinned, bytes, hipMemcpyHostToDevice, s), "upload of the tap, light and gain tables"))) return rc;
  const float* dev_tables = reinterpret_cast<const float*>((const uint8_t*)sc->dev[0] + tap_bytes);
  T.point(&la, dev_tables);
  ga.tab = dev_tables + table_bytes / 4;
  ga.nch = gp.nch; ga.map_bits = gp.map_bits; ga.map_bytes = map_bytes;
  for (int c = 0; c < 3; c++) { ga.kb[c] = gp.kb[c]; ga.ka[c] = gp.ka[c]; }
  ga.map = (const uint8_t*)map->plane + (size_t)gp.my * map->stride + (size_t)gp.mx * map_bytes;
  ga.map_stride = map->stride; ga.mw = gp.mw; ga.mh = gp.mh;
  if (!summed && !nearest) { // (the records sit 16-byte aligned: the tables before them are multiples of 1 KB, no base taps are uploaded)
    ga.xrec = reinterpret_cast<const hm_gain_tap*>(ga.tab + gain_floats); ga.yrec = ga.xrec + vp->ow;
    ga.ax.m = vp->ow; ga.ay.m = vp->oh;
  }
  if (summed) {
    const int32_t* dx = reinterpret_cast<const int32_t*>(ga.tab + gain_floats);
    const int32_t* dy = dx + mwords_x;
    ga.ax.first = dx; ga.ax.count = dx + vp->ow; ga.ax.weights = reinterpret_cast<const float*>(dx + 2 * (size_t)vp->ow); ga.ax.m = vp->ow; ga.ax.taps = mtx;
    ga.ay.first = dy; ga.ay.count = dy + vp->oh; ga.ay.weights = reinterpret_cast<const float*>(dy + 2 * (size_t)vp->oh); ga.ay.m = vp->oh; ga.ay.taps = mty;
  }
  if (summed) return hm_launch_gain_resample(&dp, &la, &ga, &r, d->ptr, d->scale, d->bias, s);
  if (nearest) return hm_launch_gain_nearest(&dp, &la, &ga, origin, src_stride, vp->w, vp->h, vp->ow, vp->oh, d->ptr, d->scale, d->bias, s);
  return hm_launch_gain_tensor(&dp, &la, &ga, origin, src_stride, vp->w, vp->h, d->ptr, d->scale, d->bias, s);
}

int hm_out_write(const hm_device_dest* d, const hm_out_plan* p, const void* src, int src_stride, const hm_out_map* map, hipStream_t s, hm_view_scratch* sc)
{
  const hm_view_plan* vp = &p->vp;
  const hm_dest_plan& dp = p->dp;
  // the kind of move: pointwise, the nearest sample, or sums under the taps of a filter
  const bool summed = !vp->crop_only && vp->filter != HM_VIEW_NEAREST, nearest = !vp->crop_only && !summed;
  // the step: plain (0), light (1), alpha with or without light (2).  HM_ALPHA_STRAIGHT without sums is r_c = x_c: the write without the step
  const hm_light_plan* lp = p->has_light ? &p->lp : nullptr;
  const bool alpha = p->has_alpha && (p->ap.mode != HM_ALPHA_STRAIGHT || summed);
  const int step = alpha ? 2 : lp ? 1 : 0;
  // (bytes of a source sample: of out_format - under an 8-bit finish or a matte dp.sample_bytes is the sibling target's)
  const int obpp = hm_out_bytes_per_pixel(p->out_format), src_bytes = obpp >= 6 ? 2 : 1;
  if (alpha && obpp != 4 && obpp != 8) return hm_fail(HM_ERR_INTERNAL, "alpha: output format %d has no four channels", p->out_format);
  const uint8_t* origin = (const uint8_t*)src + (size_t)vp->y * src_stride + (size_t)vp->x * obpp;
  if (p->has_gain && p->gp.active) return gain_write(d, p, origin, src_stride, src_bytes, map, s, sc); // (a gain step of weight 0: the write without it)
  if (!step && vp->crop_only) // the rectangle's bytes: the 2-D copy or k_to_tensor on the offset source
    return hm_dest_write(d, p->out_format, vp->w, vp->h, 0, vp->h, origin, src_stride, s);
  const LightTables T(lp);
  const size_t table_bytes = T.bytes();
  hm_light_args la = T.args(src_bytes);
  // ONE pinned block and one upload: the tap tables of both axes (summed), then the light tables; neither: no block, sc is not touched
  size_t words_x = 0, words_y = 0;
  int tx = 0, ty = 0, rc;
  bool staged = false;
  if (summed || table_bytes) {
    if (!sc || sc->pinned || sc->dev[0] || sc->dev[1]) return hm_fail(HM_ERR_INTERNAL, "device write: no free scratch for the tables");
    if (summed) { if ((rc = view_tables(vp, table_bytes, sc, &words_x, &words_y, &tx, &ty, &staged))) return rc; }
    else if (!(sc->pinned = hm_pool_pinned_alloc(table_bytes))) return hm_fail(HM_ERR_NOMEM, "out of memory");
  }
  const size_t tap_bytes = (words_x + words_y) * 4, bytes = tap_bytes + table_bytes;
  const float* host_tables = table_bytes ? reinterpret_cast<const float*>((const uint8_t*)sc->pinned + tap_bytes) : nullptr;
  if (table_bytes) T.fill(const_cast<float*>(host_tables));
  hm_alpha_args aa;
  std::memset(&aa, 0, sizeof(aa));
  if (alpha) {
    aa.mode = p->ap.mode; aa.bits = p->ap.bits; aa.src_bytes = src_bytes; aa.P = (float)((1 << p->ap.bits) - 1);
    // the background as the kernels take it: b_c = (float)background[c], with a light step lin[background[c]] of the table just filled
    for (int c = 0; c < 3; c++) aa.bg[c] = host_tables ? host_tables[(lp->lin3 ? (size_t)c << lp->bits : 0) + p->ap.background[c]] : (float)p->ap.background[c]; // (lin3: its channel's table)
  }
  if (bytes && !(sc->dev[0] = hm_pool_device_alloc(bytes))) return HM_ERR_NO_DEVICE;
  hm_resample_args r;
  std::memset(&r, 0, sizeof(r));
  if (summed) {
    hm_dest_plan pi = dp; // the intermediate is laid out like the destination - under the alpha step with four sums per pixel, whatever its channel count
    if (alpha) pi.channels = 4;
    r = resample_args_of(vp, src_bytes, origin, src_stride, sc->dev[0], words_x, tx, ty, pi);
    if (!(sc->dev[1] = hm_pool_device_alloc(resample_tmp_floats(r, pi) * sizeof(float)))) return HM_ERR_NO_DEVICE;
    r.tmp = (float*)sc->dev[1];
    if (!step) { r.staged = staged ? 1 : 0; r.stage_px = hm_knob(HM_KNOB_VIEW_STAGE_PX); } // (the light and alpha passes never stage)
  }
  const char* what = !summed ? "upload of the light tables" : table_bytes ? "upload of the tap and light tables" : "upload of the tap tables";
  if (bytes && (rc = hm_check_hip(hipMemcpyAsync(sc->dev[0], sc->pinned, bytes, hipMemcpyHostToDevice, s), what))) return rc;
  if (table_bytes) T.point(&la, reinterpret_cast<const float*>((const uint8_t*)sc->dev[0] + tap_bytes));
  const hm_light_args* pla = lp ? &la : nullptr;
  // one launch: {pointwise, nearest, summed} x {plain, light, alpha}; the plain pointwise one is hm_dest_write above
  void* dst = d->ptr;
  const float *sl = d->scale, *bs = d->bias;
  if (summed)
    return step == 2 ? hm_launch_alpha_resample(&dp, pla, &aa, &r, dst, sl, bs, s) : step == 1 ? hm_launch_light_resample(&dp, &la, &r, dst, sl, bs, s) : hm_launch_resample(&dp, &r, dst, sl, bs, s);
  if (nearest)
    return step == 2   ? hm_launch_alpha_nearest(&dp, pla, &aa, origin, src_stride, vp->w, vp->h, vp->ow, vp->oh, dst, sl, bs, s)
           : step == 1 ? hm_launch_light_nearest(&dp, &la, origin, src_stride, vp->w, vp->h, vp->ow, vp->oh, dst, sl, bs, s)
                       : hm_launch_view_nearest(&dp, origin, src_stride, vp->w, vp->h, vp->ow, vp->oh, dst, sl, bs, s);
  return step == 2 ? hm_launch_alpha_tensor(&dp, pla, &aa, origin, src_stride, vp->w, vp->h, dst, sl, bs, s) : hm_launch_light_tensor(&dp, &la, origin, src_stride, vp->w, vp->h, dst, sl, bs, s);
}

// ---- many views of one picture (hm_views_write; hm_view_multi.h holds the arithmetic, resample.hip the kernels) --------------------

// two destinations whose byte ranges [ptr, ptr + bytes) overlap: bytes as hm_dest_resolve computes them (plans[k].dp), with the pitches as resolved
int hm_dests_check_overlap(const hm_device_dest* dests, const hm_out_plan* plans, int n)
{
  std::vector<int> order((size_t)n);
  for (int k = 0; k < n; k++) order[(size_t)k] = k;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return (uintptr_t)dests[a].ptr < (uintptr_t)dests[b].ptr || (dests[a].ptr == dests[b].ptr && a < b); });
  // (sorted by start: a range that overlaps any earlier one overlaps the earlier one that ends last)
  int last = order[0];
  for (int i = 1; i < n; i++) {
    const int k = order[(size_t)i];
    const uintptr_t end_last = (uintptr_t)dests[last].ptr + (uintptr_t)plans[last].dp.bytes;
    if ((uintptr_t)dests[k].ptr < end_last)
      return hm_fail(HM_ERR_INVALID_ARG, "views: the destinations of views %d and %d overlap (%lld bytes at %p, %lld bytes at %p)", std::min(last, k), std::max(last, k),
                     (long long)plans[std::min(last, k)].dp.bytes, dests[std::min(last, k)].ptr, (long long)plans[std::max(last, k)].dp.bytes, dests[std::max(last, k)].ptr);
    if ((uintptr_t)dests[k].ptr + (uintptr_t)plans[k].dp.bytes > end_last) last = k;
  }
  return HM_OK;
}

namespace {
// one distinct axis of a group's views: n -> m under a filter; its table of m * (2 + taps) words at word `off` of the block
struct MultiAxis { int n, m, filt, taps; int64_t off; };

// one group of a multi-view write: views idx[0 .. m) share the key (hm_view_multi.h) - ONE pinned block and one upload (every distinct
// axis' tap table once, the records, the running sums), one intermediate sized for the largest chunk, and per chunk one launch per pass
int views_write_group(const hm_device_dest* dests, const hm_out_plan* plans, const int* idx, int m, bool staged, const void* src, int src_stride, hipStream_t s,
                      hm_view_scratch* sc)
{
  const hm_dest_plan& p0 = plans[idx[0]].dp;
  const bool chw = p0.layout == HM_DEV_LAYOUT_CHW;
  const int C = p0.channels, planes = chw ? C : 1, obpp = C * p0.sample_bytes;
  // the distinct axes: a table is the same whichever axis, and whichever view, reads it
  std::map<std::array<int, 3>, int> seen;
  std::vector<MultiAxis> axes;
  std::vector<int> ax((size_t)m), ay((size_t)m);
  int64_t words = 0;
  auto axis_of = [&](int n, int mm, int filt) -> int {
    const auto at = seen.find({n, mm, filt});
    if (at != seen.end()) return at->second;
    const int taps = axis_most_taps(n, mm, filt);
    if (taps < 0) return taps;
    axes.push_back(MultiAxis{n, mm, filt, taps, words});
    words += (int64_t)mm * (2 + taps);
    return seen[{n, mm, filt}] = (int)axes.size() - 1;
  };
  for (int i = 0; i < m; i++) {
    const hm_view_plan& vp = plans[idx[i]].vp;
    if ((ax[(size_t)i] = axis_of(vp.w, vp.ow, vp.filter)) < 0) return ax[(size_t)i];
    if ((ay[(size_t)i] = axis_of(vp.h, vp.oh, vp.filter)) < 0) return ay[(size_t)i];
  }
  if (words > 0x7FFFFFFF) return hm_fail(HM_ERR_NOMEM, "views: %lld words of tap tables in one group", (long long)words);
  const hm_view_multi_block lay = hm_view_multi_layout(words, m);
  uint8_t* host = (uint8_t*)hm_pool_pinned_alloc((size_t)lay.bytes);
  if (!host) return hm_fail(HM_ERR_NOMEM, "out of memory");
  sc->pinned = host;
  int32_t* tw = (int32_t*)host;
  for (const MultiAxis& a : axes) fill_axis(tw + a.off, a.n, a.m, a.filt, a.taps);
  if (staged) // (view_tables' check of the windows the staged pass loads as one run)
    for (int i = 0; i < m; i++) {
      const MultiAxis& a = axes[(size_t)ax[(size_t)i]];
      const int32_t* t = tw + a.off;
      for (int j = 0; j < a.m; j++) {
        const int lo = t[j], hi = lo + t[a.m + j];
        if (lo < 0 || hi > a.n || hi <= lo || (j && (lo < t[j - 1] || hi < t[j - 1] + t[a.m + j - 1])))
          return hm_fail(HM_ERR_INTERNAL, "view: the windows of columns %d and %d are not in order", j - 1, j);
      }
    }
  // the records, and what the chunk cut asks of every view
  hm_view_rec* rec = reinterpret_cast<hm_view_rec*>(host + lay.rec_off);
  int32_t* hsum = reinterpret_cast<int32_t*>(host + lay.hsum_off);
  int32_t* vsum = reinterpret_cast<int32_t*>(host + lay.vsum_off);
  std::vector<int64_t> bytes((size_t)m), floats((size_t)m);
  std::vector<int32_t> hg((size_t)m), vg((size_t)m);
  bool vec = true;
  for (int i = 0; i < m; i++) {
    const hm_out_plan& pl = plans[idx[i]];
    const hm_view_plan& vp = pl.vp;
    const hm_device_dest& d = dests[idx[i]];
    const MultiAxis &x = axes[(size_t)ax[(size_t)i]], &y = axes[(size_t)ay[(size_t)i]];
    hm_view_rec& r = rec[i];
    std::memset(&r, 0, sizeof(r));
    r.src = (uint64_t)(uintptr_t)((const uint8_t*)src + (size_t)vp.y * src_stride + (size_t)vp.x * obpp);
    r.dst = (uint64_t)(uintptr_t)d.ptr;
    r.row_pitch = pl.dp.row_pitch; r.plane_pitch = pl.dp.plane_pitch;
    r.n_h = vp.h; r.ow = vp.ow; r.oh = vp.oh; r.E = chw ? vp.ow : vp.ow * C;
    r.tmp_pitch = ((int64_t)r.E + 15) / 16 * 16; r.tmp_plane = r.tmp_pitch * vp.h; // (resample_args_of's intermediate: laid out like the destination)
    r.x_first = (int32_t)x.off; r.x_count = (int32_t)(x.off + x.m); r.x_weights = (int32_t)(x.off + 2 * (int64_t)x.m);
    r.y_first = (int32_t)y.off; r.y_count = (int32_t)(y.off + y.m); r.y_weights = (int32_t)(y.off + 2 * (int64_t)y.m);
    bytes[(size_t)i] = (int64_t)vp.ow * vp.h * C * 4;
    floats[(size_t)i] = r.tmp_plane * planes;
    hg[(size_t)i] = hm_view_row_groups(vp.h); vg[(size_t)i] = hm_view_row_groups(vp.oh);
    vec = vec && ((uintptr_t)d.ptr % 16) == 0 && (pl.dp.row_pitch % 16) == 0 && (!chw || (pl.dp.plane_pitch % 16) == 0);
  }
  // the chunks: the running sums and the regions of the intermediate restart with each
  const int64_t bound = hm_knob(HM_KNOB_VIEW_BATCH_BYTES);
  int64_t tmp_most = 0;
  for (int c0 = 0; c0 < m;) {
    const int n = hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), c0, m, bound);
    int64_t off = 0;
    int32_t h = 0, v = 0;
    for (int i = c0; i < c0 + n; i++) {
      rec[i].tmp_off = off; off += floats[(size_t)i];
      hsum[i] = (h += hg[(size_t)i]); vsum[i] = (v += vg[(size_t)i]);
    }
    tmp_most = std::max(tmp_most, off);
    c0 += n;
  }
  int rc;
  if (!(sc->dev[0] = hm_pool_device_alloc((size_t)lay.bytes))) return HM_ERR_NO_DEVICE;
  if (!(sc->dev[1] = hm_pool_device_alloc((size_t)tmp_most * sizeof(float)))) return HM_ERR_NO_DEVICE;
  if ((rc = hm_check_hip(hipMemcpyAsync(sc->dev[0], host, (size_t)lay.bytes, hipMemcpyHostToDevice, s), "upload of the views' tap tables and records"))) return rc;
  const uint8_t* dev = (const uint8_t*)sc->dev[0];
  for (int c0 = 0; c0 < m;) {
    const int n = hm_view_multi_chunk(bytes.data(), hg.data(), vg.data(), c0, m, bound);
    hm_resample_multi a;
    std::memset(&a, 0, sizeof(a));
    a.block = dev;
    a.recs = dev + lay.rec_off + (size_t)c0 * sizeof(hm_view_rec);
    a.hsums = reinterpret_cast<const int32_t*>(dev + lay.hsum_off) + c0;
    a.vsums = reinterpret_cast<const int32_t*>(dev + lay.vsum_off) + c0;
    a.views = n;
    a.sample_bytes = p0.sample_bytes; a.channels = C; a.src_stride = src_stride;
    a.staged = staged ? 1 : 0; a.stage_px = hm_knob(HM_KNOB_VIEW_STAGE_PX);
    a.vec = vec ? 1 : 0;
    a.h_groups = hsum[c0 + n - 1]; a.v_groups = vsum[c0 + n - 1];
    for (int i = c0; i < c0 + n; i++) { a.ow_most = std::max(a.ow_most, rec[i].ow); a.E_most = std::max(a.E_most, rec[i].E); }
    a.tmp = (float*)sc->dev[1];
    const hm_device_dest& d0 = dests[idx[0]];
    if ((rc = hm_launch_resample_multi(&p0, &a, d0.scale, d0.bias, s))) return rc;
    c0 += n;
  }
  return HM_OK;
}
} // namespace

int hm_views_write(const hm_device_dest* dests, const hm_out_plan* plans, int n, const void* src, int src_stride, hipStream_t s, hm_view_scratch* sc)
{
  if (n <= 0) return HM_OK;
  const bool multi = hm_knob(HM_KNOB_VIEW_MULTI) != 0;
  std::vector<hm_view_multi_key> keys;
  std::vector<std::vector<int>> members;
  for (int k = 0; k < n; k++) {
    const hm_out_plan& p = plans[k];
    const bool plain = !p.has_light && !p.has_alpha && !p.has_gain;
    if (!multi || !plain || p.vp.crop_only || !filter_resamples(p.vp.filter)) { // what exists, view by view, from the one picture
      const int rc = hm_out_write(&dests[k], &p, src, src_stride, nullptr, s, &sc[k]);
      if (rc) return rc;
      continue;
    }
    const bool staged = (p.vp.filter == HM_VIEW_CUBIC || p.vp.filter == HM_VIEW_LANCZOS3) && hm_knob(HM_KNOB_VIEW_H_STAGED) != 0;
    hm_view_multi_key key;
    hm_view_multi_key_make(&key, staged, p.dp.sample_bytes, p.dp.channels, p.dp.layout, p.dp.dtype, p.dp.row_pitch, p.dp.plane_pitch, (uintptr_t)dests[k].ptr,
                           p.dp.layout == HM_DEV_LAYOUT_CHW, dests[k].scale, dests[k].bias);
    size_t g = 0;
    while (g < keys.size() && !hm_view_multi_key_equal(&keys[g], &key)) g++;
    if (g == keys.size()) { keys.push_back(key); members.emplace_back(); }
    members[g].push_back(k);
  }
  for (size_t g = 0; g < members.size(); g++) { // (a group's blocks hang on the scratch entry of its first view: unused otherwise)
    const std::vector<int>& m = members[g];
    const int rc = views_write_group(dests, plans, m.data(), (int)m.size(), keys[g].staged != 0, src, src_stride, s, &sc[m[0]]);
    if (rc) return rc;
  }
  return HM_OK;
}

// ---- the stand-alone entries: pixels that are in device memory already, through the same plan and writer ---------------------------

// kind: the entry (hm_entry_steps.h) - this family leaves a null light step to hm_out_check_static, behind the alpha step's own refusals
// size_prefix: of the message about a wrong width or height (hm_to_tensor's speaks of the destination)
// map, map_w, map_h, map_bits: the gain map of a gain step (hm_gain_to_tensor), else NULL and 0
static int out_to_tensor(int kind, int out_format, int bits, int w, int h, const void* src, int src_stride, const hm_out_steps& st, const hm_device_dest* dest, void* stream,
                         const char* size_prefix = "", const hm_out_map* map = nullptr, int map_w = 0, int map_h = 0, int map_bits = 0)
{
  if (!src || !dest) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  int rc = hm_entry_steps(kind, st, false, /*light_judged_later=*/true);
  if (!rc && kind != HM_ENTRY_ICC) rc = hm_entry_icc(st, "in a stand-alone entry that has no item: hm_icc_to_tensor takes a profile");
  if (!rc && kind == HM_ENTRY_ICC && !hm_light_from_icc(st.light) && !(rc = hm_entry_icc(st, nullptr)))
    rc = hm_fail(HM_ERR_INVALID_ARG, "light: hm_icc_to_tensor takes HM_LIGHT_FROM_ICC in from_transfer and from_primaries (they are %d and %d)", st.light->from_transfer, st.light->from_primaries);
  if (rc || (rc = hm_out_check_static(out_format, dest, &st, 1)) || (rc = check_image_size(size_prefix, w, h))) return rc;
  if (map && (rc = check_image_size("gain map: ", map_w, map_h))) return rc;
  const hm_out_image img = {w, h, bits, st.light ? st.light->from_transfer : 0, st.light ? st.light->from_primaries : 0, map_w, map_h, map_bits};
  hm_out_plan p;
  if ((rc = hm_out_resolve(out_format, &img, HM_OUT_PROFILE_FIRST, dest, &st, &p))) return rc;
  const int obpp = hm_out_bytes_per_pixel(out_format);
  if (src_stride < w * obpp) return hm_fail(HM_ERR_INVALID_ARG, "src_stride %d below the bytes of a row", src_stride);
  if (obpp >= 6 && (((uintptr_t)src | (unsigned)src_stride) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
  if (map) {
    if (map->stride < map_w * hm_sample_bytes(map_bits)) return hm_fail(HM_ERR_INVALID_ARG, "gain: map_stride %d below the bytes of a row", map->stride);
    if (map_bits > 8 && (((uintptr_t)map->plane | (unsigned)map->stride) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "gain: 16-bit map samples at an odd address or stride");
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  if ((rc = hm_dest_check_pointer(dest))) return rc;
  return with_scratch((hipStream_t)stream, [&](hm_view_scratch* sc) { return hm_out_write(dest, &p, src, src_stride, map, (hipStream_t)stream, sc); });
}

int hm_gain_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const void* d_map, int map_stride, int map_w, int map_h,
                      int map_bits, const hm_device_view* view, const hm_device_light* light, const hm_device_tone* tone, const hm_device_gain* gain,
                      const hm_device_dest* dest, void* stream)
{
  if (!d_map) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const hm_out_map map = {d_map, map_stride};
  return out_to_tensor(HM_ENTRY_GAIN, out_format, bits, src_w, src_h, d_src, src_stride, {view, light, tone, nullptr, gain}, dest, stream, "", &map, map_w, map_h, map_bits);
}

int hm_to_tensor(int out_format, int width, int height, const void* d_src, int src_stride, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_DEST, out_format, 0, width, height, d_src, src_stride, {}, dest, stream, "device destination: ");
}

int hm_resample_to_tensor(int out_format, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_VIEW, out_format, 0, src_w, src_h, d_src, src_stride, {view}, dest, stream);
}

// the multi form of hm_resample_to_tensor: every view and destination is judged, in hm_resample_to_tensor's order, before anything is queued
int hm_resample_views_to_tensor(int out_format, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* views, const hm_device_dest* dests,
                                int32_t count, void* stream)
{
  if (!d_src || !views || !dests) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (count < 1 || count > HM_VIEWS_MOST) return hm_fail(HM_ERR_INVALID_ARG, "views: count %d outside 1 .. %d", count, (int)HM_VIEWS_MOST);
  int rc;
  if ((rc = check_image_size("", src_w, src_h))) return rc;
  const hm_out_image img = {src_w, src_h, 0, 0, 0, 0, 0, 0};
  std::vector<hm_out_plan> plans((size_t)count);
  for (int k = 0; k < count; k++) {
    const hm_out_steps st = {&views[k]};
    if ((rc = hm_out_check_static(out_format, &dests[k], &st, 1)) || (rc = hm_out_resolve(out_format, &img, HM_OUT_PROFILE_FIRST, &dests[k], &st, &plans[(size_t)k])))
      return hm_fail(rc, "view %d: %s", k, std::string(hm_last_error()).c_str());
  }
  if ((rc = hm_dests_check_overlap(dests, plans.data(), count))) return rc;
  const int obpp = hm_out_bytes_per_pixel(out_format);
  if (src_stride < src_w * obpp) return hm_fail(HM_ERR_INVALID_ARG, "src_stride %d below the bytes of a row", src_stride);
  if (obpp >= 6 && (((uintptr_t)d_src | (unsigned)src_stride) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  for (int k = 0; k < count; k++)
    if ((rc = hm_dest_check_pointer(&dests[k]))) return hm_fail(rc, "view %d: %s", k, std::string(hm_last_error()).c_str());
  std::vector<hm_view_scratch> sc((size_t)count, hm_view_scratch{{nullptr, nullptr}, nullptr});
  rc = hm_views_write(dests, plans.data(), count, d_src, src_stride, (hipStream_t)stream, sc.data());
  hm_view_scratch_retire((hipStream_t)stream, sc.data(), count); // (the blocks follow the stream, whatever was queued)
  return rc;
}

int hm_light_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_light* light,
                       const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_LIGHT, out_format, bits, src_w, src_h, d_src, src_stride, {view, light}, dest, stream);
}

int hm_tone_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_light* light,
                      const hm_device_tone* tone, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_TONE, out_format, bits, src_w, src_h, d_src, src_stride, {view, light, tone}, dest, stream);
}

int hm_alpha_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_light* light,
                       const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_ALPHA, out_format, bits, src_w, src_h, d_src, src_stride, {view, light, tone, alpha}, dest, stream);
}

int hm_icc_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const uint8_t* icc, size_t icc_size,
                     const hm_device_light* light, const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_ICC, out_format, bits, src_w, src_h, d_src, src_stride, {view, light, tone, alpha, nullptr, nullptr, icc, icc_size}, dest, stream);
}

int hm_ootf_to_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_light* light,
                      const hm_device_ootf* ootf, const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest, void* stream)
{
  return out_to_tensor(HM_ENTRY_OOTF, out_format, bits, src_w, src_h, d_src, src_stride, {view, light, tone, alpha, nullptr, ootf}, dest, stream);
}

// ---- the light statistics (hm_light_stats) ---------------------------------------------------------------------------------------

namespace {

// code_nits of include/heif_mi355x.h
double stats_code_nits(int k, int edge)
{
  const double top = (double)(HM_LIGHT_STATS_BINS - 1), x = edge ? std::min((double)k + 0.5, top) : (double)k;
  return 10000.0 * light_of_code(16, x / top);
}

// the pool blocks of one measurement: released when the stream has been waited for, or nothing was queued on them
struct StatsBlocks {
  void* pinned = nullptr; void* dev = nullptr;
  ~StatsBlocks() { if (pinned) hm_pool_pinned_free(pinned); if (dev) hm_pool_device_free(dev); }
};

} // namespace

int hm_light_stats_code_nits(int k, int edge, double* nits)
{
  if (!nits) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (k < 0 || k >= HM_LIGHT_STATS_BINS) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: code %d is not in 0 .. %d", k, HM_LIGHT_STATS_BINS - 1);
  if (edge != 0 && edge != 1) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: edge %d is not 0 (the code's light) or 1 (the upper edge of its bin)", edge);
  *nits = stats_code_nits(k, edge);
  return HM_OK;
}

int hm_stats_check_fraction(double fraction)
{
  if (!std::isfinite(fraction) || !(fraction > 0.0) || fraction > 1.0) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: fraction %g is not finite and in (0, 1]", fraction);
  return HM_OK;
}

int hm_stats_check_unit(float unit_nits)
{
  if (unit_nits != 0.0f && !nits_ok(unit_nits)) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: unit_nits %g is not finite, above 0 and at most 10000", (double)unit_nits);
  return HM_OK;
}

int hm_stats_unit_nits(const hm_light_plan* lp, float unit_nits, float* U) { return unit_nits_of("light statistics", lp, unit_nits, U); }

int hm_light_stats_percentile(const hm_light_stats* stats, double fraction, int32_t* code, float* nits)
{
  if (!stats) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const int rc = hm_stats_check_fraction(fraction);
  if (rc) return rc;
  if (stats->pixels == 0) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: a statistic of no pixels has no percentile");
  const uint64_t rank = std::min(std::max((uint64_t)std::ceil(fraction * (double)stats->pixels), (uint64_t)1), stats->pixels);
  uint64_t below = 0;
  int k = 0;
  for (; k < HM_LIGHT_STATS_BINS - 1; k++)
    if ((below += stats->hist[k]) >= rank) break; // (a histogram that sums to less than pixels: the last bin)
  if (code) *code = k;
  if (nits) *nits = (float)stats_code_nits(k, 1);
  return HM_OK;
}

int hm_light_stats_average(const hm_light_stats* stats, float* nits)
{
  if (!stats || !nits) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (stats->pixels == 0) return hm_fail(HM_ERR_INVALID_ARG, "light statistics: a statistic of no pixels has no average");
  double sum = 0.0;
  for (int k = 0; k < HM_LIGHT_STATS_BINS; k++) sum += (double)stats->hist[k] * stats_code_nits(k, 0);
  *nits = (float)(sum / (double)stats->pixels);
  return HM_OK;
}

hm_device_dest hm_stats_stand_in_dest(void)
{
  hm_device_dest d;
  std::memset(&d, 0, sizeof(d));
  d.ptr = reinterpret_cast<void*>((uintptr_t)256); d.len = ~(uint64_t)0 >> 1; // (never written, never asked whether it is device memory)
  d.layout = HM_DEV_LAYOUT_HWC; d.dtype = HM_DEV_F32;
  for (int c = 0; c < 4; c++) d.scale[c] = 1.0f;
  return d;
}

int hm_launch_light_stats(const hm_out_plan* p, float U, const void* src, int src_stride, hipStream_t s, hm_light_stats* out)
{
  if (!p->has_light || !out) return hm_fail(HM_ERR_INTERNAL, "light statistics: no light step in the plan");
  const hm_view_plan* vp = &p->vp;
  const int obpp = hm_out_bytes_per_pixel(p->out_format), src_bytes = obpp >= 6 ? 2 : 1, channels = obpp / src_bytes;
  const uint8_t* origin = (const uint8_t*)src + (size_t)vp->y * src_stride + (size_t)vp->x * obpp;
  // lin and the OOTF tables as the write has them (of the tone step only thr, and for U: the one filled here behind them)
  hm_light_plan lp = p->lp;
  lp.encode = 0; lp.tone = 0;
  const LightTables T(&lp);
  const size_t table_floats = T.bytes() / sizeof(float), words = HM_LIGHT_STATS_BINS + 2;
  const size_t bytes = (table_floats + HM_TONE_STEPS + words) * 4;
  hm_light_args la = T.args(src_bytes);
  int rc = hm_light_lds_check(lp.bits, lp.enc_bits, 0, lp.ootf ? 2 : 0, lp.lin3, 3);
  if (rc) return rc;
  StatsBlocks b;
  if (!(b.pinned = hm_pool_pinned_alloc(bytes))) return hm_fail(HM_ERR_NOMEM, "out of memory");
  if (!(b.dev = hm_pool_device_alloc(bytes))) return HM_ERR_NO_DEVICE;
  float* host = (float*)b.pinned;
  T.fill(host);
  fill_tone_tables((double)lp.gain, 0.0, 0.0, (double)U, 0.0, host + table_floats, nullptr);
  float* dev = (float*)b.dev;
  unsigned* dev_words = reinterpret_cast<unsigned*>(dev + table_floats + HM_TONE_STEPS);
  const uint32_t* host_words = reinterpret_cast<const uint32_t*>(host + table_floats + HM_TONE_STEPS);
  T.point(&la, dev);
  la.tone = dev + table_floats;
  // (from here on the blocks are in use by the stream: every way out waits for it)
  rc = hm_check_hip(hipMemcpyAsync(dev, host, (table_floats + HM_TONE_STEPS) * 4, hipMemcpyHostToDevice, s), "upload of the statistics' tables");
  if (!rc) rc = hm_check_hip(hipMemsetAsync(dev_words, 0, words * 4, s), "zeroing of the statistics' counters");
  if (!rc) rc = hm_launch_light_stats_kernel(&la, channels, origin, src_stride, vp->w, vp->h, dev_words, s);
  if (!rc) rc = hm_check_hip(hipMemcpyAsync(const_cast<uint32_t*>(host_words), dev_words, words * 4, hipMemcpyDeviceToHost, s), "download of the statistics' counters");
  const hipError_t e = hipStreamSynchronize(s);
  if (!rc && e != hipSuccess) rc = hm_check_hip(e, "k_light_stats execution");
  if (rc) return rc;
  hm_light_stats st;
  std::memset(&st, 0, sizeof(st));
  for (int k = 0; k < HM_LIGHT_STATS_BINS; k++) {
    st.hist[k] = host_words[k];
    st.pixels += host_words[k];
    if (host_words[k]) st.max_code = k;
  }
  if (st.pixels != (uint64_t)vp->w * (uint64_t)vp->h)
    return hm_fail(HM_ERR_INTERNAL, "light statistics: %llu pixels counted of %d x %d", (unsigned long long)st.pixels, vp->w, vp->h);
  std::memcpy(&st.max_norm, &host_words[HM_LIGHT_STATS_BINS], sizeof(float));
  st.max_nits = (float)((double)st.max_norm * (double)U / (double)lp.gain);
  if ((rc = hm_light_stats_average(&st, &st.average_nits))) return rc;
  *out = st;
  return HM_OK;
}

int hm_light_stats_of_tensor(int out_format, int bits, int src_w, int src_h, const void* d_src, int src_stride, const hm_device_view* view, const hm_device_light* light,
                             const hm_device_ootf* ootf, float unit_nits, hm_light_stats* out, void* stream)
{
  if (!d_src || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const hm_out_steps st = {view, light, nullptr, nullptr, nullptr, ootf, nullptr, 0, HM_MEASURE_STATS};
  const hm_device_dest dest = hm_stats_stand_in_dest();
  int rc = hm_entry_steps(HM_ENTRY_STATS, st);
  if (!rc) rc = hm_entry_icc(st, "in a stand-alone entry that has no item: hm_decode_item_light_stats reads the item's profile");
  if (rc || (rc = hm_stats_check_unit(unit_nits)) || (rc = hm_out_check_static(out_format, &dest, &st, 1)) || (rc = check_image_size("", src_w, src_h))) return rc;
  const hm_out_image img = {src_w, src_h, bits, light->from_transfer, light->from_primaries, 0, 0, 0};
  hm_out_plan p;
  float U = 0.0f;
  if ((rc = hm_out_resolve(out_format, &img, HM_OUT_PROFILE_FIRST, &dest, &st, &p)) || (rc = hm_stats_unit_nits(&p.lp, unit_nits, &U))) return rc;
  const int obpp = hm_out_bytes_per_pixel(out_format);
  if (src_stride < src_w * obpp) return hm_fail(HM_ERR_INVALID_ARG, "src_stride %d below the bytes of a row", src_stride);
  if (obpp >= 6 && (((uintptr_t)d_src | (unsigned)src_stride) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  return hm_launch_light_stats(&p, U, d_src, src_stride, (hipStream_t)stream, out);
}

// ---- planar views: every plane an image of its own ------------------------------------------------------------------------------

int hm_planes_view_resolve(int chroma, int w, int h, const hm_device_view* v, hm_planes_view_plan* pv)
{
  if (!v || !pv) return hm_fail(HM_ERR_INVALID_ARG, "null view");
  std::memset(pv, 0, sizeof(*pv));
  if (chroma < HM_CHROMA_MONO || chroma > HM_CHROMA_444) return hm_fail(HM_ERR_INVALID_ARG, "planar view: chroma format %d", chroma);
  int rc = check_image_size("planar view: ", w, h);
  if (rc) return rc;
  hm_view_plan vp; // the luma rectangle: hm_device_view's own refusals (no target is big-endian here)
  if ((rc = hm_view_resolve(0, w, h, v, &vp))) return rc;
  const int bad = hm_pv_geometry(chroma, vp.x, vp.y, vp.w, vp.h, vp.ow, vp.oh, pv->crop, pv->out);
  if (bad == 1) return hm_fail(HM_ERR_INVALID_ARG, "planar view: crop_x %d is odd, the chroma planes of a 4:2:%d result have half the columns", vp.x, chroma == HM_CHROMA_420 ? 0 : 2);
  if (bad == 2) return hm_fail(HM_ERR_INVALID_ARG, "planar view: crop_y %d is odd, the chroma planes of a 4:2:0 result have half the rows", vp.y);
  pv->ow = vp.ow; pv->oh = vp.oh; pv->filter = vp.filter; pv->crop_only = vp.crop_only;
  if (chroma != HM_CHROMA_MONO) // the reduction limit holds per plane and axis (a chroma axis 255 -> 1 of a luma axis 509 -> 1 ...)
    if ((rc = check_axis(pv->crop[1][2], pv->out[1][0], pv->filter, "chroma width")) || (rc = check_axis(pv->crop[1][3], pv->out[1][1], pv->filter, "chroma height"))) return rc;
  return HM_OK;
}

int hm_planes_view_geometry(int chroma, int width, int height, const hm_device_view* view, int32_t crop[4][4], int32_t out[4][2])
{
  if (!view || !crop || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_planes_view_plan pv;
  const int rc = hm_planes_view_resolve(chroma, width, height, view, &pv);
  if (rc) return rc;
  std::memcpy(crop, pv.crop, sizeof(pv.crop));
  std::memcpy(out, pv.out, sizeof(pv.out));
  return HM_OK;
}

namespace {

// a frame of a planar view write against its destination: the plan of an ow x oh result, len and overlap, the pointers, the sources
int planes_view_check(const hm_planes_view_item& f, hm_planes_plan* p)
{
  int rc = hm_planes_resolve(f.chroma, f.bits, f.pv.ow, f.pv.oh, f.alpha_bits, f.planes, p);
  if (!rc) rc = hm_planes_check_len(f.planes, p);
  if (!rc) rc = hm_planes_check_pointer(f.planes, p);
  if (rc) return rc;
  const bool semi = p->layout == HM_DEV_PLANES_SEMI;
  for (int c = 0; c < 4; c++) {
    const bool need = c == 0 || (c == 3 ? p->pl[3].present != 0 : f.chroma != HM_CHROMA_MONO);
    if (!need) continue;
    const int sb = hm_sample_bytes(c == 3 ? p->alpha_bits : f.bits);
    if (!f.src[c]) return hm_fail(HM_ERR_INVALID_ARG, "device planes: source plane %d is null", c);
    if ((int64_t)f.stride[c] < ((int64_t)f.pv.crop[c][0] + f.pv.crop[c][2]) * sb) return hm_fail(HM_ERR_INVALID_ARG, "device planes: source stride %d of plane %d below the bytes of a row", f.stride[c], c);
    if (sb == 2 && (((uintptr_t)f.src[c] | (unsigned)f.stride[c]) & 1)) return hm_fail(HM_ERR_INVALID_ARG, "16-bit samples at an odd address or stride");
    // (the geometry gives every plane the size hm_planes_resolve gives it: the kernels store pv.out, the checks cover p->pl)
    const int dc = semi && c == 2 ? 1 : c;
    if (p->pl[dc].width != f.pv.out[c][0] || p->pl[dc].height != f.pv.out[c][1])
      return hm_fail(HM_ERR_INTERNAL, "planar view: plane %d is %d x %d, the destination's %d x %d", c, f.pv.out[c][0], f.pv.out[c][1], p->pl[dc].width, p->pl[dc].height);
  }
  return HM_OK;
}

const uint8_t* plane_origin(const hm_planes_view_item& f, int c, int sb)
{
  return (const uint8_t*)f.src[c] + (size_t)f.pv.crop[c][1] * f.stride[c] + (size_t)f.pv.crop[c][0] * sb;
}

// one group: frames idx[0 .. m) of `it` share the plan p and everything else of the key
int planes_view_group(const hm_planes_view_item* it, const int* idx, int m, const hm_planes_plan& p, hipStream_t s, hm_view_scratch* sc)
{
  const hm_planes_view_item& f0 = it[idx[0]];
  const hm_planes_view_plan& pv = f0.pv;
  const hm_device_planes* d0 = f0.planes;
  const bool semi = p.layout == HM_DEV_PLANES_SEMI, nearest = pv.filter == HM_VIEW_NEAREST;
  const int present[4] = {1, p.chroma != HM_CHROMA_MONO, p.chroma != HM_CHROMA_MONO, p.pl[3].present};
  int sb[4];
  for (int c = 0; c < 4; c++) sb[c] = hm_sample_bytes(c == 3 ? p.alpha_bits : p.bits);
  // the tap tables: one per distinct (n -> m) axis - luma x, luma y, chroma x, chroma y at the most (alpha has luma's)
  struct Axis { int n, m, taps; size_t at; };
  std::vector<Axis> axes;
  int ax[4] = {0, 0, 0, 0}, ay[4] = {0, 0, 0, 0}, rc;
  size_t words = 0;
  auto axis_of = [&](int n, int mm) -> int {
    for (size_t a = 0; a < axes.size(); a++)
      if (axes[a].n == n && axes[a].m == mm) return (int)a;
    int taps = 0, f;
    for (int j = 0; j < mm; j++) { const int cnt = axis_taps(n, mm, pv.filter, j, &f, nullptr); if (cnt < 0) return cnt; taps = std::max(taps, cnt); }
    axes.push_back({n, mm, taps, words});
    words += (size_t)mm * (2 + taps);
    return (int)axes.size() - 1;
  };
  if (!nearest)
    for (int c = 0; c < 4; c++) {
      if (!present[c]) continue;
      if ((ax[c] = axis_of(pv.crop[c][2], pv.out[c][0])) < 0) return ax[c];
      if ((ay[c] = axis_of(pv.crop[c][3], pv.out[c][1])) < 0) return ay[c];
    }
  // ONE pinned block and one upload: the tables, then the frames' pointer records
  const hm_pv_block lay = hm_pv_block_layout((int64_t)words, m);
  uint8_t* host = (uint8_t*)hm_pool_pinned_alloc((size_t)lay.bytes);
  if (!host) return hm_fail(HM_ERR_NOMEM, "out of memory");
  sc->pinned = host;
  float w[HM_VIEW_MAX_TAPS + 2];
  for (const Axis& a : axes) {
    int32_t* base = reinterpret_cast<int32_t*>(host) + a.at;
    float* wt = reinterpret_cast<float*>(base + 2 * (size_t)a.m);
    for (int j = 0; j < a.m; j++) {
      const int cnt = axis_taps(a.n, a.m, pv.filter, j, &base[j], w);
      base[a.m + j] = cnt;
      for (int i = 0; i < a.taps; i++) wt[(size_t)i * a.m + j] = i < cnt ? w[i] : 0.0f;
    }
  }
  hm_pv_rec* recs = reinterpret_cast<hm_pv_rec*>(host + lay.rec_off);
  for (int i = 0; i < m; i++) {
    const hm_planes_view_item& f = it[idx[i]];
    std::memset(&recs[i], 0, sizeof(recs[i]));
    for (int c = 0; c < 4; c++) {
      if (present[c]) recs[i].src[c] = (uint64_t)(uintptr_t)plane_origin(f, c, sb[c]);
      if (p.pl[c].present) recs[i].dst[c] = (uint64_t)(uintptr_t)f.planes->plane[c].ptr;
    }
  }
  // the intermediate of one chunk of frames, reused chunk after chunk in stream order
  int64_t off[4], pitch[4];
  const int64_t frame_stride = hm_pv_tmp_layout(pv.crop, pv.out, present, off, pitch);
  const int per_chunk = (int)std::min<int64_t>(m, nearest ? HM_PV_Z_MOST : hm_pv_chunk_frames(frame_stride, hm_knob(HM_KNOB_VIEW_BATCH_BYTES)));
  if (!(sc->dev[0] = hm_pool_device_alloc((size_t)lay.bytes))) return HM_ERR_NO_DEVICE;
  if (!nearest && !(sc->dev[1] = hm_pool_device_alloc((size_t)frame_stride * per_chunk * sizeof(float)))) return HM_ERR_NO_DEVICE;
  if ((rc = hm_check_hip(hipMemcpyAsync(sc->dev[0], host, (size_t)lay.bytes, hipMemcpyHostToDevice, s), "upload of the tap tables"))) return rc;
  const int32_t* dtab = (const int32_t*)sc->dev[0];
  const hm_pv_rec* drecs = reinterpret_cast<const hm_pv_rec*>((const uint8_t*)sc->dev[0] + lay.rec_off);
  auto axis_at = [&](int a) {
    hm_pv_axis t;
    const int32_t* base = dtab + axes[(size_t)a].at;
    t.first = base; t.count = base + axes[(size_t)a].m; t.weights = reinterpret_cast<const float*>(base + 2 * (size_t)axes[(size_t)a].m);
    return t;
  };
  hm_pv_h_args ha;
  hm_pv_v_args va;
  std::memset(&ha, 0, sizeof(ha));
  std::memset(&va, 0, sizeof(va));
  int h_end = 0, v_end = 0;
  for (int c = 0; c < 4; c++) {
    if (present[c] && !nearest) {
      hm_pv_src_desc& sd = ha.pl[c];
      sd.ax = axis_at(ax[c]);
      sd.tmp_off = off[c]; sd.tmp_pitch = pitch[c];
      sd.stride = f0.stride[c]; sd.n_h = pv.crop[c][3]; sd.ow = pv.out[c][0]; sd.sample_bytes = sb[c];
      h_end += (sd.n_h + 3) / 4;
    }
    ha.y_end[c] = h_end;
    if (p.pl[c].present) {
      hm_pv_dst_desc& dd = va.pl[c];
      const bool pair = semi && c == 1;
      if (!nearest) dd.ay = axis_at(ay[c]);
      dd.pitch = p.pl[c].pitch;
      dd.tmp_off0 = off[c]; dd.tmp_off1 = pair ? off[2] : 0; dd.tmp_pitch = pitch[c];
      dd.w = pv.out[c][0]; dd.oh = pv.out[c][1];
      dd.pair = pair ? 1 : 0; dd.vec = p.pl[c].vec;
      const int sbits = c == 3 ? p.alpha_bits : p.bits;
      dd.peak = (1 << sbits) - 1; dd.shift = d0->msb_aligned ? 16 - sbits : 0;
      dd.n_w = pv.crop[c][2]; dd.n_h = pv.crop[c][3]; dd.stride0 = f0.stride[c]; dd.stride1 = pair ? f0.stride[2] : 0; dd.sample_bytes = sb[c];
      dd.scale0 = d0->scale[c]; dd.bias0 = d0->bias[c];
      if (pair) { dd.scale1 = d0->scale[2]; dd.bias1 = d0->bias[2]; }
      v_end += (dd.oh + 3) / 4;
    }
    va.y_end[c] = v_end;
  }
  ha.tmp = (float*)sc->dev[1]; va.tmp = (const float*)sc->dev[1];
  ha.frame_stride = va.frame_stride = frame_stride;
  for (int c0 = 0; c0 < m; c0 += per_chunk) {
    const int frames = std::min(per_chunk, m - c0);
    ha.recs = va.recs = drecs + c0;
    if ((rc = nearest ? hm_launch_planes_view_nearest(&va, p.dtype, frames, s) : hm_launch_planes_resample(&ha, &va, sb[0], p.dtype, frames, s))) return rc;
  }
  return HM_OK;
}

} // namespace

int hm_planes_view_write(hm_planes_view_item* it, int n, hipStream_t s, hm_view_scratch* sc, int* failed)
{
  if (failed) *failed = -1;
  if (n <= 0) return HM_OK;
  std::vector<hm_planes_plan> plans((size_t)n);
  for (int k = 0; k < n; k++) { // every destination and source, before anything is queued
    const int rc = planes_view_check(it[k], &plans[k]);
    if (rc) { if (failed) *failed = k; return rc; }
    for (int c = 0; c < 4; c++) it[k].pitches[c] = plans[k].pl[c].present ? plans[k].pl[c].pitch : 0;
  }
  std::vector<hm_pv_key> keys;
  std::vector<std::vector<int>> members;
  for (int k = 0; k < n; k++) {
    const hm_planes_view_item& f = it[k];
    const hm_planes_plan& p = plans[k];
    if (f.pv.crop_only) { // the samples of the rectangles: k_planes_to_tensor on the offset source planes, no intermediate
      const void* src[4] = {nullptr, nullptr, nullptr, nullptr};
      for (int c = 0; c < 4; c++) {
        const bool need = c == 0 || (c == 3 ? p.pl[3].present != 0 : f.chroma != HM_CHROMA_MONO);
        if (need) src[c] = plane_origin(f, c, hm_sample_bytes(c == 3 ? p.alpha_bits : f.bits));
      }
      const int rc = hm_planes_write(f.planes, f.chroma, f.bits, f.pv.ow, f.pv.oh, p.alpha_bits, src, f.stride, s, nullptr);
      if (rc) { if (failed) *failed = k; return rc; }
      continue;
    }
    hm_pv_key key;
    std::memset(&key, 0, sizeof(key));
    key.chroma = p.chroma; key.bits = p.bits; key.alpha_bits = p.alpha_bits; key.filter = f.pv.filter;
    key.layout = p.layout; key.dtype = p.dtype; key.msb_aligned = f.planes->msb_aligned;
    std::memcpy(key.crop, f.pv.crop, sizeof(key.crop));
    std::memcpy(key.out, f.pv.out, sizeof(key.out));
    for (int c = 0; c < 4; c++) {
      const bool need = c == 0 || (c == 3 ? p.pl[3].present != 0 : f.chroma != HM_CHROMA_MONO);
      key.stride[c] = need ? f.stride[c] : 0;
      if (!p.pl[c].present) continue;
      key.pitch[c] = p.pl[c].pitch;
      key.vec[c] = hm_pv_vec_class((uintptr_t)f.planes->plane[c].ptr, p.pl[c].pitch);
    }
    std::memcpy(key.scale, f.planes->scale, 16);
    std::memcpy(key.bias, f.planes->bias, 16);
    size_t g = 0;
    while (g < keys.size() && !hm_pv_key_equal(&keys[g], &key)) g++;
    if (g == keys.size()) { keys.push_back(key); members.emplace_back(); }
    members[g].push_back(k);
  }
  for (const std::vector<int>& m : members) { // (a group's blocks hang on the scratch entry of its first frame: unused otherwise)
    const int rc = planes_view_group(it, m.data(), (int)m.size(), plans[(size_t)m[0]], s, &sc[m[0]]);
    if (rc) { if (failed) *failed = m[0]; return rc; }
  }
  return HM_OK;
}

int hm_resample_planes_to_tensor(int chroma, int bits, int width, int height, int alpha_bits, const void* const d_src[4], const int32_t src_stride[4],
                                 const hm_device_view* view, const hm_device_planes* planes, void* stream)
{
  if (!d_src || !src_stride || !view || !planes) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (alpha_bits < 0) return hm_fail(HM_ERR_INVALID_ARG, "device planes: alpha bit depth %d", alpha_bits);
  hm_planes_view_item f;
  std::memset(&f, 0, sizeof(f));
  int rc = hm_planes_check_static(planes);
  if (!rc) rc = hm_planes_view_resolve(chroma, width, height, view, &f.pv);
  if (rc) return rc;
  hm_planes_plan p;
  if ((rc = hm_planes_resolve(chroma, bits, f.pv.ow, f.pv.oh, alpha_bits, planes, &p)) || (rc = hm_planes_check_len(planes, &p))) return rc;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  f.planes = planes; f.chroma = chroma; f.bits = bits; f.alpha_bits = alpha_bits;
  for (int c = 0; c < 4; c++) { f.src[c] = d_src[c]; f.stride[c] = src_stride[c]; }
  return with_scratch((hipStream_t)stream, [&](hm_view_scratch* sc) { return hm_planes_view_write(&f, 1, (hipStream_t)stream, sc, nullptr); });
}

} // extern "C"
