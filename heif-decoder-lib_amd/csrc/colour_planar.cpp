// colour_planar.cpp — planar YCbCr targets (HM_OUT_YCBCR_*): the reference's chain for the request (colour_search.cpp) run
// operation by operation over device planes, the way ColorConversionPipeline::convert_image does it
// (colorconversion.cc:435-484) - each operation reads the image the one before it left, which carries that step's output
// state as its nclx.  The one fusion: Op_YCbCr_to_RGB directly followed by Op_RGB_to_YCbCr runs as one kernel that keeps the
// R, G, B samples in registers (planar.hip); HM_PLANAR_UNFUSED runs the pair over planar RGB instead.
//
// Compiled with -ffp-contract=off (the matrix coefficients are binary32 expressions of nclx.cc).
#include <cstring>

#include "hm_planar.h"
#include "hm_plane_geom.h"

namespace {

// the profile an operation finds on the image it is handed
struct Seen { int has_nclx, matrix, primaries, full_range; };

struct Run {
  const hm_planar_image* dst;
  std::vector<void*>* temps;
  bool last = false; // the operation being run is the chain's last one: what it writes goes to the caller's planes
  hipStream_t s;
  // where plane c of the image an operation produces goes: the caller's plane if this is the last operation, else a pool block
  int out_plane(hm_planar_image& img, int c, int w, int h, int bits)
  {
    const int stride = hm_plane_stride(w, hm_sample_bytes(bits));
    if (last && dst && dst->p[c]) {
      if (dst->stride[c] < w * hm_sample_bytes(bits)) return hm_fail(HM_ERR_INVALID_ARG, "stride smaller than row");
      img.p[c] = dst->p[c]; img.stride[c] = dst->stride[c];
      return HM_OK;
    }
    const size_t bytes = (size_t)stride * hm_padded_rows(h);
    void* p = hm_pool_device_alloc(bytes);
    if (!p) return hm_fail(HM_ERR_NOMEM, "planar colour chain: %zu bytes of device memory", bytes);
    temps->push_back(p);
    img.p[c] = p; img.stride[c] = stride;
    return HM_OK;
  }
};

// The chroma format Op_RGB_to_YCbCr produces: its step's output state (rgb2yuv.cc:62-77) - the target's, unless the caller insists
// on the preferred (averaging) down-sampling: then the op, which "only implements nearest neighbour", stays at 4:4:4 and
// Op_YCbCr444_to_YCbCr420/422_average follows
int rgb_to_ycbcr_chroma(const hm_colour_desc* d)
{
  return d->chroma_upsampling == HM_UPSAMPLE_BILINEAR ? (int)HM_CHROMA_444 : hm_out_planar_chroma(d->out_format);
}

int request_plan(const hm_colour_desc* d, int ops[HM_COLOUR_MAX_OPS], int* n)
{
  int rc = hm_colour_validate(d);
  if (rc) return rc;
  if (!hm_out_is_planar(d->out_format)) return hm_fail(HM_ERR_UNSUPPORTED, "output format %d is not a planar target", d->out_format);
  hm_colour_request rq;
  hm_colour_request_of(d, &rq);
  const int st = hm_colour_make_planar_plan(&rq, ops, n);
  if (st == HM_PLAN_NO_CHAIN) return hm_colour_no_chain(d);
  if (st != HM_PLAN_OK) {
    char chain[512];
    hm_colour_chain_string(ops, *n, chain, (int)sizeof(chain));
    return hm_fail(HM_ERR_UNSUPPORTED, "the reference's chain for %d-bit chroma format %d -> planar target 0x%x holds an operation outside the GPU path: %s",
                   d->bit_depth, d->chroma, d->out_format, chain);
  }
  return HM_OK;
}

} // namespace

int hm_colour_planar_check(const hm_colour_desc* d)
{
  int ops[HM_COLOUR_MAX_OPS], n = 0;
  return request_plan(d, ops, &n);
}

int hm_planar_convert(const hm_colour_desc* d, const hm_planar_image* src, const hm_planar_image* dst, hm_planar_image* res,
                      std::vector<void*>& temps, int flags, hipStream_t s)
{
  int ops[HM_COLOUR_MAX_OPS], n = 0;
  int rc = request_plan(d, ops, &n);
  if (rc) return rc;
  hm_planar_image cur = *src;
  cur.w = d->width; cur.h = d->height; cur.chroma = d->chroma; cur.bits = d->bit_depth;
  if (!cur.p[3]) cur.alpha_bits = 0;
  else if (!cur.alpha_bits) cur.alpha_bits = cur.bits;
  if (!cur.p[0] || (cur.chroma != HM_CHROMA_MONO && (!cur.p[1] || !cur.p[2]))) return hm_fail(HM_ERR_INVALID_ARG, "null device pointer");
  if ((d->has_alpha != 0) != (cur.p[3] != nullptr)) return hm_fail(HM_ERR_INVALID_ARG, "has_alpha and the alpha plane disagree");
  if (cur.stride[0] < cur.w * hm_sample_bytes(cur.bits) ||
      (cur.chroma != HM_CHROMA_MONO && (cur.stride[1] < hm_plane_w(cur.chroma, 1, cur.w) * hm_sample_bytes(cur.bits) || cur.stride[2] < hm_plane_w(cur.chroma, 1, cur.w) * hm_sample_bytes(cur.bits))) ||
      (cur.p[3] && cur.stride[3] < cur.w * hm_sample_bytes(cur.alpha_bits)))
    return hm_fail(HM_ERR_INVALID_ARG, "stride smaller than row");
  // the ops that copy the alpha plane copy it as samples of the picture's width (chroma_sampling.cc:223-231, yuv2rgb.cc:248-251),
  // Op_RGB_to_YCbCr refuses another depth (rgb2yuv.cc:111-113): one answer for every chain that does anything
  if (n > 0 && cur.p[3] && cur.alpha_bits != cur.bits) {
    for (int i = 0; i < n; i++)
      if (ops[i] == HM_OP_RGB_TO_YCBCR_8 || ops[i] == HM_OP_RGB_TO_YCBCR_16) {
        return hm_fail_detail(HM_ERR_UNSUPPORTED, HM_DETAIL_NO_COLOUR_CHAIN, "no colour conversion: Op_RGB_to_YCbCr returns no image for an alpha plane of another depth than the picture's");
      }
    return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with a %d-bit image and a planar target", cur.alpha_bits, cur.bits);
  }
  // step 0 reads the image's own nclx; every later step the output state of the step before it: the input profile with the
  // undefined values replaced (colorconversion.cc:452-455, 520-527), a fresh one behind Op_mono_to_YCbCr420 (monochrome.cc:26-49)
  Seen seen = {d->has_nclx != 0, d->matrix, d->primaries, d->full_range != 0};
  Seen state = {1, d->has_nclx ? d->matrix : 2, d->has_nclx ? d->primaries : 2, d->has_nclx ? (d->full_range != 0) : 1};
  if (state.matrix == 2) state.matrix = 6;
  if (state.primaries == 2) state.primaries = 1;
  const Seen target = state; // (Op_RGB_to_YCbCr reads the TARGET state's profile: rgb2yuv.cc:175-180)

  Run run{dst, &temps, false, s};
  for (int i = 0; i < n && !rc; i++) {
    run.last = i == n - 1;
    hm_planar_image out = cur;
    const int bps = hm_sample_bytes(cur.bits);
    switch (ops[i]) {
      case HM_OP_DROP_ALPHA_PLANE: // alpha.cc:25-52 (never on this path: a planar target keeps the alpha plane)
        out.p[3] = nullptr; out.alpha_bits = 0;
        break;
      case HM_OP_MONO_TO_YCBCR420: { // monochrome.cc:52-156: neutral chroma planes, Y and alpha copied
        out.chroma = HM_CHROMA_420;
        const int cw = hm_plane_w(out.chroma, 1, cur.w), chh = hm_plane_h(out.chroma, 1, cur.h);
        for (int c = 1; c <= 2 && !rc; c++) {
          if ((rc = run.out_plane(out, c, cw, chh, cur.bits))) break;
          const size_t bytes = (size_t)out.stride[c] * chh;
          const hipError_t e = bps == 1 ? hipMemsetAsync((void*)out.p[c], 128, bytes, s)
                                        : hipMemsetD16Async((hipDeviceptr_t)out.p[c], (unsigned short)(128 << (cur.bits - 8)), bytes / 2, s);
          rc = hm_check_hip(e, "neutral chroma plane");
        }
        state = {1, 6, 1, 1};
        break;
      }
      case HM_OP_TO_HDR_PLANES: case HM_OP_TO_SDR_PLANES: { // hdr_sdr.cc:52-105, 138-200: every plane, alpha included
        const bool up = ops[i] == HM_OP_TO_HDR_PLANES;
        const int nb = up ? d->bit_depth : 8; // (target bits of a planar request: the image's own depth, or 8)
        if (up ? cur.bits != 8 : cur.bits == 8) { rc = hm_fail(HM_ERR_INTERNAL, "depth change on planes of %d bits", cur.bits); break; }
        for (int c = 0; c < 4 && !rc; c++) {
          if (!cur.p[c]) continue;
          const int pw = (c == 0 || c == 3) ? cur.w : hm_plane_w(cur.chroma, 1, cur.w), ph = (c == 0 || c == 3) ? cur.h : hm_plane_h(cur.chroma, 1, cur.h);
          if ((rc = run.out_plane(out, c, pw, ph, nb))) break;
          rc = up ? hm_launch_to_hdr(cur.p[c], cur.stride[c], (void*)out.p[c], out.stride[c], pw, ph, nb, s)
                  : hm_launch_to_sdr(cur.p[c], cur.stride[c], (void*)out.p[c], out.stride[c], pw, ph, cur.bits, s);
        }
        out.bits = nb;
        if (out.p[3]) out.alpha_bits = nb;
        break;
      }
      case HM_OP_BILINEAR_420_8: case HM_OP_BILINEAR_420_16: case HM_OP_BILINEAR_422_8: case HM_OP_BILINEAR_422_16: { // chroma_sampling.cc:489-710, 766-933
        out.chroma = HM_CHROMA_444;
        for (int c = 1; c <= 2 && !rc; c++) {
          if ((rc = run.out_plane(out, c, cur.w, cur.h, cur.bits))) break;
          rc = hm_launch_upsample_bilinear(cur.bits, cur.chroma == HM_CHROMA_420, cur.p[c], cur.stride[c], (void*)out.p[c], out.stride[c], cur.w, cur.h, s);
        }
        break;
      }
      case HM_OP_AVERAGE_420_8: case HM_OP_AVERAGE_420_16: case HM_OP_AVERAGE_422_8: case HM_OP_AVERAGE_422_16: { // chroma_sampling.cc:77-236, 295-434
        const bool v420 = ops[i] == HM_OP_AVERAGE_420_8 || ops[i] == HM_OP_AVERAGE_420_16;
        out.chroma = v420 ? HM_CHROMA_420 : HM_CHROMA_422;
        const int cw = hm_plane_w(out.chroma, 1, cur.w), chh = hm_plane_h(out.chroma, 1, cur.h);
        if ((rc = run.out_plane(out, 1, cw, chh, cur.bits)) || (rc = run.out_plane(out, 2, cw, chh, cur.bits))) break;
        rc = hm_launch_average_down(cur.bits, v420, cur.p[1], cur.stride[1], cur.p[2], cur.stride[2], (void*)out.p[1], out.stride[1], (void*)out.p[2], out.stride[2],
                                    cur.w, cur.h, s);
        break;
      }
      case HM_OP_YCBCR_TO_RGB_8: case HM_OP_YCBCR_TO_RGB_16: { // yuv2rgb.cc:79-254
        hm_colour_desc img = *d;
        img.bit_depth = cur.bits; img.chroma = cur.chroma;
        img.y_stride = cur.stride[0]; img.cb_stride = cur.stride[1]; img.cr_stride = cur.stride[2];
        img.has_nclx = seen.has_nclx; img.matrix = seen.matrix; img.primaries = seen.primaries; img.full_range = seen.full_range;
        float cf[4];
        hm_ycbcr_coefficients(img.has_nclx, img.matrix, img.primaries, cf);
        const int m = img.has_nclx ? img.matrix : 2;
        const bool full = img.has_nclx ? img.full_range != 0 : true;
        const int mode = m == 0 ? (full ? 1 : 2) : (m == 8 ? 3 : 0);
        const bool fuse = !(flags & HM_PLANAR_UNFUSED) && i + 1 < n && (ops[i + 1] == HM_OP_RGB_TO_YCBCR_8 || ops[i + 1] == HM_OP_RGB_TO_YCBCR_16);
        if (!fuse) {
          void* rgb[3];
          const int stride = hm_plane_stride(cur.w, bps);
          for (int c = 0; c < 3 && !rc; c++) { // (never the chain's last operation: always pool blocks of one stride)
            const bool was_last = run.last; run.last = false;
            rc = run.out_plane(out, c, cur.w, cur.h, cur.bits);
            run.last = was_last;
            rgb[c] = (void*)out.p[c];
          }
          if (!rc) rc = hm_launch_ycbcr_to_rgb_planes(&img, cf, mode, cur.p[0], cur.p[1], cur.p[2], rgb, stride, s);
          out.chroma = HM_CHROMA_444;
          break;
        }
        // fused with the Op_RGB_to_YCbCr behind it
        i++;
        run.last = i == n - 1;
        out.chroma = rgb_to_ycbcr_chroma(d);
        const int cw = hm_plane_w(out.chroma, 1, cur.w), chh = hm_plane_h(out.chroma, 1, cur.h);
        if ((rc = run.out_plane(out, 0, cur.w, cur.h, cur.bits)) || (rc = run.out_plane(out, 1, cw, chh, cur.bits)) || (rc = run.out_plane(out, 2, cw, chh, cur.bits))) break;
        hm_to_ycbcr a;
        std::memset(&a, 0, sizeof(a));
        a.w = cur.w; a.h = cur.h; a.bits = cur.bits; a.chroma = out.chroma;
        a.matrix = target.matrix; a.primaries = target.primaries; a.full_range = target.full_range;
        for (int c = 0; c < 3; c++) { a.src[c] = cur.p[c]; a.src_stride[c] = cur.stride[c]; a.dst[c] = (void*)out.p[c]; a.dst_stride[c] = out.stride[c]; }
        a.ycbcr_src = &img; std::memcpy(a.src_coef, cf, sizeof(cf)); a.src_mode = mode;
        rc = hm_launch_to_ycbcr(&a, s);
        break;
      }
      case HM_OP_RGB_TO_YCBCR_8: case HM_OP_RGB_TO_YCBCR_16: { // rgb2yuv.cc:88-275: the target's chroma format and profile
        out.chroma = rgb_to_ycbcr_chroma(d);
        const int cw = hm_plane_w(out.chroma, 1, cur.w), chh = hm_plane_h(out.chroma, 1, cur.h);
        if ((rc = run.out_plane(out, 0, cur.w, cur.h, cur.bits)) || (rc = run.out_plane(out, 1, cw, chh, cur.bits)) || (rc = run.out_plane(out, 2, cw, chh, cur.bits))) break;
        hm_to_ycbcr a;
        std::memset(&a, 0, sizeof(a));
        a.w = cur.w; a.h = cur.h; a.bits = cur.bits; a.chroma = out.chroma;
        a.matrix = target.matrix; a.primaries = target.primaries; a.full_range = target.full_range;
        for (int c = 0; c < 3; c++) { a.src[c] = cur.p[c]; a.src_stride[c] = cur.stride[c]; a.dst[c] = (void*)out.p[c]; a.dst_stride[c] = out.stride[c]; }
        rc = hm_launch_to_ycbcr(&a, s);
        break;
      }
      default: rc = hm_fail(HM_ERR_INTERNAL, "planar colour chain: operation %d", ops[i]); break;
    }
    cur = out;
    seen = state;
  }
  if (rc) return rc;
  // the caller's planes: what the chain passed through untouched (luma and alpha of the chroma ops) is copied
  if (dst) {
    for (int c = 0; c < 4; c++) {
      if (!cur.p[c]) continue;
      if (!dst->p[c]) return hm_fail(HM_ERR_INVALID_ARG, "null device pointer (output plane %d)", c);
      if (cur.p[c] == dst->p[c]) continue;
      const int pw = (c == 0 || c == 3) ? cur.w : hm_plane_w(cur.chroma, 1, cur.w), ph = (c == 0 || c == 3) ? cur.h : hm_plane_h(cur.chroma, 1, cur.h);
      const size_t row = (size_t)pw * hm_sample_bytes(c == 3 ? cur.alpha_bits : cur.bits);
      if ((size_t)dst->stride[c] < row) return hm_fail(HM_ERR_INVALID_ARG, "stride smaller than row");
      const hipError_t e = hipMemcpy2DAsync((void*)dst->p[c], (size_t)dst->stride[c], cur.p[c], (size_t)cur.stride[c], row, (size_t)ph, hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return hm_check_hip(e, "plane copy");
      cur.p[c] = dst->p[c]; cur.stride[c] = dst->stride[c];
    }
  }
  *res = cur;
  return HM_OK;
}

extern "C" int hm_colour_convert_planar(const hm_colour_desc* d, const hm_planes* in, int in_alpha_bits, const hm_planes* out, int flags, void* stream)
{
  if (!d || !in || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_planar_image src, dst, res;
  for (int c = 0; c < 4; c++) { src.p[c] = in->plane[c]; src.stride[c] = in->stride[c]; dst.p[c] = out->plane[c]; dst.stride[c] = out->stride[c]; }
  src.alpha_bits = in_alpha_bits;
  hipStream_t s = (hipStream_t)stream;
  std::vector<void*> temps;
  int rc = hm_planar_convert(d, &src, &dst, &res, temps, flags, s);
  if (!temps.empty()) { // the temporaries go back to the pool once the stream is through with them
    const hipError_t e = hipStreamSynchronize(s);
    for (void* p : temps) hm_pool_device_free(p);
    if (!rc) rc = hm_check_hip(e, "planar colour chain");
  }
  return rc;
}
