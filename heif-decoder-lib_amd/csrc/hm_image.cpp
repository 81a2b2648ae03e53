// hm_image.cpp — image-level decode: HEIF item (single hvc1 image or 'grid') -> host pixels.
//
// MI355X replacement of HeifContext::decode_image_user / decode_image_planar /
// decode_full_grid_image (libheif/context.cc:1516-1600, 1729-1885, 2120-2404):
//   host threads   : box parsing + entropy decoding (hm_hevc_parse) of every tile
//   one GPU batch  : reconstruction, deblocking, SAO and the tile paste into the YCbCr canvas
//   one GPU kernel : convert_colorspace() on the whole canvas (colorconversion.cc:487-596)
//   one D2H copy   : into a host plane laid out like HeifPixelImage (pixelimage.cc:139-218)
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <thread>
#include <vector>

#include "clap.h"
#include "hm_image_job.h"
#include "hm_overlay.h"
#include "hm_planar.h"
#include "hm_plane_geom.h"
#include "hm_unci_layout.h"

using namespace hm_img;

namespace {

size_t plane_bytes(const DevPlane& p) { return (size_t)p.stride * hm_padded_rows(p.h); }
int alloc_plane(DevPlane& p, int w, int h, int bps)
{
  p.w = w; p.h = h; p.stride = hm_plane_stride(w, bps);
  return p.mem.alloc(plane_bytes(p));
}
// the planes of a w x h image of `chroma` at `bits`: Y, then Cb and Cr unless it is 4:0:0 (luma only)
int alloc_planes(DevPlane (&P)[3], int w, int h, int chroma, int bits)
{
  int rc = HM_OK;
  for (int c = 0; c < (chroma == 0 ? 1 : 3) && !rc; c++) rc = alloc_plane(P[c], hm_plane_w(chroma, c, w), hm_plane_h(chroma, c, h), hm_sample_bytes(bits));
  return rc;
}
// a batch picture's destination: planes P as a canvas_w x canvas_h canvas, the picture at its origin; x0, y0 and the nclx fields are the caller's to set
hm_tile_dest tile_dest_of(const DevPlane (&P)[3], int canvas_w, int canvas_h)
{
  hm_tile_dest d;
  std::memset(&d, 0, sizeof(d));
  for (int c = 0; c < 3; c++) { d.plane[c] = P[c].mem.p; d.pitch[c] = P[c].stride; }
  d.canvas_width = canvas_w; d.canvas_height = canvas_h;
  return d;
}
// A buffer that queued work may still use leaves its owner: `retired` keeps it alive until the caller has synchronised the stream
// (the pool may hand a freed buffer to another thread at once).
void retire(std::vector<std::unique_ptr<DevMem>>& retired, DevMem& m) { retired.emplace_back(new DevMem()); retired.back()->swap(m); }

int require_device()
{
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available"); }
  return HM_OK;
}

// a device plane of stride x rows (its padding included) into pinned host memory of its own, queued on `s`
int plane_to_host(const void* src, int stride, int rows, hipStream_t s, uint8_t** host, int32_t* host_stride)
{
  const size_t sz = (size_t)stride * hm_padded_rows(rows);
  *host = (uint8_t*)hm_pool_pinned_alloc(sz);
  if (!*host) return hm_fail(HM_ERR_NOMEM, "out of memory");
  *host_stride = stride;
  return hm_check_hip(hipMemcpyAsync(*host, src, sz, hipMemcpyDeviceToHost, s), "D2H");
}

// The colour chain's request for a w x h picture of (bd, chroma) with profile `native`: has_nclx is the caller's to say (a grid
// canvas carries none).  P: the planes whose strides the chain reads - NULL: the packed rule of planes that are not allocated yet.
// obpp: bytes per pixel of an interleaved target (out_stride), 0 for a planar one; planar_8bit: convert_hdr_to_8bit travels in the
// planar out_format as HM_OUT_YCBCR_8BIT.  has_alpha stays 0.
hm_colour_desc colour_desc(const hm_decode_params* params, int w, int h, int bd, int chroma, const hm::NclxProfile& native, int has_nclx, const DevPlane* P, int obpp,
                           bool planar_8bit = false)
{
  hm_colour_desc cd;
  std::memset(&cd, 0, sizeof(cd));
  cd.width = w; cd.height = h; cd.bit_depth = bd; cd.chroma = chroma;
  cd.has_nclx = has_nclx; cd.matrix = native.matrix; cd.primaries = native.primaries; cd.full_range = native.full_range;
  cd.out_format = params->out_format | (planar_8bit && params->convert_hdr_to_8bit ? HM_OUT_YCBCR_8BIT : 0);
  cd.chroma_upsampling = params->chroma_upsampling;
  if (P) { cd.y_stride = P[0].stride; cd.cb_stride = P[1].stride; cd.cr_stride = P[2].stride; }
  else {
    const int bps = hm_sample_bytes(bd);
    cd.y_stride = hm_plane_stride(w, bps);
    cd.cb_stride = cd.cr_stride = chroma ? hm_plane_stride(hm_plane_w(chroma, 1, w), bps) : 0;
  }
  if (obpp > 0) cd.out_stride = hm_plane_stride(w, obpp);
  return cd;
}

// Transformative properties of the item, applied to the decoded YCbCr planes in association order
// (context.cc:1957-2020): irot -> rotate_ccw, imir -> mirror_inplace, clap -> crop.
// The replaced buffers go to `retired` (retire).
int apply_transforms(const std::vector<hm::Transform>& list, DevPlane (&P)[3], int& img_w, int& img_h, int chroma, int bd, hipStream_t s,
                     std::vector<std::unique_ptr<DevMem>>& retired)
{
  const int bps = hm_sample_bytes(bd);
  for (const hm::Transform& t : list) {
    if (t.kind == hm::Transform::Rotate) {
      if (t.angle == 0) continue;
      // a 4:2:2 image rotated by 90 / 270 degrees keeps its chroma tag while its chroma planes swap their sizes
      // (pixelimage.cc:552-586): the reference's later colour ops then read outside the planes - refuse loudly
      if (chroma == 2 && t.angle != 180) return hm_fail(HM_ERR_UNSUPPORTED, "irot %d on a 4:2:2 image is undefined in the reference", t.angle);
      for (int c = 0; c < 3; c++) {
        if (!P[c].mem.p) continue; // monochrome
        DevPlane n;
        const bool sw = t.angle != 180;
        int rc = alloc_plane(n, sw ? P[c].h : P[c].w, sw ? P[c].w : P[c].h, bps);
        if (rc) return rc;
        if ((rc = hm_launch_rotate_ccw(bps, t.angle, P[c].mem.p, P[c].stride, P[c].w, P[c].h, n.mem.p, n.stride, s))) return rc;
        P[c].mem.swap(n.mem); P[c].w = n.w; P[c].h = n.h; P[c].stride = n.stride;
        retire(retired, n.mem);
      }
      if (t.angle != 180) { const int tmp = img_w; img_w = img_h; img_h = tmp; }
    }
    else if (t.kind == hm::Transform::Mirror) {
      if (bd != 8) return hm_fail(HM_ERR_UNSUPPORTED, "Can currently only mirror images with 8 bits per pixel"); // pixelimage.cc:748-752
      for (int c = 0; c < 3; c++) {
        if (!P[c].mem.p) continue;
        DevPlane n;
        int rc = alloc_plane(n, P[c].w, P[c].h, bps);
        if (rc) return rc;
        if ((rc = hm_launch_mirror(P[c].mem.p, P[c].stride, P[c].w, P[c].h, t.horizontal, n.mem.p, n.stride, s))) return rc;
        P[c].mem.swap(n.mem);
        retire(retired, n.mem);
      }
    }
    else {
      if (t.width_n > 0x7FFFFFFFu || t.width_d > 0x7FFFFFFFu || t.height_n > 0x7FFFFFFFu || t.height_d > 0x7FFFFFFFu ||
          t.hoff_d > 0x7FFFFFFFu || t.voff_d > 0x7FFFFFFFu)
        return hm_fail(HM_ERR_BITSTREAM, "clap: Exceeded supported value range."); // box.cc:3692-3701
      hm::Clap c;
      c.width = hm::Fraction((int32_t)t.width_n, (int32_t)t.width_d);
      c.height = hm::Fraction((int32_t)t.height_n, (int32_t)t.height_d);
      c.hoff = hm::Fraction(t.hoff_n, (int32_t)t.hoff_d);
      c.voff = hm::Fraction(t.voff_n, (int32_t)t.voff_d);
      if (!c.width.valid() || !c.height.valid() || !c.hoff.valid() || !c.voff.valid())
        return hm_fail(HM_ERR_BITSTREAM, "clap: invalid fractional number"); // box.cc:3709-3713
      int left = c.left_rounded(img_w), right = c.right_rounded(img_w), top = c.top_rounded(img_h), bottom = c.bottom_rounded(img_h);
      if (left < 0) left = 0;
      if (top < 0) top = 0;
      if (right >= img_w) right = img_w - 1;
      if (bottom >= img_h) bottom = img_h - 1;
      if (left > right || top > bottom) return hm_fail(HM_ERR_BITSTREAM, "Invalid clean aperture"); // context.cc:2004-2008
      for (int k = 0; k < 3; k++) { // HeifPixelImage::crop, pixelimage.cc:797-888: plane rectangle by integer scaling
        if (!P[k].mem.p) continue;
        const int pl = (int)((int64_t)left * P[k].w / img_w), pr = (int)((int64_t)right * P[k].w / img_w);
        const int pt = (int)((int64_t)top * P[k].h / img_h), pb = (int)((int64_t)bottom * P[k].h / img_h);
        DevPlane n;
        int rc = alloc_plane(n, pr - pl + 1, pb - pt + 1, bps);
        if (rc) return rc;
        const hipError_t e = hipMemcpy2DAsync(n.mem.p, n.stride, (const uint8_t*)P[k].mem.p + (size_t)pt * P[k].stride + (size_t)pl * bps,
                                              P[k].stride, (size_t)n.w * bps, n.h, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hm_check_hip(e, "clap copy");
        P[k].mem.swap(n.mem); P[k].w = n.w; P[k].h = n.h; P[k].stride = n.stride;
        retire(retired, n.mem);
      }
      img_w = right - left + 1;
      img_h = bottom - top + 1;
    }
  }
  return HM_OK;
}

// Host worker threads for the entropy decode, kept alive between calls (spawning 48 threads costs more than the
// 1.6 ms one tile takes).  Mirrors the reference's std::async tile fan-out (context.cc:2361-2401) with a fixed crew.
class Crew {
 public:
  static Crew& instance() { static Crew c; return c; }
  // runs fn(0..n-1 claimed dynamically by the workers) on up to `threads` threads incl. the caller; returns when all are done
  void run(int threads, const std::function<void()>& fn)
  {
    if (threads <= 1) { fn(); return; }
    std::unique_lock<std::mutex> call(call_mutex_); // one fan-out at a time: concurrent callers queue up here
    {
      std::lock_guard<std::mutex> g(m_);
      while ((int)workers_.size() < threads - 1 && workers_.size() < 255) workers_.emplace_back([this] { loop(); });
      job_ = &fn;
      wanted_ = threads - 1 < (int)workers_.size() ? threads - 1 : (int)workers_.size();
      started_ = 0; running_ = 0; ++generation_;
    }
    cv_.notify_all();
    fn(); // the caller works too
    std::unique_lock<std::mutex> g(m_);
    job_ = nullptr; // late workers must not start any more
    done_.wait(g, [this] { return running_ == 0; });
  }
  // the fan-out of n pieces of work over the crew: f(i, row_threads) for i = 0 .. n - 1, claimed dynamically, on min(host_threads, n)
  // threads.  Fewer pieces than threads (a single image, or an image and its alpha plane): row_threads > 1 is the share of the
  // threads left over each piece may use itself - the rows of a WPP-coded picture parsed in parallel (the reference's decoder
  // threads, decctx.cc:1004-1116).
  template <class F>
  static void for_each(int n, int host_threads, F&& f)
  {
    if (n <= 0) return;
    int nthreads = host_threads > 0 ? host_threads : 1;
    const int row_threads = nthreads > n ? nthreads / n : 1;
    if (nthreads > n) nthreads = n;
    std::atomic<int> next{0};
    instance().run(nthreads, [&]() {
      for (;;) {
        const int i = next.fetch_add(1);
        if (i >= n) break;
        f(i, row_threads);
      }
    });
  }

 private:
  Crew() = default;
  ~Crew()
  {
    { std::lock_guard<std::mutex> g(m_); quit_ = true; }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  void loop()
  {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> g(m_);
    for (;;) {
      cv_.wait(g, [&] { return quit_ || (generation_ != seen && job_ && started_ < wanted_); });
      if (quit_) return;
      seen = generation_;
      const std::function<void()>* job = job_;
      ++started_; ++running_;
      g.unlock();
      (*job)();
      g.lock();
      if (--running_ == 0) done_.notify_all();
    }
  }
  std::mutex call_mutex_, m_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::function<void()>* job_ = nullptr;
  int wanted_ = 0, started_ = 0, running_ = 0;
  uint64_t generation_ = 0;
  bool quit_ = false;
};

int fail_from(const hm::HeifError& e) { return e.detail ? hm_fail_detail(e.status, e.detail, e.message.c_str()) : hm_fail(e.status, "%s", e.message.c_str()); }

} // namespace

extern "C" {

int hm_file_open(const uint8_t* data, size_t size, hm_file** out)
{
  if (!data || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::unique_ptr<hm_file> f(new (std::nothrow) hm_file());
  if (!f) return hm_fail(HM_ERR_NOMEM, "out of memory");
  f->bytes.assign(data, data + size);
  hm::HeifError err;
  if (!f->file.parse(f->bytes.data(), f->bytes.size(), err)) return fail_from(err);
  *out = f.release();
  return HM_OK;
}

void hm_file_close(hm_file* f) { delete f; }

uint32_t hm_file_primary_item(const hm_file* f) { return f ? f->file.primary_id() : 0; }

int hm_file_top_level_images(const hm_file* f, uint32_t* ids, int max_ids)
{
  if (!f) return hm_fail(HM_ERR_INVALID_ARG, "null file");
  const std::vector<uint32_t> v = f->file.top_level_images();
  for (int i = 0; i < (int)v.size() && i < max_ids && ids; i++) ids[i] = v[i];
  return (int)v.size();
}

int hm_file_image_info(const hm_file* f, uint32_t id, hm_image_info* info)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  std::memset(info, 0, sizeof(*info));
  hm::HeifError err;
  const hm::Item* first = it;
  if (it->type == "grid") {
    hm::GridInfo g;
    if (!f->file.grid_info(id, g, err)) return fail_from(err);
    info->is_grid = 1;
    info->grid_rows = g.rows;
    info->grid_cols = g.cols;
    info->width = (int32_t)g.width;
    info->height = (int32_t)g.height;
    first = f->file.item(g.tiles[0]);
    if (!first) return hm_fail(HM_ERR_BITSTREAM, "grid tile item missing");
    info->tile_width = first->props.ispe_width;
    info->tile_height = first->props.ispe_height;
  }
  else if (it->type == "hvc1") {
    info->width = it->props.ispe_width;
    info->height = it->props.ispe_height;
  }
  else if (it->type == "iden" || it->type == "iovl") {
    // a derived item: the size its 'ispe' declares; depth and chroma format are those of its first non-virtual child, found
    // through the first 'dimg' reference of every derived item on the way (context.cc:1377-1407)
    if (it->props.ispe_width <= 0 || it->props.ispe_height <= 0) return hm_fail(HM_ERR_BITSTREAM, "Image has no 'ispe' property");
    info->width = it->props.ispe_width;
    info->height = it->props.ispe_height;
    uint32_t cur = id;
    for (int depth = 0;; depth++) {
      const hm::Item* ci = f->file.item(cur);
      if (!ci) return hm_fail(HM_ERR_BITSTREAM, "derived image references the missing item %u", cur);
      if (ci->type != "grid" && ci->type != "iden" && ci->type != "iovl") { first = ci; break; }
      if (depth > HM_OVL_MAX_DEPTH + 1) return hm_fail(HM_ERR_BITSTREAM, "derived images nested deeper than %d", HM_OVL_MAX_DEPTH);
      const std::vector<uint32_t> refs = f->file.references(cur, "dimg");
      if (refs.empty() || refs[0] == cur) return hm_fail(HM_ERR_BITSTREAM, "Derived image does not reference any other image items");
      cur = refs[0];
    }
    if (first->type != "hvc1") return hm_fail(HM_ERR_UNSUPPORTED, "item type '%s' under a derived image is not an HEVC image", first->type.c_str());
  }
  else if (it->is_raw_leaf()) { // (a mask image: the monochrome 8-bit item HeifFile::unci_info makes of it)
    hm_unci_info u;
    if (!f->file.unci_info(id, u, err)) return fail_from(err);
    info->width = u.width; info->height = u.height;
    // the depth of the Y component, otherwise the largest of the M / R / G / B depths (get_luma_bits_per_pixel_from_configuration_unci,
    // codecs/uncompressed_image.cc:320-370)
    int luma = 0, other = 0;
    for (int c = 0; c < u.n_components; c++) {
      const int t = u.comp[c].type, d = u.comp[c].depth;
      if (t == HM_UNCI_TYPE_Y) luma = std::max(luma, d);
      else if (t == HM_UNCI_TYPE_MONO || (t >= HM_UNCI_TYPE_R && t <= HM_UNCI_TYPE_B)) other = std::max(other, d);
      if (t == HM_UNCI_TYPE_ALPHA) info->has_alpha = 1;
    }
    info->bit_depth = luma ? luma : other ? other : 8;
    info->chroma = u.colour_space == HM_UNCI_MONO ? HM_CHROMA_MONO : u.colour_space == HM_UNCI_RGB ? HM_CHROMA_444 :
                   u.sampling == HM_UNCI_SAMPLING_420 ? HM_CHROMA_420 : u.sampling == HM_UNCI_SAMPLING_422 ? HM_CHROMA_422 : HM_CHROMA_444;
    info->tile_width = (int32_t)u.tile_width; info->tile_height = (int32_t)u.tile_height;
  }
  else return hm_fail(HM_ERR_UNSUPPORTED, "item type '%s' is not an HEVC image, a grid, a derived image or an uncompressed image", it->type.c_str());
  const bool unci = it->is_raw_leaf();
  if (!unci) {
    if (!first->props.hvcc.present) return hm_fail(HM_ERR_BITSTREAM, "image without hvcC");
    info->bit_depth = first->props.hvcc.bit_depth_luma;
    info->chroma = first->props.hvcc.chroma_format;
  }
  info->has_transforms = (it->props.has_irot || it->props.has_imir || it->props.has_clap) ? 1 : 0;
  if (!unci) info->has_alpha = f->file.alpha_item_of(id) != 0;
  if (it->type == "iden" || it->type == "iovl") info->has_alpha = 0; // (context.cc:1370-1373)
  if (!info->has_alpha && it->type == "grid") { // (context.cc:1303-1368: a grid has alpha if one of its tiles has)
    hm::GridInfo g;
    hm::HeifError e2;
    if (f->file.grid_info(id, g, e2))
      for (uint32_t t : g.tiles)
        if (f->file.alpha_item_of(t)) info->has_alpha = 1;
  }
  info->has_nclx = (it->props.colr.present || (it != first && first->props.colr.present)) ? 1 : 0;
  info->coded_width = info->width; info->coded_height = info->height;
  // the size an image handle reports (context.cc:810-838): every clap sets it to the rounded aperture size,
  // a 90 / 270 degree irot swaps it, in property order
  for (const hm::Transform& t : it->props.transforms) {
    if (t.kind == hm::Transform::CleanAperture && t.width_d && t.height_d && t.width_n <= 0x7FFFFFFFu && t.width_d <= 0x7FFFFFFFu &&
        t.height_n <= 0x7FFFFFFFu && t.height_d <= 0x7FFFFFFFu) {
      info->width = hm::Fraction((int32_t)t.width_n, (int32_t)t.width_d).round();
      info->height = hm::Fraction((int32_t)t.height_n, (int32_t)t.height_d).round();
    }
    else if (t.kind == hm::Transform::Rotate && (t.angle == 90 || t.angle == 270)) {
      const int32_t tmp = info->width; info->width = info->height; info->height = tmp;
    }
  }
  return HM_OK;
}

uint32_t hm_file_alpha_item(const hm_file* f, uint32_t id) { return f ? f->file.alpha_item_of(id) : 0; }

int hm_file_item_hevc_data(const hm_file* f, uint32_t id, uint8_t** out, size_t* out_size)
{
  if (!f || !out || !out_size) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::vector<uint8_t> v;
  hm::HeifError err;
  if (!f->file.hevc_data(id, v, err)) return fail_from(err);
  uint8_t* mem = (uint8_t*)std::malloc(v.size() ? v.size() : 1);
  if (!mem) return hm_fail(HM_ERR_NOMEM, "out of memory");
  std::memcpy(mem, v.data(), v.size());
  *out = mem;
  *out_size = v.size();
  return HM_OK;
}

int hm_file_item_icc(const hm_file* f, uint32_t id, int for_handle, uint32_t* type, const uint8_t** data, size_t* size)
{
  if (!f || !type || !data || !size) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  *type = 0; *data = nullptr; *size = 0;
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  const hm::Item* src = it;
  if (it->type == "grid") {
    if (!for_handle) return HM_OK; // the grid canvas carries no profile
    if (!it->props.icc_type) { // inherited from the first tile
      hm::GridInfo g;
      hm::HeifError err;
      if (f->file.grid_info(id, g, err) && !g.tiles.empty()) src = f->file.item(g.tiles[0]);
      if (!src) return HM_OK;
    }
  }
  if (src->props.icc_type) { *type = src->props.icc_type; *data = src->props.icc.data(); *size = src->props.icc.size(); }
  return HM_OK;
}

void hm_host_free(void* plane) { hm_pool_pinned_free(plane); }

void hm_decoded_free(hm_decoded* d)
{
  if (!d) return;
  for (int c = 0; c < 3; c++) { hm_pool_pinned_free(d->plane[c]); d->plane[c] = nullptr; }
  hm_pool_pinned_free(d->alpha);
  d->alpha = nullptr;
}

} // extern "C"

namespace {

// apply_transforms on ONE plane of a w x h image (an alpha plane, a plane at a depth of its own): as the luma plane of a monochrome image
int apply_transforms_plane(const std::vector<hm::Transform>& list, DevPlane& p, int& w, int& h, int bd, hipStream_t s, std::vector<std::unique_ptr<DevMem>>& retired)
{
  DevPlane one[3];
  one[0].mem.swap(p.mem); one[0].w = p.w; one[0].h = p.h; one[0].stride = p.stride;
  const int rc = apply_transforms(list, one, w, h, 0, bd, s, retired);
  p.mem.swap(one[0].mem); p.w = one[0].w; p.h = one[0].h; p.stride = one[0].stride;
  return rc;
}

// HM_TRACE=1: wall-clock laps of the phases on stderr (diagnostics; the environment is read once)
bool trace_enabled()
{
  static const bool on = std::getenv("HM_TRACE") != nullptr;
  return on;
}
// (... and marks on one clock for everything a call spreads over threads)
void trace_mark(const char* what, int k = -1)
{
  if (!trace_enabled()) return;
  static const std::chrono::steady_clock::time_point base = std::chrono::steady_clock::now();
  std::fprintf(stderr, "[hm trace] %10.3f ms  %s %d\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - base).count(), what, k);
}
struct Lap {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* what) const
  {
    if (trace_enabled())
      std::fprintf(stderr, "[hm_decode_item] %-32s %8.3f ms\n", what,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// which coded pictures an image item consists of (context.cc:2120-2160: grid descriptor + dimg references)
// self_grid: an hvc1 item as the 1 x 1 grid of itself (ItemPlan::self_grid)
int plan_item(const hm_file* f, uint32_t id, ItemPlan& P, bool self_grid = false)
{
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  hm::HeifError err;
  P.id = id;
  P.is_grid = it->type == "grid";
  P.self_grid = false;
  if (P.is_grid) {
    hm::GridInfo g;
    if (!f->file.grid_info(id, g, err)) return fail_from(err);
    P.canvas_w = (int)g.width;
    P.canvas_h = (int)g.height;
    P.cols = g.cols; P.rows = g.rows;
    P.tiles.resize(g.tiles.size());
    for (size_t i = 0; i < g.tiles.size(); i++) {
      P.tiles[i].id = g.tiles[i];
      const hm::Item* ti = f->file.item(g.tiles[i]);
      if (ti && ti->type == "unci") return hm_fail(HM_ERR_UNSUPPORTED, "grid tile %zu (item %u) is an uncompressed ('unci') item: only coded HEVC images are grid tiles here", i, g.tiles[i]);
      if (ti && ti->is_mask()) return hm_fail(HM_ERR_UNSUPPORTED, "grid tile %zu (item %u) is a mask ('mski') item: only coded HEVC images are grid tiles here", i, g.tiles[i]);
    }
  }
  else if (it->type == "hvc1") {
    P.tiles.resize(1); P.tiles[0].id = id; P.cols = P.rows = 1;
    if (self_grid) { P.is_grid = P.self_grid = true; P.canvas_w = it->props.ispe_width; P.canvas_h = it->props.ispe_height; }
  }
  else if (it->type == "iden" || it->type == "iovl")
    return hm_fail(HM_ERR_UNSUPPORTED, "derived image item ('%s') is not supported by the pipeline and sequence calls: decode it with hm_decode_item", it->type.c_str());
  else if (it->type == "tmap")
    return hm_fail(HM_ERR_UNSUPPORTED, "a 'tmap' item (a base image with a gain map) is not an image of its own: render it with hm_decode_item_to_device_gain");
  else return hm_fail(HM_ERR_UNSUPPORTED, "item type '%s'", it->type.c_str());
  if (P.canvas_w < 0 || P.canvas_h < 0 || (P.is_grid && (P.canvas_w == 0 || P.canvas_h == 0))) return hm_fail(HM_ERR_BITSTREAM, "bad grid size");
  if (P.tiles.empty()) return hm_fail(HM_ERR_BITSTREAM, "image without coded pictures");
  const size_t nt = P.tiles.size();
  // alpha auxiliary images of grid tile items: decode_image_planar attaches them to the tile image (context.cc:2029-2078)
  P.tile_alpha.clear();
  if (P.is_grid && !P.self_grid)
    for (size_t i = 0; i < nt; i++) {
      const uint32_t a = f->file.alpha_item_of(P.tiles[i].id);
      if (!a) continue;
      const hm::Item* ai = f->file.item(a);
      if (!ai || ai->type != "hvc1") return hm_fail(HM_ERR_UNSUPPORTED, "alpha image of grid tile %zu is not a coded HEVC image", i);
      P.tile_alpha.push_back({(int)i, a});
    }
  P.reset_slots();
  return HM_OK;
}

// the failure of a coded picture whose entropy decode (or data) failed, as the image decode reports it: its wording, and the failure
std::string tile_failure_text(const ItemPlan& P, int i) { return "tile " + std::to_string(i) + " (item " + std::to_string(P.tiles[i].id) + "): " + P.messages[i]; }
int tile_failure(const ItemPlan& P, int i) { return hm_fail(P.status[i], "%s", tile_failure_text(P, i).c_str()); }
// HM_WARN_CONCEALED if one of the parsed pictures [first, first + n) of P holds concealed CTBs (damaged slice data, HM_PARSE_CONCEAL)
int concealed_warning(const ItemPlan& P, int first, int n)
{
  for (int i = first; i < first + n; i++)
    if (P.blobs[i].p && hm_pic_of(P.blobs[i].p)->concealed_ctbs) return HM_WARN_CONCEALED;
  return 0;
}

// The grid-wide checks of decode_full_grid_image and decode_and_paste_tile_image, with the reference's messages: tile i of grid P as
// its item declares it ('ispe'; iw x ih: what tile 0 declares) - context.cc:2299-2359: positions advance by the DECLARED size, all
// tiles must be equally sized and cover the output ...
int grid_tile_declared(const hm_file* f, const ItemPlan& P, int i, int iw, int ih)
{
  if (P.canvas_w > 32768 || P.canvas_h > 32768) return hm_fail(HM_ERR_BITSTREAM, "Image size exceeds the maximum of 32768x32768 (security limit)");
  const hm::Item* ti = f->file.item(P.tiles[i].id);
  const int sw = ti ? ti->props.ispe_width : 0, sh = ti ? ti->props.ispe_height : 0;
  if (sw < P.canvas_w / P.cols || sh < P.canvas_h / P.rows) return hm_fail(HM_ERR_BITSTREAM, "Grid tiles do not cover whole image");
  if (sw != iw || sh != ih) return hm_fail(HM_ERR_BITSTREAM, "Grid tiles have different sizes");
  return HM_OK;
}
// ... and a tile's decoded picture h against the canvas, which has the chroma format and depth of the grid's tile 0 (context.cc:2430-2492)
int grid_tile_picture(const hm_pic* h, int chroma, int bd)
{
  if (h->chroma_format != chroma) return hm_fail(HM_ERR_BITSTREAM, "Image tile has different chroma format than combined image");
  if (h->bit_depth_y != bd) return hm_fail(HM_ERR_BITSTREAM, "Image tile has different pixel depth than combined image");
  return HM_OK;
}

// The colour profile a decoded picture carries: what the libde265 plugin attaches from the VUI (decoder_libde265.cc:339-362),
// unless the item has a 'colr' nclx (context.cc:1844-1852).  heif_nclx_color_profile_set_* (heif.cc:1811-1905) stores
// "unspecified" for a code point it does not know and returns an error, which the plugin turns into a decoding warning
// (*warn, HM_WARN_UNKNOWN_*) - or, with strict_decoding, into a failure (HEIF_WARN_OR_FAIL, decoder_libde265.cc:339-357).
int picture_profile(const hm_pic* h, const hm::Item* ti, int strict, hm::NclxProfile& tp, int& warn)
{
  tp = hm::NclxProfile();
  tp.present = true; tp.primaries = h->colour_primaries; tp.transfer = h->transfer_characteristics;
  tp.matrix = h->matrix_coeffs; tp.full_range = h->full_range;
  warn = 0;
  if (!hm_nclx_code_known(0, tp.primaries)) { tp.primaries = 2; warn |= HM_WARN_UNKNOWN_PRIMARIES; }
  if (!hm_nclx_code_known(1, tp.transfer)) { tp.transfer = 2; warn |= HM_WARN_UNKNOWN_TRANSFER; }
  if (!hm_nclx_code_known(2, tp.matrix)) { tp.matrix = 2; warn |= HM_WARN_UNKNOWN_MATRIX; }
  if (warn && strict)
    return hm_fail(HM_ERR_BITSTREAM, "Unknown NCLX %s (strict decoding)", (warn & 1) ? "color primaries" : (warn & 2) ? "transfer characteristics" : "matrix coefficients");
  if (ti && ti->props.colr.present) tp = ti->props.colr;
  return HM_OK;
}

// decode_image_planar for an hvc1 item or a grid (context.cc:1729-2020) once the host entropy decode of its coded
// pictures is done: one GPU batch, then the item's irot / imir / clap.  Asynchronous on `s`.
// attach: the caller will convert the planes to params->out_format as they come out of this function (no alpha plane, nothing
// else in between) - then the conversion is attached to the batch, which runs deblocking, SAO, paste and colour as ONE kernel
// for the picture classes that allow it, and I.rgb holds the pixels (I.rgb_attached); it stays off whenever something works on
// the planes after the batch (tiles with transformations or alpha images, transformations of the item).
int planar_from_blobs(const hm_file* f, ItemPlan& P, const hm_decode_params* params, hipStream_t s, PlanarImage& I, bool attach = false)
{
  const hm::Item* it = f->file.item(P.id);
  hm::HeifError err;
  const int nt = (int)P.tiles.size();
  for (int i = 0; i < nt; i++)
    if (P.status[i]) return tile_failure(P, i);
  for (size_t i = 0; i < P.tile_alpha.size(); i++)
    if (P.alpha_status[i]) return hm_fail(P.alpha_status[i], "alpha image of tile %d (item %u): %s", P.tile_alpha[i].tile, P.tile_alpha[i].id, P.alpha_messages[i].c_str());
  const bool is_grid = P.is_grid;
  int canvas_w = P.canvas_w, canvas_h = P.canvas_h;

  // ---- geometry ----
  const hm_pic* h0 = hm_pic_of(P.blobs[0].p);
  const int chroma = h0->chroma_format, bd = h0->bit_depth_y;
  int rc;
  if (is_grid) {
    // the grid-wide checks, tile by tile, and the tile origins: positions advance by the size tile 0 declares
    const hm::Item* t0 = f->file.item(P.tiles[0].id);
    const int iw = t0 ? t0->props.ispe_width : 0, ih = t0 ? t0->props.ispe_height : 0;
    for (int i = 0; i < nt; i++) {
      // (a tile item with its own irot / imir / clap: decode_image_planar applies them to the tile image before the
      //  paste, context.cc:1957-2020 - handled below by decoding such a tile to planes of its own)
      if ((rc = grid_tile_declared(f, P, i, iw, ih)) || (rc = grid_tile_picture(hm_pic_of(P.blobs[i].p), chroma, bd))) return rc;
      P.tiles[i].x0 = (i % P.cols) * iw;
      P.tiles[i].y0 = (i / P.cols) * ih;
    }
  }
  else { canvas_w = hm_window_w(*h0); canvas_h = hm_window_h(*h0); }
  const int bps = hm_sample_bytes(bd);

  // colour profile of the decoded (native) image and the per-tile paste parameters; every check that can fail on file
  // data comes before the first asynchronous call
  hm::NclxProfile native;
  std::vector<hm::NclxProfile> tile_profile(nt);
  for (int i = 0; i < nt; i++) {
    const hm::Item* ti = f->file.item(P.tiles[i].id);
    hm::NclxProfile tp;
    int warn = 0;
    const int prc = picture_profile(hm_pic_of(P.blobs[i].p), ti, params->strict_decoding, tp, warn);
    if (prc) return prc;
    if (!is_grid) I.warnings |= warn; // (the warnings of grid tiles die with the tile images)
    if (i == 0) native = tp;
    tile_profile[i] = tp;
  }
  I.warnings |= concealed_warning(P, 0, nt); // (of a grid's tiles too - the image is the caller's)

  DevPlane (&Pl)[3] = I.P;
  if ((rc = alloc_planes(Pl, canvas_w, canvas_h, chroma, bd))) return rc;
  hm_batch* batch = nullptr;
  if ((rc = hm_batch_create(&batch))) return rc;
  I.batch.reset(batch);
  // grid tiles whose item carries transformative properties: their picture goes to planes of its own (the size of its
  // conformance window), is transformed there and pasted afterwards - what decode_and_paste_tile_image does with the
  // image decode_image_planar returns (context.cc:2407-2539)
  std::vector<std::unique_ptr<OwnTile>>& own = I.own;
  own.clear();
  for (int i = 0; i < nt; i++) {
    const hm::Item* ti = is_grid && !P.self_grid ? f->file.item(P.tiles[i].id) : nullptr; // (self_grid: the transformations are the item's, below)
    if (ti && !ti->props.transforms.empty() && !params->ignore_transformations) {
      const hm_pic* h = hm_pic_of(P.blobs[i].p);
      std::unique_ptr<OwnTile> o(new OwnTile());
      o->index = i;
      o->w = hm_window_w(*h); o->h = hm_window_h(*h);
      // (file data is checked before anything is queued: the tile's origin inside the canvas, channel by channel)
      for (int c = 0; c < (chroma == 0 ? 1 : 3); c++)
        if (!hm_place_tile(chroma, c, canvas_w, canvas_h, P.tiles[i].x0, P.tiles[i].y0).inside) return hm_tile_origin_refused();
      if ((rc = alloc_planes(o->P, o->w, o->h, chroma, bd))) return rc;
      const hm_tile_dest d = tile_dest_of(o->P, o->w, o->h); // (no nclx: the range rescale happens in the paste)
      const int idx = hm_batch_add_trusted(batch, P.blobs[i].p, P.blobs[i].n, &d);
      if (idx < 0) return idx;
      own.push_back(std::move(o));
      continue;
    }
    hm_tile_dest d = tile_dest_of(Pl, canvas_w, canvas_h);
    d.x0 = P.tiles[i].x0; d.y0 = P.tiles[i].y0;
    // the range rescale belongs to the grid paste only (context.cc:2504-2528)
    d.tile_has_nclx = is_grid ? 1 : 0; d.tile_full_range = tile_profile[i].full_range; d.tile_matrix = tile_profile[i].matrix;
    const int idx = hm_batch_add_trusted(batch, P.blobs[i].p, P.blobs[i].n, &d);
    if (idx < 0) return idx;
  }
  // ---- alpha auxiliary images of tile items: each is decoded to planes of its own in the same batch; the first one
  //      decides the depth of the canvas' alpha plane (context.cc:2437-2455), which starts opaque ----
  std::vector<std::unique_ptr<OwnTile>>& own_alpha = I.own_alpha;
  own_alpha.clear();
  I.tile_alpha_bd = 0;
  for (size_t k = 0; k < P.tile_alpha.size(); k++) {
    const hm_pic* h = hm_pic_of(P.alpha_blobs[k].p);
    const int i = P.tile_alpha[k].tile;
    if (I.tile_alpha_bd == 0) I.tile_alpha_bd = h->bit_depth_y;
    else if (h->bit_depth_y != I.tile_alpha_bd) return hm_fail(HM_ERR_BITSTREAM, "Image tile has different pixel depth than combined image (alpha plane)");
    if (!hm_place_tile(0, 0, canvas_w, canvas_h, P.tiles[i].x0, P.tiles[i].y0).inside) return hm_tile_origin_refused(); // (pasted like a luma plane)
    std::unique_ptr<OwnTile> o(new OwnTile());
    o->index = (int)k;
    o->chroma = h->chroma_format; o->bd = h->bit_depth_y;
    o->w = hm_window_w(*h); o->h = hm_window_h(*h);
    if ((rc = alloc_planes(o->P, o->w, o->h, o->chroma, o->bd))) return rc;
    const hm_tile_dest d = tile_dest_of(o->P, o->w, o->h);
    const int idx = hm_batch_add_trusted(batch, P.alpha_blobs[k].p, P.alpha_blobs[k].n, &d);
    if (idx < 0) return idx;
    own_alpha.push_back(std::move(o));
  }
  if (I.tile_alpha_bd) {
    const int abps = hm_sample_bytes(I.tile_alpha_bd);
    if ((rc = alloc_plane(I.tile_alpha, canvas_w, canvas_h, abps))) return rc;
    const size_t bytes = plane_bytes(I.tile_alpha);
    const hipError_t e = abps == 1 ? hipMemsetAsync(I.tile_alpha.mem.p, 0xFF, bytes, s)
                                   : hipMemsetD16Async((hipDeviceptr_t)I.tile_alpha.mem.p, (unsigned short)((1u << I.tile_alpha_bd) - 1u), bytes / 2, s);
    if (e != hipSuccess) return hm_check_hip(e, "fill of the alpha plane");
  }
  // a grid canvas the tiles do not cover completely: the reference leaves it uninitialised (tiles must cover the
  // output, context.cc:2321-2337; its right / bottom padding is never read): zero it
  for (int c = 0; c < 3; c++)
    if (Pl[c].mem.p) hipMemsetAsync(Pl[c].mem.p, 0, plane_bytes(Pl[c]), s);
  if ((rc = hm_batch_upload(batch, s))) return rc;
  I.rgb_attached = false;
  if (attach && params->out_format != 0 && !hm_out_is_planar(params->out_format) && chroma != 0 && own.empty() && own_alpha.empty() && I.tile_alpha_bd == 0 &&
      (params->ignore_transformations || it->props.transforms.empty())) {
    const int obpp = hm_out_bytes_per_pixel(params->out_format);
    if (obpp > 0) {
      // (exactly the request job_enqueue / run_slab would hand to hm_colour_convert)
      const hm_colour_desc cd = colour_desc(params, canvas_w, canvas_h, bd, chroma, native, is_grid ? 0 : 1, Pl, obpp);
      if (!I.rgb.alloc((size_t)cd.out_stride * hm_padded_rows(canvas_h))) {
        const void* py = Pl[0].mem.p; const void* pcb = Pl[1].mem.p; const void* pcr = Pl[2].mem.p;
        void* po = I.rgb.p;
        // (a request the colour chain refuses is refused by the caller's own conversion in a moment: not an error here)
        I.rgb_attached = hm_batch_set_colour(batch, &cd, 1, &py, &pcb, &pcr, &po, 0) == HM_OK;
      }
    }
  }
  if ((rc = hm_batch_execute(batch, 3, s))) return rc;
  for (std::unique_ptr<OwnTile>& o : own) {
    const hm::Item* ti = f->file.item(P.tiles[o->index].id);
    int tw = o->w, th = o->h;
    if ((rc = apply_transforms(ti->props.transforms, o->P, tw, th, chroma, bd, s, I.retired))) return rc;
    o->w = tw; o->h = th; // (the tile image's size from here on: what an alpha image of the tile is scaled to)
    const hm::NclxProfile& tp = tile_profile[o->index];
    const int rescale = (tp.present && !tp.full_range && tp.matrix != 0) ? 1 : 0; // context.cc:2504-2509
    for (int c = 0; c < 3; c++) {
      if (!o->P[c].mem.p) continue;
      const hm_tile_place at = hm_place_tile(chroma, c, canvas_w, canvas_h, P.tiles[o->index].x0, P.tiles[o->index].y0);
      if (!at.inside) return hm_tile_origin_refused();
      const int copy_w = hm_copy_extent(o->P[c].w, at.chan_w, at.x0), copy_h = hm_copy_extent(o->P[c].h, at.chan_h, at.y0);
      if ((rc = hm_launch_paste_bytes(o->P[c].mem.p, o->P[c].stride, (uint8_t*)Pl[c].mem.p + (size_t)at.y0 * Pl[c].stride + (size_t)at.x0 * bps,
                                      Pl[c].stride, copy_w * bps, copy_h, rescale, bd, c > 0, s))) return rc;
    }
    for (int c = 0; c < 3; c++) retire(I.retired, o->P[c].mem);
  }

  // ---- the tiles' alpha images: the alpha item's own transformations, its Y plane scaled (nearest neighbour) to the
  //      tile image's size if it differs (context.cc:2064-2072), pasted like a luma plane - range rescale of the
  //      tile's profile included (context.cc:2504-2528 runs over every channel of the tile image) ----
  for (std::unique_ptr<OwnTile>& o : own_alpha) {
    const ItemPlan::TileAlpha& ta = P.tile_alpha[(size_t)o->index];
    const hm::Item* ai = f->file.item(ta.id);
    int aw = o->w, ah = o->h;
    if (ai && !params->ignore_transformations && !ai->props.transforms.empty())
      if ((rc = apply_transforms(ai->props.transforms, o->P, aw, ah, o->chroma, o->bd, s, I.retired))) return rc;
    // the tile image's size: its picture's conformance window, or what its own transformations made of it
    const hm_pic* th = hm_pic_of(P.blobs[ta.tile].p);
    int tw = hm_window_w(*th), thh = hm_window_h(*th);
    for (const std::unique_ptr<OwnTile>& t : own)
      if (t->index == ta.tile) { tw = t->w; thh = t->h; }
    const int abps = hm_sample_bytes(o->bd);
    const DevPlane* ap = &o->P[0];
    DevPlane scaled;
    if (aw != tw || ah != thh) {
      if ((rc = alloc_plane(scaled, tw, thh, abps))) return rc;
      if ((rc = hm_launch_scale_nn(abps, o->P[0].mem.p, o->P[0].stride, aw, ah, scaled.mem.p, scaled.stride, tw, thh, s))) return rc;
      ap = &scaled;
    }
    const hm::NclxProfile& tp = tile_profile[ta.tile];
    const int rescale = (tp.present && !tp.full_range && tp.matrix != 0) ? 1 : 0;
    const int x0 = P.tiles[ta.tile].x0, y0 = P.tiles[ta.tile].y0; // (inside the canvas: checked above)
    const int copy_w = hm_copy_extent(tw, canvas_w, x0), copy_h = hm_copy_extent(thh, canvas_h, y0);
    rc = hm_launch_paste_bytes(ap->mem.p, ap->stride, (uint8_t*)I.tile_alpha.mem.p + (size_t)y0 * I.tile_alpha.stride + (size_t)x0 * abps,
                               I.tile_alpha.stride, copy_w * abps, copy_h, rescale, o->bd, 0, s);
    if (scaled.mem.p) retire(I.retired, scaled.mem);
    if (rc) return rc;
  }

  // ---- transformative item properties on the decoded planes (context.cc:1957-2020) ----
  int img_w = canvas_w, img_h = canvas_h;
  if (!params->ignore_transformations && !it->props.transforms.empty()) {
    if ((rc = apply_transforms(it->props.transforms, Pl, img_w, img_h, chroma, bd, s, I.retired))) return rc;
    int aw = canvas_w, ah = canvas_h; // (the alpha plane is a plane of the canvas: the grid's transformations move it along)
    if (I.tile_alpha_bd && (rc = apply_transforms_plane(it->props.transforms, I.tile_alpha, aw, ah, I.tile_alpha_bd, s, I.retired))) return rc;
  }
  I.w = img_w; I.h = img_h; I.chroma = chroma; I.bd = bd; I.native = native; I.is_grid = is_grid;
  return HM_OK;
}

} // namespace

namespace hm_img {

// The sub-grid of tile rows and columns a view's crop intersects, where decoding only those tiles provably changes no pixel of the
// crop: the item is a grid, no transformation is applied on it or on a covered tile, neither it nor a tile has an alpha image, chroma
// up-sampling is the default one (the colour ops then read chroma at x >> 1, y >> 1) and the sub-grid's origin is even in every
// subsampled direction (an odd one moves a column / row further out).  t = first tile row, row count, first tile column, column count;
// origin and size of the sub-grid's canvas in x0, y0, w, h.  false: the whole item is decoded (t = the whole grid).
// Item properties only: no coded picture is looked at.
// planes_view: the view goes to planar YCbCr (hm_device_planes).  Then the reduction covers out_format 0 alone, the picture as coded -
// a grid's planes are its tiles' planes side by side, so the sub-grid's planes are the rectangle of the whole grid's -, and the
// HM_OUT_YCBCR_* chains, whose up- and down-sampling operations read neighbours across tile borders, decode the whole item.
// ... and for an 'unci' item the sub-grid of its INTERNAL tiles, under the same conditions (a sub-sampled item has even tile sizes, so
// the sub-grid's origin is even by itself): only those tiles' byte ranges are uploaded and unpacked
static bool unci_view_subgrid(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* v, int32_t t[4], int* x0, int* y0, int* w, int* h,
                              bool planes_view)
{
  const hm::Item* it = f->file.item(id);
  hm_unci_info u;
  hm::HeifError err;
  if (!f->file.unci_info(id, u, err)) return false;
  t[1] = (int32_t)u.tile_rows; t[3] = (int32_t)u.tile_cols;
  if (!v || (v->crop_w == 0 && v->crop_h == 0)) return false;
  if (planes_view ? params->out_format != 0 : (hm_out_is_planar(params->out_format) || params->out_format == 0)) return false;
  if (!planes_view && u.colour_space == HM_UNCI_YCBCR && params->chroma_upsampling != 0) return false;
  if (!params->ignore_transformations && !it->props.transforms.empty()) return false;
  if (v->crop_w <= 0 || v->crop_h <= 0 || v->crop_x < 0 || v->crop_y < 0 || (int64_t)v->crop_x + v->crop_w > u.width || (int64_t)v->crop_y + v->crop_h > u.height) return false;
  const int tw = (int)u.tile_width, th = (int)u.tile_height;
  const int c0 = v->crop_x / tw, c1 = (v->crop_x + v->crop_w - 1) / tw, r0 = v->crop_y / th, r1 = (v->crop_y + v->crop_h - 1) / th;
  t[0] = r0; t[1] = r1 - r0 + 1; t[2] = c0; t[3] = c1 - c0 + 1;
  *x0 = c0 * tw; *y0 = r0 * th; *w = t[3] * tw; *h = t[1] * th;
  return true;
}

bool view_subgrid(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* v, int32_t t[4], int* x0, int* y0, int* w, int* h,
                  bool planes_view = false)
{
  t[0] = 0; t[1] = 1; t[2] = 0; t[3] = 1;
  const hm::Item* it = f->file.item(id);
  if (it && it->is_raw_leaf()) return unci_view_subgrid(f, id, params, v, t, x0, y0, w, h, planes_view);
  if (!it || it->type != "grid") return false;
  hm::GridInfo g;
  hm::HeifError err;
  if (!f->file.grid_info(id, g, err) || g.rows < 1 || g.cols < 1 || g.tiles.size() != (size_t)g.rows * g.cols) return false;
  t[1] = g.rows; t[3] = g.cols;
  if (!v || (v->crop_w == 0 && v->crop_h == 0)) return false;
  if (planes_view ? params->out_format != 0 : (params->chroma_upsampling != 0 || hm_out_is_planar(params->out_format) || params->out_format == 0)) return false;
  if (!params->ignore_transformations && !it->props.transforms.empty()) return false;
  if (f->file.alpha_item_of(id)) return false;
  const int gw = (int)g.width, gh = (int)g.height;
  if (v->crop_w <= 0 || v->crop_h <= 0 || v->crop_x < 0 || v->crop_y < 0 || (int64_t)v->crop_x + v->crop_w > gw || (int64_t)v->crop_y + v->crop_h > gh) return false;
  const hm::Item* t0 = f->file.item(g.tiles[0]);
  if (!t0 || !t0->props.hvcc.present) return false;
  const int iw = t0->props.ispe_width, ih = t0->props.ispe_height, chroma = t0->props.hvcc.chroma_format;
  if (iw <= 0 || ih <= 0 || (int64_t)iw * g.cols < gw || (int64_t)ih * g.rows < gh) return false;
  for (uint32_t tid : g.tiles)
    if (f->file.alpha_item_of(tid)) return false;
  int c0 = v->crop_x / iw, c1 = (v->crop_x + v->crop_w - 1) / iw, r0 = v->crop_y / ih, r1 = (v->crop_y + v->crop_h - 1) / ih;
  if ((chroma == 1 || chroma == 2) && ((c0 * iw) & 1)) c0--; // (odd tile width, odd column: the column before starts even)
  if (chroma == 1 && ((r0 * ih) & 1)) r0--;
  for (int r = r0; r <= r1; r++)
    for (int c = c0; c <= c1; c++) {
      const hm::Item* ti = f->file.item(g.tiles[(size_t)r * g.cols + c]);
      if (!ti || ti->type != "hvc1" || ti->props.ispe_width != iw || ti->props.ispe_height != ih) return false;
      if (!params->ignore_transformations && !ti->props.transforms.empty()) return false;
    }
  t[0] = r0; t[1] = r1 - r0 + 1; t[2] = c0; t[3] = c1 - c0 + 1;
  *x0 = c0 * iw; *y0 = r0 * ih;
  *w = std::min(t[3] * iw, gw - *x0); *h = std::min(t[1] * ih, gh - *y0);
  return true;
}

// Many views: the bounding rectangle of all their crops as a view of the crop alone - what view_subgrid plans the decode of.
// false: a view has no crop (it takes the whole image), or the rectangle does not fit the fields: nothing is reduced.
static bool views_bound(const hm_device_view* views, int32_t count, hm_device_view* bound)
{
  int64_t x0 = INT64_MAX, y0 = INT64_MAX, x1 = INT64_MIN, y1 = INT64_MIN;
  for (int32_t k = 0; k < count; k++) {
    const hm_device_view& v = views[k];
    if (v.crop_w <= 0 || v.crop_h <= 0 || v.crop_x < 0 || v.crop_y < 0) return false; // (no crop; or one the view's own check refuses)
    x0 = std::min<int64_t>(x0, v.crop_x); y0 = std::min<int64_t>(y0, v.crop_y);
    x1 = std::max<int64_t>(x1, (int64_t)v.crop_x + v.crop_w); y1 = std::max<int64_t>(y1, (int64_t)v.crop_y + v.crop_h);
  }
  if (count < 1 || x1 - x0 > INT32_MAX || y1 - y0 > INT32_MAX) return false;
  std::memset(bound, 0, sizeof(*bound));
  bound->crop_x = (int32_t)x0; bound->crop_y = (int32_t)y0; bound->crop_w = (int32_t)(x1 - x0); bound->crop_h = (int32_t)(y1 - y0);
  return true;
}

// the depths of an 'unci' item's colour components: *lo / *hi = the smallest and the largest
static void unci_colour_depths(const hm_unci_info& u, int* lo, int* hi)
{
  *lo = 16; *hi = 0;
  for (int c = 0; c < u.n_components; c++) {
    const int p = hm_unci_plane_of(u.colour_space, u.comp[c].type);
    if (p < 0 || p > 2) continue;
    *lo = std::min<int>(*lo, u.comp[c].depth); *hi = std::max<int>(*hi, u.comp[c].depth);
  }
}
static int unci_alpha_depth(const hm_unci_info& u)
{
  for (int c = 0; c < u.n_components; c++)
    if (u.comp[c].type == HM_UNCI_TYPE_ALPHA) return u.comp[c].depth;
  return 0;
}

// An 'unci' item as a job: no coded pictures, and everything the item or the request is refused for - before anything is queued.
static int plan_unci(DecodeJob& j)
{
  const hm_decode_params& prm = j.params;
  if (!j.allow_unci && j.f->file.item(j.id)->is_mask())
    return hm_fail(HM_ERR_UNSUPPORTED, "a mask ('mski') item is not supported by the pipeline, batch and sequence calls: decode it with hm_decode_item");
  if (!j.allow_unci)
    return hm_fail(HM_ERR_UNSUPPORTED, "an uncompressed ('unci') item is not supported by the pipeline, batch and sequence calls: decode it with hm_decode_item");
  hm::HeifError err;
  hm_unci_info& u = j.unci_info;
  if (!j.f->file.unci_info(j.id, u, err)) return fail_from(err);
  if (j.f->file.alpha_item_of(j.id)) return hm_fail(HM_ERR_UNSUPPORTED, "an alpha auxiliary image attached to an 'unci' item is not supported (an alpha component is its alpha plane)");
  if (j.target.t.gain) return hm_fail(HM_ERR_UNSUPPORTED, "a gain step on an 'unci' item is not supported");
  int lo, hi;
  unci_colour_depths(u, &lo, &hi);
  const int fmt = prm.out_format;
  const bool planar = hm_out_is_planar(fmt);
  if (u.colour_space == HM_UNCI_RGB) {
    if (planar) return hm_fail(HM_ERR_UNSUPPORTED, "an 'unci' item of R G B components has no chroma format to convert to: out_format 0 hands out its R, G, B planes");
    if (fmt != 0) { // the interleaved targets of a uniform depth; the reference finds no chain for anything else either
      const bool wide = fmt == HM_OUT_RRGGBB_LE || fmt == HM_OUT_RRGGBBAA_LE, four = fmt == HM_OUT_RGBA || fmt == HM_OUT_RRGGBBAA_LE;
      const int want = wide ? 16 : 8, ad = unci_alpha_depth(u);
      if ((!wide && fmt != HM_OUT_RGB && fmt != HM_OUT_RGBA) || lo != want || hi != want || (four && ad && ad != want))
        return hm_fail_detail(HM_ERR_UNSUPPORTED, HM_DETAIL_NO_COLOUR_CHAIN,
                              "unci: no colour chain from these R G B component depths to this target (8 bits: HM_OUT_RGB / _RGBA, 16 bits: HM_OUT_RRGGBB_LE / _RRGGBBAA_LE)");
    }
    else if (j.target.t.planes && (lo > 8) != (hi > 8)) return hm_fail(HM_ERR_UNSUPPORTED, "unci: R G B planes of byte and word samples do not go to one set of device planes");
  }
  else {
    if (lo != hi) return hm_fail(HM_ERR_UNSUPPORTED, "unci: Y Cb Cr components of different depths (%d, %d) are not supported", lo, hi);
    const int chroma = u.colour_space == HM_UNCI_MONO ? 0 : u.sampling == HM_UNCI_SAMPLING_420 ? 1 : u.sampling == HM_UNCI_SAMPLING_422 ? 2 : 3;
    const bool as_decoded = fmt == 0 || (planar && chroma != 0 && chroma == hm_out_planar_chroma(fmt));
    if (!as_decoded && (hi < 8 || hi > 12))
      return hm_fail(HM_ERR_UNSUPPORTED, "unci: a %d-bit item is handed out as coded only (out_format 0); the colour chains take 8..12 bits", hi);
  }
  ItemPlan& P = j.item[0];
  P = ItemPlan();
  P.id = j.id; P.rows = (int)u.tile_rows; P.cols = (int)u.tile_cols; P.canvas_w = u.width; P.canvas_h = u.height;
  j.n_items = 1; j.has_map = false;
  j.view_dx = j.view_dy = 0;
  j.sub_tiles[0] = 0; j.sub_tiles[1] = P.rows; j.sub_tiles[2] = 0; j.sub_tiles[3] = P.cols;
  int sw = 0, sh = 0;
  j.unci_sub = j.target.t.view && view_subgrid(j.f, j.id, &j.params, j.target.t.view, j.sub_tiles, &j.view_dx, &j.view_dy, &sw, &sh, j.target.t.planes != nullptr);
  if (!j.unci_sub) { j.view_dx = j.view_dy = 0; j.sub_tiles[0] = 0; j.sub_tiles[1] = P.rows; j.sub_tiles[2] = 0; j.sub_tiles[3] = P.cols; }
  return HM_OK;
}

int job_plan(DecodeJob& j)
{
  const hm::Item* it0 = j.f->file.item(j.id);
  j.unci = it0 && it0->is_raw_leaf();
  if (j.unci) return plan_unci(j);
  int rc = plan_item(j.f, j.id, j.item[0], j.self_grid);
  if (rc) return rc;
  j.n_items = 1;
  j.view_dx = j.view_dy = 0;
  j.sub_tiles[0] = 0; j.sub_tiles[1] = j.item[0].rows; j.sub_tiles[2] = 0; j.sub_tiles[3] = j.item[0].cols;
  int sx = 0, sy = 0, sw = 0, sh = 0;
  // the gain map of a gain step joins the job as a third item - unless its weight is 0: the write is then the one without the step.
  // Tile reduction under a view stays off with a gain step (the open step: the map's crop would have to follow the sub-grid)
  j.has_map = false;
  // the view the sub-grid is planned for: the request's, or with many views the bounding rectangle of all crops, taken as one crop - a
  // synthetic view of the crop alone
  hm_device_view bound;
  const hm_device_view* plan_view = j.target.t.view;
  if (j.target.t.views) plan_view = views_bound(j.target.t.views->views, j.target.t.views->count, &bound) ? &bound : nullptr;
  if (const hm_device_gain* g = j.target.t.gain) {
    if (hm_gain_weight(&g->params, g->headroom) != 0.0) {
      ItemPlan& M = j.item[2];
      if ((rc = plan_item(j.f, g->map_item, M))) return rc;
      M.tile_alpha.clear(); M.alpha_blobs.clear(); M.alpha_status.clear(); M.alpha_messages.clear(); // (a map has no alpha)
      j.has_map = true;
    }
  }
  else if (plan_view && view_subgrid(j.f, j.id, &j.params, plan_view, j.sub_tiles, &sx, &sy, &sw, &sh, j.target.t.planes != nullptr)) {
    const int32_t* t = j.sub_tiles;
    j.item[0] = j.item[0].sub_grid(t[0], t[1], t[2], t[3], sw, sh);
    j.view_dx = sx; j.view_dy = sy;
    return HM_OK; // (no alpha image on the item: view_subgrid)
  }
  // the alpha channel: an auxiliary image decoded like any image (context.cc:2029-2078)
  const uint32_t alpha_id = j.f->file.alpha_item_of(j.id);
  if (alpha_id) {
    if ((rc = plan_item(j.f, alpha_id, j.item[1]))) return rc;
    j.n_items = 2;
  }
  return HM_OK;
}

int job_tile_count(const DecodeJob& j)
{
  int n = 0;
  for (int i = 0; i < j.n_items; i++) n += (int)j.item[i].tiles.size();
  n += (int)j.item[0].tile_alpha.size(); // (behind the tiles of the image and of its own alpha image: the tiles' alpha pictures)
  return n + (j.has_map ? (int)j.item[2].tiles.size() : 0); // (... and behind those the pictures of the gain map)
}

// host entropy decode of coded picture k (CABAC on the calling thread, like the reference's std::async tile tasks,
// context.cc:2361-2401); distinct k may run concurrently
void job_parse_tile(DecodeJob& j, int k, int row_threads)
{
  if (j.has_map) {
    ItemPlan& M = j.item[2];
    const int m = k - (job_tile_count(j) - (int)M.tiles.size());
    if (m >= 0) { parse_picture(j.f, M.tiles[m].id, j.few_pictures != 0, j.params.strict_decoding, row_threads, M.blobs[m], M.status[m], M.messages[m]); return; }
  }
  int which = 0;
  if (k >= (int)j.item[0].tiles.size()) { which = 1; k -= (int)j.item[0].tiles.size(); }
  const bool tile_alpha = which == 1 && (j.n_items < 2 || k >= (int)j.item[1].tiles.size());
  if (tile_alpha) { if (j.n_items > 1) k -= (int)j.item[1].tiles.size(); which = 0; }
  ItemPlan& P = j.item[which];
  const uint32_t id = tile_alpha ? P.tile_alpha[k].id : P.tiles[k].id;
  int& status = tile_alpha ? P.alpha_status[k] : P.status[k];
  std::string& message = tile_alpha ? P.alpha_messages[k] : P.messages[k];
  Blob& blob = tile_alpha ? P.alpha_blobs[k] : P.blobs[k];
  parse_picture(j.f, id, j.few_pictures != 0, j.params.strict_decoding, row_threads, blob, status, message);
}

void parse_picture(const hm_file* f, uint32_t id, bool few_pictures, int strict, int row_threads, Blob& blob, int& status, std::string& message)
{
  std::vector<uint8_t> data;
  hm::HeifError e;
  if (!f->file.hevc_data(id, data, e)) { status = e.status; message = e.message; return; }
  hm_parse_options po;
  po.annexb = 0; po.threads = row_threads;
  po.record_order = (few_pictures ? HM_RECORDS_SPLIT : HM_RECORDS_AUTO) | (strict ? 0 : HM_PARSE_CONCEAL);
  const int rc = hm_hevc_parse_opts(data.data(), data.size(), &po, &blob.p, &blob.n);
  if (rc) { status = rc; message = hm_last_error(); }
}

int target_check_shape(const OutputTarget& t)
{
  const bool to_dest = t.dest || t.views; // (many views stand where dest stands)
  const bool ok = !(t.dest && t.planes) && (!t.light || to_dest) && (!t.tone || t.light) && (!t.ootf || t.light) &&(!t.alpha || (to_dest && !t.view_later)) && (!t.gain || (t.light && !t.view_later)) && (!t.view || t.dest || t.planes) && (!t.view_later || (t.view && t.dest)) &&
                  (!t.planes_later || (t.view && t.planes)) &&
                  (!t.views || (!t.dest && !t.view && !t.planes && !t.gain && !t.measure && !t.view_later && !t.planes_later && t.views->views && t.views->dests && t.views->count >= 1));
  return ok ? (int)HM_OK : hm_fail(HM_ERR_INTERNAL, "output target: dest%s view%s planes%s light%s tone%s alpha%s gain%s do not go together", t.dest ? "+" : "-", t.view ? "+" : "-",
                                   t.planes ? "+" : "-", t.light ? "+" : "-", t.tone ? "+" : "-", t.alpha ? "+" : "-", t.gain ? "+" : "-");
}

// the chroma format and depth of a planar result for a decoded image of (chroma, bd): what emit_native / emit_planar hand out
static void planar_result_format(const hm_decode_params* params, int chroma, int bd, int* rchroma, int* rbits)
{
  const bool as_decoded = params->out_format == 0 || (chroma != 0 && chroma == hm_out_planar_chroma(params->out_format));
  *rchroma = as_decoded ? chroma : hm_out_planar_chroma(params->out_format);
  *rbits = !as_decoded && params->convert_hdr_to_8bit ? 8 : bd;
}

// What a converted image reports: the output state's profile - the input one, none for a grid canvas, with undefined values
// replaced by the sRGB defaults (colorconversion.cc:452-455, 520-527) - and its depth: an 8-bit image becomes 10 bit in an RRGGBB
// target (:575-585), a deeper one 8 bit in RGB / RGBA; a planar target keeps the depth unless convert_hdr_to_8bit.
struct Reported {
  int has_nclx, primaries, transfer, matrix, full_range, bit_depth;
  void profile_to(hm_decoded* out) const { out->has_nclx = has_nclx; out->primaries = primaries; out->transfer = transfer; out->matrix = matrix; out->full_range = full_range; }
};
static Reported converted_report(const hm::NclxProfile& native, bool is_grid, int bd, int out_format, int convert_hdr_to_8bit)
{
  Reported r;
  r.has_nclx = 1;
  r.primaries = is_grid ? 2 : native.primaries; r.transfer = is_grid ? 2 : native.transfer; r.matrix = is_grid ? 2 : native.matrix;
  r.full_range = is_grid ? 1 : native.full_range;
  if (r.primaries == 2) r.primaries = 1;
  if (r.transfer == 2) r.transfer = 13;
  if (r.matrix == 2) r.matrix = 6;
  r.bit_depth = bd;
  if (hm_out_is_planar(out_format)) { if (convert_hdr_to_8bit) r.bit_depth = 8; }
  else if (bd == 8 && out_format >= HM_OUT_RRGGBB_BE && out_format <= HM_OUT_RRGGBBAA_LE) r.bit_depth = 10;
  else if (bd > 8 && (out_format == HM_OUT_RGB || out_format == HM_OUT_RGBA)) r.bit_depth = 8;
  return r;
}

// a refusal that is view k's: its index goes where the caller looks, its message in front of the check's own
static int view_refused(const ViewsRequest& V, int k, int rc)
{
  if (V.failed) *V.failed = k;
  const std::string why = hm_last_error();
  return hm_fail(rc, "view %d: %s", k, why.c_str());
}

// Many views against one image: plans[k] = the request with view k (moved by the decoded sub-grid's origin) against dests[k] - what the
// single-view entry resolves, view by view -, then the destinations against each other
static int views_resolve(const hm_decode_params* params, const OutputTarget& t, const hm_out_image& img, int know_profile, std::vector<hm_out_plan>& plans)
{
  const ViewsRequest& V = *t.views;
  hm_out_steps st = t.steps();
  int rc;
  for (int k = 0; k < V.count; k++) {
    const hm_device_view v = t.view_of(k);
    st.view = &v;
    if ((rc = hm_out_resolve(params->out_format, &img, know_profile, &V.dests[k], &st, &plans[(size_t)k]))) return view_refused(V, k, rc);
  }
  return hm_dests_check_overlap(V.dests, plans.data(), V.count);
}

// Can the target hold the result of a w x h image of (chroma, bits)?  The one statement of that question: the entry points ask it
// against what the file declares, the sequence and emit_image again against the decoded picture.  A new kind of destination gets
// its chain here.
//   dest:   hm_out_resolve - the view against the image, the destination against the view's output size, its len, the light and alpha
//           steps against the profile and depth the image reports (`reported`, may be NULL: not known yet) -, the pointer
//   planes: the result's format (planar_result_format), the view against it, the planes against the view's output size - alpha_bits
//           0: no alpha plane, -1: the decode's to say -, their len, the pointers
// w <= 0 or h <= 0: the file does not say - only what needs no size is looked at.  pointers: a device must exist and the pointers
// be its memory.
static int target_fits(const hm_decode_params* params, const OutputTarget& t, int w, int h, int chroma, int bits, int alpha_bits, const Reported* reported,
                       bool pointers)
{
  int rc;
  const bool sized = w > 0 && h > 0;
  if (t.views) { // every view against the image and its own destination, then the destinations against each other
    const ViewsRequest& V = *t.views;
    if (sized) {
      const hm_out_image img = {w, h, reported ? reported->bit_depth : 0, reported ? reported->transfer : 0, reported ? reported->primaries : 0};
      std::vector<hm_out_plan> plans((size_t)V.count);
      if ((rc = views_resolve(params, t, img, reported ? HM_OUT_PROFILE_LAST : 0, plans))) return rc;
    }
    if (pointers) {
      if ((rc = require_device())) return rc;
      for (int k = 0; k < V.count; k++)
        if ((rc = hm_dest_check_pointer(&V.dests[k]))) return view_refused(V, k, rc);
    }
  }
  if (t.dest) {
    if (sized) {
      const hm_out_steps st = t.steps();
      const hm_out_image img = {w, h, reported ? reported->bit_depth : 0, reported ? reported->transfer : 0, reported ? reported->primaries : 0};
      hm_out_plan plan;
      if ((rc = hm_out_resolve(params->out_format, &img, reported ? HM_OUT_PROFILE_LAST : 0, t.dest, &st, &plan))) return rc;
    }
    const bool stand_in = t.measure && t.measure->mode == HM_MEASURE_STATS; // (a statistic writes nothing: its destination has no memory)
    if (pointers && ((rc = require_device()) || (!stand_in && (rc = hm_dest_check_pointer(t.dest))))) return rc;
  }
  if (t.planes) {
    hm_planes_plan pp;
    if (sized) {
      int rchroma, rbits;
      planar_result_format(params, chroma, bits, &rchroma, &rbits);
      hm_planes_view_plan pv;
      pv.ow = w; pv.oh = h;
      if (t.view && (rc = hm_planes_view_resolve(rchroma, w, h, t.view, &pv))) return rc;
      if ((rc = hm_planes_resolve(rchroma, rbits, pv.ow, pv.oh, alpha_bits, t.planes, &pp)) || (rc = hm_planes_check_len(t.planes, &pp))) return rc;
    }
    // (without a size, hm_planes_write checks the pointers against the decoded result before its launch)
    if (pointers && ((rc = require_device()) || (sized && (rc = hm_planes_check_pointer(t.planes, &pp))))) return rc;
  }
  return HM_OK;
}

// the planes src[0 .. 2] (Y, Cb, Cr) and src[3] (alpha, abits > 0) of a planar result of (rchroma, rbits) into t.planes (checked against
// the result's own format before the launch): one launch of k_planes_to_tensor, or with t.view the view of every plane
// (hm_planes_view_write), written here or - t.planes_later - only described there for the caller's grouped write
static int write_planes(const hm_decode_params* params, hipStream_t s, const PlanarImage& I, const OutputTarget& t, int rchroma, int rbits, const void* const src[4],
                        const int32_t stride[4], int abits, hm_decoded* out)
{
  int rc;
  int64_t pitch[4];
  if (t.view) { // (the entry points have resolved the view against the size the file declares: here it is the decoded result)
    hm_planes_view_item item;
    std::memset(&item, 0, sizeof(item));
    if ((rc = hm_planes_view_resolve(rchroma, I.w, I.h, t.view, &item.pv))) return rc;
    item.planes = t.planes; item.chroma = rchroma; item.bits = rbits; item.alpha_bits = abits;
    for (int c = 0; c < 4; c++) { item.src[c] = src[c]; item.stride[c] = stride[c]; }
    if (t.planes_later) { // the caller's grouped write checks everything again; the pitches in use are known here
      hm_planes_plan pp;
      if ((rc = target_fits(params, t, I.w, I.h, I.chroma, I.bd, abits, nullptr, false))) return rc;
      if ((rc = hm_planes_resolve(rchroma, rbits, item.pv.ow, item.pv.oh, abits, t.planes, &pp))) return rc;
      for (int c = 0; c < 4; c++) item.pitches[c] = pp.pl[c].present ? pp.pl[c].pitch : 0;
      *t.planes_later = item;
    }
    else if ((rc = hm_planes_view_write(&item, 1, s, t.scratch, nullptr))) return rc;
    for (int c = 0; c < 4; c++) pitch[c] = item.pitches[c];
    out->width = item.pv.ow; out->height = item.pv.oh;
    for (int c = 0; c < 3; c++) { out->plane_width[c] = item.pv.out[c][0]; out->plane_height[c] = item.pv.out[c][1]; }
  }
  else if ((rc = hm_planes_write(t.planes, rchroma, rbits, I.w, I.h, abits, src, stride, s, pitch))) return rc;
  out->used_ext_dst = 1;
  for (int c = 0; c < 3; c++) out->stride[c] = (int32_t)std::min<int64_t>(pitch[c], 0x7FFFFFFF);
  out->alpha_stride = (int32_t)std::min<int64_t>(pitch[3], 0x7FFFFFFF);
  return HM_OK;
}

// the image as decoded: its planes (Y only for a monochrome image) and the alpha plane, to pinned host memory or to t.planes
static int emit_native(const hm_decode_params* params, hipStream_t s, PlanarImage& I, const DevPlane* alpha, int alpha_bd, const OutputTarget& t, hm_decoded* out)
{
  int rc;
  DevPlane (&P)[3] = I.P;
  out->out_format = params->out_format;
  for (int c = 0; c < 3; c++) {
    if (!P[c].mem.p) continue; // monochrome image: Y only
    out->plane_width[c] = P[c].w; out->plane_height[c] = P[c].h;
    if (!t.planes && (rc = plane_to_host(P[c].mem.p, P[c].stride, P[c].h, s, &out->plane[c], &out->stride[c]))) return rc;
  }
  if (t.planes) {
    const void* src[4] = {P[0].mem.p, P[1].mem.p, P[2].mem.p, alpha ? alpha->mem.p : nullptr};
    const int32_t stride[4] = {P[0].stride, P[1].stride, P[2].stride, alpha ? alpha->stride : 0};
    return write_planes(params, s, I, t, I.chroma, I.bd, src, stride, alpha ? alpha_bd : 0, out);
  }
  return alpha ? plane_to_host(alpha->mem.p, alpha->stride, alpha->h, s, &out->alpha, &out->alpha_stride) : (int)HM_OK;
}

// a planar YCbCr target of another chroma format or colourspace than the image's: the reference's chain to it, operation by
// operation (colour_planar.cpp), then its planes to pinned host memory or to t.planes
static int emit_planar(const hm_decode_params* params, hipStream_t s, PlanarImage& I, const DevPlane* alpha, int alpha_bd, const OutputTarget& t, hm_decoded* out)
{
  int rc;
  DevPlane (&P)[3] = I.P;
  hm_colour_desc cd = colour_desc(params, I.w, I.h, I.bd, I.chroma, I.native, out->has_nclx, P, 0, /*planar_8bit=*/true);
  cd.has_alpha = alpha ? 1 : 0;
  hm_planar_image src, res;
  for (int c = 0; c < 3; c++) { src.p[c] = P[c].mem.p; src.stride[c] = P[c].stride; }
  if (alpha) { src.p[3] = alpha->mem.p; src.stride[3] = alpha->stride; src.alpha_bits = alpha_bd; }
  std::vector<void*> temps;
  rc = hm_planar_convert(&cd, &src, nullptr, &res, temps, 0, s);
  for (void* tmp : temps) { I.retired.emplace_back(new DevMem()); I.retired.back()->p = tmp; } // (released once the stream has drained)
  if (rc) return rc;
  out->out_format = params->out_format;
  out->chroma = res.chroma; out->bit_depth = res.bits;
  for (int c = 0; c < 3; c++) { // (planes the chain passed through are copied from where they are: the decoded image's own)
    const int pw = hm_plane_w(res.chroma, c, I.w), ph = hm_plane_h(res.chroma, c, I.h);
    out->plane_width[c] = pw; out->plane_height[c] = ph;
    if (!t.planes && (rc = plane_to_host(res.p[c], res.stride[c], ph, s, &out->plane[c], &out->stride[c]))) return rc;
  }
  if (t.planes) {
    const int32_t stride[4] = {res.stride[0], res.stride[1], res.stride[2], res.stride[3]};
    if ((rc = write_planes(params, s, I, t, res.chroma, res.bits, res.p, stride, res.p[3] ? (res.alpha_bits ? res.alpha_bits : res.bits) : 0, out))) return rc;
  }
  else if (res.p[3] && (rc = plane_to_host(res.p[3], res.stride[3], I.h, s, &out->alpha, &out->alpha_stride))) return rc;
  converted_report(I.native, I.is_grid, I.bd, params->out_format, params->convert_hdr_to_8bit).profile_to(out); // (the depth: the chain's, above)
  return HM_OK;
}

// interleaved pixels: the colour conversion (unless the batch did it: I.rgb_attached), the alpha channel, and the pixels to t.dest -
// directly, through a view, through the light step -, to params->ext_dst or to pinned host memory
static int emit_interleaved(const hm_decode_params* params, hipStream_t s, PlanarImage& I, const DevPlane* alpha, int alpha_bd, DevMem& dout, DevPlane& alpha_sdr,
                            const OutputTarget& t, hm_decoded* out)
{
  int rc;
  DevPlane (&P)[3] = I.P;
  const int img_w = I.w, img_h = I.h, bd = I.bd;
  const int obpp = hm_out_bytes_per_pixel(params->out_format);
  if (obpp < 0) return obpp;
  hm_colour_desc cd = colour_desc(params, img_w, img_h, bd, I.chroma, I.native, out->has_nclx, P, obpp);
  cd.has_alpha = alpha ? 1 : 0;
  if (I.rgb_attached && !alpha) dout.swap(I.rgb); // (converted with the batch: planar_from_blobs)
  else {
    if ((rc = dout.alloc((size_t)cd.out_stride * hm_padded_rows(img_h)))) return rc;
    if ((rc = hm_colour_convert(&cd, P[0].mem.p, P[1].mem.p, P[2].mem.p, dout.p, s))) return rc;
  }
  // RGB24 / RRGGBB targets have no alpha: Op_drop_alpha_plane, the colour values do not depend on it.  RGBA: the 8-bit
  // ops copy the plane (yuv2rgb.cc:483-488)
  if (alpha && params->out_format == HM_OUT_RGBA) {
    const DevPlane* a8 = alpha;
    if (alpha_bd > 8) { // (a deeper image only, see above) Op_to_sdr_planes on the alpha plane
      if ((rc = alloc_plane(alpha_sdr, img_w, img_h, 1))) return rc;
      if ((rc = hm_launch_to_sdr(alpha->mem.p, alpha->stride, alpha_sdr.mem.p, alpha_sdr.stride, img_w, img_h, alpha_bd, s))) return rc;
      a8 = &alpha_sdr;
    }
    if ((rc = hm_launch_set_alpha(dout.p, cd.out_stride, img_w, img_h, a8->mem.p, a8->stride, s))) return rc;
  }
  const bool aa16 = params->out_format == HM_OUT_RRGGBBAA_BE || params->out_format == HM_OUT_RRGGBBAA_LE;
  if (alpha && aa16)
    if ((rc = hm_launch_set_alpha16(dout.p, cd.out_stride, img_w, img_h, alpha->mem.p, alpha->stride, alpha_bd, bd > 8 ? bd : 10,
                                    params->out_format == HM_OUT_RRGGBBAA_BE, s))) return rc;
  out->out_format = params->out_format;
  const Reported r = converted_report(I.native, I.is_grid, bd, params->out_format, params->convert_hdr_to_8bit);
  r.profile_to(out);
  out->bit_depth = r.bit_depth;
  out->stride[0] = cd.out_stride;
  out->plane_width[0] = img_w; out->plane_height[0] = img_h;
  if (t.views) { // many views of this one image: a plan per view, resolved against the profile and depth the image reports - every refusal before a byte
                 // is written -, then the one writer of them all (hm_views_write: the multi kernels where the views allow them)
    const ViewsRequest& V = *t.views;
    const hm_out_image img = {img_w, img_h, r.bit_depth, r.transfer, r.primaries, 0, 0, 0};
    std::vector<hm_out_plan> plans((size_t)V.count);
    if ((rc = views_resolve(params, t, img, HM_OUT_PROFILE_LAST, plans))) return rc;
    if ((rc = hm_views_write(V.dests, plans.data(), V.count, dout.p, cd.out_stride, s, V.scratch))) return rc;
    for (int k = 0; k < V.count; k++) {
      V.out[k].width = plans[(size_t)k].vp.ow; V.out[k].height = plans[(size_t)k].vp.oh;
      V.out[k].stride[0] = (int32_t)std::min<int64_t>(plans[(size_t)k].dp.row_pitch, 0x7FFFFFFF);
    }
    out->used_ext_dst = 1;
  }
  else if (t.dest) { // the image, or with a view a rectangle of it at vp.ow x vp.oh, through the steps of the request and nothing else (devdest.cpp): the light and
                // alpha steps resolved against the profile and depth this image reports - refused before a byte is written
    hm_out_steps st = t.steps();
    hm_out_image img = {img_w, img_h, r.bit_depth, r.transfer, r.primaries, 0, 0, 0};
    hm_out_map map = {nullptr, 0};
    if (const PlanarImage* G = t.gain_map) { // the gain map as decoded: its Y plane
      if (G->chroma != 0) return hm_fail(HM_ERR_UNSUPPORTED, "gain: the map decodes to chroma format %d, not 4:0:0 (colour gain maps are the open step)", G->chroma);
      img.map_w = G->w; img.map_h = G->h; img.map_bits = G->bd;
      map.plane = G->P[0].mem.p; map.stride = G->P[0].stride;
    }
    hm_out_plan plan;
    if ((rc = hm_out_resolve(params->out_format, &img, HM_OUT_PROFILE_LAST, t.dest, &st, &plan))) return rc;
    hm_device_tone measured_tone;
    const bool stats_only = t.measure && t.measure->mode == HM_MEASURE_STATS;
    if (LightMeasure* m = t.measure) { // the plan's rectangle is measured here, where the pixels are; the stream is waited for
      float U = plan.lp.unit_nits;
      if (stats_only && (rc = hm_stats_unit_nits(&plan.lp, m->unit_nits, &U))) return rc;
      if ((rc = hm_launch_light_stats(&plan, U, dout.p, cd.out_stride, s, &m->stats))) return rc;
      if (!stats_only) { // the tone step with the measured peak in place of the stand-in: the plan again - the knee is judged before a byte is written
        measured_tone = *st.tone;
        if ((rc = hm_light_stats_percentile(&m->stats, m->fraction, nullptr, &measured_tone.src_peak))) return rc;
        st.tone = &measured_tone;
        if ((rc = hm_out_resolve(params->out_format, &img, HM_OUT_PROFILE_LAST, t.dest, &st, &plan))) return rc;
      }
      m->done = true;
    }
    if (stats_only) {}
    else if (t.view_later) { t.view_later->dest = t.dest; t.view_later->vp = plan.vp; t.view_later->src = dout.p; t.view_later->src_stride = cd.out_stride; } // (a sequence: hm_view_write_batch)
    else if ((rc = hm_out_write(t.dest, &plan, dout.p, cd.out_stride, t.gain_map ? &map : nullptr, s, t.scratch))) return rc;
    if (t.view) {
      out->width = plan.vp.ow; out->height = plan.vp.oh;
      out->plane_width[0] = plan.vp.ow; out->plane_height[0] = plan.vp.oh;
    }
    out->used_ext_dst = 1;
    out->stride[0] = stats_only ? 0 : (int32_t)std::min<int64_t>(plan.dp.row_pitch, 0x7FFFFFFF);
  }
  else if (params->ext_dst && params->ext_dst_stride >= (uint32_t)(img_w * obpp) &&
      (size_t)params->ext_dst_len >= (size_t)params->ext_dst_stride * (size_t)img_h) {
    // caller-provided destination (fork API heif_decoding_options_add_external_dest)
    const hipError_t e = hipMemcpy2DAsync(params->ext_dst, params->ext_dst_stride, dout.p, cd.out_stride, (size_t)img_w * obpp, img_h,
                                          hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return hm_check_hip(e, "D2H ext_dst");
    out->used_ext_dst = 1;
    out->stride[0] = params->ext_dst_stride;
  }
  else if ((rc = plane_to_host(dout.p, cd.out_stride, img_h, s, &out->plane[0], &out->stride[0]))) return rc;
  return HM_OK;
}

// The output half of decode_image_user (context.cc:1516-1600) for a decoded image on the device: the result's fields, then one of
// the three writers above - all queued on `s`.  `dout` and `alpha_sdr` must live until the stream has drained.
// t: where the result goes (OutputTarget); what of it the entry points have refused against the size the file declares is asked
// again here of the decoded size, before anything is written.
int emit_image(const hm_decode_params* params, hipStream_t s, PlanarImage& I, const DevPlane* alpha, int alpha_bd, DevMem& dout, DevPlane& alpha_sdr, hm_decoded* out,
               const OutputTarget& t = OutputTarget())
{
  int rc;
  out->width = I.w; out->height = I.h; out->bit_depth = I.bd; out->chroma = I.chroma;
  out->warnings = I.warnings;
  // a grid canvas carries no nclx (context.cc:2250-2276); a single image keeps its own
  out->has_nclx = I.is_grid ? 0 : 1;
  out->primaries = I.native.primaries; out->transfer = I.native.transfer; out->matrix = I.native.matrix; out->full_range = I.native.full_range;
  // a planar YCbCr target converts when the image's chroma format or colourspace differs from it, and only then
  // (context.cc:1538-1552: "different_chroma || different_colorspace"; the depth alone - convert_hdr_to_8bit - does not)
  const bool planar_target = hm_out_is_planar(params->out_format);
  const bool as_decoded = params->out_format == 0 || (planar_target && I.chroma != 0 && I.chroma == hm_out_planar_chroma(params->out_format));
  // (planes are asked of the result's own format, by write_planes; the light step of the profile the conversion reports, by emit_interleaved)
  if ((t.dest || t.views) && (rc = target_fits(params, t, I.w, I.h, I.chroma, I.bd, 0, nullptr, false))) return rc;
  if (t.views && (as_decoded || planar_target)) return hm_fail(HM_ERR_UNSUPPORTED, "views take an interleaved output format (HM_OUT_RGB ...): output format %d is a planar one", params->out_format);
  if (t.planes && !as_decoded && !planar_target) return hm_fail(HM_ERR_INTERNAL, "device planes with the interleaved output format %d", params->out_format);
  if (as_decoded) return emit_native(params, s, I, alpha, alpha_bd, t, out);
  if (planar_target) return emit_planar(params, s, I, alpha, alpha_bd, t, out);
  return emit_interleaved(params, s, I, alpha, alpha_bd, dout, alpha_sdr, t, out);
}

// An 'unci' item: the payload - under a view the byte ranges of the internal tiles in j.sub_tiles - goes to the device and ONE launch
// of the unpack (unci.hip) leaves planes, or for an R G B item without transformations the interleaved pixels of the target; from there
// the image is an ordinary PlanarImage (an R G B item: tagged rgb_planes, its pixels in the slot a batch's attached conversion fills).
static int enqueue_unci(DecodeJob& j, hm_decoded* out)
{
  const hm_file* f = j.f;
  const hm_decode_params* params = &j.params;
  hipStream_t s = j.s;
  const hm_unci_info& u = j.unci_info;
  const hm::Item* it = f->file.item(j.id);
  PlanarImage& I = j.I;
  int rc;
  // ---- the bytes: checked against the layout before anything is queued ----
  std::vector<uint8_t> payload;
  hm::HeifError err;
  if (!f->file.item_data(j.id, payload, err)) return fail_from(err);
  if (payload.size() < u.payload_bytes)
    return hm_fail(HM_ERR_BITSTREAM, "unci: the item has %zu bytes of data, its layout needs %llu", payload.size(), (unsigned long long)u.payload_bytes);
  const int32_t* tiles = j.unci_sub ? j.sub_tiles : nullptr;
  hm_unci_info sub;
  std::vector<uint64_t> ranges;
  if ((rc = hm_unci_subgrid(&u, tiles, &sub)) || (rc = hm_unci_subgrid_ranges(&u, tiles, ranges))) return rc;
  const size_t n_bytes = (size_t)sub.payload_bytes;
  if ((rc = require_device())) return rc;
  j.unci_staging = hm_pool_pinned_alloc(n_bytes ? n_bytes : 1);
  if (!j.unci_staging) return hm_fail(HM_ERR_NOMEM, "out of memory");
  size_t at = 0;
  for (size_t k = 0; k + 1 < ranges.size(); k += 2) { std::memcpy((uint8_t*)j.unci_staging + at, payload.data() + ranges[k], (size_t)ranges[k + 1]); at += (size_t)ranges[k + 1]; }
  if (at != n_bytes) return hm_fail(HM_ERR_INTERNAL, "unci: the tile ranges hold %zu bytes, the sub-grid's layout %zu", at, n_bytes);
  if ((rc = j.unci_bytes.alloc((n_bytes + 3) & ~(size_t)3))) return hm_fail(rc, "out of device memory");
  if ((rc = hm_check_hip(hipMemcpyAsync(j.unci_bytes.p, j.unci_staging, n_bytes, hipMemcpyHostToDevice, s), "H2D unci payload"))) return rc;
  // ---- the image ----
  int lo, hi;
  unci_colour_depths(u, &lo, &hi);
  const int alpha_depth = unci_alpha_depth(u);
  const bool rgb = u.colour_space == HM_UNCI_RGB;
  I.w = sub.width; I.h = sub.height; I.bd = hi; I.rgb_planes = rgb;
  I.chroma = u.colour_space == HM_UNCI_MONO ? 0 : rgb ? 3 : u.sampling == HM_UNCI_SAMPLING_420 ? 1 : u.sampling == HM_UNCI_SAMPLING_422 ? 2 : 3;
  I.native = it->props.colr;
  I.is_grid = !it->props.colr.present; // (an image that carries no nclx: what a grid canvas is to the output rules - no profile handed out, the defaults converted with)
  const std::vector<hm::Transform> none;
  const std::vector<hm::Transform>& transforms = params->ignore_transformations ? none : it->props.transforms;
  const int fmt = params->out_format;
  const bool pixels = rgb && fmt != 0;
  const bool wide = fmt == HM_OUT_RRGGBB_LE || fmt == HM_OUT_RRGGBBAA_LE, four = fmt == HM_OUT_RGBA || fmt == HM_OUT_RRGGBBAA_LE;
  const int obpp = pixels ? hm_out_bytes_per_pixel(fmt) : 0;
  const bool direct = pixels && transforms.empty(); // the kernel writes the target's pixels itself
  hm_planes planes;
  std::memset(&planes, 0, sizeof(planes));
  if (!direct) {
    for (int c = 0; c < u.n_components; c++) {
      const int p = hm_unci_plane_of(u.colour_space, u.comp[c].type);
      if (p < 0) continue;
      DevPlane& D = p == 3 ? j.unci_alpha : I.P[p];
      const bool ch = p == 1 || p == 2;
      const int pw = ch && (I.chroma == 1 || I.chroma == 2) ? I.w / 2 : I.w, ph = ch && I.chroma == 1 ? I.h / 2 : I.h;
      if ((rc = alloc_plane(D, pw, ph, hm_sample_bytes(u.comp[c].depth)))) return hm_fail(rc, "out of device memory");
      planes.plane[p] = D.mem.p; planes.stride[p] = D.stride;
    }
  }
  hm_device_dest px;
  std::memset(&px, 0, sizeof(px));
  int px_stride = 0;
  if (pixels) {
    px_stride = hm_plane_stride(I.w, obpp);
    if (direct) {
      if ((rc = I.rgb.alloc((size_t)px_stride * hm_padded_rows(I.h)))) return hm_fail(rc, "out of device memory");
      px.ptr = I.rgb.p; px.len = (uint64_t)px_stride * I.h; px.layout = HM_DEV_LAYOUT_HWC; px.dtype = wide ? HM_DEV_U16 : HM_DEV_U8; px.row_pitch = px_stride;
    }
  }
  if ((rc = hm_unci_unpack(&u, j.unci_bytes.p, n_bytes, tiles, direct ? nullptr : &planes, fmt, direct ? &px : nullptr, s))) return rc;
  const DevPlane* alpha = alpha_depth && !direct ? &j.unci_alpha : nullptr;
  if (!transforms.empty()) {
    // every plane of an R G B item on its own (their depths may differ), the planes of a YCbCr item together, the alpha plane like a luma plane
    if (rgb) {
      for (int c = 0; c < 3; c++) {
        int w = I.w, h = I.h;
        int depth = 8;
        for (int k = 0; k < u.n_components; k++) if (hm_unci_plane_of(u.colour_space, u.comp[k].type) == c) depth = u.comp[k].depth;
        if ((rc = apply_transforms_plane(transforms, I.P[c], w, h, depth > 8 ? 16 : 8, s, I.retired))) return rc;
        if (c == 2) { I.w = w; I.h = h; }
      }
    }
    else if ((rc = apply_transforms(transforms, I.P, I.w, I.h, I.chroma, I.bd > 8 ? 16 : 8, s, I.retired))) return rc;
    int aw = sub.width, ah = sub.height;
    if (alpha && (rc = apply_transforms_plane(transforms, j.unci_alpha, aw, ah, alpha_depth > 8 ? 16 : 8, s, I.retired))) return rc;
  }
  if (pixels && !direct) { // through the planes and an interleave
    px_stride = hm_plane_stride(I.w, obpp);
    if ((rc = I.rgb.alloc((size_t)px_stride * hm_padded_rows(I.h)))) return hm_fail(rc, "out of device memory");
    const void* src[4] = {I.P[0].mem.p, I.P[1].mem.p, I.P[2].mem.p, four && alpha ? alpha->mem.p : nullptr};
    const int32_t stride[4] = {I.P[0].stride, I.P[1].stride, I.P[2].stride, alpha ? alpha->stride : 0};
    if ((rc = hm_launch_unci_interleave(src, stride, wide, I.w, I.h, four ? 4 : 3, I.rgb.p, px_stride, s))) return rc;
  }
  if (pixels) { I.rgb_attached = true; alpha = nullptr; } // (the alpha component is in the pixels already)
  out->has_alpha = alpha_depth ? 1 : 0;
  // what the colour ops refuse of an alpha plane (job_enqueue states the reasons)
  if (alpha && fmt == HM_OUT_RGBA && alpha_depth != 8 && I.bd == 8) return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with an 8-bit image and an RGBA target", alpha_depth);
  if (alpha && (fmt == HM_OUT_RRGGBBAA_BE || fmt == HM_OUT_RRGGBBAA_LE) && (alpha_depth > 8) != (I.bd > 8))
    return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with a %d-bit image and an RRGGBBAA target", alpha_depth, I.bd);
  OutputTarget t = j.target.t;
  t.scratch = &j.view_scratch;
  hm_device_view shifted = j.target.view; // (the crop inside the sub-grid that was unpacked)
  if (t.view && (shifted.crop_w || shifted.crop_h)) { shifted.crop_x -= j.view_dx; shifted.crop_y -= j.view_dy; }
  if (t.view) t.view = &shifted;
  return emit_image(params, s, I, alpha, alpha_depth, j.dout, j.alpha_sdr, out, t);
}

// Everything after the host entropy decode, queued on j.s without waiting: GPU batch(es), transforms, alpha, colour
// conversion (HeifContext::decode_image_user, context.cc:1516-1600) and the copy to (pinned) host memory.
int job_enqueue(DecodeJob& j, hm_decoded* out)
{
  const hm_file* f = j.f;
  const hm_decode_params* params = &j.params;
  hipStream_t s = j.s;
  std::memset(out, 0, sizeof(*out));
  j.enqueued = true; // from here on the destructor drains the stream before buffers are released
  if (j.unci) return enqueue_unci(j, out);
  Lap lap;
  PlanarImage &I = j.I, &A = j.A;
  int rc = planar_from_blobs(f, j.item[0], params, s, I, /*attach=*/j.n_items == 1);
  if (rc) return rc;
  // ---- alpha channel: the auxiliary image's Y plane becomes the alpha plane, scaled nearest-neighbour if its size
  //      differs (context.cc:2029-2078) ----
  const DevPlane* alpha = nullptr;
  if (j.n_items > 1) {
    if ((rc = planar_from_blobs(f, j.item[1], params, s, A))) return rc;
    // what the colour ops refuse is refused before more work is queued: an 8-bit image's chain to RGBA has no op that
    // changes the alpha plane's depth and the interleave wants 8 bits (rgb2rgb.cc:81-84); a deeper image's chain runs
    // Op_to_sdr_planes, which brings a deeper alpha plane to 8 bits too (hdr_sdr.cc:176-195)
    if (params->out_format == HM_OUT_RGBA && A.bd != 8 && I.bd == 8) return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with an 8-bit image and an RGBA target", A.bd);
    // RRGGBBAA: the alpha plane travels through the image's depth op (Op_to_hdr_planes reads every plane as 8 bit) or is
    // copied as 16-bit words (rgb2rgb.cc:207-211, yuv2rgb.cc:575-592): only planes of the image's own depth class work
    if ((params->out_format == HM_OUT_RRGGBBAA_BE || params->out_format == HM_OUT_RRGGBBAA_LE) && (A.bd > 8) != (I.bd > 8))
      return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with a %d-bit image and an RRGGBBAA target", A.bd, I.bd);
    alpha = &A.P[0];
    if (A.w != I.w || A.h != I.h) {
      if ((rc = alloc_plane(j.alpha_scaled, I.w, I.h, hm_sample_bytes(A.bd)))) return rc;
      if ((rc = hm_launch_scale_nn(hm_sample_bytes(A.bd), A.P[0].mem.p, A.P[0].stride, A.w, A.h, j.alpha_scaled.mem.p, j.alpha_scaled.stride, I.w, I.h, s))) return rc;
      alpha = &j.alpha_scaled;
    }
    out->has_alpha = 1;
  }
  else if (I.tile_alpha_bd) {
    // the canvas' own alpha plane (tiles with alpha images); an alpha image of the grid item itself - handled above -
    // replaces it (transfer_plane_from_image_as, context.cc:2072)
    if (params->out_format == HM_OUT_RGBA && I.tile_alpha_bd != 8 && I.bd == 8) return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with an 8-bit image and an RGBA target", I.tile_alpha_bd);
    if ((params->out_format == HM_OUT_RRGGBBAA_BE || params->out_format == HM_OUT_RRGGBBAA_LE) && (I.tile_alpha_bd > 8) != (I.bd > 8))
      return hm_fail(HM_ERR_UNSUPPORTED, "alpha plane of %d bits with a %d-bit image and an RRGGBBAA target", I.tile_alpha_bd, I.bd);
    alpha = &I.tile_alpha;
    out->has_alpha = 1;
  }
  const int alpha_bd = j.n_items > 1 ? A.bd : I.tile_alpha_bd;
  lap("planar decode queued");
  OutputTarget t = j.target.t;
  t.scratch = &j.view_scratch;
  if (j.has_map) { // the gain map: an image decoded like any other, on the job's stream; its own irot / imir / clap apply
    if ((rc = planar_from_blobs(f, j.item[2], params, s, j.G))) return rc;
    t.gain_map = &j.G;
  }
  hm_device_view shifted = j.target.view; // (the crop inside the sub-grid that was decoded)
  if (t.view && (shifted.crop_w || shifted.crop_h)) { shifted.crop_x -= j.view_dx; shifted.crop_y -= j.view_dy; }
  if (t.view) t.view = &shifted;
  t.views_dx = j.view_dx; t.views_dy = j.view_dy; // (many views: each crop moves the same way, view by view)
  rc = emit_image(params, s, I, alpha, alpha_bd, j.dout, j.alpha_sdr, out, t);
  if (rc) return rc;
  lap("colour + D2H queued");
  return HM_OK;
}

// what of a planar destination needs no file: params (ext_dst, an interleaved target), the planes' static checks, a null pointer of Y
static int check_planes_params(const hm_decode_params* params, const hm_device_planes* planes)
{
  if (params->ext_dst) return hm_fail(HM_ERR_INVALID_ARG, "params->ext_dst must be NULL with device planes");
  if (params->out_format != 0 && !hm_out_is_planar(params->out_format)) {
    if (hm_out_bytes_per_pixel(params->out_format) > 0)
      return hm_fail(HM_ERR_INVALID_ARG, "device planes take planar YCbCr (out_format 0 or HM_OUT_YCBCR_*): interleaved output format %d goes through hm_decode_item_to_device",
                     params->out_format);
    return hm_fail(HM_ERR_INVALID_ARG, "device planes: output format %d is not a planar one", params->out_format);
  }
  const int rc = hm_planes_check_static(planes);
  if (rc) return rc;
  if (!planes->plane[0].ptr) return hm_fail(HM_ERR_INVALID_ARG, "device planes: plane[0].ptr is null");
  return HM_OK;
}

// ---- the three phases of check_target_request; a sequence (decode_sequence) loops each over its frames ----
// the request alone.  frame: of a sequence (its null-ptr message names the frame), else -1
static int check_request_alone(const hm_decode_params* params, const OutputTarget& t, int frame = -1)
{
  int rc = target_check_shape(t);
  if (rc) return rc;
  if (t.views) { // what the single-view entry asks of a view's request, view by view
    const ViewsRequest& V = *t.views;
    if (params->ext_dst) return hm_fail(HM_ERR_INVALID_ARG, "params->ext_dst must be NULL with a device destination");
    hm_out_steps st = t.steps();
    for (int k = 0; k < V.count; k++) {
      st.view = &V.views[k];
      if ((rc = hm_out_check_static(params->out_format, &V.dests[k], &st, 0))) return view_refused(V, k, rc);
      if (!V.dests[k].ptr) { hm_fail(HM_ERR_INVALID_ARG, "device destination: null ptr"); return view_refused(V, k, HM_ERR_INVALID_ARG); }
    }
  }
  if (t.dest) {
    if (params->ext_dst) return hm_fail(HM_ERR_INVALID_ARG, "params->ext_dst must be NULL with a device destination");
    const hm_out_steps st = t.steps();
    if ((rc = hm_out_check_static(params->out_format, t.dest, &st, 0))) return rc;
    if (!t.dest->ptr)
      return frame < 0 ? hm_fail(HM_ERR_INVALID_ARG, "device destination: null ptr")
                       : hm_fail(HM_ERR_INVALID_ARG, "device destination of frame %d: null ptr", frame);
  }
  return t.planes ? check_planes_params(params, t.planes) : (int)HM_OK;
}

// the target against what the file declares for `id`, kept in `info` for the pointers.  A file that fails here, or declares nothing usable
// for planes, is "size unknown" (info.width 0): such an item fails the decode with its own message.
// alpha_bits: -1, the decode's to say whether there is an alpha plane and of which depth; 0: none (the frames of a sequence)
// (params->ignore_transformations picks the coded size for a frame of a sequence too, where the sequence's own loops took
//  info.width: a frame carries no transformations, the two sizes are one)
static int check_request_declared(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& t, int alpha_bits,
                                  hm_image_info& info)
{
  const bool usable = hm_file_image_info(f, id, &info) == HM_OK &&
                      (!t.planes || (info.bit_depth >= 8 && info.bit_depth <= 16 && info.chroma >= 0 && info.chroma <= 3));
  if (!usable) info.width = 0;
  else if (params->ignore_transformations) { info.width = info.coded_width; info.height = info.coded_height; }
  return target_fits(params, t, info.width, info.height, info.chroma, info.bit_depth, alpha_bits, nullptr, false);
}

// a device and the pointers: a destination's needs no size; the planes' are judged against the declared result, which target_fits
// resolves once more for it (view, planes, len: as the sequence always did - for a single item the second pass is new, and repeats
// what has just passed)
static int check_request_pointers(const hm_decode_params* params, const OutputTarget& t, int alpha_bits, const hm_image_info& info)
{
  return target_fits(params, t, t.planes ? info.width : 0, info.height, info.chroma, info.bit_depth, alpha_bits, nullptr, true);
}

int check_target_request(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& t)
{
  hm_image_info info{};
  int rc;
  if ((rc = check_request_alone(params, t)) || (rc = check_request_declared(f, id, params, t, -1, info))) return rc;
  return check_request_pointers(params, t, -1, info);
}

hm_device_tone tone_for_item(const hm_file* f, uint32_t id, const hm_device_tone* tone)
{
  hm_device_tone t = *tone;
  if (t.src_peak != 0.0f) return t;
  const hm::Item* it = f && id && !f->file.is_movie() ? f->file.item(id) : nullptr;
  t.src_peak = it ? hm_tone_peak_of(it->props.has_clli, it->props.clli[0], it->props.has_mdcv, it->props.mdcv_lum[0]) : 1000.0f;
  return t;
}

int job_complete(DecodeJob& j, hm_decoded*)
{
  const hipError_t e = hipStreamSynchronize(j.s);
  if (e != hipSuccess) return hm_check_hip(e, "kernel execution");
  // (the reconstruction bounds its cross-wave waits: a wave that gave up has flagged its launch)
  for (PlanarImage* im : {&j.I, &j.A, &j.G})
    if (im->batch) {
      const int rc = hm_batch_check(im->batch.get());
      if (rc) return rc;
    }
  return HM_OK;
}

} // namespace hm_img

// ---- derived image items: 'iden' and 'iovl' -------------------------------------------------------------------------------
// HeifContext::decode_derived_image / decode_overlay_image (context.cc:2542-2675).  A derived item is resolved recursively into
// the coded images (hvc1 items, grids) under it; the entropy decode of ALL their pictures - tiles and alpha pictures included -
// runs in one fan-out of the crew; every coded image then goes through the planar path of hm_decode_item on the call's stream (one
// hm_batch each: merging them is not part of this), and k_overlay (overlay.hip) composes the layers of an overlay in one pass.
//   iden : the child decoded with the transformation list child ++ iden (also applied to the attached alpha plane)
//   iovl : layers bottom to top, each clipped to the canvas (DESIGN Q20); children that do not touch the canvas - under a view: the
//          crop - are not decoded.  A nested overlay is composed into R, G, B planes first and enters as a layer with matrix 0 at
//          full range (the copy arm of Op_YCbCr_to_RGB).  An hvc1 child for which the reference finds no colour chain (anything but
//          4:4:4) is decoded as the 1 x 1 grid of itself (DESIGN Q19).
namespace {

bool is_derived_item(const hm_file* f, uint32_t id)
{
  const hm::Item* it = f->file.item(id);
  return it && (it->type == "iden" || it->type == "iovl");
}

// the size an image handle reports after `list` (context.cc:810-838): what hm_file_image_info does for an item's own list
void handle_size_after(const std::vector<hm::Transform>& list, int64_t& w, int64_t& h)
{
  for (const hm::Transform& t : list) {
    if (t.kind == hm::Transform::CleanAperture && t.width_d && t.height_d && t.width_n <= 0x7FFFFFFFu && t.width_d <= 0x7FFFFFFFu &&
        t.height_n <= 0x7FFFFFFFu && t.height_d <= 0x7FFFFFFFu) {
      w = hm::Fraction((int32_t)t.width_n, (int32_t)t.width_d).round();
      h = hm::Fraction((int32_t)t.height_n, (int32_t)t.height_d).round();
    }
    else if (t.kind == hm::Transform::Rotate && (t.angle == 90 || t.angle == 270)) std::swap(w, h);
  }
}

// the size item `id` will have as a layer, from what the file declares (no picture is looked at): the plan decides with it which
// children are decoded; the rectangle the kernel gets comes from the decoded size
int declared_layer_size(const hm_file* f, uint32_t id, bool ignore_transformations, int depth, int64_t& w, int64_t& h)
{
  if (depth > HM_OVL_MAX_DEPTH) return hm_fail(HM_ERR_BITSTREAM, "derived images nested deeper than %d", HM_OVL_MAX_DEPTH);
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_BITSTREAM, "derived image references the missing item %u", id);
  hm::HeifError err;
  if (it->type == "iden") {
    const uint32_t child = f->file.derived_child(id, err);
    if (!child) return fail_from(err);
    const int rc = declared_layer_size(f, child, ignore_transformations, depth + 1, w, h);
    if (rc) return rc;
  }
  else if (it->type == "iovl") {
    hm::OverlayInfo o;
    if (!f->file.overlay_info(id, o, err)) return fail_from(err);
    w = o.width; h = o.height;
  }
  else if (it->type == "grid") {
    hm::GridInfo g;
    if (!f->file.grid_info(id, g, err)) return fail_from(err);
    w = g.width; h = g.height;
  }
  else if (it->type == "hvc1") { w = it->props.ispe_width; h = it->props.ispe_height; }
  else return hm_fail(HM_ERR_UNSUPPORTED, "item type '%s' under a derived image", it->type.c_str());
  if (!ignore_transformations) handle_size_after(it->props.transforms, w, h);
  return HM_OK;
}

// what the kernel (or emit_image) gets of a decoded node
struct LayerImage {
  DevPlane* P[3] = {nullptr, nullptr, nullptr}; // Y, Cb, Cr - or G, B, R of a composed overlay
  DevPlane* alpha = nullptr;
  int w = 0, h = 0, chroma = 0;
  int has_nclx = 0, matrix = 2, primaries = 2, full_range = 1;
};

struct DerivedNode {
  uint32_t id = 0;
  bool overlay = false;
  std::vector<hm::Transform> list; // overlay: its own transformations ++ those of the 'iden' items above; coded: those of the 'iden' items above
  // a coded image (hvc1 / grid)
  std::unique_ptr<DecodeJob> job;
  // an overlay
  hm::OverlayInfo info;
  std::vector<std::unique_ptr<DerivedNode>> children; // NULL: the child touches nothing that is asked for and is not decoded
  DevPlane rgb[3]; // R, G, B of the composed canvas (a nested or transformed overlay)
};

// everything one call holds; the stream is drained before any of it is released
struct DerivedRun {
  const hm_file* f = nullptr;
  hm_decode_params params{};       // the caller's
  hm_decode_params child_params{}; // what the coded images are decoded with: native planes, no caller buffer
  hipStream_t s = nullptr;
  std::unique_ptr<DerivedNode> root;
  std::vector<DecodeJob*> jobs;    // every coded image under the root, in decode order
  std::vector<std::unique_ptr<DevMem>> retired;
  std::vector<void*> pinned;       // layer tables
  PlanarImage final_image;
  DevMem dout;
  DevPlane alpha_sdr;
  hm_view_scratch view_scratch{};
  bool enqueued = false;
  ~DerivedRun()
  {
    if (enqueued) hipStreamSynchronize(s);
    for (void* p : pinned) hm_pool_pinned_free(p);
    hm_view_scratch_free(&view_scratch);
  }
};

// deepest coded picture (image, tiles, alpha pictures) under a coded image item, from the hvcC boxes
int declared_depth(const hm_file* f, uint32_t id)
{
  const hm::Item* it = f->file.item(id);
  if (!it) return 0;
  int bd = 0;
  auto take = [&](uint32_t pid) {
    const hm::Item* pi = f->file.item(pid);
    if (pi && pi->props.hvcc.present) bd = std::max(bd, std::max(pi->props.hvcc.bit_depth_luma, pi->props.hvcc.bit_depth_chroma));
    const uint32_t a = f->file.alpha_item_of(pid);
    const hm::Item* ai = a ? f->file.item(a) : nullptr;
    if (ai && ai->type == "hvc1" && ai->props.hvcc.present) bd = std::max(bd, ai->props.hvcc.bit_depth_luma);
    if (ai && ai->type == "grid")
      for (uint32_t t : f->file.references(a, "dimg")) {
        const hm::Item* ti = f->file.item(t);
        if (ti && ti->props.hvcc.present) bd = std::max(bd, ti->props.hvcc.bit_depth_luma);
      }
  };
  take(id);
  if (it->type == "grid")
    for (uint32_t t : f->file.references(id, "dimg")) take(t);
  return bd;
}

// Resolves item `id` into a node.  above: the transformations of the 'iden' items passed on the way down (applied behind the
// node's own); crop (may be NULL; the root only): the rectangle of the result a view asks for; path: the derived items above
// (reference cycles).  Every refusal that needs no picture happens here, before a device is needed.
int build_node(DerivedRun& R, uint32_t id, int depth, const std::vector<hm::Transform>& above, const hm_device_view* crop, std::vector<uint32_t>& path,
               std::unique_ptr<DerivedNode>& out)
{
  const hm_file* f = R.f;
  if (depth > HM_OVL_MAX_DEPTH) return hm_fail(HM_ERR_BITSTREAM, "derived images nested deeper than %d", HM_OVL_MAX_DEPTH);
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_BITSTREAM, "derived image references the missing item %u", id);
  for (uint32_t p : path)
    if (p == id) return hm_fail(HM_ERR_BITSTREAM, "derived image items reference each other in a cycle (item %u)", id);
  hm::HeifError err;
  const bool ignore = R.params.ignore_transformations != 0;
  if (it->type == "iden" || it->type == "iovl") {
    if (f->file.alpha_item_of(id)) return hm_fail(HM_ERR_UNSUPPORTED, "an alpha auxiliary image attached to the derived item %u ('%s') is not supported", id, it->type.c_str());
    std::vector<hm::Transform> list;
    if (!ignore) { list = it->props.transforms; list.insert(list.end(), above.begin(), above.end()); }
    path.push_back(id);
    int rc = HM_OK;
    if (it->type == "iden") {
      const uint32_t child = f->file.derived_child(id, err);
      if (!child) return fail_from(err);
      rc = build_node(R, child, depth + 1, list, nullptr, path, out);
      path.pop_back();
      return rc;
    }
    std::unique_ptr<DerivedNode> n(new DerivedNode());
    n->id = id; n->overlay = true; n->list = list;
    if (!f->file.overlay_info(id, n->info, err)) return fail_from(err);
    if (n->info.width > 32768 || n->info.height > 32768) return hm_fail(HM_ERR_BITSTREAM, "Image size exceeds the maximum of 32768x32768 (security limit)");
    const bool use_crop = crop && list.empty() && crop->crop_w > 0 && crop->crop_h > 0;
    n->children.resize(n->info.children.size());
    for (size_t i = 0; i < n->info.children.size(); i++) {
      int64_t w = 0, h = 0;
      if ((rc = declared_layer_size(f, n->info.children[i], ignore, depth + 1, w, h))) return rc;
      const hm_ovl_rect r = hm::overlay_clip(n->info.width, n->info.height, w, h, n->info.dx[i], n->info.dy[i], false);
      const bool touches = use_crop ? hm::overlay_touches(r, crop->crop_x, crop->crop_y, crop->crop_w, crop->crop_h) : hm::overlay_touches(r);
      if (!touches) continue;
      if ((rc = build_node(R, n->info.children[i], depth + 1, {}, nullptr, path, n->children[i]))) return rc;
    }
    path.pop_back();
    out = std::move(n);
    return HM_OK;
  }
  if (it->type != "hvc1" && it->type != "grid") return hm_fail(HM_ERR_UNSUPPORTED, "item type '%s' under a derived image", it->type.c_str());
  const int bd = declared_depth(f, id);
  if (bd > 8) return hm_fail(HM_ERR_UNSUPPORTED, "derived images over pictures or alpha planes deeper than 8 bits (item %u: %d bits) are not supported", id, bd);
  std::unique_ptr<DerivedNode> n(new DerivedNode());
  n->id = id;
  if (!ignore) n->list = above;
  n->job.reset(new DecodeJob());
  DecodeJob& j = *n->job;
  j.f = f; j.id = id; j.params = R.child_params; j.s = R.s;
  // Q19: the reference's first conversion has a chain for a 4:4:4 picture only
  j.self_grid = it->type == "hvc1" && it->props.hvcc.present && it->props.hvcc.chroma_format != 3;
  const int rc = job_plan(j);
  if (rc) return rc;
  R.jobs.push_back(&j);
  out = std::move(n);
  return HM_OK;
}

// the targets a derived item is refused for (no picture is looked at)
int derived_target_check(const DerivedNode& root, const hm_decode_params* params, bool planes)
{
  const int of = params->out_format;
  if (root.overlay) {
    if (planes || (of != HM_OUT_RGB && of != HM_OUT_RGBA))
      return hm_fail(HM_ERR_UNSUPPORTED, "an overlay ('iovl') item decodes to interleaved HM_OUT_RGB / HM_OUT_RGBA only (%s)",
                     planes ? "device planes asked for" : of == 0 ? "out_format 0 asked for" : hm_out_is_planar(of) ? "a planar HM_OUT_YCBCR_* target asked for" : "an RRGGBB target asked for");
    return HM_OK;
  }
  const bool native = planes || of == 0 || hm_out_is_planar(of);
  if (native && !root.job->item[0].is_grid)
    return hm_fail(HM_ERR_UNSUPPORTED, "an 'iden' item over a 4:4:4 coded image has R, G, B planes in the reference: planar and native targets are not supported");
  return HM_OK;
}

int derived_prepare(DerivedRun& R, const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, bool planes)
{
  R.f = f; R.params = *params; R.s = (hipStream_t)params->stream;
  R.child_params = *params;
  R.child_params.out_format = 0; R.child_params.ext_dst = nullptr; R.child_params.ext_dst_len = 0; R.child_params.ext_dst_stride = 0;
  std::vector<uint32_t> path;
  int rc = build_node(R, id, 0, {}, view, path, R.root);
  if (rc) return rc;
  return derived_target_check(*R.root, params, planes);
}

// a coded image on the device: hm_decode_item's planar path, its alpha plane at the image's size, then `list`
int produce_coded(DerivedRun& R, DerivedNode& n, LayerImage& L)
{
  DecodeJob& j = *n.job;
  hipStream_t s = R.s;
  j.enqueued = true;
  int rc = planar_from_blobs(R.f, j.item[0], &j.params, s, j.I);
  if (rc) return rc;
  DevPlane* alpha = nullptr;
  if (j.n_items > 1) { // (job_enqueue: the auxiliary image's Y plane, scaled nearest neighbour to the image's size)
    if ((rc = planar_from_blobs(R.f, j.item[1], &j.params, s, j.A))) return rc;
    alpha = &j.A.P[0];
    if (j.A.w != j.I.w || j.A.h != j.I.h) {
      if ((rc = alloc_plane(j.alpha_scaled, j.I.w, j.I.h, 1))) return rc;
      if ((rc = hm_launch_scale_nn(1, j.A.P[0].mem.p, j.A.P[0].stride, j.A.w, j.A.h, j.alpha_scaled.mem.p, j.alpha_scaled.stride, j.I.w, j.I.h, s))) return rc;
      alpha = &j.alpha_scaled;
    }
  }
  else if (j.I.tile_alpha_bd) alpha = &j.I.tile_alpha;
  if (!n.list.empty()) {
    int w = j.I.w, h = j.I.h;
    if ((rc = apply_transforms(n.list, j.I.P, w, h, j.I.chroma, j.I.bd, s, j.I.retired))) return rc;
    int aw = j.I.w, ah = j.I.h;
    if (alpha && (rc = apply_transforms_plane(n.list, *alpha, aw, ah, 8, s, j.I.retired))) return rc;
    j.I.w = w; j.I.h = h;
  }
  for (int c = 0; c < 3; c++) L.P[c] = j.I.P[c].mem.p ? &j.I.P[c] : nullptr;
  L.alpha = alpha;
  L.w = j.I.w; L.h = j.I.h; L.chroma = j.I.chroma;
  // (emit_image: a grid canvas carries no nclx, a single image its own)
  L.has_nclx = j.I.is_grid ? 0 : 1;
  L.matrix = j.I.native.matrix; L.primaries = j.I.native.primaries; L.full_range = j.I.native.full_range;
  return HM_OK;
}

void layer_of(const LayerImage& L, const hm_ovl_rect& r, hm_overlay_layer& o)
{
  std::memset(&o, 0, sizeof(o));
  o.rect = r;
  const DevPlane* pl[4] = {L.P[0], L.P[1], L.P[2], L.alpha};
  for (int c = 0; c < 4; c++)
    if (pl[c]) { o.plane[c] = pl[c]->mem.p; o.pitch[c] = pl[c]->stride; o.plane_w[c] = pl[c]->w; o.plane_h[c] = pl[c]->h; }
  o.width = L.w; o.height = L.h; o.chroma = L.chroma;
  o.has_nclx = L.has_nclx; o.matrix = L.matrix; o.primaries = L.primaries; o.full_range = L.full_range;
}

int launch_overlay(DerivedRun& R, const hm_overlay_job& job, const std::vector<hm_overlay_layer>& layers)
{
  void* pinned = nullptr;
  void* device = nullptr;
  const int rc = hm_launch_overlay(&job, layers.data(), (int)layers.size(), &pinned, &device, R.s);
  if (pinned) R.pinned.push_back(pinned);
  if (device) { R.retired.emplace_back(new DevMem()); R.retired.back()->p = device; }
  return rc;
}

int produce_node(DerivedRun& R, DerivedNode& n, LayerImage& L);

// the layers of an overlay decoded and composed: interleaved into `interleaved` (out_kind RGB24 / RGBA32, pitch), or into n.rgb
int compose_overlay(DerivedRun& R, DerivedNode& n, int out_kind, void* interleaved, int pitch)
{
  const int cw = (int)n.info.width, ch = (int)n.info.height;
  std::vector<hm_overlay_layer> layers;
  int rc;
  for (size_t i = 0; i < n.children.size(); i++) {
    if (!n.children[i]) continue;
    LayerImage L;
    if ((rc = produce_node(R, *n.children[i], L))) return rc;
    const hm_ovl_rect r = hm::overlay_clip(cw, ch, L.w, L.h, n.info.dx[i], n.info.dy[i], L.alpha == nullptr);
    if (!hm::overlay_touches(r)) continue; // (the decoded size differs from the declared one)
    layers.emplace_back();
    layer_of(L, r, layers.back());
  }
  hm_overlay_job job;
  std::memset(&job, 0, sizeof(job));
  job.width = cw; job.height = ch;
  for (int c = 0; c < 3; c++) job.background[c] = (uint8_t)(n.info.background[c] >> 8); // fill_RGB_16bit, pixelimage.cc:947-1019
  job.out_kind = out_kind;
  if (out_kind == HM_OVL_OUT_PLANES) {
    for (int c = 0; c < 3; c++) {
      if ((rc = alloc_plane(n.rgb[c], cw, ch, 1))) return rc;
      job.out[c] = n.rgb[c].mem.p;
    }
    job.out_pitch = n.rgb[0].stride;
  }
  else { job.out[0] = interleaved; job.out_pitch = pitch; }
  return launch_overlay(R, job, layers);
}

int produce_node(DerivedRun& R, DerivedNode& n, LayerImage& L)
{
  if (!n.overlay) return produce_coded(R, n, L);
  int rc = compose_overlay(R, n, HM_OVL_OUT_PLANES, nullptr, 0);
  if (rc) return rc;
  int w = (int)n.info.width, h = (int)n.info.height;
  if (!n.list.empty() && (rc = apply_transforms(n.list, n.rgb, w, h, 3, 8, R.s, R.retired))) return rc;
  // R, G, B as the planes of a GBR image: Cr -> R, Y -> G, Cb -> B (yuv2rgb.cc:207-212)
  L.P[0] = &n.rgb[1]; L.P[1] = &n.rgb[2]; L.P[2] = &n.rgb[0];
  L.alpha = nullptr;
  L.w = w; L.h = h; L.chroma = 3;
  L.has_nclx = 1; L.matrix = 0; L.primaries = 2; L.full_range = 1;
  return HM_OK;
}

// what a derived item is refused for without looking at a picture (the device entry points ask before they need a device)
int derived_refusal(const hm_file* f, uint32_t id, const hm_decode_params* params, bool planes)
{
  DerivedRun R;
  return derived_prepare(R, f, id, params, nullptr, planes);
}

// hm_decode_item and its device forms on a derived item
int decode_derived(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& target, hm_decoded* out)
{
  std::memset(out, 0, sizeof(*out));
  Lap lap;
  DerivedRun R;
  int rc = derived_prepare(R, f, id, params, target.view, target.planes != nullptr);
  if (rc) return rc;
  OutputTarget t = target;
  t.scratch = &R.view_scratch;
  // ---- host: the entropy decode of every coded picture under the item, one fan-out ----
  std::vector<std::pair<DecodeJob*, int>> work;
  for (DecodeJob* j : R.jobs)
    for (int k = 0, nk = job_tile_count(*j); k < nk; k++) work.push_back({j, k});
  const int nt = (int)work.size();
  for (DecodeJob* j : R.jobs) j->few_pictures = nt <= 64;
  Crew::for_each(nt, params->host_threads, [&](int i, int row_threads) { job_parse_tile(*work[i].first, work[i].second, row_threads); });
  lap("host entropy decode done");
  // what only the pictures say, before anything is queued: the composition is one of 8-bit samples
  for (DecodeJob* j : R.jobs)
    for (int i = 0; i < j->n_items; i++) {
      ItemPlan& P = j->item[i];
      for (size_t k = 0; k < P.blobs.size(); k++) {
        if (P.status[k]) return tile_failure(P, (int)k);
        const hm_pic* h = hm_pic_of(P.blobs[k].p);
        if (h->bit_depth_y > 8 || h->bit_depth_c > 8)
          return hm_fail(HM_ERR_UNSUPPORTED, "derived images over pictures or alpha planes deeper than 8 bits (item %u: %d bits) are not supported", P.tiles[k].id, (int)h->bit_depth_y);
        if (i == 0 && P.self_grid != (h->chroma_format != 3) && !P.is_grid)
          return hm_fail(HM_ERR_BITSTREAM, "item %u: the picture's chroma format differs from its hvcC", P.tiles[k].id);
      }
      for (size_t k = 0; k < P.alpha_blobs.size(); k++) {
        if (P.alpha_status[k]) return hm_fail(P.alpha_status[k], "alpha image of tile %d (item %u): %s", P.tile_alpha[k].tile, P.tile_alpha[k].id, P.alpha_messages[k].c_str());
        if (hm_pic_of(P.alpha_blobs[k].p)->bit_depth_y > 8)
          return hm_fail(HM_ERR_UNSUPPORTED, "derived images over pictures or alpha planes deeper than 8 bits (item %u) are not supported", P.tile_alpha[k].id);
      }
    }
  R.enqueued = true;
  rc = [&]() -> int {
  DerivedNode& root = *R.root;
  PlanarImage& I = R.final_image;
  if (!root.overlay) { // 'iden' over a coded image: the image itself with the longer list
    LayerImage L;
    if ((rc = produce_coded(R, root, L))) return rc;
    if (L.alpha) out->has_alpha = 1;
    rc = emit_image(params, R.s, root.job->I, L.alpha, 8, R.dout, R.alpha_sdr, out, t);
    if (L.alpha && !rc) out->has_alpha = 1;
  }
  else {
    const int obpp = params->out_format == HM_OUT_RGBA ? 4 : 3;
    const int kind = obpp == 4 ? HM_OVL_OUT_RGBA32 : HM_OVL_OUT_RGB24;
    int w = (int)root.info.width, h = (int)root.info.height;
    if (root.list.empty()) { // the kernel writes the interleaved result directly
      const int pitch = hm_plane_stride(w, obpp);
      if ((rc = I.rgb.alloc((size_t)pitch * hm_padded_rows(h)))) return rc;
      if ((rc = compose_overlay(R, root, kind, I.rgb.p, pitch))) return rc;
    }
    else { // planes, the transformations (as a 4:4:4 image), then the same kernel with that one opaque layer interleaves
      LayerImage L;
      if ((rc = produce_node(R, root, L))) return rc;
      w = L.w; h = L.h;
      const int pitch = hm_plane_stride(w, obpp);
      if ((rc = I.rgb.alloc((size_t)pitch * hm_padded_rows(h)))) return rc;
      std::vector<hm_overlay_layer> one(1);
      layer_of(L, hm::overlay_clip(w, h, w, h, 0, 0, true), one[0]);
      hm_overlay_job job;
      std::memset(&job, 0, sizeof(job));
      job.width = w; job.height = h; job.out_kind = kind; job.out[0] = I.rgb.p; job.out_pitch = pitch;
      if ((rc = launch_overlay(R, job, one))) return rc;
    }
    // everything behind is hm_decode_item's: the result as an 8-bit 4:4:4 image whose conversion is done (I.rgb_attached) and
    // which carries no profile of its own, like a grid canvas - the converted image then reports the sRGB defaults
    I.w = w; I.h = h; I.chroma = 3; I.bd = 8; I.is_grid = true; I.rgb_attached = true;
    I.native = hm::NclxProfile();
    rc = emit_image(params, R.s, I, nullptr, 0, R.dout, R.alpha_sdr, out, t); // (planes: refused by derived_prepare)
  }
  return rc;
  }();
  if (!rc) {
    const hipError_t e = hipStreamSynchronize(R.s);
    if (e != hipSuccess) rc = hm_check_hip(e, "kernel execution");
  }
  if (!rc)
    for (DecodeJob* j : R.jobs)
      for (PlanarImage* im : {&j->I, &j->A})
        if (im->batch && !rc) rc = hm_batch_check(im->batch.get());
  lap("stream drained");
  if (rc) {
    hipStreamSynchronize(R.s);
    hm_decoded_free(out);
  }
  return rc;
}

} // namespace

// A request resolved against the file: the one statement of that order (hm_image_job.h)
int hm_img::resolve_request(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& asked, bool refuse_derived,
                            ResolvedRequest& r)
{
  int rc;
  r.t = asked;
  r.id = id;
  if (asked.tone && !asked.ootf) { r.tone = tone_for_item(f, id, asked.tone); r.t.tone = &r.tone; }
  if (asked.gain) { // (item `id`'s properties: a 'tmap' item's clli describes the alternate rendition; the job decodes its base image)
    if ((rc = hm_gain_for_item(f, id, params, asked.view, asked.gain, &r.id, &r.gain))) return rc;
    r.t.gain = &r.gain;
  }
  if (refuse_derived && is_derived_item(f, r.id) && (rc = derived_refusal(f, r.id, params, asked.planes != nullptr))) return rc;
  if (hm_light_from_icc(asked.light)) { // the profile of the item that is decoded (with a gain step: the base image), read before anything is queued
    uint32_t type = 0;
    hm_icc_info info;
    if ((rc = hm_file_item_icc(f, r.id, 1, &type, &r.t.icc, &r.t.icc_size))) return rc;
    if (!type) return hm_fail(HM_ERR_INVALID_ARG, "light: HM_LIGHT_FROM_ICC, and item %u has no ICC profile", r.id);
    if ((rc = hm_icc_parse(r.t.icc, r.t.icc_size, &info))) return rc;
  }
  return check_target_request(f, r.id, params, r.t);
}

extern "C" {

static int decode_grid_cut(const hm_file* f, uint32_t id, const hm_decode_params* params, const int32_t* devices, int n_devices, bool pipelined, hm_decoded* out, bool* applicable,
                           const hm_device_dest* dest = nullptr); // (below, behind the slabs)
static int decode_item(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& target, hm_decoded* out);

int hm_decode_item(const hm_file* f, uint32_t id, const hm_decode_params* params, hm_decoded* out)
{
  if (!f || !params || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  return decode_item(f, id, params, OutputTarget(), out);
}

// the device forms of hm_decode_item: what can be refused is refused before any work is queued - the destination is not written
static int decode_item_to(int kind, const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_out_steps& st,
                          const hm_device_dest* dest, const hm_device_planes* planes, hm_decoded* out)
{
  if (!f || !params || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  OutputTarget asked;
  int rc = OutputTarget::of_entry(kind, st, dest, planes, asked);
  if (rc) return rc;
  std::memset(out, 0, sizeof(*out));
  ResolvedRequest r;
  if ((rc = resolve_request(f, id, params, asked, true, r))) return rc;
  return decode_item(f, r.id, params, r.t, out);
}

int hm_decode_item_to_device(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_DEST, f, id, params, {}, dest, nullptr, out);
}

int hm_decode_item_to_device_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_VIEW, f, id, params, {view}, dest, nullptr, out);
}

int hm_decode_item_to_device_light(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                   const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_LIGHT, f, id, params, {view, light}, dest, nullptr, out);
}

int hm_decode_item_to_device_tone(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                  const hm_device_tone* tone, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_TONE, f, id, params, {view, light, tone}, dest, nullptr, out);
}

int hm_decode_item_to_device_alpha(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                   const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_ALPHA, f, id, params, {view, light, tone, alpha}, dest, nullptr, out);
}

int hm_decode_item_to_device_ootf(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                  const hm_device_ootf* ootf, const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_OOTF, f, id, params, {view, light, tone, alpha, nullptr, ootf}, dest, nullptr, out);
}

// Many views of one item: one request front, one decode, one writer (hm_views_write).  The arrays are the entry's to judge; the views
// themselves go through the phases of check_target_request, which loops over them as a sequence loops over its frames.
int hm_decode_item_to_device_views(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* views, const hm_device_dest* dests,
                                   int32_t count, const hm_device_light* light, const hm_device_tone* tone, const hm_device_alpha* alpha, const hm_device_ootf* ootf,
                                   hm_decoded* out, int32_t* failed_view)
{
  if (failed_view) *failed_view = -1;
  if (!f || !params || !out || !views || !dests) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (count < 1 || count > HM_VIEWS_MOST) return hm_fail(HM_ERR_INVALID_ARG, "views: count %d outside 1 .. %d", count, (int)HM_VIEWS_MOST);
  const hm_out_steps st = {nullptr, light, tone, alpha, nullptr, ootf};
  int rc = hm_entry_steps(HM_ENTRY_VIEWS, st);
  if (rc) return rc;
  const hm::Item* it = f->file.item(id);
  if (it && it->is_raw_leaf())
    return hm_fail(HM_ERR_UNSUPPORTED, "views: an uncompressed ('unci') or mask ('mski') item is not supported by hm_decode_item_to_device_views yet (its views upload by internal tile): "
                                       "call hm_decode_item_to_device_view per view");
  std::vector<hm_view_scratch> scratch((size_t)count, hm_view_scratch{{nullptr, nullptr}, nullptr});
  ViewsRequest V;
  V.views = views; V.dests = dests; V.count = count; V.out = out; V.scratch = scratch.data(); V.failed = failed_view;
  OutputTarget asked;
  asked.views = &V; asked.light = light; asked.tone = tone; asked.alpha = alpha; asked.ootf = ootf;
  ResolvedRequest r;
  if ((rc = resolve_request(f, id, params, asked, true, r))) return rc;
  std::memset(out, 0, sizeof(*out) * (size_t)count);
  hm_decoded one;
  rc = decode_item(f, r.id, params, r.t, &one); // (it returns with the stream drained, whatever happened: the scratch entries are free to go)
  for (hm_view_scratch& sc : scratch) hm_view_scratch_free(&sc);
  if (rc) { std::memset(out, 0, sizeof(*out) * (size_t)count); return rc; }
  for (int32_t k = 0; k < count; k++) { // the one decode's fields, with the sizes view k wrote
    hm_decoded o = one;
    o.width = out[k].width; o.height = out[k].height; o.stride[0] = out[k].stride[0];
    o.plane_width[0] = o.width; o.plane_height[0] = o.height;
    out[k] = o;
  }
  return HM_OK;
}

int hm_plan_views(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* views, int32_t count, int32_t tiles[4])
{
  if (!f || !params || !views || !tiles) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (count < 1 || count > HM_VIEWS_MOST) return hm_fail(HM_ERR_INVALID_ARG, "views: count %d outside 1 .. %d", count, (int)HM_VIEWS_MOST);
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  hm_device_view bound;
  const bool reduced = !it->is_raw_leaf() && views_bound(views, count, &bound); // (an 'unci' item is refused by the entry: its whole grid)
  int x0, y0, w, h;
  view_subgrid(f, id, params, reduced ? &bound : nullptr, tiles, &x0, &y0, &w, &h);
  return HM_OK;
}

// The entries that measure (include/heif_mi355x.h "Light statistics").  Everything that can be refused without a picture is refused
// with *out and *stats as they were: resolve_request runs before anything is cleared.  tone: the caller's (the measured entry), else NULL.
static int decode_item_measuring(int kind, const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                 const hm_device_ootf* ootf, const hm_device_tone* tone, const hm_device_dest* dest, LightMeasure& m, hm_light_stats* stats,
                                 hm_decoded* out)
{
  if (!f || !params || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_device_tone stand_in;
  if (tone) {
    if (tone->src_peak != 0.0f)
      return hm_fail(HM_ERR_INVALID_ARG, "tone: src_peak %g in the measured entry, which measures the peak (must be 0): hm_decode_item_to_device_tone takes an explicit peak", (double)tone->src_peak);
    // until the pixels are measured the step carries a peak whose knee cannot fail: dst_peak itself (KS = 1)
    stand_in = *tone;
    stand_in.src_peak = std::isfinite(tone->dst_peak) && tone->dst_peak > 0.0f && tone->dst_peak <= 10000.0f ? tone->dst_peak : 1000.0f;
  }
  OutputTarget asked;
  int rc = OutputTarget::of_entry(kind, {view, light, tone ? &stand_in : nullptr, nullptr, nullptr, ootf}, dest, nullptr, asked);
  if (rc || (rc = hm_stats_check_fraction(m.fraction)) || (rc = hm_stats_check_unit(m.unit_nits))) return rc;
  asked.measure = &m;
  if (!f->file.item(id)) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  if (is_derived_item(f, id)) return hm_fail(HM_ERR_UNSUPPORTED, "light statistics: item %u is a derived image ('iden' / 'iovl'), which is not supported", id);
  ResolvedRequest r;
  if ((rc = resolve_request(f, id, params, asked, false, r))) return rc;
  if ((rc = decode_item(f, r.id, params, r.t, out))) return rc;
  if (!m.done) { hm_decoded_free(out); return hm_fail(HM_ERR_UNSUPPORTED, "light statistics: output format %d has no interleaved pixels to measure", params->out_format); }
  if (stats) *stats = m.stats;
  return HM_OK;
}

int hm_decode_item_light_stats(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                               const hm_device_ootf* ootf, float unit_nits, hm_light_stats* stats, hm_decoded* out)
{
  if (!stats) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  LightMeasure m;
  m.mode = HM_MEASURE_STATS; m.unit_nits = unit_nits;
  const hm_device_dest dest = hm_stats_stand_in_dest();
  return decode_item_measuring(HM_ENTRY_STATS, f, id, params, view, light, ootf, nullptr, &dest, m, stats, out);
}

int hm_decode_item_to_device_measured(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                      const hm_device_ootf* ootf, const hm_device_tone* tone, double fraction, const hm_device_dest* dest, hm_decoded* out,
                                      hm_light_stats* stats)
{
  if (!tone) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  LightMeasure m;
  m.mode = HM_MEASURE_TONE; m.fraction = fraction;
  return decode_item_measuring(HM_ENTRY_MEASURED, f, id, params, view, light, ootf, tone, dest, m, stats, out);
}

int hm_file_item_icc_info(const hm_file* f, uint32_t id, hm_icc_info* out)
{
  if (!f || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(out, 0, sizeof(*out));
  uint32_t type = 0;
  const uint8_t* data = nullptr;
  size_t size = 0;
  const int rc = hm_file_item_icc(f, id, 1, &type, &data, &size);
  if (rc) return rc;
  return type ? hm_icc_parse(data, size, out) : (int)HM_ICC_NO_PROFILE;
}

int hm_file_item_light_levels(const hm_file* f, uint32_t id, hm_light_levels* out)
{
  if (!f || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(out, 0, sizeof(*out));
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  const hm::ItemProps& ip = it->props;
  out->has_clli = ip.has_clli ? 1 : 0; out->has_mdcv = ip.has_mdcv ? 1 : 0;
  out->max_content_light_level = ip.clli[0]; out->max_pic_average_light_level = ip.clli[1];
  for (int c = 0; c < 3; c++) { out->display_primaries_x[c] = ip.mdcv_xy[2 * c]; out->display_primaries_y[c] = ip.mdcv_xy[2 * c + 1]; }
  out->white_point_x = ip.mdcv_xy[6]; out->white_point_y = ip.mdcv_xy[7];
  out->max_display_mastering_luminance = ip.mdcv_lum[0]; out->min_display_mastering_luminance = ip.mdcv_lum[1];
  return HM_OK;
}

int hm_decode_item_to_device_planes(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_planes* planes, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_PLANES, f, id, params, {}, nullptr, planes, out);
}

int hm_decode_item_to_device_planes_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_planes* planes,
                                         hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_PLANES_VIEW, f, id, params, {view}, nullptr, planes, out);
}

int hm_plan_planes_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t tiles[4])
{
  if (!f || !params || !view || !tiles) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!f->file.item(id)) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  int x0, y0, w, h;
  view_subgrid(f, id, params, view, tiles, &x0, &y0, &w, &h, true);
  return HM_OK;
}

int hm_file_item_kind(const hm_file* f, uint32_t id)
{
  if (!f) return hm_fail(HM_ERR_INVALID_ARG, "null file");
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  if (it->type == "hvc1") return HM_ITEM_HVC1;
  if (it->type == "grid") return HM_ITEM_GRID;
  if (it->type == "iden") return HM_ITEM_IDEN;
  if (it->type == "iovl") return HM_ITEM_IOVL;
  if (it->type == "tmap") return HM_ITEM_TMAP;
  if (it->type == "unci") return HM_ITEM_UNCI;
  if (it->is_mask()) return HM_ITEM_MSKI;
  return HM_ITEM_OTHER;
}

int hm_file_unci_info(const hm_file* f, uint32_t id, hm_unci_info* info)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!f->file.item(id)) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  hm::HeifError err;
  return f->file.unci_info(id, *info, err) ? (int)HM_OK : fail_from(err);
}

// ---- region items ('rgan'): what the file layer read at open, handed out; hm_regions_to_device gathers it for the rasteriser ----

int hm_file_region_items(const hm_file* f, uint32_t image_id, uint32_t* ids, int max_ids)
{
  if (!f) return hm_fail(HM_ERR_INVALID_ARG, "null file");
  const std::vector<uint32_t> v = f->file.region_items_of(image_id);
  for (int i = 0; i < (int)v.size() && i < max_ids && ids; i++) ids[i] = v[i];
  return (int)v.size();
}

int hm_file_region_item_info(const hm_file* f, uint32_t region_item, hm_region_item_info* info)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm::HeifError err;
  const hm::RegionItem* r = f->file.region_item(region_item, err);
  if (!r) return fail_from(err);
  info->reference_width = r->reference_width; info->reference_height = r->reference_height;
  info->n_regions = (int32_t)r->regions.size(); info->field_bits = r->field_bits;
  return HM_OK;
}

static const hm::Region* region_of(const hm_file* f, uint32_t region_item, int index, int* rc)
{
  hm::HeifError err;
  const hm::RegionItem* r = f ? f->file.region_item(region_item, err) : nullptr;
  if (!f) { *rc = hm_fail(HM_ERR_INVALID_ARG, "null file"); return nullptr; }
  if (!r) { *rc = fail_from(err); return nullptr; }
  if (index < 0 || (size_t)index >= r->regions.size()) { *rc = hm_fail(HM_ERR_INVALID_ARG, "region item %u has %zu regions, no region %d", region_item, r->regions.size(), index); return nullptr; }
  return &r->regions[(size_t)index];
}

static void region_describe(const hm::Region& g, hm_region* out)
{
  std::memset(out, 0, sizeof(*out));
  out->type = g.type; out->x = g.x; out->y = g.y; out->w = g.w; out->h = g.h;
  out->n_points = (uint32_t)(g.points.size() / 2);
  out->mask_item = g.mask_item;
  out->mask_bytes = g.type == HM_REGION_INLINE_MASK ? (uint64_t)g.bits.size() : g.type == HM_REGION_REFERENCED_MASK ? (uint64_t)g.w * g.h : 0;
}

int hm_file_region(const hm_file* f, uint32_t region_item, int index, hm_region* out)
{
  if (!out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  int rc = HM_OK;
  const hm::Region* g = region_of(f, region_item, index, &rc);
  if (!g) return rc;
  region_describe(*g, out);
  return HM_OK;
}

int hm_file_region_points(const hm_file* f, uint32_t region_item, int index, int32_t* xy, int max_points)
{
  int rc = HM_OK;
  const hm::Region* g = region_of(f, region_item, index, &rc);
  if (!g) return rc;
  const int n = (int)(g->points.size() / 2);
  for (int i = 0; i < n && i < max_points && xy; i++) { xy[2 * i] = g->points[2 * (size_t)i]; xy[2 * i + 1] = g->points[2 * (size_t)i + 1]; }
  return n;
}

int hm_file_region_inline_mask(const hm_file* f, uint32_t region_item, int index, const uint8_t** bits, size_t* len)
{
  if (!bits || !len) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  int rc = HM_OK;
  const hm::Region* g = region_of(f, region_item, index, &rc);
  if (!g) return rc;
  if (g->type != HM_REGION_INLINE_MASK) return hm_fail(HM_ERR_INVALID_ARG, "region %d of item %u is not an inline mask (type %d)", index, region_item, g->type);
  *bits = g->bits.data(); *len = g->bits.size();
  return HM_OK;
}

int hm_regions_to_device(const hm_file* f, const uint32_t* region_items, int n, const hm_device_view* view, int mode, const hm_regions_dest* dest,
                         hm_regions_out* out)
{
  if (!f || !region_items || n <= 0 || !dest) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::vector<hm_region> desc;
  std::vector<const void*> data;
  std::vector<std::vector<uint8_t>> joined; // payloads of mask items that lie in several extents
  uint32_t rw = 0, rh = 0;
  hm::HeifError err;
  for (int k = 0; k < n; k++) {
    const hm::RegionItem* r = f->file.region_item(region_items[k], err);
    if (!r) return fail_from(err);
    if (k && (r->reference_width != rw || r->reference_height != rh))
      return hm_fail(HM_ERR_UNSUPPORTED, "region item %u has the reference size %u x %u, item %u before it %u x %u: one call rasterises one reference space",
                     region_items[k], r->reference_width, r->reference_height, region_items[0], rw, rh);
    rw = r->reference_width; rh = r->reference_height;
    for (const hm::Region& g : r->regions) {
      hm_region d;
      region_describe(g, &d);
      const void* p = nullptr;
      if (g.type == HM_REGION_POLYGON || g.type == HM_REGION_POLYLINE) p = g.points.data();
      else if (g.type == HM_REGION_INLINE_MASK) p = g.bits.data();
      else if (g.type == HM_REGION_REFERENCED_MASK) { // the mask item's payload is its samples: no decode
        hm_unci_info u;
        if (!f->file.unci_info(g.mask_item, u, err)) return fail_from(err); // (a depth other than 8)
        const uint8_t* bytes = nullptr;
        size_t len = 0;
        hm::HeifError e2;
        if (!f->file.item_span(g.mask_item, &bytes, &len, e2)) {
          joined.emplace_back();
          if (!f->file.item_data(g.mask_item, joined.back(), err)) return fail_from(err);
          bytes = joined.back().data(); len = joined.back().size();
        }
        if ((uint64_t)len < d.mask_bytes) return hm_fail(HM_ERR_BITSTREAM, "mask item %u has %zu bytes of data, %u x %u samples need %llu", g.mask_item, len, g.w, g.h, (unsigned long long)d.mask_bytes);
        p = bytes;
      }
      desc.push_back(d);
      data.push_back(p);
    }
  }
  if (out) std::memset(out, 0, sizeof(*out));
  hm_device_view whole;
  std::memset(&whole, 0, sizeof(whole));
  const hm_device_view* v = view ? view : &whole;
  const bool crop_all = v->crop_w == 0 && v->crop_h == 0;
  const int ow = v->out_w || v->out_h ? v->out_w : crop_all ? (int)rw : v->crop_w, oh = v->out_w || v->out_h ? v->out_h : crop_all ? (int)rh : v->crop_h;
  int rc = hm_rasterise_regions(desc.data(), data.data(), (int)desc.size(), (int)rw, (int)rh, view, mode, dest, nullptr);
  if (rc) return rc;
  if ((rc = hm_check_hip(hipStreamSynchronize(nullptr), "regions: wait for the rasteriser"))) return rc;
  if (out) {
    out->width = ow; out->height = oh; out->n_regions = (int32_t)desc.size(); out->planes = mode == HM_REGIONS_LABELS ? 1 : (int32_t)desc.size();
    out->bytes = hm_regions_dest_bytes(mode, (int)desc.size(), ow, oh, dest);
    out->reference_width = rw; out->reference_height = rh;
  }
  return HM_OK;
}

static void gain_params_of(const hm::GainMapInfo& g, hm_gain_params* p)
{
  std::memset(p, 0, sizeof(*p));
  p->base_headroom = g.base_headroom; p->alternate_headroom = g.alternate_headroom;
  for (int c = 0; c < 3; c++) {
    p->map_min[c] = g.map_min[c]; p->map_max[c] = g.map_max[c]; p->gamma[c] = g.gamma[c];
    p->base_offset[c] = g.base_offset[c]; p->alternate_offset[c] = g.alternate_offset[c];
  }
  p->use_base_primaries = g.use_base_colour_space ? 1 : 0;
}

int hm_file_gain_map_info(const hm_file* f, uint32_t tmap_id, hm_gain_map_info* info)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(info, 0, sizeof(*info));
  const hm::Item* it = f->file.item(tmap_id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", tmap_id);
  hm::GainMapInfo g;
  hm::HeifError err;
  if (!f->file.gain_map_info(tmap_id, g, err)) return fail_from(err);
  info->base_item = g.base; info->map_item = g.map;
  gain_params_of(g, &info->params);
  info->alt_has_nclx = it->props.colr.present ? 1 : 0;
  info->alt_primaries = it->props.colr.present ? it->props.colr.primaries : 0;
  info->alt_transfer = it->props.colr.present ? it->props.colr.transfer : 0;
  return HM_OK;
}

uint32_t hm_file_gain_map_of(const hm_file* f, uint32_t base_id) { return f ? f->file.gain_map_of(base_id) : 0; }

int hm_file_item_aux_type(const hm_file* f, uint32_t id, char* out, int cap)
{
  if (!f || (cap > 0 && !out) || cap < 0) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  const std::string& t = it->props.aux_type;
  if (cap > 0) {
    const size_t n = std::min(t.size(), (size_t)cap - 1);
    std::memcpy(out, t.data(), n);
    out[n] = 0;
  }
  return (int)std::min<size_t>(t.size(), 0x7FFFFFFF);
}

// The gain step of a decode, resolved before anything is queued: *base = the base image's item, *own = the step with map_item the
// map's item and explicit parameters.  Everything the file says about the map is judged here: its kind, chroma format and depth, and
// the geometry against the sizes the file declares (judged again against the decoded sizes by the write).
int hm_gain_for_item(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_gain* gain, uint32_t* base,
                         hm_device_gain* own)
{
  *own = *gain;
  *base = id;
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  if (gain->reserved[0] || gain->reserved[1] || gain->reserved[2] || gain->reserved[3]) return hm_fail(HM_ERR_INVALID_ARG, "gain: reserved is not 0");
  int rc;
  if (gain->map_item == 0) {
    if (it->type != "tmap") return hm_fail(HM_ERR_INVALID_ARG, "gain: item %u is not a 'tmap' item (give map_item and the parameters for a base image)", id);
    hm_gain_map_info info;
    if ((rc = hm_file_gain_map_info(f, id, &info))) return rc;
    if ((rc = hm_gain_check(&info.params, gain->headroom, HM_ERR_BITSTREAM))) return rc;
    own->map_item = info.map_item; own->params = info.params;
    *base = info.base_item;
    const hm::Item* bi = f->file.item(info.base_item);
    if (!bi) return hm_fail(HM_ERR_BITSTREAM, "'tmap' item %u references the missing item %u", id, info.base_item);
    const int base_primaries = bi->props.colr.present && bi->props.colr.primaries != 2 ? bi->props.colr.primaries : 1;
    if (!info.params.use_base_primaries && info.alt_has_nclx && info.alt_primaries != 2 && info.alt_primaries != base_primaries)
      return hm_fail(HM_ERR_UNSUPPORTED, "gain: applying the gain in the alternate primaries (%d, the base has %d) is not supported (the open step)", info.alt_primaries, base_primaries);
  }
  else {
    if (it->type == "tmap") return hm_fail(HM_ERR_INVALID_ARG, "gain: map_item %u with the 'tmap' item %u (a 'tmap' item brings its own map)", gain->map_item, id);
    if ((rc = hm_gain_check(&gain->params, gain->headroom, HM_ERR_INVALID_ARG))) return rc;
  }
  const hm::Item* bi = f->file.item(*base);
  const hm::Item* mi = f->file.item(own->map_item);
  if (!mi) return hm_fail(gain->map_item ? HM_ERR_INVALID_ARG : HM_ERR_BITSTREAM, "gain: no item %u for the map", own->map_item);
  if (!bi || (bi->type != "hvc1" && bi->type != "grid")) return hm_fail(HM_ERR_UNSUPPORTED, "gain: the base image (item %u) is not a coded image or a grid", *base);
  if (mi->type != "hvc1" && mi->type != "grid") return hm_fail(HM_ERR_UNSUPPORTED, "gain: the map (item %u, '%s') is not a coded image or a grid", own->map_item, mi->type.c_str());
  if (own->map_item == *base) return hm_fail(HM_ERR_INVALID_ARG, "gain: the map is the base image itself");
  hm_image_info binfo, minfo;
  if ((rc = hm_file_image_info(f, own->map_item, &minfo))) return rc;
  if (minfo.chroma != 0) return hm_fail(HM_ERR_UNSUPPORTED, "gain: a map that is not 4:0:0 (chroma format %d: a colour gain map) is not supported (the open step)", minfo.chroma);
  if (minfo.bit_depth > HM_GAIN_MAX_BITS) return hm_fail(HM_ERR_UNSUPPORTED, "gain: a map of %d bits is not supported (8 .. %d are; deeper maps are the open step)", minfo.bit_depth, (int)HM_GAIN_MAX_BITS);
  if (hm_file_image_info(f, *base, &binfo) != HM_OK) return HM_OK; // (the decode fails with its own message)
  const bool raw = params->ignore_transformations != 0;
  const int W = raw ? binfo.coded_width : binfo.width, H = raw ? binfo.coded_height : binfo.height;
  const int MW = raw ? minfo.coded_width : minfo.width, MH = raw ? minfo.coded_height : minfo.height;
  if (W <= 0 || H <= 0 || MW <= 0 || MH <= 0) return HM_OK;
  hm_view_plan vp;
  std::memset(&vp, 0, sizeof(vp));
  if (view) { if ((rc = hm_view_resolve(params->out_format, W, H, view, &vp))) return rc; }
  else { vp.w = vp.ow = W; vp.h = vp.oh = H; vp.crop_only = 1; }
  hm_gain_plan gp;
  std::memset(&gp, 0, sizeof(gp));
  return hm_gain_geometry(W, H, MW, MH, minfo.bit_depth, &vp, &gp);
}

// (*out is zeroed before the gain step is judged: decode_item_to)
int hm_decode_item_to_device_gain(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_light* light,
                                  const hm_device_tone* tone, const hm_device_gain* gain, const hm_device_dest* dest, hm_decoded* out)
{
  return decode_item_to(HM_ENTRY_GAIN, f, id, params, {view, light, tone, nullptr, gain}, dest, nullptr, out);
}

int hm_file_overlay_info(const hm_file* f, uint32_t id, hm_overlay_info* info, uint32_t* children, int32_t* offsets, int max_children)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(info, 0, sizeof(*info));
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  hm::OverlayInfo o;
  hm::HeifError err;
  if (!f->file.overlay_info(id, o, err)) return fail_from(err);
  info->canvas_width = (int32_t)std::min<uint32_t>(o.width, 0x7FFFFFFFu);
  info->canvas_height = (int32_t)std::min<uint32_t>(o.height, 0x7FFFFFFFu);
  for (int c = 0; c < 4; c++) info->background[c] = o.background[c];
  info->n_children = (int32_t)o.children.size();
  for (int i = 0; i < (int)o.children.size() && i < max_children; i++) {
    if (children) children[i] = o.children[i];
    if (offsets) { offsets[2 * i] = o.dx[i]; offsets[2 * i + 1] = o.dy[i]; }
  }
  return HM_OK;
}

int hm_file_derived_child(const hm_file* f, uint32_t id, uint32_t* child)
{
  if (!f || !child) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  *child = 0;
  if (!f->file.item(id)) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  hm::HeifError err;
  const uint32_t c = f->file.derived_child(id, err);
  if (!c) return fail_from(err);
  *child = c;
  return HM_OK;
}

int hm_plan_overlay(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t* decoded, int max_children)
{
  if (!f || !params) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  const hm::Item* it = f->file.item(id);
  if (!it) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  if (it->type != "iovl") return hm_fail(HM_ERR_INVALID_ARG, "item %u is not an overlay", id);
  DerivedRun R;
  R.f = f; R.params = *params; R.child_params = *params; R.child_params.out_format = 0;
  std::vector<uint32_t> path;
  const int rc = build_node(R, id, 0, {}, view, path, R.root);
  if (rc) return rc;
  const int n = (int)R.root->children.size();
  for (int i = 0; i < n && i < max_children && decoded; i++) decoded[i] = R.root->children[i] ? 1 : 0;
  return n;
}

int hm_plan_view(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, int32_t tiles[4])
{
  if (!f || !params || !view || !tiles) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!f->file.item(id)) return hm_fail(HM_ERR_INVALID_ARG, "no item %u", id);
  int x0, y0, w, h;
  view_subgrid(f, id, params, view, tiles, &x0, &y0, &w, &h);
  return HM_OK;
}

// target: with a view or a light step the item is always decoded as one job (its plan is reduced to the tiles the crop touches), never
// slab by slab; planar output is one job too (the cut below declines it)
static int decode_item(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& target, hm_decoded* out)
{
  std::memset(out, 0, sizeof(*out)); // (whatever fails below: nothing of an earlier call is left in it)
  if (is_derived_item(f, id)) return decode_derived(f, id, params, target, out);
  const hm::Item* item = f->file.item(id);
  const bool unci = item && item->is_raw_leaf(); // (a leaf without coded pictures: nothing to cut into slabs)
  if (!unci && !target.view && !target.views && !target.light && !target.alpha) { // (r06) a grid of more tiles than parsing threads, to interleaved pixels: slab by slab under the entropy decode (decode_grid_cut)
    bool applicable = false;
    const int prc = decode_grid_cut(f, id, params, nullptr, 1, /*pipelined=*/true, out, &applicable, target.dest);
    if (prc || applicable) return prc;
  }
  std::memset(out, 0, sizeof(*out));
  Lap lap;
  DecodeJob job;
  job.f = f; job.id = id; job.params = *params; job.s = (hipStream_t)params->stream;
  job.target.set(target);
  job.allow_unci = true;
  int rc = job_plan(job);
  if (rc) return rc;
  // ---- host: entropy-decode every coded picture (CABAC on the CPU, spread over threads like the reference's
  //      heif_context_set_threads tile fan-out, context.cc:2361-2401) ----
  const int nt = job_tile_count(job);
  job.few_pictures = nt <= 64; // one image at a time: its tiles are the whole batch - split chains for every class (hm_image_job.h)
  Crew::for_each(nt, params->host_threads, [&](int i, int row_threads) { job_parse_tile(job, i, row_threads); });
  lap("host entropy decode done");
  rc = job_enqueue(job, out);
  if (!rc) rc = job_complete(job, out);
  lap("stream drained");
  if (rc) { // (the job's destructor drains the stream; the pinned outputs go back after that)
    hipStreamSynchronize(job.s);
    hm_decoded_free(out);
  }
  return rc;
}

} // extern "C"

// ---- image sequences: many frames, one batch ------------------------------------------------------------------------
// The fork decodes the samples of a movie track one by one, each with a fresh decoder (context.cc:1603-1727).  Every sample is an
// independent intra picture, so hm_decode_sequence puts `count` of them into ONE device batch instead: their entropy decode is
// spread over the host crew like a grid's tiles, one upload, the reconstruction kernels and the fused tail run once over all
// frames, and each frame is then copied out on its own.  The colour conversion attached to a batch has one description for
// all its images (hm_batch_set_colour), so frames are grouped by what that description holds - picture size, depth, chroma
// format and the colour profile of the VUI - and each group is a batch of its own (a sequence written by one encoder is one
// group).  Frames whose conversion cannot be attached (native planar output, monochrome pictures) share one batch without
// conversion, and what converts them runs behind it, per frame, as in hm_decode_item.
namespace {

struct SeqFrame {
  ItemPlan P;        // one coded picture
  PlanarImage I;     // its planes on the device (I.batch stays empty: the group owns the batch)
  DevMem dout;       // converted pixels when the conversion is not attached
  DevPlane alpha_sdr; // (unused: frames carry no alpha)
  hm_colour_desc cd{};
  bool attach = false;
  int group = -1;
};

struct SeqGroup {
  std::unique_ptr<hm_batch, void (*)(hm_batch*)> batch{nullptr, hm_batch_destroy};
  std::vector<int> frames;
  bool attach = false;
};

} // namespace

extern "C" {

int hm_file_sequence_info(const hm_file* f, hm_sequence_info* info)
{
  if (!f || !info) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(info, 0, sizeof(*info));
  if (!f->file.is_movie()) return HM_OK;
  info->is_sequence = 1;
  info->frame_count = f->file.movie().frame_count;
  info->duration = f->file.movie().duration;
  return HM_OK;
}

static int decode_sequence(const hm_file* f, const uint32_t* frames, uint32_t first, int32_t count, const hm_decode_params* params, const hm_frame_dest* dests,
                           const OutputTarget& target, hm_decoded* out, int32_t* failed_frame);

int hm_decode_sequence(const hm_file* f, uint32_t first, int32_t count, const hm_decode_params* params, const hm_frame_dest* dests,
                       hm_decoded* out, int32_t* failed_frame)
{
  return decode_sequence(f, nullptr, first, count, params, dests, OutputTarget(), out, failed_frame);
}

// the device forms: failed_frame is set before any check; f, params and out are decode_sequence's to judge.  The family has no plain
// entry by frame IDs - its _view entry takes a NULL view -: HM_ENTRY_DEST is hm_decode_sequence_to_device, which counts from `first`.
// A frame carries no properties: the tone step's src_peak == 0 is 1000 (tone_for_item with id 0).
static int decode_frames_to(int kind, const hm_file* f, const uint32_t* frames, uint32_t first, int32_t count, const hm_decode_params* params,
                            const hm_out_steps& st, const hm_device_dest* dests, const hm_device_planes* planes, hm_decoded* out,
                            int32_t* failed_frame)
{
  if (failed_frame) *failed_frame = -1;
  if (!frames && kind != HM_ENTRY_DEST) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  OutputTarget t;
  int rc = OutputTarget::of_entry(kind, st, dests, planes, t, /*view_may_be_null=*/true);
  if (rc || (rc = hm_entry_icc(st, "in the frames family: the profile of a track's sample entry is not read"))) return rc;
  hm_device_tone own{};
  if (t.tone && !t.ootf) { own = tone_for_item(f, 0, t.tone); t.tone = &own; }
  return decode_sequence(f, frames, first, count, params, nullptr, t, out, failed_frame);
}

int hm_decode_sequence_to_device(const hm_file* f, uint32_t first, int32_t count, const hm_decode_params* params, const hm_device_dest* dests,
                                 hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_DEST, f, nullptr, first, count, params, {}, dests, nullptr, out, failed_frame);
}

int hm_decode_frames_to_device_view(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_view* view,
                                    const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_VIEW, f, frames, 0, count, params, {view}, dests, nullptr, out, failed_frame);
}

int hm_decode_frames_to_device_light(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_view* view,
                                     const hm_device_light* light, const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_LIGHT, f, frames, 0, count, params, {view, light}, dests, nullptr, out, failed_frame);
}

int hm_decode_frames_to_device_tone(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_view* view,
                                    const hm_device_light* light, const hm_device_tone* tone, const hm_device_dest* dests, hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_TONE, f, frames, 0, count, params, {view, light, tone}, dests, nullptr, out, failed_frame);
}

int hm_decode_frames_to_device_ootf(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_view* view,
                                    const hm_device_light* light, const hm_device_ootf* ootf, const hm_device_tone* tone, const hm_device_dest* dests, hm_decoded* out,
                                    int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_OOTF, f, frames, 0, count, params, {view, light, tone, nullptr, nullptr, ootf}, dests, nullptr, out, failed_frame);
}

int hm_decode_frames_to_device_planes(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_planes* planes,
                                      hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_PLANES, f, frames, 0, count, params, {}, nullptr, planes, out, failed_frame);
}

int hm_decode_frames_to_device_planes_view(const hm_file* f, const uint32_t* frames, int32_t count, const hm_decode_params* params, const hm_device_view* view,
                                           const hm_device_planes* planes, hm_decoded* out, int32_t* failed_frame)
{
  return decode_frames_to(HM_ENTRY_PLANES_VIEW, f, frames, 0, count, params, {view}, nullptr, planes, out, failed_frame);
}

// frames (NULL: first .. first + count - 1): the 1-based IDs of the frames, in any order, repeats allowed.
// target: dest or planes are arrays of `count` entries, frame k's at [k] - every frame goes to caller-owned device memory; view: the same
// rectangle of every frame, resampled, in one batched write behind the frames' conversions (hm_view_write_batch, hm_planes_view_write);
// light: every frame's write runs the light step, frame by frame (hm_out_write) - no batched form
static int decode_sequence(const hm_file* f, const uint32_t* frames, uint32_t first, int32_t count, const hm_decode_params* params, const hm_frame_dest* dests,
                           const OutputTarget& target, hm_decoded* out, int32_t* failed_frame)
{
  const hm_device_dest* ddests = target.dest;
  const hm_device_planes* pdests = target.planes;
  const hm_device_view* view = target.view;
  const hm_device_light* light = target.light;
  auto target_of = [&](int k) { // frame k's own
    OutputTarget t = target;
    if (t.dest) t.dest += k;
    if (t.planes) t.planes += k;
    return t;
  };
  if (failed_frame) *failed_frame = -1;
  if (!f || !params || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (count <= 0) return hm_fail(HM_ERR_INVALID_ARG, "frame count %d", count);
  if (const int src = target_check_shape(target)) return src;
  for (int k = 0; k < count; k++) std::memset(&out[k], 0, sizeof(out[k]));
  if (!f->file.is_movie()) return hm_fail(HM_ERR_INVALID_ARG, "the file is not an image sequence");
  const uint32_t n_frames = f->file.movie().frame_count;
  if (frames) {
    for (int k = 0; k < count; k++)
      if (frames[k] < 1 || frames[k] > n_frames) {
        if (failed_frame) *failed_frame = k;
        return hm_fail(HM_ERR_INVALID_ARG, "frames[%d] = %u outside 1..%u", k, frames[k], n_frames);
      }
  }
  else if (first < 1 || (uint64_t)first + (uint64_t)count - 1 > n_frames)
    return hm_fail(HM_ERR_INVALID_ARG, "frames %u..%llu outside 1..%u", first, (unsigned long long)first + count - 1, n_frames);
  auto frame_id = [&](int k) { return frames ? frames[k] : first + (uint32_t)k; };
  if (params->ext_dst) return hm_fail(HM_ERR_INVALID_ARG, "params->ext_dst: a sequence takes its caller buffers from dests");
  if (ddests || pdests) {
    // check_target_request's phases, each over every frame before the next begins: what can be refused without the frames' sizes, the
    // target against the size the track declares (the decoded size: below, behind the entropy decode, before anything is queued), a device
    // and the pointers.  A planar destination names the frame in every phase; an interleaved one only in the second, which it runs
    // only with a view (as hm_decode_item_to_device_view).  Frames carry no alpha.
    std::vector<hm_image_info> declared((size_t)count);
    auto each_frame = [&](bool names_frame, auto&& phase) {
      for (int k = 0; k < count; k++)
        if (const int rc = phase(k)) { if (names_frame && failed_frame) *failed_frame = k; return rc; }
      return (int)HM_OK;
    };
    int rc;
    if ((rc = each_frame(pdests != nullptr, [&](int k) { return check_request_alone(params, target_of(k), k); }))) return rc;
    auto declared_fits = [&](int k) { return check_request_declared(f, frame_id(k), params, target_of(k), 0, declared[k]); };
    if ((pdests || view) && (rc = each_frame(true, declared_fits))) return rc;
    if (pdests && (rc = require_device())) return rc; // (names no frame)
    if ((rc = each_frame(pdests != nullptr, [&](int k) { return check_request_pointers(params, target_of(k), 0, declared[k]); }))) return rc;
  }
  const bool planar_target = hm_out_is_planar(params->out_format);
  if (params->out_format && !planar_target) {
    const int obpp = hm_out_bytes_per_pixel(params->out_format);
    if (obpp < 0) return obpp;
  }
  hipStream_t s = (hipStream_t)params->stream;
  Lap lap;

  // ---- host: the entropy decode of every frame on the crew (the few-pictures record order below 65 frames, as a
  //      grid's tiles get it in hm_decode_item) ----
  std::vector<std::unique_ptr<SeqFrame>> F((size_t)count);
  for (int k = 0; k < count; k++) {
    F[k].reset(new SeqFrame());
    const int rc = plan_item(f, frame_id(k), F[k]->P);
    if (rc) { if (failed_frame) *failed_frame = k; return rc; }
  }
  const bool few = count <= 64;
  Crew::for_each(count, params->host_threads, [&](int k, int row_threads) {
    ItemPlan& P = F[k]->P;
    parse_picture(f, P.tiles[0].id, few, params->strict_decoding, row_threads, P.blobs[0], P.status[0], P.messages[0]);
  });
  lap("sequence: host entropy decode done");

  // ---- every check that can fail on a frame's data, frame by frame in order, before anything is queued: the first broken
  //      frame fails the call with its own status and message (those of hm_decode_item on it) and no caller buffer is touched ----
  for (int k = 0; k < count; k++) {
    SeqFrame& Fr = *F[k];
    auto fail = [&](int rc) { if (failed_frame) *failed_frame = k; return rc; };
    if (Fr.P.status[0]) return fail(tile_failure(Fr.P, 0));
    const hm_pic* h = hm_pic_of(Fr.P.blobs[0].p);
    PlanarImage& I = Fr.I;
    int warn = 0;
    const int prc = picture_profile(h, f->file.item(Fr.P.id), params->strict_decoding, I.native, warn);
    if (prc) return fail(prc);
    I.warnings = warn | concealed_warning(Fr.P, 0, 1);
    I.w = hm_window_w(*h); I.h = hm_window_h(*h);
    I.chroma = h->chroma_format; I.bd = h->bit_depth_y; I.is_grid = false;
    if (ddests || pdests) { // against the frame's own decoded size and format, the light step against the profile and depth it will report;
                            // planes with the pointers: the check hm_planes_write repeats before its launch
      const Reported reported = converted_report(I.native, false, I.bd, params->out_format, params->convert_hdr_to_8bit);
      const int drc = target_fits(params, target_of(k), I.w, I.h, I.chroma, I.bd, 0, &reported, pdests != nullptr);
      if (drc) return fail(drc);
    }
    if (planar_target) { // converted frame by frame behind the batch (emit_image); its refusals come here, before anything is queued
      if (I.chroma == 0 || I.chroma != hm_out_planar_chroma(params->out_format)) {
        Fr.cd = colour_desc(params, I.w, I.h, I.bd, I.chroma, I.native, /*has_nclx=*/1, I.P, 0, /*planar_8bit=*/true); // (no planes yet: no strides)
        const int pipe = hm_colour_pipeline(&Fr.cd);
        if (pipe < 0) return fail(pipe);
      }
    }
    else if (params->out_format) { // (the request job_enqueue hands to the conversion: a single image keeps its own nclx)
      Fr.cd = colour_desc(params, I.w, I.h, I.bd, I.chroma, I.native, /*has_nclx=*/1, nullptr, hm_out_bytes_per_pixel(params->out_format));
      const int pipe = hm_colour_pipeline(&Fr.cd); // (the conversion's own refusal, with its message)
      if (pipe < 0) return fail(pipe);
      Fr.attach = I.chroma != 0;
    }
  }

  // ---- groups: one batch per colour description (see above) ----
  std::vector<std::unique_ptr<SeqGroup>> groups;
  {
    std::map<std::vector<int32_t>, int> index;
    for (int k = 0; k < count; k++) {
      SeqFrame& Fr = *F[k];
      std::vector<int32_t> key{Fr.attach ? 1 : 0};
      if (Fr.attach) {
        const hm_colour_desc& cd = Fr.cd;
        key.insert(key.end(), {cd.width, cd.height, cd.bit_depth, cd.chroma, cd.matrix, cd.primaries, cd.full_range});
      }
      auto it = index.find(key);
      if (it == index.end()) {
        it = index.emplace(key, (int)groups.size()).first;
        groups.emplace_back(new SeqGroup());
        groups.back()->attach = Fr.attach;
      }
      Fr.group = it->second;
      groups[(size_t)it->second]->frames.push_back(k);
    }
  }
  struct ViewBlocks { // what the batched view write works on: released once the stream has drained (Drain goes first)
    std::vector<hm_view_scratch> sc;
    ~ViewBlocks() { for (hm_view_scratch& x : sc) hm_view_scratch_free(&x); }
  } view_blocks;
  std::vector<hm_view_item> view_items;
  std::vector<hm_planes_view_item> planes_items;
  if ((view || light) && ddests) { view_blocks.sc.assign((size_t)count, hm_view_scratch{}); view_items.assign((size_t)count, hm_view_item{}); }
  if (view && pdests) { view_blocks.sc.assign((size_t)count, hm_view_scratch{}); planes_items.assign((size_t)count, hm_planes_view_item{}); }
  struct Drain { // (declared behind everything the queued work uses: destroyed first, it drains the stream before they go)
    hipStream_t s; bool on = false;
    ~Drain() { if (on) hipStreamSynchronize(s); }
  } drain{s};
  auto release_all = [&](int rc) {
    if (drain.on) hipStreamSynchronize(s);
    for (int k = 0; k < count; k++) { hm_decoded_free(&out[k]); std::memset(&out[k], 0, sizeof(out[k])); }
    return rc;
  };

  // ---- device: planes, one batch per group, the conversion attached where it can be ----
  int rc = HM_OK;
  for (std::unique_ptr<SeqGroup>& G : groups) {
    hm_batch* b = nullptr;
    if ((rc = hm_batch_create(&b))) return release_all(rc);
    G->batch.reset(b);
    std::vector<const void*> ys, cbs, crs;
    std::vector<void*> outs;
    for (int k : G->frames) {
      SeqFrame& Fr = *F[k];
      PlanarImage& I = Fr.I;
      if ((rc = alloc_planes(I.P, I.w, I.h, I.chroma, I.bd))) return release_all(rc);
      const hm_tile_dest d = tile_dest_of(I.P, I.w, I.h);
      const int idx = hm_batch_add_trusted(b, Fr.P.blobs[0].p, Fr.P.blobs[0].n, &d);
      if (idx < 0) return release_all(idx);
      drain.on = true;
      for (int c = 0; c < 3; c++) // (as hm_decode_item does: the planes' padding leaves the device zeroed)
        if (I.P[c].mem.p) hipMemsetAsync(I.P[c].mem.p, 0, plane_bytes(I.P[c]), s);
      if (G->attach) {
        if ((rc = I.rgb.alloc((size_t)Fr.cd.out_stride * hm_padded_rows(I.h)))) return release_all(rc);
        ys.push_back(I.P[0].mem.p); cbs.push_back(I.P[1].mem.p); crs.push_back(I.P[2].mem.p); outs.push_back(I.rgb.p);
      }
    }
    if ((rc = hm_batch_upload(b, s))) return release_all(rc);
    if (G->attach) {
      const SeqFrame& F0 = *F[(size_t)G->frames[0]];
      const bool ok = hm_batch_set_colour(b, &F0.cd, (int)G->frames.size(), ys.data(), cbs.data(), crs.data(), outs.data(), 0) == HM_OK;
      for (int k : G->frames) F[k]->I.rgb_attached = ok;
    }
    if ((rc = hm_batch_execute(b, 3, s))) return release_all(rc);
  }
  lap("sequence: batches queued");
  // ---- per frame: the conversion where it was not attached, and the copy out (to the frame's caller buffer if it has one) ----
  for (int k = 0; k < count; k++) {
    SeqFrame& Fr = *F[k];
    hm_decode_params pk = *params;
    if (dests) { pk.ext_dst = dests[k].ext_dst; pk.ext_dst_len = dests[k].ext_dst_len; pk.ext_dst_stride = dests[k].ext_dst_stride; }
    OutputTarget t = target_of(k);
    if (t.light) t.scratch = &view_blocks.sc[(size_t)k]; // (written here, on the frame's own scratch entry: nothing is left for the batched write)
    else if (t.view && t.dest) t.view_later = &view_items[(size_t)k];
    if (t.view && t.planes) t.planes_later = &planes_items[(size_t)k];
    if ((rc = emit_image(&pk, s, Fr.I, nullptr, 0, Fr.dout, Fr.alpha_sdr, &out[k], t))) {
      if (failed_frame && (t.planes_later || t.light)) *failed_frame = k;
      return release_all(rc);
    }
  }
  // ---- the view of every frame: one pair of tap tables and one launch per pass for all frames that share them ----
  if (view && ddests && !light && (rc = hm_view_write_batch(params->out_format, view_items.data(), count, s, view_blocks.sc.data()))) return release_all(rc);
  if (view && pdests) { // ... and of every frame's planes: the tables of at most four axes per group (hm_planes_view_write)
    int bad = -1;
    if ((rc = hm_planes_view_write(planes_items.data(), count, s, view_blocks.sc.data(), &bad))) {
      if (failed_frame) *failed_frame = bad;
      return release_all(rc);
    }
  }
  lap("sequence: colour + D2H queued");
  const hipError_t e = hipStreamSynchronize(s);
  drain.on = false;
  if (e != hipSuccess) return release_all(hm_check_hip(e, "kernel execution"));
  for (std::unique_ptr<SeqGroup>& G : groups)
    if ((rc = hm_batch_check(G->batch.get()))) return release_all(rc);
  lap("sequence: stream drained");
  return HM_OK;
}

} // extern "C"

// ---- one grid over several devices -----------------------------------------------------------------------------------
// The reference fans the tiles of a grid out inside one process (context.cc:2281-2294, 2361-2401); the tiles are independent
// coded pictures, so the device-side form of that fan-out needs no exchange between devices: the grid's tile
// rows are cut into contiguous slabs, one per entry of `devices`; every slab is decoded, filtered, pasted and converted on
// its device (its own batch, its own stream, a host thread that makes the device current) and copied from there straight
// into its rows of the caller's destination (`ext_dst`) or of the one pinned output plane - no collective, no second copy.
// Colour conversion is per pixel with nearest-neighbour chroma, so slabs that start on even rows need no halo.
// What does not cut this way runs on devices[0] alone: single images, planar output, alpha planes, transformative
// properties of the grid item, forced bilinear up-sampling (a one-row chroma halo), tile heights that are odd.
namespace {

struct Slab {
  int device = 0;
  int row0 = 0, rows = 0; // tile rows
  int y0 = 0, h = 0;      // canvas rows
  ItemPlan P;
  int rc = HM_OK;
  std::string message;
  // what is in flight between slab_enqueue and slab_finish
  hipStream_t s = nullptr;
  std::unique_ptr<PlanarImage> I;
  std::unique_ptr<DevMem> dout;
};

// Queue one slab on its device: decode + convert + the copy to dst (row 0 of the slab), all on a stream of its own.  Returns
// without waiting; slab_finish waits and reports.  Runs on any thread (it makes the slab's device current).
// ddest (may be NULL): the slab's rows go to the caller's device memory instead (canvas_h: the height of the whole image); the kernel that
// writes them is row-local, so every layout cuts into slabs like the host copy does.  dest_ready: recorded on params->stream when the
// call came in - the slab's stream is non-blocking and knows nothing of that stream, so the write (not the decode in front of it) waits
// for whatever the caller had queued on the destination by then.
void slab_enqueue(const hm_file* f, const hm_decode_params* params, Slab& S, uint8_t* dst, size_t dst_stride, int canvas_w,
                  const hm_device_dest* ddest = nullptr, int canvas_h = 0, hipEvent_t dest_ready = nullptr)
{
  auto fail = [&](int rc) { S.rc = rc; S.message = hm_last_error(); };
  trace_mark("slab enqueue begins, row", S.row0);
  hipError_t e = hipSetDevice(S.device);
  if (e != hipSuccess) return fail(hm_check_hip(e, "hipSetDevice"));
  if (!(S.s = hm_pool_stream_get())) return fail(HM_ERR_NO_DEVICE);
  S.I.reset(new PlanarImage());
  S.dout.reset(new DevMem());
  PlanarImage& I = *S.I;
  DevMem& dout = *S.dout;
  trace_mark("  stream created", S.row0);
  int rc = planar_from_blobs(f, S.P, params, S.s, I, /*attach=*/true);
  trace_mark("  batch queued", S.row0);
  if (!rc) {
    const int obpp = hm_out_bytes_per_pixel(params->out_format);
    // (a grid canvas carries no nclx: context.cc:2250-2276)
    const hm_colour_desc cd = colour_desc(params, canvas_w, S.h, I.bd, I.chroma, I.native, /*has_nclx=*/0, I.P, obpp);
    if (I.rgb_attached) dout.swap(I.rgb); // (converted with the batch)
    else {
      rc = dout.alloc((size_t)cd.out_stride * hm_padded_rows(S.h));
      if (!rc) rc = hm_colour_convert(&cd, I.P[0].mem.p, I.P[1].mem.p, I.P[2].mem.p, dout.p, S.s);
    }
    if (!rc && ddest) {
      if (dest_ready) rc = hm_check_hip(hipStreamWaitEvent(S.s, dest_ready, 0), "wait for the caller's stream");
      if (!rc) rc = hm_dest_write(ddest, params->out_format, canvas_w, canvas_h, S.y0, S.h, dout.p, cd.out_stride, S.s);
    }
    else if (!rc) {
      e = hipMemcpy2DAsync(dst, dst_stride, dout.p, cd.out_stride, (size_t)canvas_w * obpp, (size_t)S.h, hipMemcpyDeviceToHost, S.s);
      rc = hm_check_hip(e, "D2H of a slab");
    }
  }
  if (rc) fail(rc);
  trace_mark("slab enqueue ends, row", S.row0);
}

// ... wait for it: the slab's pixels are in host memory (or S.rc says why not); its image, batch and output buffer go back
// before the stream they worked on.  Also after a failed slab_enqueue: nothing of the slab may be in flight when its buffers go.
void slab_finish(Slab& S)
{
  if (!S.s) return;
  hipSetDevice(S.device);
  const hipError_t e = hipStreamSynchronize(S.s);
  trace_mark("slab stream drained, row", S.row0);
  int rc = S.rc;
  if (!rc) rc = hm_check_hip(e, "kernel execution");
  if (!rc && S.I && S.I->batch) rc = hm_batch_check(S.I->batch.get());
  if (rc && !S.rc) { S.rc = rc; S.message = hm_last_error(); }
  S.I.reset();
  trace_mark("  image + batch released", S.row0);
  S.dout.reset();
  trace_mark("  output released", S.row0);
  hm_pool_stream_put(S.s, S.device); // (drained above)
  S.s = nullptr;
  trace_mark("slab released, row", S.row0);
}

// decode + convert one slab on its device and copy it to dst, returning when the pixels are in host memory
void run_slab(const hm_file* f, const hm_decode_params* params, Slab& S, uint8_t* dst, size_t dst_stride, int canvas_w)
{
  slab_enqueue(f, params, S, dst, dst_stride, canvas_w);
  slab_finish(S);
}

} // namespace

extern "C" {

// Contiguous slabs of tile rows for n devices (sizes differ by at most one row, devices beyond the row count get none):
// first[d] / count[d] = tile rows of device d.  Pure host arithmetic (the same cut as shard.row_slabs of the harness).
int hm_plan_device_slabs(int grid_rows, int n_devices, int32_t* first, int32_t* count)
{
  if (grid_rows < 0 || n_devices <= 0 || !first || !count) return hm_fail(HM_ERR_INVALID_ARG, "bad argument");
  const int base = grid_rows / n_devices, extra = grid_rows % n_devices;
  for (int d = 0; d < n_devices; d++) {
    first[d] = d * base + (d < extra ? d : extra);
    count[d] = base + (d < extra ? 1 : 0);
  }
  return HM_OK;
}

// One grid as slabs of tile rows (see above).  devices[0 .. n_devices): a slab per entry, all entropy decode first, every slab on a
// thread of its own - hm_decode_item_devices.  pipelined (r06; n_devices == 1): ONE device takes the grid in slabs of a few tile rows,
// and a slab is queued - on a stream of its own, nothing waited for - as soon as its tiles are parsed: the kernels and the copy of
// slab k run under the entropy decode of the slabs behind it (one 12 MP grid of 48 tiles on 16 threads: ~2.3 ms of entropy decode,
// behind which 0.43 ms of queueing, 0.7 ms of kernels and 0.66 ms of copy used to start).
// *applicable = false (and nothing touched) when the item does not cut this way.
static int decode_grid_cut(const hm_file* f, uint32_t id, const hm_decode_params* params, const int32_t* devices, int n_devices, bool pipelined, hm_decoded* out, bool* applicable,
                           const hm_device_dest* ddest)
{
  *applicable = false;
  if (is_derived_item(f, id)) return HM_OK; // (not applicable: composed on one device)
  ItemPlan plan;
  int rc = plan_item(f, id, plan);
  if (rc) return rc;
  const hm::Item* it = f->file.item(id);
  const hm::Item* t0 = plan.is_grid ? f->file.item(plan.tiles[0].id) : nullptr;
  const int ih = t0 ? t0->props.ispe_height : 0;
  const int nt = (int)plan.tiles.size();
  int nthreads = params->host_threads > 0 ? params->host_threads : 1;
  if (nthreads > nt) nthreads = nt;
  const bool cut = (pipelined || n_devices > 1) && plan.is_grid && plan.rows >= 2 && params->out_format != 0 && !hm_out_is_planar(params->out_format) && hm_out_bytes_per_pixel(params->out_format) > 0 &&
                   params->chroma_upsampling == 0 && !f->file.alpha_item_of(id) && plan.tile_alpha.empty() &&
                   (params->ignore_transformations || !it || it->props.transforms.empty()) && ih > 0 && (ih % 2) == 0 && params->stream == nullptr;
  // The checks of the declared grid (grid_tile_declared) look at the grid BEFORE it is cut - a slab only ever sees its own reduced
  // canvas - and so does every tile's luma origin inside the canvas.  A grid that fails one is not cut: hm_decode_item on the first
  // device reports it exactly as it always does, its message over the one left here (r04 advice: such a grid came back HM_OK with
  // rows of the destination never written).
  bool geometry_ok = cut;
  if (cut) {
    const int iw = t0->props.ispe_width;
    if (iw <= 0) geometry_ok = false;
    for (int i = 0; geometry_ok && i < nt; i++) {
      const long x0 = (long)(i % plan.cols) * iw, y0 = (long)(i / plan.cols) * ih;
      if (grid_tile_declared(f, plan, i, iw, ih) || x0 >= plan.canvas_w || y0 >= plan.canvas_h) geometry_ok = false;
    }
  }
  // pipelined: up to eight slabs of whole tile rows (each costs a batch and a launch of every kernel; what is left behind the
  // entropy decode is the LAST slab's kernels and copy, so small slabs win - one 12 MP grid of 8 x 6 tiles, 16 threads, median of 40
  // calls: one batch 4.58 ms, slabs of 3 / 2 / 1 rows 4.00 / 3.89 / 3.41 ms); a grid the threads parse in one round has nothing to overlap
  int slab_rows = 0;
  if (cut && geometry_ok && pipelined) {
    const int forced = hm_knob(HM_KNOB_GRID_SLAB_ROWS); // (A/B measurements: 0 = one batch behind the entropy decode, n = rows per slab)
    if (forced == 0) return HM_OK;
    slab_rows = std::max(1, (plan.rows + 7) / 8);
    if (forced > 0) slab_rows = forced;
    if (nt <= nthreads || slab_rows >= plan.rows) return HM_OK; // (not applicable)
  }
  if (!cut || !geometry_ok) return HM_OK;
  *applicable = true;
  std::memset(out, 0, sizeof(*out));
  trace_mark("grid cut begins, slabs of rows", slab_rows);

  // ---- the slabs ----
  std::vector<int32_t> first, count, dev_of;
  if (pipelined) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return hm_fail(HM_ERR_NO_DEVICE, "no current HIP device");
    for (int r = 0; r < plan.rows; r += slab_rows) { first.push_back(r); count.push_back(std::min(slab_rows, plan.rows - r)); dev_of.push_back(cur); }
  }
  else {
    first.resize(n_devices); count.resize(n_devices);
    hm_plan_device_slabs(plan.rows, n_devices, first.data(), count.data());
    dev_of.assign(devices, devices + n_devices);
  }
  std::vector<std::unique_ptr<Slab>> slabs;
  for (size_t d = 0; d < first.size(); d++) {
    if (count[d] == 0) continue;
    const int y0 = std::min(first[d] * ih, plan.canvas_h), y1 = std::min((first[d] + count[d]) * ih, plan.canvas_h);
    if (y1 <= y0) continue; // (tile rows below the canvas: nothing of them is visible)
    std::unique_ptr<Slab> S(new Slab());
    S->device = dev_of[d]; S->row0 = first[d]; S->rows = count[d]; S->y0 = y0; S->h = y1 - y0;
    S->P = plan.sub_grid(first[d], count[d], 0, plan.cols, plan.canvas_w, S->h);
    slabs.push_back(std::move(S));
  }
  if (slabs.empty()) return hm_fail(HM_ERR_BITSTREAM, "grid without visible tile rows");

  // ---- the destination: the caller's buffer or one pinned plane ----
  const int obpp = hm_out_bytes_per_pixel(params->out_format);
  const int img_w = plan.canvas_w, img_h = plan.canvas_h;
  uint8_t* dst = nullptr;
  size_t dst_stride = 0;
  struct DestReady { // the caller's work on the destination so far, as an event the slabs' streams wait for before they write
    hipEvent_t e = nullptr;
    ~DestReady() { if (e) hipEventDestroy(e); } // (behind slab_finish of every slab on each way out: nothing waits for it any more)
  } dest_ready;
  if (ddest) { // (pipelined, one device) caller-owned device memory: checked against the grid's size before the first slab is queued
    hm_dest_plan dp;
    if ((rc = hm_dest_resolve(params->out_format, img_w, img_h, ddest, &dp)) || (rc = hm_dest_check_len(ddest, &dp))) return rc;
    dst_stride = (size_t)dp.row_pitch;
    if ((rc = hm_check_hip(hipEventCreateWithFlags(&dest_ready.e, hipEventDisableTiming), "hipEventCreate"))) return rc;
    if ((rc = hm_check_hip(hipEventRecord(dest_ready.e, (hipStream_t)params->stream), "hipEventRecord on the caller's stream"))) return rc;
    out->used_ext_dst = 1;
  }
  else if (params->ext_dst && params->ext_dst_stride >= (uint32_t)(img_w * obpp) && (size_t)params->ext_dst_len >= (size_t)params->ext_dst_stride * (size_t)img_h) {
    dst = (uint8_t*)params->ext_dst; dst_stride = params->ext_dst_stride;
    out->used_ext_dst = 1;
  }
  else {
    dst_stride = (size_t)hm_plane_stride(img_w, obpp);
    out->plane[0] = (uint8_t*)hm_pool_pinned_alloc(dst_stride * hm_padded_rows(img_h)); // (portable pinned memory: every device copies into it)
    if (!out->plane[0]) return hm_fail(HM_ERR_NOMEM, "out of memory");
    dst = out->plane[0];
  }

  // ---- host: entropy-decode tiles [t0, t0 + n) (as hm_decode_item), all threads on them; the blobs go to their slab ----
  const int few = nt <= 64;
  int tile_warnings = 0, bd = 8, chroma = 1;
  // (a cut grid has more tiles than threads: one thread per tile, whatever share of the crew for_each offers)
  auto parse_tile = [&](int i) { parse_picture(f, plan.tiles[i].id, few != 0, params->strict_decoding, 1, plan.blobs[i], plan.status[i], plan.messages[i]); };
  auto parse_range = [&](int t_first, int t_n) -> int {
    Crew::for_each(t_n, nthreads, [&](int k, int) { parse_tile(t_first + k); });
    for (int i = t_first; i < t_first + t_n; i++)
      if (plan.status[i]) return tile_failure(plan, i);
    tile_warnings |= concealed_warning(plan, t_first, t_n);
    return HM_OK;
  };
  // (slabs are taken in order: slab 0 - tile 0 of the grid - first)
  auto take_blobs = [&](Slab& S) -> int {
    const int t_first = S.row0 * plan.cols, t_n = S.rows * plan.cols;
    for (int k = 0; k < t_n; k++) { S.P.blobs[k].p = plan.blobs[t_first + k].p; S.P.blobs[k].n = plan.blobs[t_first + k].n; plan.blobs[t_first + k].p = nullptr; plan.blobs[t_first + k].n = 0; }
    if (&S == slabs[0].get()) { bd = hm_pic_of(S.P.blobs[0].p)->bit_depth_y; chroma = hm_pic_of(S.P.blobs[0].p)->chroma_format; }
    // every tile against tile 0 of the WHOLE grid, in the order of the one-batch decode (planar_from_blobs compares a slab's tiles with
    // the slab's own first tile only: a later tile row of another depth or chroma format would otherwise come back HM_OK under slab 0's
    // metadata)
    for (int k = 0; k < t_n; k++)
      if (const int trc = grid_tile_picture(hm_pic_of(S.P.blobs[k].p), chroma, bd)) return trc;
    return HM_OK;
  };
  auto give_up = [&](int src) { // (whatever is in flight is waited for before the destination goes back)
    for (const std::unique_ptr<Slab>& S : slabs) slab_finish(*S);
    hm_decoded_free(out);
    return src;
  };

  if (pipelined) {
    // ONE run of the parsing threads over all tiles, in order; a thread of its own queues slab k as soon as its tiles are parsed
    // (queueing a slab - batch, planes, the copy of its command streams to pinned memory, the launches - is ~0.2 ms of host time
    //  that would otherwise stand between two rounds of the parsing threads; a barrier per slab would also wait for the slowest
    //  tile of every round: measured 3 x 0.8 ms instead of 2.3 ms for the 48 tiles of a 12 MP grid)
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> done(slabs.size(), 0); // tiles of slab k that have been through the parser (under mu)
    int parse_rc = HM_OK;
    std::string parse_msg;
    auto slab_of_tile = [&](int i) { return (size_t)((i / plan.cols) / slab_rows); }; // (slabs below the canvas do not exist: clamped)
    auto queue_slabs = [&]() {
      for (size_t k = 0; k < slabs.size(); k++) {
        Slab& S = *slabs[k];
        const int t_first = S.row0 * plan.cols, t_n = S.rows * plan.cols;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return done[k] >= t_n; });
        }
        for (int i = t_first; i < t_first + t_n && !parse_rc; i++)
          if (plan.status[i]) { parse_rc = plan.status[i]; parse_msg = tile_failure_text(plan, i); }
        if (parse_rc) return; // (this slab and the ones behind it are not queued)
        tile_warnings |= concealed_warning(plan, t_first, t_n);
        trace_mark("slab parsed, row", S.row0);
        if (const int trc = take_blobs(S)) { parse_rc = trc; parse_msg = hm_last_error(); return; } // (the slabs in front are drained below)
        slab_enqueue(f, params, S, ddest ? nullptr : dst + (size_t)S.y0 * dst_stride, dst_stride, img_w, ddest, img_h, dest_ready.e);
        if (S.rc) return; // (reported below)
      }
    };
    std::thread queuer;
    try { queuer = std::thread(queue_slabs); }
    catch (...) {} // (no thread to be had: the slabs are queued behind the entropy decode, on this thread)
    {
      Crew::for_each(nt, nthreads, [&](int i, int) {
        parse_tile(i);
        const size_t k = slab_of_tile(i);
        if (k < slabs.size()) {
          bool full;
          { std::lock_guard<std::mutex> lk(mu); full = ++done[k] >= slabs[k]->rows * plan.cols; }
          if (full) cv.notify_one();
        }
      });
    }
    if (queuer.joinable()) queuer.join();
    else queue_slabs(); // (every slab is complete by now: no wait)
    trace_mark("slabs queued");
    for (const std::unique_ptr<Slab>& S : slabs) slab_finish(*S);
    trace_mark("slabs drained");
    if (parse_rc) { hm_decoded_free(out); return hm_fail(parse_rc, "%s", parse_msg.c_str()); }
  }
  else {
    if ((rc = parse_range(0, nt))) return give_up(rc);
    for (const std::unique_ptr<Slab>& S : slabs)
      if ((rc = take_blobs(*S))) return give_up(rc);
    // every slab on its device: the first on this thread, the others on threads of their own
    std::vector<std::thread> threads;
    for (size_t k = 1; k < slabs.size(); k++) {
      Slab* S = slabs[k].get();
      try { threads.emplace_back([=]() { run_slab(f, params, *S, dst + (size_t)S->y0 * dst_stride, dst_stride, img_w); }); }
      catch (...) { S->rc = HM_ERR_NOMEM; S->message = "could not start a thread for a device slab"; }
    }
    run_slab(f, params, *slabs[0], dst + (size_t)slabs[0]->y0 * dst_stride, dst_stride, img_w);
    for (std::thread& t : threads) t.join();
  }
  for (const std::unique_ptr<Slab>& S : slabs)
    if (S->rc) {
      const int src = S->rc;
      if (pipelined) hm_fail(src, "%s", S->message.c_str()); // (one device: the message hm_decode_item would give)
      else hm_fail(src, "tile rows %d-%d on device %d: %s", S->row0, S->row0 + S->rows - 1, S->device, S->message.c_str());
      hm_decoded_free(out);
      return src;
    }

  // ---- what the decoded image says about itself (as job_enqueue for a converted grid canvas) ----
  out->width = img_w; out->height = img_h; out->bit_depth = bd; out->chroma = chroma;
  out->out_format = params->out_format;
  const Reported r = converted_report(hm::NclxProfile(), /*is_grid=*/true, bd, params->out_format, 0);
  r.profile_to(out);
  out->bit_depth = r.bit_depth;
  out->stride[0] = (int32_t)std::min<size_t>(dst_stride, 0x7FFFFFFF);
  out->plane_width[0] = img_w; out->plane_height[0] = img_h;
  out->warnings = tile_warnings;
  return HM_OK;
}

int hm_decode_item_devices(const hm_file* f, uint32_t id, const hm_decode_params* params, const int32_t* devices, int n_devices, hm_decoded* out)
{
  if (!f || !params || !out || !devices || n_devices <= 0 || n_devices > 64) return hm_fail(HM_ERR_INVALID_ARG, "bad argument");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return hm_fail(HM_ERR_NO_DEVICE, "no HIP device available");
  for (int d = 0; d < n_devices; d++)
    if (devices[d] < 0 || devices[d] >= n_dev) return hm_fail(HM_ERR_INVALID_ARG, "device %d of the list does not exist (%d devices)", devices[d], n_dev);
  int prev_dev = 0;
  hipGetDevice(&prev_dev);
  struct Restore { int d; ~Restore() { hipSetDevice(d); } } restore{prev_dev};
  bool applicable = false;
  const int rc = decode_grid_cut(f, id, params, devices, n_devices, /*pipelined=*/false, out, &applicable);
  if (rc || applicable) return rc;
  if (hipSetDevice(devices[0]) != hipSuccess) return hm_fail(HM_ERR_NO_DEVICE, "hipSetDevice(%d) failed", devices[0]);
  return hm_decode_item(f, id, params, out);
}

} // extern "C"
