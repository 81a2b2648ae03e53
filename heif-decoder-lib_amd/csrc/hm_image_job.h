// hm_image_job.h — internal: one image decode (HEIF item -> pixels) split into the phases the image-at-a-time entry
// (hm_decode_item) runs back to back and the pipelined entry (hm_pipeline_*, pipeline.cpp) overlaps across images:
//   job_plan         which coded pictures (grid tiles, alpha auxiliary image, gain map), where they go host, cheap
//   job_parse_tile   entropy decode of one coded picture -> command stream                          host, the Amdahl term
//   job_enqueue      H2D, reconstruction, filters, paste, transforms, colour, D2H on the job's stream  asynchronous
//   job_complete     wait for the stream
// Not part of the C ABI.
#ifndef HM_IMAGE_JOB_H
#define HM_IMAGE_JOB_H

#include <memory>
#include <string>
#include <vector>

#include "heif_file.h"
#include "hm_devdest.h"
#include "hm_entry_steps.h"
#include "hm_internal.h"
#include "hm_stream.h"

struct hm_file {
  std::vector<uint8_t> bytes;
  hm::HeifFile file;
};

namespace hm_img {

struct DevMem {
  void* p = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  int alloc(size_t n)
  {
    p = hm_pool_device_alloc(n);
    return p ? HM_OK : HM_ERR_NO_DEVICE;
  }
  void swap(DevMem& o) { void* t = p; p = o.p; o.p = t; }
  ~DevMem() { if (p) hm_pool_device_free(p); }
};

// one plane of the decoded image on the device, libheif plane layout (pixelimage.cc:139-218)
struct DevPlane {
  DevMem mem;
  int w = 0, h = 0, stride = 0; // samples, samples, bytes
};

struct Blob {
  uint8_t* p = nullptr;
  size_t n = 0;
  Blob() = default;
  Blob(const Blob&) = delete;
  Blob& operator=(const Blob&) = delete;
  Blob(Blob&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  ~Blob() { if (p) hm_free(p); }
};

// A decoded image on the device: what HeifContext::decode_image_planar returns (YCbCr planes after the item's
// transformative properties), plus everything that must outlive the asynchronous work that produced it.
// planes of a grid tile whose item carries its own irot / imir / clap: decoded there, transformed, then pasted
struct OwnTile { int index = 0; DevPlane P[3]; int w = 0, h = 0; int chroma = 1, bd = 8; };
struct PlanarImage {
  DevPlane P[3];
  int w = 0, h = 0, chroma = 1, bd = 8;
  hm::NclxProfile native; // profile of the decoded image (VUI, overridden by an item 'colr' nclx)
  bool is_grid = false;
  int warnings = 0; // HM_WARN_* of the (single) coded picture
  std::vector<std::unique_ptr<DevMem>> retired;
  // (a member, not a local of the function that queues work on them: every early return of that function leaves them
  //  alive until the job's destructor has drained the stream)
  std::vector<std::unique_ptr<OwnTile>> own;
  // a grid whose TILE items carry alpha auxiliary images (context.cc:2029-2078 inside decode_image_planar, reached per
  // tile from decode_and_paste_tile_image; the canvas then gets an alpha plane, :2437-2455): the tiles' alpha pictures
  // and the canvas-sized alpha plane they are pasted into (opaque where a tile has none)
  std::vector<std::unique_ptr<OwnTile>> own_alpha;
  DevPlane tile_alpha;
  int tile_alpha_bd = 0; // 0: no tile of the grid has an alpha image
  std::unique_ptr<hm_batch, void (*)(hm_batch*)> batch{nullptr, hm_batch_destroy};
  // the interleaved pixels, when the colour conversion was attached to the batch (hm_batch_set_colour: the fused tail kernels
  // where the pictures allow them, else the same kernels as hm_colour_convert) - planar_from_blobs, `attach`
  DevMem rgb;
  bool rgb_attached = false;
  // the colour-space tag: P[0..2] are R, G, B planes (an 'unci' item of R G B components, each plane at its own depth) - handed out
  // as decoded, or as the interleaved pixels in `rgb`; no colour chain starts from them
  bool rgb_planes = false;
};

struct TilePlan { uint32_t id = 0; int x0 = 0, y0 = 0; };
// the coded pictures of one image item (a single hvc1 image or the tiles of a grid)
struct ItemPlan {
  uint32_t id = 0;
  bool is_grid = false;
  // a coded image decoded as the 1 x 1 grid of itself (DESIGN Q19: an hvc1 child of a derived item for which the reference finds no
  // colour chain): the grid's paste and profile rules on its one picture; its own transformations stay the item's, not a tile's
  bool self_grid = false;
  int canvas_w = 0, canvas_h = 0, cols = 0, rows = 0;
  std::vector<TilePlan> tiles;
  std::vector<Blob> blobs;           // command streams, filled by job_parse_tile
  std::vector<int> status;
  std::vector<std::string> messages;
  // grids: alpha auxiliary images of the tile items - (tile index, alpha item) pairs and their command streams
  struct TileAlpha { int tile = 0; uint32_t id = 0; };
  std::vector<TileAlpha> tile_alpha;
  std::vector<Blob> alpha_blobs;
  std::vector<int> alpha_status;
  std::vector<std::string> alpha_messages;
  // a slot (command stream, status, message) per coded picture of `tiles` and of `tile_alpha`, empty: nothing parsed yet
  void reset_slots()
  {
    blobs.clear(); blobs.resize(tiles.size());
    status.assign(tiles.size(), HM_OK);
    messages.assign(tiles.size(), std::string());
    alpha_blobs.clear(); alpha_blobs.resize(tile_alpha.size());
    alpha_status.assign(tile_alpha.size(), HM_OK);
    alpha_messages.assign(tile_alpha.size(), std::string());
  }
  // tile rows [r0, r0 + n) and columns [c0, c0 + m) of this grid as a grid of its own on a canvas of w x h, nothing parsed yet:
  // everything behind sees an ordinary smaller grid (a view's sub-grid, a slab of tile rows).  For grids without tile alpha images.
  ItemPlan sub_grid(int r0, int n, int c0, int m, int w, int h) const
  {
    ItemPlan S;
    S.id = id; S.is_grid = true; S.rows = n; S.cols = m; S.canvas_w = w; S.canvas_h = h;
    for (int r = r0; r < r0 + n; r++)
      for (int c = c0; c < c0 + m; c++) S.tiles.push_back(tiles[(size_t)r * cols + c]);
    S.reset_slots();
    return S;
  }
};

// The light statistics of a decode (include/heif_mi355x.h "Light statistics"): the entry's request and, behind the decode, its result.
// mode HM_MEASURE_STATS: the pixels are measured and not written (the target's dest is hm_stats_stand_in_dest); HM_MEASURE_TONE: measured,
// then written through the tone step with src_peak = the percentile's nits (the target's tone step carries a stand-in peak until then).
struct LightMeasure {
  int mode = HM_MEASURE_NONE;
  float unit_nits = 0.0f;   // STATS: as the caller gave it (TONE: the tone step's)
  double fraction = 1.0;    // TONE: of the percentile
  bool done = false;
  hm_light_stats stats{};   // filled by emit_image
};

// Many views of one item (hm_decode_item_to_device_views): the caller's arrays - views[k] into dests[k], k < count -, out[k] for the sizes
// written, count zeroed scratch entries the entry owns, and where the index of a view that was refused goes (may be NULL)
struct ViewsRequest {
  const hm_device_view* views = nullptr;
  const hm_device_dest* dests = nullptr;
  int32_t count = 0;
  hm_decoded* out = nullptr;
  hm_view_scratch* scratch = nullptr;
  int32_t* failed = nullptr;
};

// Where the result of a decode goes beside hm_decoded: every function between an entry point and emit_image takes one of these.
// All null: pinned host memory (or params->ext_dst).  The pointers are the caller's; target_check_shape states what goes together.
// On the way in a target passes one front, each part of it stated once: of_entry (which pointers the entry's kind takes:
// hm_entry_steps.h), resolve_request (the request against the file: the tone step's peak, the gain step's items) and
// check_target_request (its three phases: the request alone, against what the file declares, a device and the pointers).
struct OutputTarget {
  const hm_device_dest* dest = nullptr;        // the interleaved pixels go to caller-owned device memory; nothing is copied to the host
  const hm_device_view* view = nullptr;        // ... a rectangle of the image, resampled (with dest or planes)
  const hm_device_planes* planes = nullptr;    // a planar result (out_format 0 / HM_OUT_YCBCR_*) goes to caller-owned device memory, plane by plane
  const hm_device_light* light = nullptr;      // the light step in the write of dest
  const hm_device_tone* tone = nullptr;        // ... with a tone step inside it (src_peak resolved by resolve_request: never 0 here)
  const hm_device_alpha* alpha = nullptr;      // the alpha step in the write of dest (alone, or beside light and tone)
  const hm_device_gain* gain = nullptr;        // the gain step beside light (resolved by resolve_request: map_item is the map's item, params are explicit)
  const struct PlanarImage* gain_map = nullptr; // ... and its decoded map (job_enqueue sets it; null with a gain step of weight 0)
  const hm_device_ootf* ootf = nullptr;        // the OOTF step beside light (a tone step beside it keeps its zeros: they resolve to display_peak)
  const uint8_t* icc = nullptr;                // the ICC profile a light step with HM_LIGHT_FROM_ICC reads (resolve_request: the item's own, inside the
  size_t icc_size = 0;                         // open file, which outlives the job)
  LightMeasure* measure = nullptr;             // the light statistics of the interleaved pixels (with dest and light), the entry's own: it outlives the decode
  hm_view_scratch* scratch = nullptr;          // tap tables and the intermediate of the resampling step, the tables of the light step
  hm_view_item* view_later = nullptr;          // view + dest: the view is not written, only described there - the caller writes it with those of other images
  hm_planes_view_item* planes_later = nullptr; // the same for view + planes
  const ViewsRequest* views = nullptr;         // many views of the interleaved pixels, each into a destination of its own (in place of dest and view)
  int views_dx = 0, views_dy = 0;              // ... the origin of the sub-grid that was decoded: every crop moves by it (job_enqueue sets it)
  hm_device_view view_of(int k) const          // view k of `views` as the decoded image sees it
  {
    hm_device_view v = views->views[k];
    if (v.crop_w || v.crop_h) { v.crop_x -= views_dx; v.crop_y -= views_dy; }
    return v;
  }
  // the target of a device entry of `kind` (hm_entry_kind): its destination - d or p, whichever the entry has - with the step pointers
  // the caller passed, or the refusal ("null argument" for a null destination, else hm_entry_steps')
  static int of_entry(int kind, const hm_out_steps& st, const hm_device_dest* d, const hm_device_planes* p, OutputTarget& t,
                      bool view_may_be_null = false)
  {
    if (!d && !p) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
    const int rc = hm_entry_steps(kind, st, view_may_be_null);
    if (rc) return rc;
    t = OutputTarget();
    t.dest = d; t.planes = p; t.view = st.view; t.light = st.light; t.tone = st.tone; t.alpha = st.alpha; t.gain = st.gain; t.ootf = st.ootf;
    return HM_OK;
  }
  hm_out_steps steps() const { return hm_out_steps{view, light, tone, alpha, gain, ootf, icc, icc_size, measure ? measure->mode : (int)HM_MEASURE_NONE}; } // the request of the device write (hm_devdest.h)
};
// views excludes dest, view, planes, gain, measure and both *_later, and stands where dest stands for light and alpha;
// dest xor planes (or neither); light only with dest; tone only with light; ootf only with light; alpha only with dest and never with view_later; gain only with light and
// never with view_later; view only with one of the two; a *_later only with view and its own kind of destination
int target_check_shape(const OutputTarget& t);

// a job's own copies of the caller's structs (the pipeline outlives them; hm_decode_params keeps its layout, so they travel beside
// the job's copy of it).  t points into the copies: a null pointer there means "not given".
struct OwnedTarget {
  hm_device_dest dest{};
  hm_device_view view{};
  hm_device_planes planes{};
  hm_device_light light{};
  hm_device_tone tone{};
  hm_device_alpha alpha{};
  hm_device_gain gain{};
  hm_device_ootf ootf{};
  OutputTarget t;
  OwnedTarget() = default;
  OwnedTarget(const OwnedTarget&) = delete;
  OwnedTarget& operator=(const OwnedTarget&) = delete;
  void set(const OutputTarget& from)
  {
    t = OutputTarget();
    if (from.dest) { dest = *from.dest; t.dest = &dest; }
    if (from.view) { view = *from.view; t.view = &view; }
    if (from.planes) { planes = *from.planes; t.planes = &planes; }
    if (from.light) { light = *from.light; t.light = &light; }
    if (from.tone) { tone = *from.tone; t.tone = &tone; }
    if (from.alpha) { alpha = *from.alpha; t.alpha = &alpha; }
    if (from.gain) { gain = *from.gain; t.gain = &gain; }
    if (from.ootf) { ootf = *from.ootf; t.ootf = &ootf; }
    t.icc = from.icc; t.icc_size = from.icc_size; // (the file's bytes: the job holds the file)
    t.measure = from.measure;
    t.views = from.views; // (the caller's arrays: the item entry returns before they go)
  }
};

struct DecodeJob {
  const hm_file* f = nullptr;
  uint32_t id = 0;
  hm_decode_params params{};
  // where the result goes (target.set): with a light step the item is decoded as one job, never slab by slab.
  // With a view, job_plan reduces item[0] to the sub-grid of tiles the crop touches where that changes no pixel - sub_tiles = its
  // first tile row, row count, first tile column, column count in the whole grid - and the crop moves by the sub-grid's origin
  // (view_dx, view_dy)
  OwnedTarget target;
  int view_dx = 0, view_dy = 0;
  int32_t sub_tiles[4] = {0, 0, 0, 0};
  hm_view_scratch view_scratch{}; // what job_enqueue hands to emit_image as the target's scratch
  bool self_grid = false; // item[0] is planned as the 1 x 1 grid of itself (ItemPlan::self_grid)
  hipStream_t s = nullptr;
  ItemPlan item[3];   // [0] the image, [1] its alpha auxiliary image, [2] the gain map of a gain step (has_map)
  int n_items = 0;    // of [0] and [1]
  bool has_map = false; // item[2] is planned: a gain step whose weight is not 0
  PlanarImage I, A, G;
  DevPlane alpha_scaled;
  DevPlane alpha_sdr; // a deeper alpha plane brought to 8 bits (Op_to_sdr_planes) for an RGBA target
  DevMem dout;
  int few_pictures = 0; // the job's pictures are a whole (small) batch: HM_RECORDS_SPLIT - with few pictures the rows of a picture are
                        // the parallel work, which only the split-chain kernels offer (profiles/r03_class_shape_sweeps.txt)
  bool enqueued = false;
  // An 'unci' item (ISO/IEC 23001-17): a leaf without coded pictures - job_plan plans zero entropy decodes, job_enqueue uploads the
  // payload (under a view: the byte ranges of the internal tiles in sub_tiles) and launches the unpack (unci.hip).  allow_unci: the
  // entry takes such items (hm_decode_item and its device forms; the pipeline, batch and sequence entries refuse them in job_plan).
  bool allow_unci = false, unci = false, unci_sub = false;
  hm_unci_info unci_info{};
  void* unci_staging = nullptr; // pinned: the bytes on their way to the device
  DevMem unci_bytes;
  DevPlane unci_alpha;          // the plane of an alpha component
  // everything above is touched by asynchronous work: the stream is drained before any of it is released (the pool may
  // hand a freed block to another thread at once)
  ~DecodeJob()
  {
    if (enqueued) hipStreamSynchronize(s);
    hm_view_scratch_free(&view_scratch);
    if (unci_staging) hm_pool_pinned_free(unci_staging);
  }
};

int job_plan(DecodeJob& j);
int job_tile_count(const DecodeJob& j);
void job_parse_tile(DecodeJob& j, int k, int row_threads = 1); // k = 0 .. job_tile_count - 1 (main image tiles first, then alpha, then the gain map's); thread-safe per tile;
                                                                // row_threads > 1: WPP rows of this picture in parallel (hm_hevc_parse_mt)
// the entropy decode of one coded picture (hvc1 item or movie sample `id`) into `blob`, or its failure in status / message
void parse_picture(const hm_file* f, uint32_t id, bool few_pictures, int strict, int row_threads, Blob& blob, int& status, std::string& message);
int job_enqueue(DecodeJob& j, hm_decoded* out);
// everything about a target (dest or planes, with its view and steps) that can be refused before the entropy decode, in three phases
// (hm_image.cpp: check_request_alone, check_request_declared, check_request_pointers; a sequence loops each over its frames):
//   the request itself - its shape, params->ext_dst, the static checks of the destination and the steps, a null pointer;
//   the target against what hm_image_info declares for the item (target_fits: size, and for planes the result's chroma format and depth
//   where the file decides them; the crop of a view against the declared size, the destination against the view's output size);
//   a device, the pointers
int check_target_request(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& t);
// the tone step an entry point hands on: the caller's, with src_peak == 0 replaced by the peak of item `id` (its clli, its mdcv, 1000;
// id 0 or a frame of a sequence: 1000).  The other refusals are check_target_request's.
hm_device_tone tone_for_item(const hm_file* f, uint32_t id, const hm_device_tone* tone);
// A request resolved against the file, in the one order every entry keeps: the tone step's src_peak from the item asked for (only
// without an OOTF step: beside one 0 is display_peak and no property is read); the ICC profile of a light step with HM_LIGHT_FROM_ICC - of
// the item that is decoded, parsed here: an item without one, or with one the reader refuses, fails -; the gain step from that item too (hm_gain_for_item: a
// 'tmap' item's own properties) - the item to decode becomes the base image; refuse_derived: what a derived item is refused for without
// looking at a picture (the item entries; the pipeline leaves it to job_plan); check_target_request.  t points into tone and gain.
struct ResolvedRequest {
  hm_device_tone tone{};
  hm_device_gain gain{};
  OutputTarget t;
  uint32_t id = 0; // the item to decode
  ResolvedRequest() = default;
  ResolvedRequest(const ResolvedRequest&) = delete;
  ResolvedRequest& operator=(const ResolvedRequest&) = delete;
};
int resolve_request(const hm_file* f, uint32_t id, const hm_decode_params* params, const OutputTarget& asked, bool refuse_derived,
                    ResolvedRequest& r);
int job_complete(DecodeJob& j, hm_decoded* out);

} // namespace hm_img

// The gain step of a decode of item `id`, resolved before anything is queued: *base = the base image's item (the item the job decodes),
// *own = the step with map_item the map's item and explicit parameters (a 'tmap' item's: from its payload).  Everything the file says
// about the map is judged here: its kind, chroma format and depth, and the geometry against the sizes the file declares.
extern "C" int hm_gain_for_item(const hm_file* f, uint32_t id, const hm_decode_params* params, const hm_device_view* view, const hm_device_gain* gain, uint32_t* base,
                                hm_device_gain* own);
#endif
