// heif_file.h — minimal ISOBMFF / HEIF reader for the decode path (host side).
// Counterpart of the parts of libheif/file.cc, box.cc and codecs/hevc.cc the hot path needs:
// item locations (iloc), item infos (iinf), references (iref: dimg/auxl/thmb), properties
// (ipco/ipma: hvcC, ispe, pixi, colr, irot, imir, clap, auxC, clli, mdcv, cmpd, uncC, mskC), primary item (pitm), idat, and the payload of a 'tmap'
// item (ISO 21496-1 gain map: include/heif_mi355x.h states its layout).  'unci' items (ISO/IEC 23001-17): libheif/codecs/uncompressed_box.cc.
// Region items ('rgan') and mask items ('mski' + mskC): libheif/region.cc, codecs/mask_image.cc, context.cc:1166-1237; the rules of
// include/heif_mi355x.h, "Regions and masks".
// Movie mode (the fork's image sequences): a 'moov' track of HEVC-intra samples, each sample a top-level image
// (file.cc:474-483, 1154-1244; context.cc:646-700 of the reference).
#ifndef HM_HEIF_FILE_H
#define HM_HEIF_FILE_H

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "heif_mi355x.h"

namespace hm {

struct HeifError {
  int status;          // hm_status
  std::string message;
  int detail = 0;      // hm_error_detail
};

struct NclxProfile {
  bool present = false;
  int primaries = 2, transfer = 2, matrix = 2, full_range = 1;
};

struct HvcC {
  bool present = false;
  int chroma_format = 1, bit_depth_luma = 8, bit_depth_chroma = 8, length_size = 4;
  std::vector<std::vector<uint8_t>> nals; // parameter-set NAL units in order
};

// One transformative item property; a decoder applies them in the order of the item's ipma associations
// (context.cc:1957-2020 of the reference).
struct Transform {
  enum Kind { Rotate = 1, Mirror = 2, CleanAperture = 3 } kind;
  int angle = 0;            // irot: counter-clockwise, degrees (0, 90, 180, 270)  (box.cc:3590-3600)
  int horizontal = 0;       // imir: axis & 1 -> heif_transform_mirror_direction_horizontal (box.cc:3626-3639)
  uint32_t width_n = 0, width_d = 1, height_n = 0, height_d = 1; // clap (box.cc:3676-3716)
  int32_t hoff_n = 0; uint32_t hoff_d = 1;
  int32_t voff_n = 0; uint32_t voff_d = 1;
};

// 'cmpd' + 'uncC' of an 'unci' item as the boxes state them (uncompressed_box.cc:131-279); HeifFile::unci_info judges them
struct UncC {
  bool present = false, has_cmpd = false;
  int version = 0;
  uint32_t profile = 0;                 // fourcc as a big-endian number
  std::vector<uint16_t> cmpd_types;     // component_type per cmpd entry
  struct Component { uint16_t index; uint16_t depth; uint8_t format, align_size; };
  std::vector<Component> components;
  int sampling = 0, interleave = 0, block_size = 0, flags = 0;
  uint32_t pixel_size = 0, row_align = 0, tile_align = 0;
  uint64_t tile_cols = 1, tile_rows = 1;
  bool generic_compression = false;     // a 'cmpC' or 'icbr' property is associated
};

struct ItemProps {
  HvcC hvcc;
  UncC uncc;
  int ispe_width = 0, ispe_height = 0;
  NclxProfile colr;
  // raw colour profile of a 'colr' box of type 'prof' / 'rICC' (ICC data, passed through untouched: box.cc Box_colr,
  // nclx.h color_profile_raw); an item may carry both an nclx and an ICC profile
  uint32_t icc_type = 0;     // fourcc as a big-endian number, 0 = none
  std::vector<uint8_t> icc;
  bool has_irot = false, has_imir = false, has_clap = false;
  int irot_angle = 0;
  std::vector<Transform> transforms; // irot / imir / clap in association order
  std::string aux_type;
  // 'clli' / 'mdcv' (box.cc:3120-3178 of the reference: plain boxes, no version word): the raw fields
  bool has_clli = false, has_mdcv = false;
  uint16_t clli[2] = {0, 0};   // max_content_light_level, max_pic_average_light_level
  uint16_t mdcv_xy[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // display_primaries x0 y0 x1 y1 x2 y2, white point x y
  uint32_t mdcv_lum[2] = {0, 0}; // max / min display mastering luminance, 0.0001 cd/m2
  // 'mskC' (codecs/mask_image.cc:33-45): a full box holding bits_per_pixel
  bool has_mskc = false;
  int mskc_bits = 0;
};

struct Extent { uint64_t offset, length; };

struct Item {
  uint32_t id = 0;
  std::string type;           // "hvc1", "grid", "Exif", ...
  int construction_method = 0; // 0 file offset, 1 idat
  uint64_t base_offset = 0;
  std::vector<Extent> extents;
  ItemProps props;
  bool hidden = false;
  // a mask image: an 'mski' item that carries its 'mskC' (one without is no image: "Missing required box for mask codec")
  bool is_mask() const { return type == "mski" && props.has_mskc; }
  // a leaf without coded pictures whose samples lie uncompressed in its payload: an 'unci' item, or a mask image as a monochrome one
  bool is_raw_leaf() const { return type == "unci" || is_mask(); }
};

// One region of an 'rgan' item as its payload states it (RegionGeometry::parse, region.cc:203-422)
struct Region {
  int type = 0;                  // HM_REGION_*
  int32_t x = 0, y = 0;
  uint32_t w = 0, h = 0;         // size; an ellipse's radii.  A referenced mask: a stated 0 replaced by the mask item's ispe
  std::vector<int32_t> points;   // x, y pairs (polygon, polyline)
  std::vector<uint8_t> bits;     // an inline mask's (w * h + 7) / 8 bytes
  uint32_t mask_item = 0;        // a referenced mask: its entry of the item's 'mask' reference
};
// An 'rgan' item read at open; a damaged one keeps its error for the calls that read it
struct RegionItem {
  HeifError err{0, ""};          // status 0: the item reads
  uint32_t reference_width = 0, reference_height = 0;
  int field_bits = 16;
  std::vector<Region> regions;
};

struct GridInfo {
  int rows = 0, cols = 0;
  uint32_t width = 0, height = 0;
  std::vector<uint32_t> tiles; // item ids, row-major
};

// 'iovl' descriptor + 'dimg' references (context.cc:318-369, 2579-2616): the layers in reference order, bottom first
struct OverlayInfo {
  uint32_t width = 0, height = 0;
  uint16_t background[4] = {0, 0, 0, 0}; // R G B A, 16 bit (the canvas is filled with R G B >> 8; A is ignored)
  std::vector<uint32_t> children;
  std::vector<int32_t> dx, dy;
};

// 'tmap' payload + 'dimg' references (include/heif_mi355x.h states the layout): every fraction as numerator / denominator in double
struct GainMapInfo {
  uint32_t base = 0, map = 0; // dimg [0], [1]
  int writer_version = 0;
  bool multichannel = false, use_base_colour_space = false;
  double base_headroom = 0, alternate_headroom = 0;
  double map_min[3] = {0, 0, 0}, map_max[3] = {0, 0, 0}, gamma[3] = {1, 1, 1}, base_offset[3] = {0, 0, 0}, alternate_offset[3] = {0, 0, 0};
};

// The fork's movie mode: ftyp lists the compatible brand 'hevc' or 'hevx' and a 'moov' box exists; 'meta' is then
// ignored.  Every sample of the (first) track is an image: IDs 1..frame_count, ID 1 the primary one.
struct Movie {
  uint32_t frame_count = 0;        // samples_per_chunk of the one 'stsc' entry (context.cc:654-676)
  uint64_t duration = 0;           // mvhd duration (box.cc:1214-1230)
  uint32_t width = 0, height = 0;  // tkhd width / height >> 16: every frame's handle size (context.cc:678-700)
  uint32_t chunk_offset = 0;       // the first 'stco' offset: where sample 0 starts (box.cc:1944-1952)
  uint32_t sample_size = 0;        // 'stsz' constant size, 0 = per entry
  std::vector<uint64_t> sample_start; // per-entry 'stsz': start of sample k relative to chunk_offset (prefix sums)
  std::vector<uint32_t> entry_size;
  std::vector<std::vector<std::vector<uint8_t>>> nal_arrays; // hvcC NAL arrays of the 'hvc1' sample entry, in order
  Item frame;                      // what every frame looks like as an item (hvc1, hvcC, ispe = tkhd size)
};

class HeifFile {
 public:
  // parses the box structure; returns false and fills err on malformed input
  bool parse(const uint8_t* data, size_t size, HeifError& err);
  uint32_t primary_id() const { return primary_; }
  const std::map<uint32_t, Item>& items() const { return items_; }
  const Item* item(uint32_t id) const;
  std::vector<uint32_t> top_level_images() const;
  // raw item payload (concatenated extents)
  bool item_data(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const;
  // what a decoder plugin receives for an hvc1 item: hvcC NALs then the item's NALs, each with a
  // 4-byte big-endian length (codecs/hevc.cc:226-247 + file.cc:1496-1535 in the reference)
  bool hevc_data(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const;
  // 'grid' descriptor + 'dimg' references (context.cc:172-221, 2142-2153)
  bool grid_info(uint32_t id, GridInfo& g, HeifError& err) const;
  std::vector<uint32_t> references(uint32_t from, const char* type) const;
  // 'iovl' payload (hm_overlay_plan.h) + 'dimg' references
  bool overlay_info(uint32_t id, OverlayInfo& o, HeifError& err) const;
  // the one image an 'iden' item derives from (context.cc:2542-2576); 0 and err when the references are not exactly one other item
  uint32_t derived_child(uint32_t id, HeifError& err) const;
  // the auxiliary image that is the alpha channel of image `id` (0 if none): an 'auxl' reference to `id` from an item
  // whose auxC names an alpha type (context.cc:885-945)
  uint32_t alpha_item_of(uint32_t id) const;
  // a 'tmap' item: its two 'dimg' references and its payload
  bool gain_map_info(uint32_t id, GainMapInfo& g, HeifError& err) const;
  // the first 'tmap' item whose first 'dimg' reference is `base` (0 if none)
  uint32_t gain_map_of(uint32_t base) const;
  // an 'unci' item: its cmpd / uncC / ispe judged and turned into the description the layout starts from (hm_unci_layout.h)
  // ... and a mask image ('mski' + mskC, 8 bits) as the monochrome 8-bit item in component interleave its payload is (mask_image.cc:95-125)
  bool unci_info(uint32_t id, hm_unci_info& info, HeifError& err) const;
  // an 'rgan' item: nullptr and err when `id` is none or the item is damaged
  const RegionItem* region_item(uint32_t id, HeifError& err) const;
  // the 'rgan' items whose 'cdsc' reference names `image`, in item-id order
  std::vector<uint32_t> region_items_of(uint32_t image) const;
  // where an item's payload lies when it is ONE run of bytes of the file (or of idat): *p, *n; false: several extents (item_data joins them)
  bool item_span(uint32_t id, const uint8_t** p, size_t* n, HeifError& err) const;
  bool is_movie() const { return movie_mode_; }
  const Movie& movie() const { return movie_; }

 private:
  struct Ref { std::string type; uint32_t from; std::vector<uint32_t> to; };
  bool parse_meta(const uint8_t* p, size_t n, HeifError& err);
  bool parse_iprp(const uint8_t* p, size_t n, HeifError& err);
  bool parse_moov(const uint8_t* p, size_t n, HeifError& err);
  void parse_region_item(uint32_t id, RegionItem& r) const;
  std::map<uint32_t, RegionItem> regions_;
  bool movie_sample(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const;
  bool movie_mode_ = false;
  Movie movie_;
  const uint8_t* data_ = nullptr;
  size_t size_ = 0;
  uint32_t primary_ = 0;
  std::map<uint32_t, Item> items_;
  std::vector<Ref> refs_;
  std::vector<uint8_t> idat_;
};

} // namespace hm
#endif
