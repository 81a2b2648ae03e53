// heif_file.cpp — see heif_file.h.  Written from ISO/IEC 14496-12 and 23008-12 box definitions.
#include "heif_file.h"
#include "hm_overlay_plan.h"
#include "hm_unci_layout.h"

#include <algorithm>
#include <cstring>

#include "heif_mi355x.h"

namespace hm {
namespace {

struct Rd {
  const uint8_t* p;
  size_t n, pos = 0;
  bool ok = true;
  Rd(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
  size_t left() const { return n - pos; }
  uint64_t u(int bytes)
  {
    if (left() < (size_t)bytes) { ok = false; pos = n; return 0; }
    uint64_t v = 0;
    for (int i = 0; i < bytes; i++) v = (v << 8) | p[pos++];
    return v;
  }
  void skip(size_t k) { if (left() < k) { ok = false; pos = n; } else pos += k; }
  std::string fourcc()
  {
    if (left() < 4) { ok = false; pos = n; return ""; }
    std::string s((const char*)p + pos, 4);
    pos += 4;
    return s;
  }
  std::string cstr()
  {
    std::string s;
    while (pos < n && p[pos]) s.push_back((char)p[pos++]);
    if (pos < n) pos++;
    return s;
  }
};

struct Box {
  std::string type;
  const uint8_t* body;
  size_t size;
};

// iterate the boxes of a container
bool next_box(Rd& r, Box& b)
{
  if (r.left() < 8) return false;
  uint64_t sz = r.u(4);
  b.type = r.fourcc();
  size_t hdr = 8;
  if (sz == 1) { sz = r.u(8); hdr = 16; }
  else if (sz == 0) sz = r.left() + hdr;
  if (b.type == "uuid") { r.skip(16); hdr += 16; }
  if (!r.ok || sz < hdr || sz - hdr > r.left()) { r.ok = false; return false; }
  b.body = r.p + r.pos;
  b.size = (size_t)(sz - hdr);
  r.pos += b.size;
  return true;
}

} // namespace

const Item* HeifFile::item(uint32_t id) const
{
  if (movie_mode_) return id >= 1 && id <= movie_.frame_count ? &movie_.frame : nullptr;
  auto it = items_.find(id);
  return it == items_.end() ? nullptr : &it->second;
}

std::vector<uint32_t> HeifFile::references(uint32_t from, const char* type) const
{
  for (const Ref& r : refs_)
    if (r.from == from && r.type == type) return r.to;
  return {};
}

uint32_t HeifFile::alpha_item_of(uint32_t id) const
{
  uint32_t alpha = 0;
  for (const Ref& r : refs_) {
    if (r.type != "auxl" || r.from == id) continue;
    const Item* aux = item(r.from);
    if (!aux) continue;
    const std::string& t = aux->props.aux_type;
    if (t != "urn:mpeg:avc:2015:auxid:1" && t != "urn:mpeg:hevc:2015:auxid:1" && t != "urn:mpeg:mpegB:cicp:systems:auxiliary:alpha") continue;
    for (uint32_t to : r.to)
      if (to == id) alpha = r.from; // a later reference replaces an earlier one (Image::set_alpha_channel)
  }
  return alpha;
}

std::vector<uint32_t> HeifFile::top_level_images() const
{
  // images that are not tiles / thumbnails / auxiliary images of another item
  std::vector<uint32_t> out;
  if (movie_mode_) { // every sample, in track order (context.cc:664-673)
    out.resize(movie_.frame_count);
    for (uint32_t k = 0; k < movie_.frame_count; k++) out[k] = k + 1;
    return out;
  }
  for (const auto& kv : items_) {
    const Item& it = kv.second;
    if (it.type != "hvc1" && it.type != "grid" && it.type != "iden" && it.type != "iovl" && it.type != "unci" && !it.is_mask()) continue;
    bool sub = false;
    for (const Ref& r : refs_) {
      if (r.type == "mask") // (the mask of a region is no image of its own: context.cc:1230, remove_top_level_image)
        for (uint32_t t : r.to) if (t == it.id) sub = true;
      if ((r.type == "thmb" || r.type == "auxl") && r.from == it.id) sub = true;
      if (r.type == "dimg") {
        const Item* from = item(r.from);
        if (from && from->type == "tmap") continue; // (base and gain map of a 'tmap' item stay images of their own)
        for (uint32_t t : r.to) if (t == it.id) sub = true;
      }
    }
    if (!sub && !it.hidden) out.push_back(it.id);
  }
  return out;
}

bool HeifFile::parse(const uint8_t* data, size_t size, HeifError& err)
{
  data_ = data;
  size_ = size;
  items_.clear();
  refs_.clear();
  regions_.clear();
  idat_.clear();
  primary_ = 0;
  movie_mode_ = false;
  movie_ = Movie();
  Rd r(data, size);
  Box b;
  bool have_ftyp = false, movie_brand = false;
  std::vector<Box> metas;
  const Box* moov = nullptr;
  Box moov_box;
  while (next_box(r, b)) {
    if (b.type == "ftyp") {
      have_ftyp = true;
      // compatible brands only, not the major brand (Box_ftyp::has_compatible_brand, box.cc:1057-1085)
      for (size_t o = 8; o + 4 <= b.size; o += 4)
        if (!std::memcmp(b.body + o, "hevc", 4) || !std::memcmp(b.body + o, "hevx", 4)) movie_brand = true;
    }
    else if (b.type == "meta") metas.push_back(b);
    else if (b.type == "moov" && !moov) { moov_box = b; moov = &moov_box; }
  }
  // the fork's movie mode (file.cc:474-483): the brand and a 'moov' box; 'meta' is then not read (context.cc:435-437)
  if (movie_brand && moov) {
    if (!parse_moov(moov->body, moov->size, err)) return false;
    movie_mode_ = true;
    primary_ = 1;
    return true;
  }
  for (const Box& m : metas)
    if (!parse_meta(m.body, m.size, err)) return false;
  if (!have_ftyp) { err = {HM_ERR_BITSTREAM, "no ftyp box: not a HEIF file"}; return false; }
  if (metas.empty()) { err = {HM_ERR_BITSTREAM, "no meta box"}; return false; }
  if (!primary_ || !items_.count(primary_)) { err = {HM_ERR_BITSTREAM, "no primary item"}; return false; }
  // the region items: read now, judged by the calls that read them (a damaged one does not fail the file)
  regions_.clear();
  for (const auto& kv : items_)
    if (kv.second.type == "rgan") parse_region_item(kv.first, regions_[kv.first]);
  return true;
}

bool HeifFile::parse_meta(const uint8_t* p, size_t n, HeifError& err)
{
  Rd r(p, n);
  r.skip(4); // FullBox version/flags
  Box b;
  const uint8_t* iprp = nullptr;
  size_t iprp_n = 0;
  while (next_box(r, b)) {
    Rd q(b.body, b.size);
    if (b.type == "pitm") {
      const int ver = (int)q.u(1); q.skip(3);
      primary_ = (uint32_t)q.u(ver == 0 ? 2 : 4);
    }
    else if (b.type == "iinf") {
      const int ver = (int)q.u(1); q.skip(3);
      const uint32_t cnt = (uint32_t)q.u(ver == 0 ? 2 : 4);
      Box e;
      for (uint32_t i = 0; i < cnt && next_box(q, e); i++) {
        if (e.type != "infe") continue;
        Rd f(e.body, e.size);
        const int v = (int)f.u(1);
        const uint32_t flags = (uint32_t)f.u(3);
        if (v < 2) continue;
        Item it;
        it.id = (uint32_t)f.u(v == 2 ? 2 : 4);
        f.skip(2); // protection index
        it.type = f.fourcc();
        it.hidden = (flags & 1) != 0;
        if (!f.ok) { err = {HM_ERR_BITSTREAM, "truncated infe box"}; return false; }
        Item& dst = items_[it.id];
        dst.id = it.id; dst.type = it.type; dst.hidden = it.hidden;
      }
    }
    else if (b.type == "iloc") {
      const int ver = (int)q.u(1); q.skip(3);
      const int a = (int)q.u(1), c = (int)q.u(1);
      const int offset_size = a >> 4, length_size = a & 15, base_size = c >> 4, index_size = (ver == 1 || ver == 2) ? (c & 15) : 0;
      const uint32_t cnt = (uint32_t)q.u(ver < 2 ? 2 : 4);
      for (uint32_t i = 0; i < cnt && q.ok; i++) {
        const uint32_t id = (uint32_t)q.u(ver < 2 ? 2 : 4);
        int cm = 0;
        if (ver == 1 || ver == 2) cm = (int)(q.u(2) & 15);
        q.skip(2); // data_reference_index
        const uint64_t base = q.u(base_size);
        const int ext = (int)q.u(2);
        Item& it = items_[id];
        it.id = id;
        it.construction_method = cm;
        it.base_offset = base;
        it.extents.clear();
        for (int k = 0; k < ext && q.ok; k++) {
          if (index_size) q.u(index_size);
          Extent e;
          e.offset = q.u(offset_size);
          e.length = q.u(length_size);
          it.extents.push_back(e);
        }
      }
      if (!q.ok) { err = {HM_ERR_BITSTREAM, "truncated iloc box"}; return false; }
    }
    else if (b.type == "iref") {
      const int ver = (int)q.u(1); q.skip(3);
      Box e;
      while (next_box(q, e)) {
        Rd f(e.body, e.size);
        Ref ref;
        ref.type = e.type;
        ref.from = (uint32_t)f.u(ver == 0 ? 2 : 4);
        const int cnt = (int)f.u(2);
        for (int i = 0; i < cnt; i++) ref.to.push_back((uint32_t)f.u(ver == 0 ? 2 : 4));
        if (!f.ok) { err = {HM_ERR_BITSTREAM, "truncated iref box"}; return false; }
        refs_.push_back(ref);
      }
    }
    else if (b.type == "iprp") { iprp = b.body; iprp_n = b.size; }
    else if (b.type == "idat") idat_.assign(b.body, b.body + b.size);
  }
  if (iprp && !parse_iprp(iprp, iprp_n, err)) return false;
  return true;
}

bool HeifFile::parse_iprp(const uint8_t* p, size_t n, HeifError& err)
{
  Rd r(p, n);
  Box b;
  std::vector<Box> props;
  std::vector<Box> ipmas;
  while (next_box(r, b)) {
    if (b.type == "ipco") {
      Rd q(b.body, b.size);
      Box e;
      while (next_box(q, e)) props.push_back(e);
    }
    else if (b.type == "ipma") ipmas.push_back(b);
  }
  for (const Box& m : ipmas) {
    Rd q(m.body, m.size);
    const int ver = (int)q.u(1);
    const uint32_t flags = (uint32_t)q.u(3);
    const uint32_t cnt = (uint32_t)q.u(4);
    for (uint32_t i = 0; i < cnt && q.ok; i++) {
      const uint32_t id = (uint32_t)q.u(ver < 1 ? 2 : 4);
      const int na = (int)q.u(1);
      for (int k = 0; k < na && q.ok; k++) {
        uint32_t idx;
        if (flags & 1) idx = (uint32_t)q.u(2) & 0x7FFF;
        else idx = (uint32_t)q.u(1) & 0x7F;
        if (idx == 0 || idx > props.size()) continue;
        auto f = items_.find(id);
        if (f == items_.end()) continue;
        ItemProps& ip = f->second.props;
        const Box& pb = props[idx - 1];
        Rd d(pb.body, pb.size);
        if (pb.type == "ispe") { d.skip(4); ip.ispe_width = (int)d.u(4); ip.ispe_height = (int)d.u(4); }
        else if (pb.type == "colr") {
          const std::string ct = d.fourcc();
          if (ct == "nclx") {
            ip.colr.present = true;
            ip.colr.primaries = (int)d.u(2);
            ip.colr.transfer = (int)d.u(2);
            ip.colr.matrix = (int)d.u(2);
            ip.colr.full_range = (int)(d.u(1) >> 7);
          }
          else if (ct == "prof" || ct == "rICC") { // the rest of the box is the profile
            ip.icc_type = ((uint32_t)(uint8_t)ct[0] << 24) | ((uint32_t)(uint8_t)ct[1] << 16) | ((uint32_t)(uint8_t)ct[2] << 8) | (uint8_t)ct[3];
            ip.icc.assign(pb.body + d.pos, pb.body + pb.size);
          }
        }
        else if (pb.type == "irot") {
          ip.has_irot = true;
          ip.irot_angle = (int)(d.u(1) & 3);
          Transform t; t.kind = Transform::Rotate; t.angle = ip.irot_angle * 90;
          ip.transforms.push_back(t);
        }
        else if (pb.type == "imir") {
          ip.has_imir = true;
          Transform t; t.kind = Transform::Mirror; t.horizontal = (int)(d.u(1) & 1);
          ip.transforms.push_back(t);
        }
        else if (pb.type == "clap") {
          ip.has_clap = true;
          Transform t; t.kind = Transform::CleanAperture;
          t.width_n = (uint32_t)d.u(4); t.width_d = (uint32_t)d.u(4);
          t.height_n = (uint32_t)d.u(4); t.height_d = (uint32_t)d.u(4);
          t.hoff_n = (int32_t)(uint32_t)d.u(4); t.hoff_d = (uint32_t)d.u(4);
          t.voff_n = (int32_t)(uint32_t)d.u(4); t.voff_d = (uint32_t)d.u(4);
          ip.transforms.push_back(t);
        }
        else if (pb.type == "auxC") { d.skip(4); ip.aux_type = d.cstr(); }
        else if (pb.type == "clli") { ip.has_clli = true; for (int i = 0; i < 2; i++) ip.clli[i] = (uint16_t)d.u(2); }
        else if (pb.type == "mdcv") {
          ip.has_mdcv = true;
          for (int i = 0; i < 8; i++) ip.mdcv_xy[i] = (uint16_t)d.u(2);
          for (int i = 0; i < 2; i++) ip.mdcv_lum[i] = (uint32_t)d.u(4);
        }
        else if (pb.type == "cmpd") {
          UncC& u = ip.uncc;
          u.has_cmpd = true;
          u.cmpd_types.clear();
          const uint32_t cnt = (uint32_t)d.u(4);
          for (uint32_t c = 0; c < cnt && d.ok && d.left(); c++) {
            const uint16_t type = (uint16_t)d.u(2);
            if (type >= 0x8000) d.cstr(); // component_type_uri
            u.cmpd_types.push_back(type);
          }
        }
        else if (pb.type == "uncC") {
          UncC& u = ip.uncc;
          u.present = true;
          u.components.clear();
          u.version = (int)d.u(1); d.skip(3);
          u.profile = (uint32_t)d.u(4);
          if (u.version == 0) {
            const uint32_t cnt = (uint32_t)d.u(4);
            for (uint32_t c = 0; c < cnt && d.ok && d.left(); c++) {
              UncC::Component k;
              k.index = (uint16_t)d.u(2);
              k.depth = (uint16_t)(d.u(1) + 1);
              k.format = (uint8_t)d.u(1);
              k.align_size = (uint8_t)d.u(1);
              u.components.push_back(k);
            }
            u.sampling = (int)d.u(1);
            u.interleave = (int)d.u(1);
            u.block_size = (int)d.u(1);
            u.flags = (int)d.u(1);
            u.pixel_size = (uint32_t)d.u(4);
            u.row_align = (uint32_t)d.u(4);
            u.tile_align = (uint32_t)d.u(4);
            u.tile_cols = d.u(4) + 1;
            u.tile_rows = d.u(4) + 1;
          }
        }
        else if (pb.type == "cmpC" || pb.type == "icbr") ip.uncc.generic_compression = true;
        else if (pb.type == "mskC") { // (a box too short to hold its byte is no mskC: the item stays what it was without one)
          if (pb.size >= 5) { ip.has_mskc = true; ip.mskc_bits = pb.body[4]; }
        }
        else if (pb.type == "hvcC") {
          HvcC& h = ip.hvcc;
          h.present = true;
          h.nals.clear();
          d.skip(1 + 1 + 4 + 6 + 1); // version, profile byte, compat flags, constraint flags, level
          d.skip(2 + 1);             // min_spatial_segmentation, parallelismType
          h.chroma_format = (int)(d.u(1) & 3);
          h.bit_depth_luma = (int)(d.u(1) & 7) + 8;
          h.bit_depth_chroma = (int)(d.u(1) & 7) + 8;
          d.skip(2); // avgFrameRate
          h.length_size = (int)(d.u(1) & 3) + 1;
          const int arrays = (int)d.u(1);
          for (int a = 0; a < arrays && d.ok; a++) {
            d.skip(1);
            const int nn = (int)d.u(2);
            for (int j = 0; j < nn && d.ok; j++) {
              const size_t len = (size_t)d.u(2);
              if (d.left() < len) { d.ok = false; break; }
              h.nals.emplace_back(d.p + d.pos, d.p + d.pos + len);
              d.pos += len;
            }
          }
        }
        if (!d.ok) { err = {HM_ERR_BITSTREAM, "truncated property box '" + pb.type + "'"}; return false; }
      }
    }
  }
  return true;
}

bool HeifFile::item_data(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const
{
  const Item* it = item(id);
  if (!it) { err = {HM_ERR_INVALID_ARG, "no such item"}; return false; }
  out.clear();
  for (const Extent& e : it->extents) {
    const uint64_t off = it->base_offset + e.offset;
    const uint8_t* src;
    size_t avail;
    if (it->construction_method == 1) { src = idat_.data(); avail = idat_.size(); }
    else if (it->construction_method == 0) { src = data_; avail = size_; }
    else { err = {HM_ERR_UNSUPPORTED, "iloc construction method 2"}; return false; }
    uint64_t len = e.length;
    if (len == 0 && off <= avail) len = avail - off; // "until end of file"
    if (off > avail || len > avail - off) { err = {HM_ERR_BITSTREAM, "item extent outside the file"}; return false; }
    out.insert(out.end(), src + off, src + off + len);
  }
  return true;
}

bool HeifFile::hevc_data(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const
{
  if (movie_mode_) return movie_sample(id, out, err);
  const Item* it = item(id);
  if (!it || it->type != "hvc1") { err = {HM_ERR_INVALID_ARG, "item is not an hvc1 image"}; return false; }
  if (!it->props.hvcc.present) { err = {HM_ERR_BITSTREAM, "hvc1 item without hvcC property"}; return false; }
  out.clear();
  for (const auto& nal : it->props.hvcc.nals) {
    const uint32_t n = (uint32_t)nal.size();
    out.push_back((uint8_t)(n >> 24)); out.push_back((uint8_t)(n >> 16)); out.push_back((uint8_t)(n >> 8)); out.push_back((uint8_t)n);
    out.insert(out.end(), nal.begin(), nal.end());
  }
  std::vector<uint8_t> payload;
  if (!item_data(id, payload, err)) return false;
  const int ls = it->props.hvcc.length_size;
  if (ls == 4) out.insert(out.end(), payload.begin(), payload.end());
  else { // re-frame to 4-byte lengths
    size_t p = 0;
    while (p + ls <= payload.size()) {
      uint32_t n = 0;
      for (int i = 0; i < ls; i++) n = (n << 8) | payload[p++];
      if (n > payload.size() - p) { err = {HM_ERR_BITSTREAM, "NAL length exceeds item data"}; return false; }
      out.push_back((uint8_t)(n >> 24)); out.push_back((uint8_t)(n >> 16)); out.push_back((uint8_t)(n >> 8)); out.push_back((uint8_t)n);
      out.insert(out.end(), payload.begin() + p, payload.begin() + p + n);
      p += n;
    }
  }
  return true;
}

bool HeifFile::grid_info(uint32_t id, GridInfo& g, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || it->type != "grid") { err = {HM_ERR_INVALID_ARG, "item is not a grid"}; return false; }
  std::vector<uint8_t> d;
  if (!item_data(id, d, err)) return false;
  if (d.size() < 8) { err = {HM_ERR_BITSTREAM, "grid descriptor too small"}; return false; } // context.cc:174-178
  if (d[0] != 0) { err = {HM_ERR_UNSUPPORTED, "Grid image version " + std::to_string((int)d[0]) + " is not supported"}; return false; } // :180-187
  const int field = (d[1] & 1) ? 4 : 2;
  if (d.size() < (size_t)(4 + 2 * field)) { err = {HM_ERR_BITSTREAM, "grid descriptor too small"}; return false; }
  g.rows = d[2] + 1;
  g.cols = d[3] + 1;
  auto rd = [&](size_t o) { uint32_t v = 0; for (int i = 0; i < field; i++) v = (v << 8) | d[o + i]; return v; };
  g.width = rd(4);
  g.height = rd(4 + field);
  g.tiles = references(id, "dimg");
  if ((int)g.tiles.size() != g.rows * g.cols) { err = {HM_ERR_BITSTREAM, "grid: number of dimg references != rows*cols"}; return false; }
  return true;
}

bool HeifFile::overlay_info(uint32_t id, OverlayInfo& o, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || it->type != "iovl") { err = {HM_ERR_INVALID_ARG, "item is not an overlay"}; return false; }
  std::vector<uint8_t> d;
  if (!item_data(id, d, err)) return false;
  o.children = references(id, "dimg");
  OverlayPayload p;
  std::string msg;
  const int rc = parse_overlay_payload(d.data(), d.size(), o.children.size(), p, msg);
  if (rc) { err = {rc == 2 ? HM_ERR_UNSUPPORTED : HM_ERR_BITSTREAM, msg, rc == 2 ? HM_DETAIL_UNSUPPORTED_DATA_VERSION : HM_DETAIL_INVALID_OVERLAY_DATA}; return false; }
  if (p.dx.size() != o.children.size()) { err = {HM_ERR_BITSTREAM, "Number of image offsets does not match the number of image references", HM_DETAIL_INVALID_OVERLAY_DATA}; return false; } // context.cc:2612-2616
  o.width = p.width; o.height = p.height;
  for (int i = 0; i < 4; i++) o.background[i] = p.background[i];
  o.dx = p.dx; o.dy = p.dy;
  return true;
}

uint32_t HeifFile::derived_child(uint32_t id, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || it->type != "iden") { err = {HM_ERR_INVALID_ARG, "item is not an identity derivation"}; return 0; }
  const std::vector<uint32_t> r = references(id, "dimg");
  if (r.size() != 1) { err = {HM_ERR_BITSTREAM, "'iden' image with more than one reference image"}; return 0; } // context.cc:2558-2562 (also: none)
  if (r[0] == id) { err = {HM_ERR_BITSTREAM, "'iden' image referring to itself"}; return 0; }
  return r[0];
}

bool HeifFile::gain_map_info(uint32_t id, GainMapInfo& g, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || it->type != "tmap") { err = {HM_ERR_INVALID_ARG, "item is not a 'tmap' item"}; return false; }
  const std::vector<uint32_t> r = references(id, "dimg");
  if (r.size() != 2) { err = {HM_ERR_BITSTREAM, "'tmap' item with " + std::to_string(r.size()) + " 'dimg' references, not 2 (base image, gain map)"}; return false; }
  if (r[0] == id || r[1] == id || r[0] == r[1]) { err = {HM_ERR_BITSTREAM, "'tmap' item whose references are not two other items"}; return false; }
  for (uint32_t to : r)
    if (!item(to)) { err = {HM_ERR_BITSTREAM, "'tmap' item references the missing item " + std::to_string(to)}; return false; }
  g = GainMapInfo();
  g.base = r[0]; g.map = r[1];
  std::vector<uint8_t> d;
  if (!item_data(id, d, err)) return false;
  Rd rd(d.data(), d.size());
  const unsigned version = (unsigned)rd.u(1);
  if (rd.ok && version != 0) { err = {HM_ERR_UNSUPPORTED, "'tmap' version " + std::to_string(version) + " is not supported"}; return false; }
  const unsigned minimum = (unsigned)rd.u(2);
  if (rd.ok && minimum != 0) { err = {HM_ERR_UNSUPPORTED, "'tmap' minimum_version " + std::to_string(minimum) + " is not supported"}; return false; }
  g.writer_version = (int)rd.u(2);
  const unsigned flags = (unsigned)rd.u(1);
  g.multichannel = (flags & 0x80) != 0;
  g.use_base_colour_space = (flags & 0x40) != 0;
  bool zero_den = false;
  auto fraction = [&](bool is_signed) {
    const uint32_t n = (uint32_t)rd.u(4), den = (uint32_t)rd.u(4);
    if (den == 0) { zero_den = true; return 0.0; }
    return (is_signed ? (double)(int32_t)n : (double)n) / (double)den;
  };
  g.base_headroom = fraction(false);
  g.alternate_headroom = fraction(false);
  const int channels = g.multichannel ? 3 : 1;
  for (int c = 0; c < channels; c++) {
    g.map_min[c] = fraction(true);
    g.map_max[c] = fraction(true);
    g.gamma[c] = fraction(false);
    g.base_offset[c] = fraction(true);
    g.alternate_offset[c] = fraction(true);
  }
  if (!rd.ok) { err = {HM_ERR_BITSTREAM, "'tmap' payload of " + std::to_string(d.size()) + " bytes is truncated"}; return false; }
  if (zero_den) { err = {HM_ERR_BITSTREAM, "'tmap' payload with a zero denominator"}; return false; }
  for (int c = 0; c < channels; c++)
    if (g.gamma[c] == 0.0) { err = {HM_ERR_BITSTREAM, "'tmap' payload with a zero gamma"}; return false; }
  for (int c = channels; c < 3; c++) {
    g.map_min[c] = g.map_min[0]; g.map_max[c] = g.map_max[0]; g.gamma[c] = g.gamma[0];
    g.base_offset[c] = g.base_offset[0]; g.alternate_offset[c] = g.alternate_offset[0];
  }
  return true;
}

// uncompressed_image_type_is_supported + get_heif_chroma_uncompressed (codecs/uncompressed_image.cc:40-317), with the depths the
// device unpack takes (1..16) instead of the reference's 8 and 16
bool HeifFile::unci_info(uint32_t id, hm_unci_info& info, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || !it->is_raw_leaf()) { err = {HM_ERR_INVALID_ARG, "item is not an 'unci' image"}; return false; }
  const UncC& u = it->props.uncc;
  auto unsupported = [&](const std::string& m) { err = {HM_ERR_UNSUPPORTED, m}; return false; };
  std::memset(&info, 0, sizeof(info));
  if (it->is_mask()) { // the payload's bytes, row after row, tight (MaskImageCodec::decode_mask_image): one 8-bit monochrome component
    if (it->props.ispe_width <= 0 || it->props.ispe_height <= 0) { err = {HM_ERR_BITSTREAM, "Missing required ispe box for mask codec"}; return false; }
    if (it->props.mskc_bits != 8) return unsupported("mski: bits_per_pixel " + std::to_string(it->props.mskc_bits) + " is not supported (8 is)");
    info.width = it->props.ispe_width; info.height = it->props.ispe_height;
    info.colour_space = HM_UNCI_MONO; info.n_components = 1;
    info.comp[0] = {HM_UNCI_TYPE_MONO, 8, 0};
    info.sampling = HM_UNCI_SAMPLING_NONE; info.interleave = HM_UNCI_INTERLEAVE_COMPONENT;
    info.tile_cols = info.tile_rows = 1; info.tile_width = (uint32_t)info.width; info.tile_height = (uint32_t)info.height;
    hm_unci_layout L;
    const int rc = hm_unci_layout_compute(&info, &L);
    if (rc) { err = {rc, hm_last_error()}; return false; }
    info.payload_bytes = L.total_bytes;
    return true;
  }
  if (it->props.ispe_width <= 0 || it->props.ispe_height <= 0) { err = {HM_ERR_BITSTREAM, "Missing required ispe box for uncompressed codec"}; return false; }
  if (!u.present) { err = {HM_ERR_BITSTREAM, "Missing required uncC box for uncompressed codec"}; return false; }
  if (u.generic_compression) return unsupported("unci: generic compression ('cmpC' / 'icbr') is not supported");
  if (u.version > 1) return unsupported("uncC version " + std::to_string(u.version) + " is not supported");
  info.width = it->props.ispe_width; info.height = it->props.ispe_height;
  if (u.version == 1) { // a profile stands for the whole description
    static const struct { const char* name; int n; uint16_t types[4]; } profiles[] = {
      {"rgb3", 3, {HM_UNCI_TYPE_R, HM_UNCI_TYPE_G, HM_UNCI_TYPE_B, 0}},
      {"rgba", 4, {HM_UNCI_TYPE_R, HM_UNCI_TYPE_G, HM_UNCI_TYPE_B, HM_UNCI_TYPE_ALPHA}},
      {"abgr", 4, {HM_UNCI_TYPE_ALPHA, HM_UNCI_TYPE_B, HM_UNCI_TYPE_G, HM_UNCI_TYPE_R}}};
    const char fcc[4] = {(char)(u.profile >> 24), (char)(u.profile >> 16), (char)(u.profile >> 8), (char)u.profile};
    bool found = false;
    for (const auto& p : profiles) {
      if (std::memcmp(fcc, p.name, 4)) continue;
      found = true;
      info.n_components = p.n;
      for (int c = 0; c < p.n; c++) info.comp[c] = {p.types[c], 8, 0};
    }
    if (!found) return unsupported("uncC version 1 with the profile '" + std::string(fcc, 4) + "' (rgb3, rgba and abgr are supported)");
    info.sampling = HM_UNCI_SAMPLING_NONE; info.interleave = HM_UNCI_INTERLEAVE_PIXEL;
    info.tile_cols = info.tile_rows = 1;
  }
  else {
    if (!u.has_cmpd) { err = {HM_ERR_BITSTREAM, "Missing required cmpd or uncC version 1 box for uncompressed codec"}; return false; }
    if (u.components.empty() || u.components.size() > HM_UNCI_MAX_COMPONENTS)
      return unsupported("unci: " + std::to_string(u.components.size()) + " components (1.." + std::to_string((int)HM_UNCI_MAX_COMPONENTS) + " are supported)");
    info.n_components = (int)u.components.size();
    for (int c = 0; c < info.n_components; c++) {
      const UncC::Component& k = u.components[c];
      if (k.index >= u.cmpd_types.size()) { err = {HM_ERR_BITSTREAM, "unci: component index " + std::to_string(k.index) + " outside the cmpd box"}; return false; }
      const uint16_t type = u.cmpd_types[k.index];
      if (type > 7 && type != HM_UNCI_TYPE_PADDED) return unsupported("Uncompressed image with component_type " + std::to_string(type) + " is not implemented yet");
      if (k.format != 0) return unsupported("Uncompressed image with component_format " + std::to_string(k.format) + " is not implemented yet");
      if (k.depth > 16) return unsupported("Uncompressed image with component_bit_depth " + std::to_string(k.depth) + " is not supported (1..16 are)");
      info.comp[c] = {type, (uint8_t)k.depth, k.align_size};
    }
    if (u.block_size != 0) return unsupported("Uncompressed block_size of " + std::to_string(u.block_size) + " is not implemented yet");
    if (u.flags & 0x80) return unsupported("Uncompressed components_little_endian == 1 is not implemented yet");
    if (u.flags & 0x40) return unsupported("Uncompressed block_pad_lsb == 1 is not implemented yet");
    if (u.flags & 0x20) return unsupported("Uncompressed block_little_endian == 1 is not implemented yet");
    if (u.flags & 0x10) return unsupported("Uncompressed block_reversed == 1 is not implemented yet");
    if (u.sampling > HM_UNCI_SAMPLING_420) return unsupported("Uncompressed sampling_type of " + std::to_string(u.sampling) + " is not implemented yet");
    if (u.interleave > HM_UNCI_INTERLEAVE_TILE_COMPONENT) return unsupported("Uncompressed interleave_type of " + std::to_string(u.interleave) + " is not implemented yet");
    info.sampling = u.sampling; info.interleave = u.interleave;
    info.pixel_size = u.pixel_size; info.row_align = u.row_align; info.tile_align = u.tile_align;
    if (u.tile_cols > (uint64_t)info.width || u.tile_rows > (uint64_t)info.height) return unsupported("unci: more tiles than pixels");
    info.tile_cols = (uint32_t)u.tile_cols; info.tile_rows = (uint32_t)u.tile_rows;
  }
  if (info.width % info.tile_cols || info.height % info.tile_rows)
    return unsupported("unci: image size " + std::to_string(info.width) + " x " + std::to_string(info.height) + " is not divisible by the tile counts " +
                       std::to_string(info.tile_cols) + " x " + std::to_string(info.tile_rows));
  info.tile_width = info.width / info.tile_cols; info.tile_height = info.height / info.tile_rows;
  // the colour space from the set of component types, padded ones aside; a type twice has no plane of its own
  unsigned set = 0;
  for (int c = 0; c < info.n_components; c++) {
    const int t = info.comp[c].type;
    if (t == HM_UNCI_TYPE_PADDED) continue;
    if (set & (1u << t)) return unsupported("unci: component type " + std::to_string(t) + " appears twice");
    set |= 1u << t;
  }
  const unsigned colour = set & ~(1u << HM_UNCI_TYPE_ALPHA);
  if (colour == (1u << HM_UNCI_TYPE_MONO)) info.colour_space = HM_UNCI_MONO;
  else if (colour == ((1u << HM_UNCI_TYPE_Y) | (1u << HM_UNCI_TYPE_CB) | (1u << HM_UNCI_TYPE_CR))) info.colour_space = HM_UNCI_YCBCR;
  else if (colour == ((1u << HM_UNCI_TYPE_R) | (1u << HM_UNCI_TYPE_G) | (1u << HM_UNCI_TYPE_B))) info.colour_space = HM_UNCI_RGB;
  else return unsupported("unci: could not determine chroma (the components are neither mono, Y Cb Cr nor R G B)");
  hm_unci_layout L;
  const int rc = hm_unci_layout_compute(&info, &L);
  if (rc) { err = {rc, hm_last_error()}; return false; }
  info.payload_bytes = L.total_bytes;
  return true;
}

// ---- region items ------------------------------------------------------------------------------------------------------------------
// RegionItem::parse (region.cc:30-116) with the departures include/heif_mi355x.h states: an unknown geometry type is refused (the
// reference goes on without skipping the region's bytes), an inline mask holds (w * h + 7) / 8 bytes and the regions behind it start
// behind those bytes (the reference takes w * h / 8 and does not step over them), and the magnitude limits.
void HeifFile::parse_region_item(uint32_t id, RegionItem& r) const
{
  r = RegionItem();
  std::vector<uint8_t> d;
  if (!item_data(id, d, r.err)) return;
  auto fail = [&](int status, const std::string& m) { r.err = {status, "region item " + std::to_string(id) + ": " + m}; r.regions.clear(); };
  if (d.size() < 8) return fail(HM_ERR_BITSTREAM, "Less than 8 bytes of data");
  Rd q(d.data(), d.size());
  q.skip(1); // version: unused
  const int fb = (q.u(1) & 1) ? 4 : 2;
  r.field_bits = fb * 8;
  const int64_t lim = HM_REGION_COORD_LIMIT;
  bool over = false;
  auto us = [&]() { const uint64_t v = q.u(fb); if (v >= (uint64_t)lim) over = true; return (uint32_t)v; };
  auto sg = [&]() { const uint64_t v = q.u(fb); const int64_t s = fb == 4 ? (int64_t)(int32_t)(uint32_t)v : (int64_t)(int16_t)(uint16_t)v; if (s < -lim || s >= lim) over = true; return (int32_t)s; };
  r.reference_width = us(); r.reference_height = us();
  const int count = (int)q.u(1);
  if (!q.ok) return fail(HM_ERR_BITSTREAM, "Region data incomplete");
  const std::vector<uint32_t> masks = references(id, "mask");
  size_t next_mask = 0;
  for (int i = 0; i < count; i++) {
    Region g;
    g.type = (int)q.u(1);
    if (!q.ok) return fail(HM_ERR_BITSTREAM, "Region data incomplete");
    const std::string where = "region " + std::to_string(i);
    switch (g.type) {
      case HM_REGION_POINT: g.x = sg(); g.y = sg(); break;
      case HM_REGION_RECTANGLE: case HM_REGION_ELLIPSE: case HM_REGION_REFERENCED_MASK: case HM_REGION_INLINE_MASK:
        g.x = sg(); g.y = sg(); g.w = us(); g.h = us(); break;
      case HM_REGION_POLYGON: case HM_REGION_POLYLINE: {
        const uint64_t n = q.u(fb);
        if (!q.ok || n * 2 * (uint64_t)fb > q.left()) return fail(HM_ERR_BITSTREAM, where + ": insufficient data remaining for the points of a polygon");
        g.points.resize((size_t)n * 2);
        for (size_t k = 0; k < g.points.size(); k++) g.points[k] = sg();
        break;
      }
      default:
        return fail(HM_ERR_UNSUPPORTED, where + " has the unknown geometry type " + std::to_string(g.type) + " (0..6 are defined)");
    }
    if (!q.ok) return fail(HM_ERR_BITSTREAM, where + ": insufficient data remaining for a region of type " + std::to_string(g.type));
    if (over) return fail(HM_ERR_UNSUPPORTED, where + ": a coordinate outside -2^28 <= v < 2^28 or a size of 2^28 or more (the limits of the rasteriser's exact arithmetic)");
    if (g.type == HM_REGION_ELLIPSE && (g.w > HM_REGION_MAX_RADIUS || g.h > HM_REGION_MAX_RADIUS))
      return fail(HM_ERR_UNSUPPORTED, where + ": an ellipse radius above 32767 (the limit of the rasteriser's exact arithmetic)");
    if (g.type == HM_REGION_INLINE_MASK) {
      const unsigned method = (unsigned)q.u(1);
      if (!q.ok) return fail(HM_ERR_BITSTREAM, where + ": insufficient data remaining for inline mask region");
      if (method != 0) return fail(HM_ERR_UNSUPPORTED, where + ": Deflate compressed inline mask is not yet supported (mask_coding_method " + std::to_string(method) + ")");
      const uint64_t bytes = ((uint64_t)g.w * g.h + 7) / 8;
      if (bytes > q.left()) return fail(HM_ERR_BITSTREAM, where + ": insufficient data remaining for inline mask region data[]");
      g.bits.assign(q.p + q.pos, q.p + q.pos + bytes);
      q.skip((size_t)bytes);
    }
    if (g.type == HM_REGION_REFERENCED_MASK) {
      if (next_mask >= masks.size()) return fail(HM_ERR_BITSTREAM, where + " is referenced mask " + std::to_string(next_mask) + ", the 'mask' reference has " + std::to_string(masks.size()) + " entries");
      g.mask_item = masks[next_mask++];
      const Item* m = item(g.mask_item);
      if (!m || !m->is_mask()) return fail(HM_ERR_UNSUPPORTED, where + ": the 'mask' reference names item " + std::to_string(g.mask_item) + ", which is not a mask image ('mski' with mskC)");
      const uint32_t mw = (uint32_t)std::max(0, m->props.ispe_width), mh = (uint32_t)std::max(0, m->props.ispe_height);
      if (!g.w) g.w = mw;
      if (!g.h) g.h = mh;
      if (g.w != mw || g.h != mh)
        return fail(HM_ERR_UNSUPPORTED, where + ": a referenced mask of " + std::to_string(g.w) + " x " + std::to_string(g.h) + " on a mask item of " + std::to_string(mw) + " x " + std::to_string(mh) + " (masks are not scaled)");
      if (mw >= (uint64_t)lim || mh >= (uint64_t)lim) return fail(HM_ERR_UNSUPPORTED, where + ": a mask size of 2^28 or more");
    }
    r.regions.push_back(std::move(g));
  }
}

const RegionItem* HeifFile::region_item(uint32_t id, HeifError& err) const
{
  auto it = regions_.find(id);
  if (it == regions_.end()) { err = {HM_ERR_INVALID_ARG, "item " + std::to_string(id) + " is not a region item ('rgan')"}; return nullptr; }
  if (it->second.err.status) { err = it->second.err; return nullptr; }
  return &it->second;
}

std::vector<uint32_t> HeifFile::region_items_of(uint32_t image) const
{
  std::vector<uint32_t> out;
  for (const auto& kv : regions_) // (item-id order)
    for (const Ref& r : refs_) {
      if (r.type != "cdsc" || r.from != kv.first) continue;
      bool names = false;
      for (uint32_t t : r.to) names |= t == image;
      if (names) { out.push_back(kv.first); break; }
    }
  return out;
}

bool HeifFile::item_span(uint32_t id, const uint8_t** p, size_t* n, HeifError& err) const
{
  const Item* it = item(id);
  if (!it || it->extents.size() != 1 || it->construction_method > 1) { err = {HM_ERR_UNSUPPORTED, "item data in several extents"}; return false; }
  const uint8_t* src = it->construction_method == 1 ? idat_.data() : data_;
  const size_t avail = it->construction_method == 1 ? idat_.size() : size_;
  const uint64_t off = it->base_offset + it->extents[0].offset;
  uint64_t len = it->extents[0].length;
  if (len == 0 && off <= avail) len = avail - off;
  if (off > avail || len > avail - off) { err = {HM_ERR_BITSTREAM, "item extent outside the file"}; return false; }
  *p = src + off; *n = (size_t)len;
  return true;
}

uint32_t HeifFile::gain_map_of(uint32_t base) const
{
  if (movie_mode_) return 0;
  for (const auto& kv : items_) {
    if (kv.second.type != "tmap") continue;
    const std::vector<uint32_t> r = references(kv.first, "dimg");
    if (!r.empty() && r[0] == base) return kv.first;
  }
  return 0;
}

// ---- the fork's movie mode ---------------------------------------------------------------------------------------
// The box layouts below are the fork's parsers (box.cc), which differ from ISO/IEC 14496-12 where noted.  The fork also
// insists on a 'meta' box beside 'moov' (file.cc:486-553) that it then does not use; a movie file without one is read here.

namespace {

// the first child box of the given type inside a container body (Box::get_child_box)
bool child(const uint8_t* p, size_t n, const char* type, Box& out)
{
  Rd r(p, n);
  Box b;
  while (next_box(r, b))
    if (b.type == type) { out = b; return true; }
  return false;
}

} // namespace

bool HeifFile::parse_moov(const uint8_t* p, size_t n, HeifError& err)
{
  Movie& M = movie_;
  auto missing = [&](const char* t) { err = {HM_ERR_BITSTREAM, std::string("movie: no '") + t + "' box"}; return false; };
  auto truncated = [&](const char* t) { err = {HM_ERR_BITSTREAM, std::string("movie: truncated '") + t + "' box"}; return false; };
  // every box the fork requires of a movie track (file.cc:557-627), found the way it finds them: first child of its type
  Box mvhd, trak, tkhd, mdia, mdhd, minf, vmhd, stbl, stsd, hvc1, hvcc, stsz, stts, stsc, stco, stss, ccst;
  if (!child(p, n, "mvhd", mvhd)) return missing("mvhd");
  if (!child(p, n, "trak", trak)) return missing("trak");
  if (!child(trak.body, trak.size, "tkhd", tkhd)) return missing("tkhd");
  if (!child(trak.body, trak.size, "mdia", mdia)) return missing("mdia");
  if (!child(mdia.body, mdia.size, "mdhd", mdhd)) return missing("mdhd");
  if (!child(mdia.body, mdia.size, "minf", minf)) return missing("minf");
  if (!child(minf.body, minf.size, "vmhd", vmhd)) return missing("vmhd");
  if (!child(minf.body, minf.size, "stbl", stbl)) return missing("stbl");
  if (!child(stbl.body, stbl.size, "stsd", stsd)) return missing("stsd");
  if (stsd.size < 8) return truncated("stsd");
  if (!child(stsd.body + 8, stsd.size - 8, "hvc1", hvc1)) return missing("hvc1"); // (FullBox header + entry_count, box.cc:1562-1567)

  { // mvhd (box.cc:1214-1249): version 1 has 64-bit times and duration
    Rd d(mvhd.body, mvhd.size);
    const int ver = (int)d.u(1); d.skip(3);
    if (ver == 1) { d.skip(8 + 8 + 4); M.duration = d.u(8); }
    else { d.skip(4 + 4 + 4); M.duration = d.u(4); }
    d.skip(4 + 2 + 2 + 8 + 36 + 24 + 4);
    if (!d.ok) return truncated("mvhd");
  }
  { // tkhd (box.cc:1324-1362): width and height are 16.16 fixed point
    Rd d(tkhd.body, tkhd.size);
    const int ver = (int)d.u(1); d.skip(3);
    d.skip(ver == 1 ? 8 + 8 + 4 + 4 + 8 : 4 + 4 + 4 + 4 + 4);
    d.skip(8 + 2 + 2 + 2 + 2 + 36);
    const uint32_t w = (uint32_t)d.u(4), h = (uint32_t)d.u(4);
    if (!d.ok) return truncated("tkhd");
    M.width = w >> 16; M.height = h >> 16;
  }
  const uint8_t* hvc1_children = nullptr;
  size_t hvc1_children_n = 0;
  { // hvc1 sample entry (box.cc:1616-1647): the fork reads compressorname as a NUL-terminated string and then skips
    // 32 - strlen - 1 bytes - 32 bytes in all when the NUL lies within them, a failed read when it does not
    Rd d(hvc1.body, hvc1.size);
    d.skip(6 + 2 + 2 + 2 + 12 + 2 + 2 + 4 + 4 + 4 + 2);
    size_t len = 0;
    while (d.pos + len < d.n && d.p[d.pos + len]) len++;
    if (!d.ok || d.pos + len >= d.n || len > 31) return truncated("hvc1");
    d.skip(32);
    d.skip(2 + 2); // depth, pre_defined
    if (!d.ok) return truncated("hvc1");
    hvc1_children = d.p + d.pos;
    hvc1_children_n = d.left();
  }
  if (!child(hvc1_children, hvc1_children_n, "hvcC", hvcc)) return missing("hvcC");
  if (!child(hvc1_children, hvc1_children_n, "ccst", ccst)) return missing("ccst");
  if (!child(stbl.body, stbl.size, "stsz", stsz)) return missing("stsz");
  if (!child(stbl.body, stbl.size, "stts", stts)) return missing("stts");
  if (!child(stbl.body, stbl.size, "stsc", stsc)) return missing("stsc");
  if (!child(stbl.body, stbl.size, "stco", stco)) return missing("stco");
  if (!child(stbl.body, stbl.size, "stss", stss)) return missing("stss");

  Item& F = M.frame;
  F.id = 0;
  F.type = "hvc1";
  { // hvcC (codecs/hevc.cc:32-110): the arrays are kept apart - frame k takes unit k-1 of each; empty units are dropped
    HvcC& h = F.props.hvcc;
    Rd d(hvcc.body, hvcc.size);
    d.skip(1 + 1 + 4 + 6 + 1 + 2 + 1);
    h.chroma_format = (int)(d.u(1) & 3);
    h.bit_depth_luma = (int)(d.u(1) & 7) + 8;
    h.bit_depth_chroma = (int)(d.u(1) & 7) + 8;
    d.skip(2);
    h.length_size = (int)(d.u(1) & 3) + 1;
    const int arrays = (int)d.u(1);
    for (int a = 0; a < arrays && d.ok; a++) {
      d.skip(1);
      const int nn = (int)d.u(2);
      std::vector<std::vector<uint8_t>> units;
      for (int j = 0; j < nn && d.ok; j++) {
        const size_t len = (size_t)d.u(2);
        if (d.left() < len) { d.ok = false; break; }
        if (len) units.emplace_back(d.p + d.pos, d.p + d.pos + len);
        d.pos += len;
      }
      for (const auto& u : units) h.nals.push_back(u);
      M.nal_arrays.push_back(std::move(units));
    }
    if (!d.ok) return truncated("hvcC");
    h.present = true;
  }
  F.props.ispe_width = (int)M.width;
  F.props.ispe_height = (int)M.height;
  uint32_t stsz_count = 0;
  { // stsz (box.cc:1765-1781): entries only when the constant size is 0
    Rd d(stsz.body, stsz.size);
    d.skip(4);
    M.sample_size = (uint32_t)d.u(4);
    stsz_count = (uint32_t)d.u(4);
    if (!d.ok) return truncated("stsz");
    if (M.sample_size == 0) {
      if (d.left() / 4 < stsz_count) return truncated("stsz");
      M.entry_size.resize(stsz_count);
      for (uint32_t k = 0; k < stsz_count; k++) M.entry_size[k] = (uint32_t)d.u(4);
    }
  }
  { // stsc (box.cc:1894-1910): exactly one entry (context.cc:654-676); its samples_per_chunk is the frame count
    Rd d(stsc.body, stsc.size);
    d.skip(4);
    const uint32_t entries = (uint32_t)d.u(4);
    if (!d.ok || d.left() / 12 < entries) return truncated("stsc");
    if (entries != 1) { err = {HM_ERR_BITSTREAM, "'stsc' box more than one chunk"}; return false; }
    d.skip(4);
    M.frame_count = (uint32_t)d.u(4);
  }
  { // stco (box.cc:1944-1952): the fork reads the entry count and the first offset only
    Rd d(stco.body, stco.size);
    d.skip(4 + 4);
    M.chunk_offset = (uint32_t)d.u(4);
    if (!d.ok) return truncated("stco");
  }
  // The fork's stsz lookups (box.cc:1718-1744) index the entries with the sample number unchecked: a table shorter
  // than the frame count is read out of bounds there - refused here.
  if (M.sample_size == 0 && stsz_count < M.frame_count) {
    err = {HM_ERR_BITSTREAM, "movie: 'stsz' has " + std::to_string(stsz_count) + " entries for " + std::to_string(M.frame_count) + " samples"};
    return false;
  }
  if (M.frame_count == 0) { err = {HM_ERR_BITSTREAM, "no primary item"}; return false; } // (image 1 is the primary one)
  // Every sample holds at least one byte: a track of more samples than the file has bytes cannot lie inside it (and
  // would make the list of images larger than the file).
  if (M.frame_count > size_) { err = {HM_ERR_BITSTREAM, "movie: more samples than bytes in the file"}; return false; }
  if (M.sample_size == 0) {
    M.sample_start.resize(M.frame_count);
    uint64_t o = 0;
    for (uint32_t k = 0; k < M.frame_count; k++) { M.sample_start[k] = o; o += M.entry_size[k]; }
  }
  return true;
}

// what the fork hands its decoder for sample ID `id` (file.cc:1154-1244 with Box_hvcC::get_header, codecs/hevc.cc:196-224):
// unit id-1 of every hvcC NAL array (the array's last unit when it is shorter), each with a 4-byte length, then the
// sample's bytes as they are stored
bool HeifFile::movie_sample(uint32_t id, std::vector<uint8_t>& out, HeifError& err) const
{
  const Movie& M = movie_;
  if (id < 1 || id > M.frame_count) { err = {HM_ERR_INVALID_ARG, "item is not an hvc1 image"}; return false; }
  out.clear();
  for (const auto& arr : M.nal_arrays) {
    // (an empty array: the fork takes unit -1 of it - refused)
    if (arr.empty()) { err = {HM_ERR_BITSTREAM, "movie: hvcC NAL array without units"}; return false; }
    const std::vector<uint8_t>& nal = (size_t)(id - 1) < arr.size() ? arr[id - 1] : arr.back();
    const uint32_t n = (uint32_t)nal.size();
    out.push_back((uint8_t)(n >> 24)); out.push_back((uint8_t)(n >> 16)); out.push_back((uint8_t)(n >> 8)); out.push_back((uint8_t)n);
    out.insert(out.end(), nal.begin(), nal.end());
  }
  const uint32_t k = id - 1;
  const uint64_t size = M.sample_size ? M.sample_size : M.entry_size[k];
  const uint64_t start = (uint64_t)M.chunk_offset + (M.sample_size ? (uint64_t)M.sample_size * k : M.sample_start[k]);
  // (64-bit sums here; the fork's 32-bit ones could only wrap past 4 GiB)
  if (start > size_ || size > size_ - start) {
    err = {HM_ERR_BITSTREAM, "movie: sample " + std::to_string(id) + " lies outside the file (file position " + std::to_string(start) + ")"};
    return false;
  }
  out.insert(out.end(), data_ + start, data_ + start + size);
  return true;
}

} // namespace hm
