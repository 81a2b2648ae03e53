// unci_layout.cpp - see hm_unci_layout.h: the layout of an 'unci' item from its hm_unci_info, in 64-bit arithmetic with overflow checks.
#include "hm_unci_layout.h"

#include <cstring>

#include "hm_internal.h"

namespace {

// checked 64-bit arithmetic: a failed operation poisons the sum
struct Sum {
  bool ok = true;
  uint64_t mul(uint64_t a, uint64_t b) { uint64_t r = 0; if (__builtin_mul_overflow(a, b, &r)) ok = false; return r; }
  uint64_t add(uint64_t a, uint64_t b) { uint64_t r = 0; if (__builtin_add_overflow(a, b, &r)) ok = false; return r; }
  uint64_t align_up(uint64_t v, uint64_t a)
  {
    if (a == 0) return v;
    const uint64_t r = v % a;
    return r ? add(v, a - r) : v;
  }
  uint64_t bits_to_bytes(uint64_t bits) { return add(bits, 7) / 8; }
};

bool is_chroma(int type) { return type == HM_UNCI_TYPE_CB || type == HM_UNCI_TYPE_CR; }
uint32_t slot_bits(const hm_unci_component& c) { return c.align_size ? 8u * c.align_size : c.depth; }

// one pixel of pixel mode walked from bit phase `phase`: off[c] = bits from the pixel's start to component c's most significant bit;
// returns the pixel's length in bits
uint32_t walk_pixel(const hm_unci_info* I, uint32_t phase, uint32_t off[HM_UNCI_MAX_COMPONENTS])
{
  uint32_t pos = phase;
  for (int c = 0; c < I->n_components; c++) {
    const hm_unci_component& k = I->comp[c];
    if (k.align_size) { pos = (pos + 7) & ~7u; pos += 8u * k.align_size - k.depth; }
    off[c] = pos - phase;
    pos += k.depth;
  }
  return pos - phase;
}

} // namespace

int hm_unci_plane_of(int cs, int type)
{
  if (type == HM_UNCI_TYPE_ALPHA) return 3;
  if (cs == HM_UNCI_MONO) return type == HM_UNCI_TYPE_MONO ? 0 : -1;
  if (cs == HM_UNCI_YCBCR) return type >= HM_UNCI_TYPE_Y && type <= HM_UNCI_TYPE_CR ? type - HM_UNCI_TYPE_Y : -1;
  if (cs == HM_UNCI_RGB) return type >= HM_UNCI_TYPE_R && type <= HM_UNCI_TYPE_B ? type - HM_UNCI_TYPE_R : -1;
  return -1;
}

int hm_unci_layout_compute(const hm_unci_info* I, hm_unci_layout* L)
{
  if (!I || !L) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(L, 0, sizeof(*L));
  if (I->n_components < 1 || I->n_components > HM_UNCI_MAX_COMPONENTS) return hm_fail(HM_ERR_UNSUPPORTED, "unci: %d components (1..%d are supported)", I->n_components, HM_UNCI_MAX_COMPONENTS);
  if (I->tile_cols < 1 || I->tile_rows < 1 || I->tile_width < 1 || I->tile_height < 1) return hm_fail(HM_ERR_BITSTREAM, "unci: empty tile grid");
  if (I->tile_width > 0x7FFFFFFFu / I->tile_cols || I->tile_height > 0x7FFFFFFFu / I->tile_rows) return hm_fail(HM_ERR_BITSTREAM, "unci: image size overflows");
  if (I->interleave < 0 || I->interleave > HM_UNCI_INTERLEAVE_TILE_COMPONENT) return hm_fail(HM_ERR_UNSUPPORTED, "Uncompressed interleave_type of %d is not implemented yet", I->interleave);
  if (I->sampling < 0 || I->sampling > HM_UNCI_SAMPLING_420) return hm_fail(HM_ERR_UNSUPPORTED, "Uncompressed sampling_type of %d is not implemented yet", I->sampling);
  if (I->colour_space < HM_UNCI_MONO || I->colour_space > HM_UNCI_RGB) return hm_fail(HM_ERR_INVALID_ARG, "unci: colour space %d", I->colour_space);
  const bool sub = I->sampling != HM_UNCI_SAMPLING_NONE;
  if (I->interleave == HM_UNCI_INTERLEAVE_MIXED && !sub) return hm_fail(HM_ERR_UNSUPPORTED, "unci: mixed interleave mode is only valid with sub-sampling (ISO/IEC 23001-17 5.2.1.6.4)");
  if (sub && I->interleave != HM_UNCI_INTERLEAVE_COMPONENT && I->interleave != HM_UNCI_INTERLEAVE_MIXED)
    return hm_fail(HM_ERR_UNSUPPORTED, "unci: YCbCr sub-sampling is only valid with component or mixed interleave mode (ISO/IEC 23001-17 5.2.1.5.3)");
  if (sub && I->colour_space != HM_UNCI_YCBCR) return hm_fail(HM_ERR_UNSUPPORTED, "unci: sub-sampling of an item that is not YCbCr");
  if (sub && ((I->tile_width & 1) || (I->sampling == HM_UNCI_SAMPLING_420 && (I->tile_height & 1))))
    return hm_fail(HM_ERR_UNSUPPORTED, "unci: a sub-sampled item with an odd tile size %u x %u", I->tile_width, I->tile_height);
  if (I->pixel_size && I->interleave != HM_UNCI_INTERLEAVE_PIXEL)
    return hm_fail(HM_ERR_UNSUPPORTED, "Uncompressed pixel_size of %u is only valid with interleave_type 1 (ISO/IEC 23001-17 5.2.1.7)", I->pixel_size);
  int first_chroma = -1, second_chroma = -1;
  for (int c = 0; c < I->n_components; c++) {
    const hm_unci_component& k = I->comp[c];
    if (k.depth < 1 || k.depth > 16) return hm_fail(HM_ERR_UNSUPPORTED, "Uncompressed image with component_bit_depth %d is not supported (1..16 are)", k.depth);
    if (k.type > 7 && k.type != HM_UNCI_TYPE_PADDED) return hm_fail(HM_ERR_UNSUPPORTED, "Uncompressed image with component_type %d is not implemented yet", k.type);
    if (k.align_size && 8u * k.align_size < k.depth) return hm_fail(HM_ERR_UNSUPPORTED, "unci: component_align_size %d is smaller than the component's %d bits", k.align_size, k.depth);
    if (is_chroma(k.type)) { if (first_chroma < 0) first_chroma = c; else if (second_chroma < 0) second_chroma = c; }
  }
  Sum S;
  const uint64_t n_tiles = (uint64_t)I->tile_cols * I->tile_rows;
  const uint32_t tw = I->tile_width, th = I->tile_height;
  L->n = I->n_components; L->tile_cols = I->tile_cols; L->tile_rows = I->tile_rows;
  for (int c = 0; c < L->n; c++) {
    hm_unci_comp_layout& o = L->c[c];
    const hm_unci_component& k = I->comp[c];
    const bool ch = sub && is_chroma(k.type);
    o.tw = ch ? tw / 2 : tw;
    o.th = ch && I->sampling == HM_UNCI_SAMPLING_420 ? th / 2 : th;
    o.depth = k.depth;
    o.plane = hm_unci_plane_of(I->colour_space, k.type);
    o.first_len = o.stride = slot_bits(k);
    o.off0 = o.off1 = slot_bits(k) - k.depth;
  }
  // bytes of one row of component c inside a tile, modes 0, 2, 3, 4
  auto row_bytes = [&](int c, uint32_t slot) { return S.align_up(S.bits_to_bytes(S.mul(L->c[c].tw, slot)), I->row_align); };
  uint64_t tile_bytes = 0;
  switch (I->interleave) {
    case HM_UNCI_INTERLEAVE_COMPONENT:
    case HM_UNCI_INTERLEAVE_MIXED: {
      const bool mixed = I->interleave == HM_UNCI_INTERLEAVE_MIXED;
      if (mixed) {
        if (first_chroma < 0 || second_chroma < 0) return hm_fail(HM_ERR_UNSUPPORTED, "unci: mixed interleave mode without two chroma components");
        const hm_unci_component &a = I->comp[first_chroma], &b = I->comp[second_chroma];
        if ((a.align_size || b.align_size) && ((slot_bits(a) & 7) || (slot_bits(b) & 7)))
          return hm_fail(HM_ERR_UNSUPPORTED, "unci: mixed interleave mode with one chroma component byte-aligned and the other not");
      }
      uint64_t off = 0;
      for (int c = 0; c < L->n; c++) {
        hm_unci_comp_layout& o = L->c[c];
        if (mixed && c == second_chroma) { // inside the pair, behind the first one's slot
          const hm_unci_comp_layout& f = L->c[first_chroma];
          o.base = f.base; o.row_stride = f.row_stride; o.first_len = o.stride = f.stride;
          o.off0 = o.off1 = slot_bits(I->comp[first_chroma]) + slot_bits(I->comp[c]) - I->comp[c].depth;
          continue;
        }
        uint32_t slot = slot_bits(I->comp[c]);
        if (mixed && c == first_chroma) { slot += slot_bits(I->comp[second_chroma]); o.first_len = o.stride = slot; }
        o.base = off;
        o.row_stride = row_bytes(c, slot);
        off = S.add(off, S.mul(o.th, o.row_stride));
      }
      tile_bytes = S.align_up(off, I->tile_align);
      break;
    }
    case HM_UNCI_INTERLEAVE_ROW: {
      uint64_t all = 0;
      for (int c = 0; c < L->n; c++) { L->c[c].base = all; all = S.add(all, row_bytes(c, slot_bits(I->comp[c]))); }
      for (int c = 0; c < L->n; c++) L->c[c].row_stride = all;
      tile_bytes = S.align_up(S.mul(th, all), I->tile_align);
      break;
    }
    case HM_UNCI_INTERLEAVE_TILE_COMPONENT: {
      uint64_t at = 0;
      for (int c = 0; c < L->n; c++) {
        hm_unci_comp_layout& o = L->c[c];
        o.row_stride = row_bytes(c, slot_bits(I->comp[c]));
        o.tile_stride = S.align_up(S.mul(o.th, o.row_stride), I->tile_align);
        o.base = at;
        at = S.add(at, S.mul(n_tiles, o.tile_stride));
      }
      L->total_bytes = at;
      break;
    }
    case HM_UNCI_INTERLEAVE_PIXEL: {
      uint32_t off0[HM_UNCI_MAX_COMPONENTS], off1[HM_UNCI_MAX_COMPONENTS];
      uint32_t len0 = walk_pixel(I, 0, off0), len1;
      if (I->pixel_size) {
        if ((uint64_t)I->pixel_size * 8 < len0) return hm_fail(HM_ERR_UNSUPPORTED, "unci: pixel_size %u is smaller than the %u bits of a pixel", I->pixel_size, len0);
        if (I->pixel_size > 0x0FFFFFFFu) return hm_fail(HM_ERR_BITSTREAM, "unci: pixel_size %u overflows", I->pixel_size);
        len0 = len1 = 8 * I->pixel_size;
        std::memcpy(off1, off0, sizeof(off1));
      }
      else len1 = walk_pixel(I, len0 & 7, off1);
      const uint64_t row = S.align_up(S.bits_to_bytes(S.add(len0, S.mul(tw - 1, len1))), I->row_align);
      for (int c = 0; c < L->n; c++) {
        hm_unci_comp_layout& o = L->c[c];
        o.base = 0; o.row_stride = row; o.first_len = len0; o.stride = len1; o.off0 = off0[c]; o.off1 = off1[c];
      }
      tile_bytes = S.align_up(S.mul(th, row), I->tile_align);
      break;
    }
  }
  if (I->interleave != HM_UNCI_INTERLEAVE_TILE_COMPONENT) {
    for (int c = 0; c < L->n; c++) L->c[c].tile_stride = tile_bytes;
    L->total_bytes = S.mul(n_tiles, tile_bytes);
  }
  (void)S.mul(L->total_bytes, 8); // (bit positions fit 64 bits)
  if (!S.ok) return hm_fail(HM_ERR_BITSTREAM, "unci: the layout's size overflows");
  return HM_OK;
}

int hm_unci_subgrid(const hm_unci_info* info, const int32_t t[4], hm_unci_info* sub)
{
  *sub = *info;
  if (!t) return HM_OK;
  if (t[0] < 0 || t[1] < 1 || t[2] < 0 || t[3] < 1 || (uint64_t)t[0] + t[1] > info->tile_rows || (uint64_t)t[2] + t[3] > info->tile_cols)
    return hm_fail(HM_ERR_INVALID_ARG, "unci: tiles %d+%d x %d+%d outside the %u x %u grid", t[0], t[1], t[2], t[3], info->tile_rows, info->tile_cols);
  sub->tile_rows = (uint32_t)t[1]; sub->tile_cols = (uint32_t)t[3];
  sub->width = (int32_t)(sub->tile_cols * info->tile_width); sub->height = (int32_t)(sub->tile_rows * info->tile_height);
  hm_unci_layout L;
  const int rc = hm_unci_layout_compute(sub, &L);
  if (rc) return rc;
  sub->payload_bytes = L.total_bytes;
  return HM_OK;
}

int hm_unci_subgrid_ranges(const hm_unci_info* info, const int32_t tiles[4], std::vector<uint64_t>& r)
{
  r.clear();
  hm_unci_info sub;
  hm_unci_layout L;
  int rc;
  if ((rc = hm_unci_subgrid(info, tiles, &sub)) || (rc = hm_unci_layout_compute(info, &L))) return rc;
  const int32_t whole[4] = {0, (int32_t)info->tile_rows, 0, (int32_t)info->tile_cols};
  const int32_t* t = tiles ? tiles : whole;
  auto push = [&](uint64_t off, uint64_t len) {
    if (!len) return;
    if (!r.empty() && r[r.size() - 2] + r.back() == off) r.back() += len;
    else { r.push_back(off); r.push_back(len); }
  };
  const bool per_component = info->interleave == HM_UNCI_INTERLEAVE_TILE_COMPONENT;
  for (int c = 0; c < (per_component ? L.n : 1); c++)
    for (int row = t[0]; row < t[0] + t[1]; row++)
      push((per_component ? L.c[c].base : 0) + ((uint64_t)row * info->tile_cols + t[2]) * L.c[c].tile_stride, (uint64_t)t[3] * L.c[c].tile_stride);
  return HM_OK;
}

extern "C" {

int hm_unci_sample_bit(const hm_unci_info* info, int component, int x, int y, uint64_t* bit)
{
  if (!info || !bit) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_unci_layout L;
  const int rc = hm_unci_layout_compute(info, &L);
  if (rc) return rc;
  if (component < 0 || component >= L.n) return hm_fail(HM_ERR_INVALID_ARG, "unci: no component %d", component);
  const hm_unci_comp_layout& c = L.c[component];
  if (x < 0 || y < 0 || (uint64_t)x >= (uint64_t)c.tw * L.tile_cols || (uint64_t)y >= (uint64_t)c.th * L.tile_rows)
    return hm_fail(HM_ERR_INVALID_ARG, "unci: sample (%d, %d) outside component %d", x, y, component);
  *bit = hm_unci_bit_of(c, L.tile_cols, (uint32_t)x, (uint32_t)y);
  return HM_OK;
}

int hm_unci_payload_bytes(const hm_unci_info* info, uint64_t* bytes)
{
  if (!info || !bytes) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  hm_unci_layout L;
  const int rc = hm_unci_layout_compute(info, &L);
  if (rc) return rc;
  *bytes = L.total_bytes;
  return HM_OK;
}

} // extern "C"
