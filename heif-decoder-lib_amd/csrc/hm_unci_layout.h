// hm_unci_layout.h - the byte layout of an ISO/IEC 23001-17 uncompressed ('unci') item in closed form: host arithmetic, no device.
//
// The rules (ISO/IEC 23001-17 5.2), as tests/unci_ref.py walks them bit by bit:
//   Bit packing.          Components are packed MSB-first.
//   Component alignment.  A component with component_align_size a > 0 starts on a byte boundary and occupies a bytes; its value sits in
//                         the low bits.  a * 8 < depth: the item is refused.
//   Row alignment.        A row ends on a byte boundary.  It is then padded to a multiple of row_align_size, counted from the row's own start.
//   Tile alignment.       A tile is padded to a multiple of tile_align_size, counted from the tile's own start.
//   Pixel padding.        pixel_size, in pixel mode only, pads every pixel to that many bytes.
//   Chroma tile sizes.    Chroma components have tile width / 2 (4:2:2 and 4:2:0) and tile height / 2 (4:2:0).
//   Orders, per interleave mode:
//     0 component         tile -> component -> row
//     1 pixel             tile -> row -> pixel -> component
//     2 mixed             tile -> components in order -> row; the two chroma components are sample-interleaved at the place of whichever
//                         comes first
//     3 row               tile -> row -> component
//     4 tile-component    component -> tile -> row
//   Unused components.    Components of a type that is not mapped to a plane (padded = 12) occupy their bits like any other.
//
// The closed form.  Every row of every mode starts on a byte boundary, so the most significant bit of sample (x, y) of component c -
// tile (tx, ty) = (x / tw, y / th), (lx, ly) inside it - lies at bit
//     8 * (base + (ty * tile_cols + tx) * tile_stride + ly * row_stride)  +  (lx == 0 ? off0 : first_len + (lx - 1) * stride + off1)
// with the eleven numbers of hm_unci_comp_layout per component.  Outside pixel mode a sample occupies a slot of (a ? 8 a : depth) bits
// (a chroma pair of mixed mode: both slots), first_len = stride = the slot and off0 = off1 = the padding in front of the value.
// Pixel mode with a byte-aligned component and no pixel_size is the one case where a pixel's length depends on the bit phase it starts
// at; but BEHIND its first aligned component a pixel's bits no longer depend on that phase, so every pixel ENDS at one phase E: pixel 0
// of a row starts at phase 0, every other pixel at phase E, and two pixel walks - from phase 0 and from phase E - give first_len, off0
// and stride, off1.  No table is needed: the kernel never walks bits.
#ifndef HM_UNCI_LAYOUT_H
#define HM_UNCI_LAYOUT_H

#include <stdint.h>

#include <vector>

#include "heif_mi355x.h"

struct hm_unci_comp_layout {
  uint64_t base;        // bytes: modes 0..3 the component's offset inside a tile, mode 4 the start of the component's tiles
  uint64_t tile_stride; // bytes from a tile to the next (mode 4: of this component's tiles)
  uint64_t row_stride;  // bytes from a row of this component to its next row inside a tile
  uint32_t first_len;   // bits from the row's start to sample 1's pixel / slot
  uint32_t stride;      // bits from sample x's pixel / slot to sample x + 1's, x >= 1
  uint32_t off0, off1;  // bits from the pixel's / slot's start to the value's most significant bit, for x == 0 / x >= 1
  uint32_t tw, th;      // the tile's size in samples of this component
  uint32_t depth;
  int32_t  plane;       // the output plane (0..2 Y Cb Cr / R G B / Y, 3 alpha), -1: not mapped
};

struct hm_unci_layout {
  int32_t  n;
  uint32_t tile_cols, tile_rows;
  hm_unci_comp_layout c[HM_UNCI_MAX_COMPONENTS];
  uint64_t total_bytes; // what the payload must hold
};

// the layout of `info` (its payload_bytes is not looked at), or the refusal of it: every product in 64 bits, checked
int hm_unci_layout_compute(const hm_unci_info* info, hm_unci_layout* L);
// `info` reduced to the sub-grid tiles[4] = first tile row, row count, first tile column, column count (NULL: `info` itself)
int hm_unci_subgrid(const hm_unci_info* info, const int32_t tiles[4], hm_unci_info* sub);
// where the sub-grid's bytes lie in the whole payload: (offset, length) pairs in the order hm_unci_unpack wants them laid end
// to end (neighbouring ranges are merged); HM_OK or a negative status
int hm_unci_subgrid_ranges(const hm_unci_info* info, const int32_t tiles[4], std::vector<uint64_t>& ranges);
// the output plane of component type `type` in colour space `cs`, -1: none
int hm_unci_plane_of(int cs, int type);

static inline uint64_t hm_unci_bit_of(const hm_unci_comp_layout& c, uint32_t tile_cols, uint32_t x, uint32_t y)
{
  const uint32_t tx = x / c.tw, lx = x - tx * c.tw, ty = y / c.th, ly = y - ty * c.th;
  const uint64_t byte = c.base + ((uint64_t)ty * tile_cols + tx) * c.tile_stride + (uint64_t)ly * c.row_stride;
  return byte * 8 + (lx == 0 ? (uint64_t)c.off0 : (uint64_t)c.first_len + (uint64_t)(lx - 1) * c.stride + c.off1);
}

#endif
