"""Serial model of ISO/IEC 23001-17 5.2 for 'unci' items: one bit reader that walks the payload sample by sample, written from the
text of the rules and not from the closed form of csrc/hm_unci_layout.h.

The rules:
  Bit packing.          Components are packed MSB-first.
  Component alignment.  A component with component_align_size a > 0 starts on a byte boundary and occupies a bytes; its value sits
                        in the low bits.  a * 8 < depth: the item is refused.
  Row alignment.        A row ends on a byte boundary.  It is then padded to a multiple of row_align_size, counted from the row's
                        own start.
  Tile alignment.       A tile is padded to a multiple of tile_align_size, counted from the tile's own start.
  Pixel padding.        pixel_size, in pixel mode only, pads every pixel to that many bytes.
  Chroma tile sizes.    Chroma components have tile width / 2 (4:2:2 and 4:2:0) and tile height / 2 (4:2:0).
  Orders, per interleave mode:
    0 component         tile -> component -> row
    1 pixel             tile -> row -> pixel -> component
    2 mixed             tile -> components in order -> row; the two chroma components are sample-interleaved at the place of
                        whichever comes first
    3 row               tile -> row -> component
    4 tile-component    component -> tile -> row
  Unused components.    Components of a type that is not mapped to a plane (padded = 12) occupy their bits like any other.

A description (`desc`) is a dict: width, height, components = [(type, depth, align_size)], sampling, interleave, pixel_size,
row_align, tile_align, tile_cols, tile_rows.  describe() reads one from a file with a box walker of its own."""
import struct

import numpy as np

MONO, Y, CB, CR, R, G, B, ALPHA, PADDED = 0, 1, 2, 3, 4, 5, 6, 7, 12
COMPONENT, PIXEL, MIXED, ROW, TILE_COMPONENT = range(5)
S_NONE, S_422, S_420 = 0, 1, 2


class Reader:
    """MSB-first bit reader with the three alignment rules"""

    def __init__(self, data):
        self.data, self.pos = data, 0  # pos in bits

    def bits(self, n):
        v = 0
        for _ in range(n):
            byte = self.data[self.pos >> 3]  # (IndexError: the payload is too short)
            v = (v << 1) | ((byte >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def to_byte(self):
        self.pos = (self.pos + 7) & ~7

    def pad_from(self, start_bit, multiple):
        """pad to a multiple of `multiple` bytes counted from start_bit (a byte boundary)"""
        self.to_byte()
        if multiple:
            n = (self.pos - start_bit) // 8
            if n % multiple:
                self.pos += 8 * (multiple - n % multiple)


def _tile_size(desc, ctype):
    tw, th = desc["width"] // desc["tile_cols"], desc["height"] // desc["tile_rows"]
    if ctype in (CB, CR):
        if desc["sampling"] in (S_422, S_420):
            tw //= 2
        if desc["sampling"] == S_420:
            th //= 2
    return tw, th


def decode(desc, payload):
    """-> (planes, positions, consumed): planes[c] / positions[c] = uint16 samples / uint64 bit positions of every sample's most
    significant bit, per component in uncC order, each of its own (sub-sampled) size; consumed = bytes the walk used"""
    comps = desc["components"]
    cols, rows = desc["tile_cols"], desc["tile_rows"]
    size = [_tile_size(desc, t) for t, _, _ in comps]
    planes = [np.zeros((th * rows, tw * cols), np.uint16) for tw, th in size]
    where = [np.zeros((th * rows, tw * cols), np.uint64) for tw, th in size]
    r = Reader(payload)

    def sample(c, x, y):
        _, depth, align = comps[c]
        if align:
            assert align * 8 >= depth
            r.to_byte()
            r.bits(align * 8 - depth)
        where[c][y, x] = r.pos
        planes[c][y, x] = r.bits(depth)

    def component_row(c, ty, tx, ly):
        tw, th = size[c]
        start = r.pos
        for lx in range(tw):
            sample(c, tx * tw + lx, ty * th + ly)
        r.pad_from(start, desc["row_align"])

    mode = desc["interleave"]
    if mode == TILE_COMPONENT:
        for c in range(len(comps)):
            for ty in range(rows):
                for tx in range(cols):
                    tile = r.pos
                    for ly in range(size[c][1]):
                        component_row(c, ty, tx, ly)
                    r.pad_from(tile, desc["tile_align"])
        return planes, where, (r.pos + 7) // 8
    chroma = [c for c, (t, _, _) in enumerate(comps) if t in (CB, CR)]
    for ty in range(rows):
        for tx in range(cols):
            tile = r.pos
            if mode == COMPONENT:
                for c in range(len(comps)):
                    for ly in range(size[c][1]):
                        component_row(c, ty, tx, ly)
            elif mode == ROW:
                for ly in range(size[0][1]):
                    for c in range(len(comps)):
                        component_row(c, ty, tx, ly)
            elif mode == PIXEL:
                tw, th = size[0]
                for ly in range(th):
                    start = r.pos
                    for lx in range(tw):
                        pixel = r.pos
                        for c in range(len(comps)):
                            sample(c, tx * tw + lx, ty * th + ly)
                        if desc["pixel_size"]:
                            r.to_byte()
                            assert r.pos - pixel <= 8 * desc["pixel_size"]
                            r.pos = pixel + 8 * desc["pixel_size"]
                    r.pad_from(start, desc["row_align"])
            elif mode == MIXED:
                assert len(chroma) == 2
                for c in range(len(comps)):
                    if c == chroma[1]:
                        continue
                    tw, th = size[c]
                    for ly in range(th):
                        if c != chroma[0]:
                            component_row(c, ty, tx, ly)
                            continue
                        start = r.pos
                        for lx in range(tw):
                            sample(chroma[0], tx * tw + lx, ty * th + ly)
                            sample(chroma[1], tx * tw + lx, ty * th + ly)
                        r.pad_from(start, desc["row_align"])
            else:
                raise ValueError(mode)
            r.pad_from(tile, desc["tile_align"])
    return planes, where, (r.pos + 7) // 8


def colour_space(desc):
    types = {t for t, _, _ in desc["components"]} - {PADDED, ALPHA}
    return {frozenset({MONO}): 0, frozenset({Y, CB, CR}): 1, frozenset({R, G, B}): 2}[frozenset(types)]


def output_planes(desc, planes):
    """the model's planes as the library hands them out: [colour 0, 1, 2, alpha], None where there is none"""
    base = {0: MONO, 1: Y, 2: R}[colour_space(desc)]
    out = [None] * 4
    for c, (t, _, _) in enumerate(desc["components"]):
        if t == ALPHA:
            out[3] = planes[c]
        elif t != PADDED:
            out[t - base] = planes[c]
    return out


def interleaved(desc, planes, channels, bits):
    """R G B [A] pixels of `bits` (8 / 16) per element from the model's planes; alpha opaque where the item has none"""
    p = output_planes(desc, planes)
    h, w = p[0].shape
    dt = np.uint8 if bits == 8 else np.uint16
    out = np.zeros((h, w, channels), dt)
    for k in range(3):
        out[..., k] = p[k].astype(dt)
    if channels == 4:
        out[..., 3] = p[3].astype(dt) if p[3] is not None else (1 << bits) - 1
    return out


# ---- a box walker of its own: the primary 'unci' item's description and payload -------------------------------------------------

def _boxes(b, o, e):
    while o + 8 <= e:
        size, kind = struct.unpack(">I4s", b[o:o + 8])
        h = 8
        if size == 1:
            size, h = struct.unpack(">Q", b[o + 8:o + 16])[0], 16
        if size == 0:
            size = e - o
        yield kind, o + h, o + size
        o += size


def _find(b, o, e, kind):
    for k, s, t in _boxes(b, o, e):
        if k == kind:
            return s, t
    raise KeyError(kind)


PROFILES = {b"rgb3": [R, G, B], b"rgba": [R, G, B, ALPHA], b"abgr": [ALPHA, B, G, R]}


def describe(data):
    """(desc, payload) of the primary item of an 'unci' file (one extent, construction method 0)"""
    ms, me = _find(data, 0, len(data), b"meta")
    ms += 4
    s, _ = _find(data, ms, me, b"pitm")
    ver = data[s]
    primary = struct.unpack(">H" if ver == 0 else ">I", data[s + 4:s + (6 if ver == 0 else 8)])[0]
    # iloc: the item's one extent
    s, _ = _find(data, ms, me, b"iloc")
    ver = data[s]
    offset_size, length_size, base_size = data[s + 4] >> 4, data[s + 4] & 15, data[s + 5] >> 4
    index_size = data[s + 5] & 15 if ver in (1, 2) else 0
    o = s + 6

    def u(n):
        nonlocal o
        v = int.from_bytes(data[o:o + n], "big")
        o += n
        return v

    payload = None
    for _ in range(u(2 if ver < 2 else 4)):
        iid = u(2 if ver < 2 else 4)
        method = u(2) & 15 if ver in (1, 2) else 0
        u(2)
        base = u(base_size)
        extents = [(u(index_size), u(offset_size), u(length_size)) for _ in range(u(2))]
        if iid == primary:
            assert method == 0 and len(extents) == 1
            payload = data[base + extents[0][1]:base + extents[0][1] + extents[0][2]]
    # the item's properties in association order
    ps, pe = _find(data, ms, me, b"iprp")
    cs, ce = _find(data, ps, pe, b"ipco")
    props = list(_boxes(data, cs, ce))
    s, _ = _find(data, ps, pe, b"ipma")
    ver, flags = data[s], int.from_bytes(data[s + 1:s + 4], "big")
    o = s + 4
    mine = []
    for _ in range(u(4)):
        iid = u(2 if ver < 1 else 4)
        idx = [(u(2) & 0x7FFF) if flags & 1 else (u(1) & 0x7F) for _ in range(u(1))]
        if iid == primary:
            mine = idx
    desc, types = {"pixel_size": 0, "row_align": 0, "tile_align": 0, "tile_cols": 1, "tile_rows": 1, "sampling": 0, "interleave": PIXEL}, None
    for i in mine:
        kind, s, e = props[i - 1]
        if kind == b"ispe":
            desc["width"], desc["height"] = struct.unpack(">II", data[s + 4:s + 12])
        elif kind == b"cmpd":
            n = struct.unpack(">I", data[s:s + 4])[0]
            types = list(struct.unpack(">%dH" % n, data[s + 4:s + 4 + 2 * n]))  # (no URI types in what is read here)
        elif kind == b"uncC":
            ver, profile = data[s], data[s + 4:s + 8]
            if ver == 1:
                desc["components"] = [(t, 8, 0) for t in PROFILES[profile]]
                continue
            n = struct.unpack(">I", data[s + 8:s + 12])[0]
            o = s + 12
            raw = [(u(2), u(1) + 1, u(1), u(1)) for _ in range(n)]
            desc["sampling"], desc["interleave"], desc["block_size"], desc["flags"] = u(1), u(1), u(1), u(1)
            desc["pixel_size"], desc["row_align"], desc["tile_align"] = u(4), u(4), u(4)
            desc["tile_cols"], desc["tile_rows"] = u(4) + 1, u(4) + 1
            desc["raw_components"] = raw
    if "raw_components" in desc:
        desc["components"] = [(types[i], d, a) for i, d, _, a in desc.pop("raw_components")]
    return desc, payload
