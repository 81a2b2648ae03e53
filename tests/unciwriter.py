"""Writes synthetic ISO/IEC 23001-17 'unci' files: a serial bit writer that packs planes by the rules of unci_ref.py (its inverse,
walk for walk), and the boxes of a one-item HEIF file around the payload."""
import struct

import numpy as np

import unci_ref as U


class Writer:
    def __init__(self):
        self.out, self.pos = bytearray(), 0

    def bits(self, v, n):
        for k in range(n - 1, -1, -1):
            if self.pos >> 3 == len(self.out):
                self.out.append(0)
            if (v >> k) & 1:
                self.out[self.pos >> 3] |= 0x80 >> (self.pos & 7)
            self.pos += 1

    def to_byte(self):
        self.pos = (self.pos + 7) & ~7
        self._grow()

    def _grow(self):
        while len(self.out) * 8 < self.pos:
            self.out.append(0)

    def pad_from(self, start_bit, multiple):
        self.to_byte()
        if multiple:
            n = (self.pos - start_bit) // 8
            if n % multiple:
                self.pos += 8 * (multiple - n % multiple)
        self._grow()


def random_planes(desc, seed):
    """one plane per component (uncC order) of random samples of the component's depth"""
    rng = np.random.default_rng(seed)
    planes = []
    for t, depth, _ in desc["components"]:
        tw, th = U._tile_size(desc, t)
        planes.append(rng.integers(0, 1 << depth, (th * desc["tile_rows"], tw * desc["tile_cols"]), dtype=np.uint32).astype(np.uint16))
    return planes


def pack(desc, planes, pad_bits=1):
    """the payload of `planes` under `desc`; pad_bits: the value of every padding bit in front of an aligned value (the unpack must
    not see them)"""
    comps = desc["components"]
    cols, rows = desc["tile_cols"], desc["tile_rows"]
    size = [U._tile_size(desc, t) for t, _, _ in comps]
    w = Writer()

    def sample(c, x, y):
        _, depth, align = comps[c]
        if align:
            w.to_byte()
            w.bits((1 << (align * 8 - depth)) - 1 if pad_bits else 0, align * 8 - depth)
        w.bits(int(planes[c][y, x]), depth)

    def component_row(c, ty, tx, ly):
        tw, th = size[c]
        start = w.pos
        for lx in range(tw):
            sample(c, tx * tw + lx, ty * th + ly)
        w.pad_from(start, desc["row_align"])

    mode = desc["interleave"]
    if mode == U.TILE_COMPONENT:
        for c in range(len(comps)):
            for ty in range(rows):
                for tx in range(cols):
                    tile = w.pos
                    for ly in range(size[c][1]):
                        component_row(c, ty, tx, ly)
                    w.pad_from(tile, desc["tile_align"])
        return bytes(w.out)
    chroma = [c for c, (t, _, _) in enumerate(comps) if t in (U.CB, U.CR)]
    for ty in range(rows):
        for tx in range(cols):
            tile = w.pos
            if mode == U.COMPONENT:
                for c in range(len(comps)):
                    for ly in range(size[c][1]):
                        component_row(c, ty, tx, ly)
            elif mode == U.ROW:
                for ly in range(size[0][1]):
                    for c in range(len(comps)):
                        component_row(c, ty, tx, ly)
            elif mode == U.PIXEL:
                tw, th = size[0]
                for ly in range(th):
                    start = w.pos
                    for lx in range(tw):
                        pixel = w.pos
                        for c in range(len(comps)):
                            sample(c, tx * tw + lx, ty * th + ly)
                        if desc["pixel_size"]:
                            w.to_byte()
                            w.pos = pixel + 8 * desc["pixel_size"]
                            w._grow()
                    w.pad_from(start, desc["row_align"])
            elif mode == U.MIXED:
                for c in range(len(comps)):
                    if c == chroma[1]:
                        continue
                    tw, th = size[c]
                    for ly in range(th):
                        if c != chroma[0]:
                            component_row(c, ty, tx, ly)
                            continue
                        start = w.pos
                        for lx in range(tw):
                            sample(chroma[0], tx * tw + lx, ty * th + ly)
                            sample(chroma[1], tx * tw + lx, ty * th + ly)
                        w.pad_from(start, desc["row_align"])
            w.pad_from(tile, desc["tile_align"])
    return bytes(w.out)


def make_desc(width, height, components, interleave=U.COMPONENT, sampling=U.S_NONE, pixel_size=0, row_align=0, tile_align=0, tile_cols=1, tile_rows=1):
    return dict(width=width, height=height, components=list(components), interleave=interleave, sampling=sampling, pixel_size=pixel_size,
                row_align=row_align, tile_align=tile_align, tile_cols=tile_cols, tile_rows=tile_rows)


def _box(kind, body):
    return struct.pack(">I4s", 8 + len(body), kind) + body


def _full(kind, version, flags, body):
    return _box(kind, struct.pack(">I", (version << 24) | flags) + body)


def uncc_box(desc, block_size=0, flags=0, formats=None, version=0, profile=b"\0\0\0\0"):
    if version == 1:
        return _full(b"uncC", 1, 0, profile)
    comps = desc["components"]
    body = profile + struct.pack(">I", len(comps))
    for i, (_, depth, align) in enumerate(comps):
        body += struct.pack(">HBBB", desc.get("indices", list(range(len(comps))))[i], depth - 1, formats[i] if formats else 0, align)
    body += struct.pack(">BBBBIIIII", desc["sampling"], desc["interleave"], block_size, flags, desc["pixel_size"], desc["row_align"], desc["tile_align"],
                        desc["tile_cols"] - 1, desc["tile_rows"] - 1)
    return _full(b"uncC", 0, 0, body)


def cmpd_box(desc):
    return _box(b"cmpd", struct.pack(">I", len(desc["components"])) + b"".join(struct.pack(">H", t) for t, _, _ in desc["components"]))


def heif_file(desc, payload, uncc=None, cmpd=True, extra_props=(), item_type=b"unci", ispe=True, extra_items=(), extra_refs=()):
    """a HEIF file whose primary item 1 is the 'unci' item: ispe, cmpd, uncC and extra_props (whole boxes) as its properties, the
    payload in an mdat.  extra_items: (id, type) of further items that share the payload and the properties; extra_refs: (type, from,
    [to]) item references"""
    props = []
    if ispe:
        props.append(_full(b"ispe", 0, 0, struct.pack(">II", desc["width"], desc["height"])))
    if cmpd:
        props.append(cmpd_box(desc))
    props.append(uncc if uncc is not None else uncc_box(desc))
    props += list(extra_props)
    items = [(1, item_type)] + list(extra_items)
    ipma = struct.pack(">I", len(items))
    for iid, _ in items:
        ipma += struct.pack(">HB", iid, len(props)) + bytes(0x80 | (i + 1) for i in range(len(props)))
    iprp = _box(b"iprp", _box(b"ipco", b"".join(props)) + _full(b"ipma", 0, 0, ipma))
    iinf = struct.pack(">H", len(items)) + b"".join(_full(b"infe", 2, 0, struct.pack(">HH4s", iid, 0, t) + b"\0") for iid, t in items)
    hdlr = _full(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"pict") + b"\0" * 13)
    pitm = _full(b"pitm", 0, 0, struct.pack(">H", 1))
    iref = b""
    if extra_refs:
        iref = _full(b"iref", 0, 0, b"".join(_box(t, struct.pack(">HH", frm, len(to)) + b"".join(struct.pack(">H", x) for x in to)) for t, frm, to in extra_refs))

    def meta(offset):
        iloc = struct.pack(">BBH", 0x44, 0x00, len(items)) + b"".join(struct.pack(">HHHII", iid, 0, 1, offset, len(payload)) for iid, _ in items)
        return _full(b"meta", 0, 0, hdlr + pitm + _full(b"iloc", 0, 0, iloc) + _full(b"iinf", 0, 0, iinf) + iref + iprp)

    ftyp = _box(b"ftyp", b"mif1" + struct.pack(">I", 0) + b"mif1heic")
    offset = len(ftyp) + len(meta(0)) + 8
    return ftyp + meta(offset) + _box(b"mdat", payload)


def cases():
    """name -> description of the synthetic cases the CPU and GPU tests share (each at most 64 K samples)"""
    M, Y, CB, CR, R, G, B, A, X = U.MONO, U.Y, U.CB, U.CR, U.R, U.G, U.B, U.ALPHA, U.PADDED
    c = {}
    c["depths_1_3_9_pixel"] = make_desc(37, 5, [(R, 1, 0), (G, 3, 0), (B, 9, 0)], U.PIXEL)
    c["depths_12_15_16_row"] = make_desc(21, 6, [(R, 12, 0), (G, 15, 0), (B, 16, 0)], U.ROW, tile_cols=3, tile_rows=2)
    c["depths_1_3_9_component"] = make_desc(37, 5, [(R, 1, 0), (G, 3, 0), (B, 9, 0)], U.COMPONENT)
    c["depths_12_15_16_tile_component"] = make_desc(22, 6, [(B, 12, 0), (R, 15, 0), (G, 16, 0), (A, 1, 0)], U.TILE_COMPONENT, tile_cols=2, tile_rows=3, tile_align=7)
    c["mono_1bit"] = make_desc(67, 3, [(M, 1, 0)], U.COMPONENT)
    c["pixel_5_16_3"] = make_desc(40, 3, [(R, 5, 0), (G, 16, 0), (B, 3, 0)], U.PIXEL)         # 16-bit samples at bit phases 5, 13, 21, 29
    c["pixel_5_16_4"] = make_desc(67, 2, [(R, 5, 0), (G, 16, 0), (B, 4, 0)], U.PIXEL)         # 25-bit pixels: every one of the 32 phases
    c["align2_depth9"] = make_desc(19, 4, [(R, 9, 2), (G, 9, 2), (B, 9, 2)], U.PIXEL)
    c["align2_depth9_component"] = make_desc(19, 4, [(Y, 9, 2), (CB, 9, 2), (CR, 9, 0)], U.COMPONENT)
    c["pixel_7_7p1_7"] = make_desc(30, 20, [(R, 7, 0), (G, 7, 1), (B, 7, 0)], U.PIXEL, tile_cols=3, tile_rows=2)  # the phase-dependent case
    c["pixel_3_5a1_2_9a2"] = make_desc(11, 3, [(A, 3, 0), (R, 5, 1), (G, 2, 0), (B, 9, 2)], U.PIXEL)
    c["pixel_size_larger"] = make_desc(12, 4, [(R, 8, 0), (G, 8, 0), (B, 8, 0)], U.PIXEL, pixel_size=7, tile_cols=2)
    c["pixel_size_bits"] = make_desc(13, 3, [(R, 5, 0), (G, 6, 0), (B, 5, 0)], U.PIXEL, pixel_size=3)
    c["row_align_30_tile_align_37"] = make_desc(20, 6, [(R, 8, 0), (G, 8, 0), (B, 8, 0)], U.COMPONENT, row_align=30, tile_align=37, tile_cols=2, tile_rows=2)
    c["row_align_30_tile_align_37_pixel"] = make_desc(20, 6, [(R, 7, 0), (G, 8, 0), (B, 8, 0)], U.PIXEL, row_align=30, tile_align=37, tile_cols=2, tile_rows=2)
    c["tiles_1x1"] = make_desc(9, 7, [(R, 8, 0), (G, 8, 0), (B, 8, 0), (A, 8, 0)], U.PIXEL, tile_cols=9, tile_rows=7)
    c["tiles_1x1_component_5bit"] = make_desc(9, 7, [(R, 5, 0), (G, 5, 0), (B, 5, 0)], U.COMPONENT, tile_cols=9, tile_rows=7)
    c["padded_3bit_pixel"] = make_desc(10, 4, [(R, 8, 0), (X, 3, 0), (G, 8, 0), (B, 8, 0)], U.PIXEL)
    c["padded_3bit_component"] = make_desc(10, 4, [(R, 8, 0), (X, 3, 0), (G, 8, 0), (B, 8, 0)], U.COMPONENT, tile_cols=2)
    for mode, name in ((U.COMPONENT, "component"), (U.MIXED, "mixed")):
        c["yuv420_2x2_" + name] = make_desc(12, 8, [(Y, 8, 0), (CB, 8, 0), (CR, 8, 0)], mode, U.S_420, tile_cols=2, tile_rows=2)
        c["yuv422_2x2_" + name] = make_desc(12, 6, [(Y, 8, 0), (CR, 8, 0), (CB, 8, 0)], mode, U.S_422, tile_cols=2, tile_rows=2)
        c["yuv420_10bit_2x2_" + name] = make_desc(20, 12, [(CB, 10, 0), (Y, 10, 0), (CR, 10, 0), (A, 10, 0)], mode, U.S_420, row_align=3, tile_cols=2, tile_rows=2)
    c["yuv444_row_8bit"] = make_desc(33, 6, [(Y, 8, 0), (CB, 8, 0), (CR, 8, 0)], U.ROW, tile_cols=3)
    c["wide_1030x3"] = make_desc(1030, 3, [(R, 8, 0), (G, 8, 0), (B, 8, 0)], U.PIXEL)
    c["tall_3x1030"] = make_desc(3, 1030, [(R, 8, 0), (G, 8, 0), (B, 8, 0)], U.COMPONENT, tile_rows=5)
    c["wide_1030x3_11bit"] = make_desc(1030, 3, [(M, 11, 0)], U.COMPONENT, tile_cols=2)
    c["rgba16_pixel"] = make_desc(15, 4, [(R, 16, 0), (G, 16, 0), (B, 16, 0), (A, 16, 0)], U.PIXEL, tile_cols=3)
    c["rgb16_component"] = make_desc(15, 4, [(B, 16, 0), (R, 16, 0), (G, 16, 0)], U.COMPONENT, tile_cols=3)
    c["mono_alpha_8"] = make_desc(13, 5, [(M, 8, 0), (A, 8, 0)], U.ROW)
    return c


def synthetic(desc, seed=1, **file_args):
    """(file bytes, planes per component, payload) of random samples under `desc`"""
    planes = random_planes(desc, seed)
    payload = pack(desc, planes)
    return heif_file(desc, payload, **file_args), planes, payload
