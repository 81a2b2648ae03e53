"""overlaywriter.py - TEST TOOL: HEIF files with derived image items ('iovl' overlays, 'iden' identity derivations) over coded
'hvc1' items and 'grid' items, with alpha auxiliary images and transformative properties per item.  Box helpers are heifwriter's.

    w = Writer()
    a = w.hvc1(picture, (64, 64), chroma_format=1)
    g = w.grid([w.hvc1(p, (64, 64)) for p in four], 2, 2, 128, 128)
    w.alpha(alpha_picture, (64, 64), a)
    o = w.iovl([(g, 0, 0), (a, 10, -3)], (96, 80), background=(0x1234, 0x8000, 0xFFFF, 0))
    data = w.finish(primary=o)
"""
import struct

from heifwriter import _box, _colr, _full, _hvcc, _transform_box, split_nals

ALPHA_URN = "urn:mpeg:hevc:2015:auxid:1"


def iovl_payload(offsets, canvas, background=(0, 0, 0, 0), wide=False, version=0):
    """ImageOverlay's payload (context.cc:318-369): version, flags, 4 x 16-bit background, canvas size, one signed (x, y) per layer"""
    fmt_u, fmt_s = (">I", ">i") if wide else (">H", ">h")
    out = bytes([version, 1 if wide else 0]) + struct.pack(">4H", *background)
    out += struct.pack(fmt_u, canvas[0]) + struct.pack(fmt_u, canvas[1])
    for x, y in offsets:
        out += struct.pack(fmt_s, x) + struct.pack(fmt_s, y)
    return out


class Writer:
    def __init__(self):
        self.items = []   # (id, type, payload, hidden)
        self.props = []
        self.index_of = {}
        self.assoc = {}
        self.refs = []    # (type, from, [to])

    def _prop(self, box):
        if box not in self.index_of:
            self.props.append(box)
            self.index_of[box] = len(self.props)
        return self.index_of[box]

    def _add(self, typ, payload, assoc, hidden=False):
        iid = len(self.items) + 1
        self.items.append((iid, typ, payload, hidden))
        self.assoc[iid] = assoc
        return iid

    def _transforms(self, transforms):
        return [0x8000 | self._prop(_transform_box(t)) for t in (transforms or [])]

    def hvc1(self, picture, size, chroma_format=1, bit_depth=8, colr=None, transforms=None, hidden=False):
        """picture: [u32 BE len][NAL] string with VPS / SPS / PPS first; size: the declared 'ispe'"""
        nals = split_nals(picture)
        params = [n for n in nals if ((n[0] >> 1) & 0x3F) in (32, 33, 34)]
        vcl = [n for n in nals if ((n[0] >> 1) & 0x3F) not in (32, 33, 34)]
        a = [0x8000 | self._prop(_hvcc(params, chroma_format, bit_depth)), self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *size)))]
        if colr is not None:
            a.append(self._prop(_colr(colr)))
        return self._add(b"hvc1", b"".join(struct.pack(">I", len(n)) + n for n in vcl), a + self._transforms(transforms), hidden)

    def grid(self, tiles, rows, cols, out_w, out_h, transforms=None):
        gid = self._add(b"grid", bytes([0, 0, rows - 1, cols - 1]) + struct.pack(">HH", out_w, out_h),
                        [self._prop(_full(b"ispe", 0, 0, struct.pack(">II", out_w, out_h)))] + self._transforms(transforms))
        self.refs.append((b"dimg", gid, list(tiles)))
        return gid

    def alpha(self, picture, size, target, chroma_format=0, bit_depth=8, transforms=None):
        aid = self.hvc1(picture, size, chroma_format, bit_depth, transforms=transforms)
        self.assoc[aid].append(0x8000 | self._prop(_full(b"auxC", 0, 0, ALPHA_URN.encode() + b"\0")))
        self.refs.append((b"auxl", aid, [target]))
        return aid

    def iovl(self, layers, canvas, background=(0, 0, 0, 0), wide=False, transforms=None, ispe=None, payload=None, refs=None):
        """layers: [(item id, dx, dy)] bottom first.  payload / refs: raw overrides (malformed files)."""
        if payload is None:
            payload = iovl_payload([(x, y) for _, x, y in layers], canvas, background, wide)
        oid = self._add(b"iovl", payload, [self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *(ispe or canvas))))] + self._transforms(transforms))
        to = refs if refs is not None else [i for i, _, _ in layers]
        if to:
            self.refs.append((b"dimg", oid, list(to)))
        return oid

    def iden(self, children, size, transforms=None):
        """children: the 'dimg' references (exactly one in a well-formed file); size: the declared 'ispe'"""
        did = self._add(b"iden", b"", [self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *size)))] + self._transforms(transforms))
        if children:
            self.refs.append((b"dimg", did, list(children)))
        return did

    def set_refs(self, from_id, to):
        """replace the 'dimg' references of an item (cycles, references to itself or to missing items)"""
        self.refs = [r for r in self.refs if not (r[0] == b"dimg" and r[1] == from_id)]
        self.refs.append((b"dimg", from_id, list(to)))

    def finish(self, primary):
        items = self.items
        iref = b"".join(_box(t, struct.pack(">HH", frm, len(to)) + b"".join(struct.pack(">H", i) for i in to)) for t, frm, to in self.refs)
        iref = _full(b"iref", 0, 0, iref) if iref else b""
        wide = len(self.props) > 127
        ipma = struct.pack(">I", len(self.assoc))
        for iid in sorted(self.assoc):
            ipma += struct.pack(">HB", iid, len(self.assoc[iid]))
            for v in self.assoc[iid]:
                ipma += struct.pack(">H", v) if wide else bytes([(0x80 if v & 0x8000 else 0) | (v & 0x7F)])
        iprp = _box(b"iprp", _box(b"ipco", b"".join(self.props)) + _full(b"ipma", 0, 1 if wide else 0, ipma))
        hdlr = _full(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"pict") + b"\0" * 13)
        pitm = _full(b"pitm", 0, 0, struct.pack(">H", primary))
        iinf = struct.pack(">H", len(items))
        for iid, typ, _, hidden in items:
            iinf += _full(b"infe", 2, 1 if hidden else 0, struct.pack(">HH4s", iid, 0, typ) + b"\0")
        iinf = _full(b"iinf", 0, 0, iinf)
        ftyp = _box(b"ftyp", b"heic" + struct.pack(">I", 0) + b"mif1heic")

        def meta_with(offsets):
            iloc = bytes([0x44, 0x00]) + struct.pack(">H", len(items))
            for (iid, _, payload, _), off in zip(items, offsets):
                iloc += struct.pack(">HHH", iid, 0, 1) + struct.pack(">II", off, len(payload))
            return _full(b"meta", 0, 0, hdlr + pitm + _full(b"iloc", 0, 0, iloc) + iinf + iref + iprp)

        off = len(ftyp) + len(meta_with([0] * len(items))) + 8
        offsets = []
        for _, _, payload, _ in items:
            offsets.append(off)
            off += len(payload)
        return ftyp + meta_with(offsets) + _box(b"mdat", b"".join(p for _, _, p, _ in items))
