"""regionwriter.py - TEST TOOL: HEIF files with region items ('rgan') and mask items ('mski' + 'mskC') beside the items of
overlaywriter.Writer, with their 'cdsc' and 'mask' references; raw-payload overrides for malformed files.

    w = Writer()
    img = w.hvc1(picture, (64, 64))
    m = w.mski(bytes(37 * 21), (37, 21))
    r = w.rgan([("rectangle", 3, 4, 10, 5), ("polygon", [(0, 0), (9, 0), (4, 7)]), ("referenced_mask", -2, 1, 0, 0, m)], (64, 64), annotates=[img])
    data = w.finish(primary=img)

A region is a tuple: ("point", x, y), ("rectangle", x, y, w, h), ("ellipse", x, y, rx, ry), ("polygon", points), ("polyline", points),
("inline_mask", x, y, w, h, bit string[, mask_coding_method]), ("referenced_mask", x, y, w, h, mask item id), or ("raw", type byte, bytes)."""
import struct

import overlaywriter
from heifwriter import _full

TYPES = {"point": 0, "rectangle": 1, "ellipse": 2, "polygon": 3, "referenced_mask": 4, "inline_mask": 5, "polyline": 6}


def pack_bits(rows):
    """the bit string of an inline mask: rows of 0 / 1 values, most significant bit first, rows not byte aligned"""
    flat = [int(bool(v)) for row in rows for v in row]
    out = bytearray((len(flat) + 7) // 8)
    for i, v in enumerate(flat):
        if v:
            out[i >> 3] |= 0x80 >> (i & 7)
    return bytes(out)


def region_payload(regions, reference_size, wide=False, version=0, count=None):
    """RegionItem's payload (region.cc:30-116): version, flags (bit 0: 32-bit fields), reference size, region count, the regions"""
    u, s = (">I", ">i") if wide else (">H", ">h")
    out = bytes([version, 1 if wide else 0]) + struct.pack(u, reference_size[0]) + struct.pack(u, reference_size[1])
    out += bytes([len(regions) if count is None else count])
    for r in regions:
        kind = r[0]
        if kind == "raw":
            out += bytes([r[1]]) + r[2]
            continue
        out += bytes([TYPES[kind]])
        if kind == "point":
            out += struct.pack(s, r[1]) + struct.pack(s, r[2])
        elif kind in ("polygon", "polyline"):
            out += struct.pack(u, len(r[1])) + b"".join(struct.pack(s, x) + struct.pack(s, y) for x, y in r[1])
        else:
            out += struct.pack(s, r[1]) + struct.pack(s, r[2]) + struct.pack(u, r[3]) + struct.pack(u, r[4])
            if kind == "inline_mask":
                out += bytes([r[6] if len(r) > 6 else 0]) + bytes(r[5])
    return out


class Writer(overlaywriter.Writer):
    def mski(self, data, size, bits=8, hidden=True, mskc=True, ispe=True):
        """a mask item: `data` its payload (8 bits: size[0] * size[1] samples, row after row); mskc False: no 'mskC' property"""
        a = []
        if ispe:
            a.append(self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *size))))
        if mskc is True:
            a.append(0x8000 | self._prop(_full(b"mskC", 0, 0, bytes([bits]))))
        elif mskc:  # a raw box (malformed files)
            a.append(0x8000 | self._prop(mskc))
        return self._add(b"mski", bytes(data), a, hidden)

    def unci_mono8(self, data, size, hidden=False):
        """the same samples as a monochrome 8-bit 'unci' item in component interleave (ISO/IEC 23001-17)"""
        cmpd = overlaywriter._box(b"cmpd", struct.pack(">IH", 1, 0))
        uncc = _full(b"uncC", 0, 0, b"\0\0\0\0" + struct.pack(">I", 1) + struct.pack(">HBBB", 0, 7, 0, 0) + struct.pack(">BBBBIIIII", 0, 0, 0, 0, 0, 0, 0, 0, 0))
        a = [self._prop(_full(b"ispe", 0, 0, struct.pack(">II", *size))), self._prop(cmpd), 0x8000 | self._prop(uncc)]
        return self._add(b"unci", bytes(data), a, hidden)

    def rgan(self, regions, reference_size, annotates=(), wide=False, payload=None, masks=None, hidden=True):
        """a region item; annotates: the images its 'cdsc' reference names; the 'mask' reference lists the mask items of its
        referenced-mask regions in order.  payload / masks: raw overrides (malformed files)"""
        if payload is None:
            payload = region_payload(regions, reference_size, wide)
        rid = self._add(b"rgan", payload, [], hidden)
        if annotates:
            self.refs.append((b"cdsc", rid, list(annotates)))
        to = list(masks) if masks is not None else [r[5] for r in regions if r[0] == "referenced_mask"]
        if to:
            self.refs.append((b"mask", rid, to))
        return rid
