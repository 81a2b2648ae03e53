"""HEIF writer for HDR test files (test tool): a single image or a 'grid' whose primary item carries 'clli' / 'mdcv' properties
(ISO/IEC 23008-12: content light level, mastering display colour volume - plain boxes, no version word).  The box helpers are
heifwriter's; the properties of a grid go to the grid item, the one that is decoded."""
import struct

from heifwriter import _box, _colr, _full, _hvcc, split_nals


def clli_box(max_cll, max_pall=0):
    return _box(b"clli", struct.pack(">HH", max_cll, max_pall))


def mdcv_box(primaries, white, max_lum, min_lum):
    """primaries: three (x, y) pairs and white: one, in units of 0.00002; max_lum / min_lum in units of 0.0001 cd/m2"""
    body = b"".join(struct.pack(">HH", x, y) for x, y in primaries) + struct.pack(">HH", *white) + struct.pack(">II", max_lum, min_lum)
    return _box(b"mdcv", body)


# BT.2020 primaries and D65 in mdcv units (ITU-T H.265 D.3.28 lists these very numbers as an example)
BT2020_XY = ((35400, 14600), (8500, 39850), (6550, 2300))
D65_XY = (15635, 16450)


def write_hdr_heic(pictures, size, bit_depth=10, colr=(9, 16, 1, 0), grid=None, clli=None, mdcv=None, raw_props=(), ispe=None):
    """pictures: [len][NAL] strings; size: (w, h) of one picture; grid: None or (rows, cols, out_w, out_h).
    clli: None, (max_cll, max_pall) or bytes (the box's body as it is - a truncated one); mdcv: None or (max_lum, min_lum) raw, with the
    BT.2020 primaries; raw_props: further whole boxes for the primary item; ispe: bytes, the body of the coded images' 'ispe' as it is."""
    props, assoc, items = [], {}, []

    def prop(box):
        if box not in props:
            props.append(box)
        return props.index(box) + 1

    light = []
    if clli is not None:
        light.append(_box(b"clli", clli) if isinstance(clli, (bytes, bytearray)) else clli_box(*clli))
    if mdcv is not None:
        light.append(mdcv_box(BT2020_XY, D65_XY, *mdcv))
    light += list(raw_props)
    for k, lp in enumerate(pictures):
        nals = split_nals(lp)
        params = [n for n in nals if ((n[0] >> 1) & 0x3F) in (32, 33, 34)]
        vcl = [n for n in nals if ((n[0] >> 1) & 0x3F) not in (32, 33, 34)]
        items.append((k + 1, b"hvc1", b"".join(struct.pack(">I", len(n)) + n for n in vcl)))
        assoc[k + 1] = [0x8000 | prop(_hvcc(params, 1, bit_depth)), prop(_box(b"ispe", ispe) if ispe is not None else _full(b"ispe", 0, 0, struct.pack(">II", *size))),
                        prop(_colr(colr))]
    primary, iref = 1, b""
    if grid is not None:
        rows, cols, ow, oh = grid
        primary = len(pictures) + 1
        items.append((primary, b"grid", bytes([0, 0, rows - 1, cols - 1]) + struct.pack(">HH", ow, oh)))
        assoc[primary] = [prop(_full(b"ispe", 0, 0, struct.pack(">II", ow, oh)))]
        dimg = _box(b"dimg", struct.pack(">HH", primary, len(pictures)) + b"".join(struct.pack(">H", k + 1) for k in range(len(pictures))))
        iref = _full(b"iref", 0, 0, dimg)
    assoc[primary] += [prop(b) for b in light]
    ipma = struct.pack(">I", len(assoc))
    for iid in sorted(assoc):
        ipma += struct.pack(">HB", iid, len(assoc[iid]))
        for v in assoc[iid]:
            ipma += bytes([(0x80 if v & 0x8000 else 0) | (v & 0x7F)])
    iprp = _box(b"iprp", _box(b"ipco", b"".join(props)) + _full(b"ipma", 0, 0, ipma))
    hdlr = _full(b"hdlr", 0, 0, struct.pack(">I4s", 0, b"pict") + b"\0" * 13)
    pitm = _full(b"pitm", 0, 0, struct.pack(">H", primary))
    iinf = struct.pack(">H", len(items))
    for iid, typ, _ in items:
        iinf += _full(b"infe", 2, 0, struct.pack(">HH4s", iid, 0, typ) + b"\0")
    iinf = _full(b"iinf", 0, 0, iinf)
    ftyp = _box(b"ftyp", b"heic" + struct.pack(">I", 0) + b"mif1heic")

    def meta_with(offsets):
        iloc = bytes([0x44, 0x00]) + struct.pack(">H", len(items))
        for (iid, _, payload), off in zip(items, offsets):
            iloc += struct.pack(">HHH", iid, 0, 1) + struct.pack(">II", off, len(payload))
        return _full(b"meta", 0, 0, hdlr + pitm + _full(b"iloc", 0, 0, iloc) + iinf + iref + iprp)

    off = len(ftyp) + len(meta_with([0] * len(items))) + 8
    offsets = []
    for _, _, payload in items:
        offsets.append(off)
        off += len(payload)
    return ftyp + meta_with(offsets) + _box(b"mdat", b"".join(p for _, _, p in items))
