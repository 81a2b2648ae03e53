"""iccwriter.py - TEST TOOL: ICC.1 profiles made at test time - a 128-byte header, a tag table, and tags of the types 'XYZ ', 'curv',
'para' and 'cicp' (ICC.1:2022 7.2, 7.3, 10.31, 10.6, 10.18, 10.3).  Nothing here is taken from a profile file.

    p = profile([(b"rXYZ", xyz(0.5151, 0.2412, -0.0011)), ..., (b"rTRC", SRGB_PARA), (b"gTRC", SRGB_PARA), (b"bTRC", SRGB_PARA)])

Tags whose data are the same bytes object share one offset (the usual way three equal curves are stored); every tag's data start on a
multiple of four.  Malformed profiles come from the keyword arguments (size_field, count, raw entries) or from patching the bytes."""
import struct

D50 = (0xF6D6, 0x10000, 0xD32D)  # the connection-space illuminant as s15Fixed16 (ICC.1 7.2.16)


def s15f16(x):
    return struct.pack(">i", int(round(x * 65536.0)))


def xyz(x, y, z):
    return b"XYZ \0\0\0\0" + s15f16(x) + s15f16(y) + s15f16(z)


def xyz_raw(ix, iy, iz):
    return b"XYZ \0\0\0\0" + struct.pack(">iii", ix, iy, iz)


def curv(entries):
    """entries: () the identity; a 1-tuple (g,): Y = X^g as u8Fixed8; else u16 samples"""
    entries = list(entries)
    if len(entries) == 1:
        return b"curv\0\0\0\0" + struct.pack(">IH", 1, int(round(entries[0] * 256.0))) + b"\0\0"
    return b"curv\0\0\0\0" + struct.pack(">I", len(entries)) + b"".join(struct.pack(">H", e) for e in entries)


def para(ftype, params):
    """params: g, a, b, c, d, e, f - as many as the function type has (1, 3, 4, 5, 7)"""
    return b"para\0\0\0\0" + struct.pack(">HH", ftype, 0) + b"".join(s15f16(p) for p in params)


def cicp(primaries, transfer, matrix=0, full_range=1):
    return b"cicp\0\0\0\0" + bytes([primaries, transfer, matrix, full_range])


SRGB_PARAMS = (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045)


def srgb_para():
    return para(3, SRGB_PARAMS)


def header(size, version=(4, 3), cls=b"mntr", space=b"RGB ", pcs=b"XYZ ", signature=b"acsp"):
    h = struct.pack(">I4s", size, b"test") + bytes([version[0], version[1] << 4, 0, 0]) + cls + space + pcs
    h += struct.pack(">6H", 2024, 1, 1, 0, 0, 0) + signature + b"\0" * 4 + struct.pack(">I", 0) + b"\0" * 8 + b"\0" * 8 + struct.pack(">I", 0)
    h += struct.pack(">iii", *D50) + b"test" + b"\0" * 16 + b"\0" * 28
    assert len(h) == 128
    return h


def profile(tags, version=(4, 3), cls=b"mntr", space=b"RGB ", pcs=b"XYZ ", signature=b"acsp", size_field=None, count=None, trailing=b""):
    """tags: [(signature, data)].  size_field / count: what the size field and the tag count say instead of the truth."""
    n = len(tags)
    pos = 128 + 4 + 12 * n
    body, offsets, table = b"", {}, b""
    for sig, data in tags:
        if id(data) not in offsets:
            pad = (-pos) % 4
            body += b"\0" * pad
            pos += pad
            offsets[id(data)] = pos
            body += data
            pos += len(data)
        table += sig + struct.pack(">II", offsets[id(data)], len(data))
    size = pos
    out = header(size if size_field is None else size_field, version, cls, space, pcs, signature)
    return out + struct.pack(">I", n if count is None else count) + table + body + trailing


def tag_entries(p):
    """[(signature, offset, size, position of the entry)] of a profile's tag table"""
    n = struct.unpack_from(">I", p, 128)[0]
    return [(p[132 + 12 * k:136 + 12 * k],) + struct.unpack_from(">II", p, 136 + 12 * k) + (132 + 12 * k,) for k in range(n)]


def patched(p, pos, fmt, value):
    b = bytearray(p)
    struct.pack_into(fmt, b, pos, value)
    return bytes(b)


def rgb_profile(colorants, curves, extra=(), **kw):
    """colorants: three (X, Y, Z) columns - r, g, b; curves: one tag data (shared by the three) or three"""
    if isinstance(curves, (bytes, bytearray)):
        curves = (curves,) * 3
    tags = [(b"wtpt", xyz_raw(*D50))]
    tags += [(s, xyz(*c)) for s, c in zip((b"rXYZ", b"gXYZ", b"bXYZ"), colorants)]
    tags += list(zip((b"rTRC", b"gTRC", b"bTRC"), curves)) + list(extra)
    return profile(tags, **kw)


def gray_profile(curve, extra=(), **kw):
    return profile([(b"wtpt", xyz_raw(*D50)), (b"kTRC", curve)] + list(extra), space=b"GRAY", **kw)
