"""Model of the ICC reading of the light step, written from ICC.1:2022 (7.2 the header, 7.3 the tag table, 10.6 curveType, 10.18
parametricCurveType with its table of function types, 10.31 XYZType, 10.3 cicpType, 9.2 the matrix/TRC tags, Annex E the linear
Bradford adaptation) and from the text under "ICC" in include/heif_mi355x.h - what is evaluated in which order, so that a float64
restatement gives the library's float32 tables bit for bit.  The curves run through math.pow, the C library's pow."""
import math
import struct

import numpy as np

import light_ref

F = np.float32
IDENTITY, GAMMA, TABLE, PARA = 0, 1, 2, 3
RGB, GRAY = 1, 2
PARA_COUNT = (1, 3, 4, 5, 7)
BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]], np.float64)
ILLUMINANT = np.array([0xF6D6, 0x10000, 0xD32D], np.float64) / 65536.0
D65_XYZ = np.array([light_ref.D65[0] / light_ref.D65[1], 1.0, (1.0 - light_ref.D65[0] - light_ref.D65[1]) / light_ref.D65[1]], np.float64)


def _s15f16(b, o):
    return struct.unpack_from(">i", b, o)[0] / 65536.0


def read_curve(b, off):
    """a TRC tag's data at `off`: dict(kind, count, p, table)"""
    typ = b[off:off + 4]
    if typ == b"curv":
        n = struct.unpack_from(">I", b, off + 8)[0]
        if n == 0:
            return dict(kind=IDENTITY, count=0, p=[0.0] * 7, table=None)
        if n == 1:
            return dict(kind=GAMMA, count=1, p=[struct.unpack_from(">H", b, off + 12)[0] / 256.0] + [0.0] * 6, table=None)
        return dict(kind=TABLE, count=n, p=[0.0] * 7, table=[v / 65535.0 for v in struct.unpack_from(f">{n}H", b, off + 12)])
    assert typ == b"para", typ
    f = struct.unpack_from(">H", b, off + 8)[0]
    p = [_s15f16(b, off + 12 + 4 * k) for k in range(PARA_COUNT[f])]
    return dict(kind=PARA, count=f, p=p + [0.0] * (7 - len(p)), table=None)


def parse(b):
    """what a well-formed matrix/TRC (or GRAY) profile says"""
    tags = {}
    for k in range(struct.unpack_from(">I", b, 128)[0]):
        sig, off, size = struct.unpack_from(">4sII", b, 132 + 12 * k)
        tags.setdefault(sig, (off, size))
    out = dict(major=b[8], minor=b[9] >> 4, space=RGB if b[16:20] == b"RGB " else GRAY, has_cicp=b"cicp" in tags, cicp=[0, 0, 0, 0], cicp_known=False)
    if out["has_cicp"]:
        o = tags[b"cicp"][0]
        out["cicp"] = list(b[o + 8:o + 12])
        out["cicp_known"] = out["cicp"][0] in light_ref.PRIMARIES and out["cicp"][1] in light_ref.TRANSFERS
    if out["space"] == GRAY:
        out["colorant"] = np.zeros((3, 3))
        out["curves"] = [read_curve(b, tags[b"kTRC"][0])] * 3
        out["same_curves"] = True
        return out
    out["colorant"] = np.array([[_s15f16(b, tags[s][0] + 8 + 4 * r) for s in (b"rXYZ", b"gXYZ", b"bXYZ")] for r in range(3)], np.float64)
    trc = [tags[s] for s in (b"rTRC", b"gTRC", b"bTRC")]
    out["curves"] = [read_curve(b, o) for o, _ in trc]
    data = [b[o:o + n] for o, n in trc]
    out["same_curves"] = data[0] == data[1] == data[2]
    return out


def curve(c, x):
    """Y of a curve at X in [0, 1], clamped to [0, 1] (float64, scalar)"""
    kind, p = c["kind"], c["p"]
    if kind == IDENTITY:
        y = x
    elif kind == GAMMA:
        y = math.pow(x, p[0])
    elif kind == TABLE:
        t, n = c["table"], c["count"]
        pos = x * (n - 1)
        i = min(int(pos), n - 2)
        y = t[i] + (pos - i) * (t[i + 1] - t[i])
    else:
        g, a, b, cc, d, e, f = p
        P = lambda X: math.pow(max(a * X + b, 0.0), g)
        ft = c["count"]
        if ft == 0:
            y = math.pow(x, g)
        elif ft == 1:
            y = P(x) if x >= -b / a else 0.0
        elif ft == 2:
            y = P(x) + cc if x >= -b / a else cc
        elif ft == 3:
            y = P(x) if x >= d else cc * x
        else:
            y = P(x) + e if x >= d else cc * x + f
    return 1.0 if y >= 1.0 else y if y > 0.0 else 0.0  # (a negative zero is 0)


def table(prof, channel, bits, gain):
    """lin_c[v] = (float)(g * Y_c(v / peak)), g = (double)gain"""
    peak = float((1 << bits) - 1)
    g = float(F(gain))
    c = prof["curves"][channel]
    return np.array([g * curve(c, v / peak) for v in range(1 << bits)], np.float64).astype(F)


def adaptation():
    """A: XYZ under the D65 white of the H.273 primaries -> XYZ under the connection-space illuminant, linear Bradford"""
    gain = (BRADFORD @ ILLUMINANT) / (BRADFORD @ D65_XYZ)
    return np.linalg.inv(BRADFORD) @ np.diag(gain) @ BRADFORD


def matrix(prof, to_primaries):
    """(A T)^-1 M, float64"""
    if prof["space"] == GRAY:
        return np.eye(3)
    return np.linalg.solve(adaptation() @ light_ref.to_xyz(to_primaries), prof["colorant"])


def colorants_of(primaries):
    """the colorant columns a profile of these H.273 primaries carries: A T, column k = (X, Y, Z) of r / g / b"""
    AT = adaptation() @ light_ref.to_xyz(primaries)
    return [tuple(AT[:, k]) for k in range(3)]
