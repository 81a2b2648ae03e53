"""The writer-made profiles the ICC tests share (tests/iccwriter.py makes them, tests/icc_ref.py says what they mean): one per curve
type and function type, v2 and v4 headers, three distinct curves, GRAY, cicp tags."""
import math

import icc_ref
import iccwriter as w

P3 = icc_ref.colorants_of(12)
BT709 = icc_ref.colorants_of(1)


def _srgb_samples(n):
    return [int(round(65535.0 * (x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4))) for x in (k / (n - 1) for k in range(n))]


def _wiggle(n):
    """not monotone: a ramp with a ripple on it"""
    return [min(65535, max(0, int(round(65535.0 * (k / (n - 1) + 0.04 * math.sin(k * 0.37)))))) for k in range(n)]


CURVES = {
    "curv0": w.curv(()),
    "curv1": w.curv((2.19921875,)),
    "curv2": w.curv((0, 65535)),
    "curv2_inverted": w.curv((65535, 0)),
    "curv256_srgb": w.curv(_srgb_samples(256)),
    "curv1024_not_monotone": w.curv(_wiggle(1024)),
    "para0": w.para(0, (2.2,)),
    "para1": w.para(1, (2.0, 1.25, -0.25)),
    "para1_negative_base": w.para(1, (1.5, -1.0, 0.5)),       # X >= 0.5: the base a X + b is negative there and counts as 0
    "para1_above_one": w.para(1, (2.0, 1.5, 0.0)),            # (1.5 X)^2 passes 1 at X = 2/3: clamped
    "para2": w.para(2, (2.4, 0.9, 0.1, 0.05)),
    "para2_negative_c": w.para(2, (2.0, 1.0, -0.5, -0.125)),  # below the split Y = c < 0: clamped to 0
    "para3_srgb": w.srgb_para(),
    "para4": w.para(4, (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045, 0.01, 0.002)),
    "para4_above_one": w.para(4, (1.8, 1.0, 0.0, 0.5, 0.1, 0.25, 0.0)),
}
DISTINCT = (w.para(0, (1.8,)), w.srgb_para(), w.curv(_wiggle(1024)))


def one_curve(name, **kw):
    return w.rgb_profile(P3, CURVES[name], **kw)


def display_p3(**kw):
    """what a phone writes: P3 colorants (Bradford-adapted to D50), one parametric sRGB-shaped curve for the three channels"""
    return w.rgb_profile(P3, CURVES["para3_srgb"], **kw)


def three_curves(**kw):
    return w.rgb_profile(P3, DISTINCT, **kw)


def equal_but_separate(**kw):
    """three tags with equal bytes at three offsets"""
    return w.rgb_profile(P3, tuple(bytes(bytearray(CURVES["para3_srgb"])) for _ in range(3)), **kw)


def gray(name="curv1", **kw):
    return w.gray_profile(CURVES[name], **kw)


def with_cicp(primaries, transfer, **kw):
    return w.rgb_profile(P3, DISTINCT, extra=[(b"cicp", w.cicp(primaries, transfer))], **kw)


def all_profiles():
    """name -> bytes: every well-formed profile of the host tests"""
    out = {name: one_curve(name) for name in CURVES}
    out["v2_para3"] = display_p3(version=(2, 4))
    out["v2_curv1024"] = one_curve("curv1024_not_monotone", version=(2, 1), cls=b"scnr")
    out["spac"] = display_p3(cls=b"spac")
    out["three_curves"] = three_curves()
    out["equal_but_separate"] = equal_but_separate()
    out["gray"] = gray()
    out["gray_para"] = gray("para3_srgb", version=(2, 4))
    out["cicp_known"] = with_cicp(12, 13)
    out["cicp_unknown_transfer"] = with_cicp(12, 2)
    out["cicp_unknown_primaries"] = with_cicp(22, 13)
    out["bt709_colorants"] = w.rgb_profile(BT709, CURVES["para3_srgb"])
    return out
