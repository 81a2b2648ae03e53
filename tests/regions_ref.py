"""regions_ref.py - the serial model of the region rasteriser: a plain per-pixel loop written from the membership rules of
include/heif_mi355x.h ("Regions and masks") alone, in Python integers (no overflow question arises), and a census of which rule
decided each pixel.

A region is the tuple tests/regionwriter.py takes, with a referenced mask's samples in place of its item id:
("point", x, y), ("rectangle", x, y, w, h), ("ellipse", x, y, rx, ry), ("polygon", points), ("polyline", points),
("inline_mask", x, y, w, h, bit string), ("referenced_mask", x, y, w, h, samples as a h x w uint8 array)."""
import numpy as np

CENSUS_KEYS = ("point_in", "point_out", "rect_in", "rect_out", "ellipse_in", "ellipse_out", "on_segment", "interior_parity_only", "poly_out",
               "inline_bit_0", "inline_bit_1", "mask_value", "clipped_away")


def on_segment(px, py, a, b):
    ax, ay = a
    bx, by = b
    dx, dy = bx - ax, by - ay
    m = max(abs(dx), abs(dy))
    if not (min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)):
        return False
    return 2 * abs(dx * (py - ay) - dy * (px - ax)) <= m  # (m == 0: the box is the point A)


def on_polyline(px, py, pts, closed):
    n = len(pts)
    if n == 0:
        return False
    if n == 1:
        return (px, py) == tuple(pts[0])
    segs = n if closed else n - 1
    return any(on_segment(px, py, pts[k], pts[(k + 1) % n]) for k in range(segs))


def interior(px, py, pts):
    count = 0
    n = len(pts)
    for k in range(n):
        (ax, ay), (bx, by) = pts[k], pts[(k + 1) % n]
        if (ay <= py) == (by <= py):
            continue
        if ay > by:
            ax, ay, bx, by = bx, by, ax, ay
        if (px - ax) * (by - ay) < (bx - ax) * (py - ay):
            count += 1
    return count % 2 == 1


def value(region, px, py, census=None):
    """the region's value at pixel (px, py) of the canvas: 0 / 255, a referenced mask its sample"""
    def note(key):
        if census is not None:
            census[key] = census.get(key, 0) + 1
    kind = region[0]
    if kind == "point":
        hit = (px, py) == (region[1], region[2])
        note("point_in" if hit else "point_out")
        return 255 if hit else 0
    if kind == "rectangle":
        _, x, y, w, h = region
        hit = x <= px < x + w and y <= py < y + h
        note("rect_in" if hit else "rect_out")
        return 255 if hit else 0
    if kind == "ellipse":
        _, x, y, rx, ry = region
        hit = abs(px - x) <= rx and abs(py - y) <= ry and (px - x) ** 2 * ry ** 2 + (py - y) ** 2 * rx ** 2 <= rx ** 2 * ry ** 2
        note("ellipse_in" if hit else "ellipse_out")
        return 255 if hit else 0
    if kind in ("polygon", "polyline"):
        pts = [(int(x), int(y)) for x, y in region[1]]
        if on_polyline(px, py, pts, kind == "polygon"):
            note("on_segment")
            return 255
        if kind == "polygon" and interior(px, py, pts):
            note("interior_parity_only")
            return 255
        note("poly_out")
        return 0
    if kind == "inline_mask":
        _, x, y, w, h, bits = region[:6]
        if not (0 <= px - x < w and 0 <= py - y < h):
            return 0
        i = (py - y) * w + (px - x)
        bit = (bits[i >> 3] >> (7 - (i & 7))) & 1
        note("inline_bit_1" if bit else "inline_bit_0")
        return 255 if bit else 0
    if kind == "referenced_mask":
        _, x, y, w, h, samples = region
        if not (0 <= px - x < w and 0 <= py - y < h):
            return 0
        note("mask_value")
        return int(samples[py - y][px - x])
    raise ValueError(kind)


def clipped_census(region, canvas, census):
    """pixels of the region's own geometry that lie off the canvas (they are clipped away): counted for the census only"""
    cw, ch = canvas
    kind = region[0]
    if kind in ("polygon", "polyline"):
        xs, ys = [p[0] for p in region[1]] or [0], [p[1] for p in region[1]] or [0]
        box = (min(xs), min(ys), max(xs), max(ys)) if region[1] else None
    elif kind == "point":
        box = (region[1], region[2], region[1], region[2])
    elif kind == "ellipse":
        box = (region[1] - region[3], region[2] - region[4], region[1] + region[3], region[2] + region[4])
    else:
        box = (region[1], region[2], region[1] + region[3] - 1, region[2] + region[4] - 1)
    if box is None:
        return
    x0, y0, x1, y1 = (max(-200, box[0]), max(-200, box[1]), min(400, box[2]), min(400, box[3]))
    for py in range(y0, y1 + 1):
        for px in range(x0, x1 + 1):
            if 0 <= px < cw and 0 <= py < ch:
                continue
            if value(region, px, py) != 0:
                census["clipped_away"] = census.get("clipped_away", 0) + 1


def stack(regions, canvas, crop=None, census=None):
    """R x h x w uint8: one plane per region over the crop (x, y, w, h) of the canvas (None: all of it)"""
    cw, ch = canvas
    x0, y0, w, h = crop if crop is not None else (0, 0, cw, ch)
    assert 0 <= x0 and 0 <= y0 and x0 + w <= cw and y0 + h <= ch
    out = np.zeros((len(regions), h, w), dtype=np.uint8)
    for r, region in enumerate(regions):
        for py in range(h):
            for px in range(w):
                out[r, py, px] = value(region, x0 + px, y0 + py, census)
        if census is not None:
            clipped_census(region, canvas, census)
    return out


def labels(planes):
    """h x w uint8 from the stack: 1 + the index of the LAST region whose value is >= 128, else 0"""
    out = np.zeros(planes.shape[1:], dtype=np.uint8)
    for r in range(planes.shape[0]):
        out[planes[r] >= 128] = r + 1
    return out
