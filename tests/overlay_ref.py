"""overlay_ref.py - TEST INFRASTRUCTURE: the reference's overlay composition restated in numpy.

  parse_overlay / fill_rgb_16bit / overlay_literal : ImageOverlay::parse (context.cc:318-369), HeifPixelImage::fill_RGB_16bit
      (pixelimage.cc:947-1019) and HeifPixelImage::overlay (pixelimage.cc:1035-1153) line by line, the index arithmetic kept as
      written (32-bit unsigned where the reference's is).  Planes are w x h arrays without padding and EVERY access is checked:
      a sample outside the plane raises OutsideOfPlane.  Where that happens is DESIGN Q20's predicate - found here, not assumed.
  compose_clipped : every layer clipped to the canvas (ISO/IEC 23008-12), vectorised.
  layer_rgb : a decoded child (Y, Cb, Cr planes + what Op_YCbCr_to_RGB<uint8_t> sees of its profile) as R, G, B planes
      (planar_ref.op_ycbcr_to_rgb; a monochrome child through Op_mono_to_YCbCr420's neutral chroma).
"""
import numpy as np

import planar_ref

U32 = 0xFFFFFFFF
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


class OutsideOfPlane(Exception):
    pass


class OverlayError(Exception):
    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind  # "invalid" (heif_suberror_Invalid_overlay_data) | "version" (heif_suberror_Unsupported_data_version)


def _readvec(data, ptr, n):
    v = 0
    for i in range(n):
        v = (v << 8) | data[ptr + i]
    return v, ptr + n


def _readvec_signed(data, ptr, n):
    v, ptr = _readvec(data, ptr, n)
    if v & (1 << (8 * n - 1)):
        v -= 1 << (8 * n)
    return v, ptr


def parse_overlay(num_images, data):
    """-> dict(background=[r, g, b, a], width, height, offsets=[(x, y)])"""
    if len(data) < 2 + 4 * 2:
        raise OverlayError("invalid", "Overlay image data incomplete")
    version = data[0]
    if version != 0:
        raise OverlayError("version", f"Overlay image data version {version} is not implemented yet")
    flags = data[1]
    field_len = 4 if flags & 1 else 2
    ptr = 2
    if ptr + 4 * 2 + 2 * field_len + num_images * 2 * field_len > len(data):
        raise OverlayError("invalid", "Overlay image data incomplete")
    bkg = []
    for _ in range(4):
        c, ptr = _readvec(data, ptr, 2)
        bkg.append(c)
    width, ptr = _readvec(data, ptr, field_len)
    height, ptr = _readvec(data, ptr, field_len)
    if width == 0 or height == 0:
        raise OverlayError("invalid", "Overlay image with zero width or height.")
    offsets = []
    for _ in range(num_images):
        x, ptr = _readvec_signed(data, ptr, field_len)
        y, ptr = _readvec_signed(data, ptr, field_len)
        offsets.append((x, y))
    return dict(background=bkg, width=width, height=height, offsets=offsets)


def fill_rgb_16bit(w, h, bkg):
    """three w x h uint8 planes filled with the 16-bit values >> 8 (the canvas has no alpha plane: bkg[3] is not used)"""
    return [np.full((h, w), (bkg[c] >> 8) & 0xFF, dtype=np.uint8) for c in range(3)]


def _negate_negative_int32(x):
    assert x <= 0
    return INT32_MAX + 1 if x == INT32_MIN else -x


def _check(plane, row, col, n=1):
    h, w = plane.shape
    if row < 0 or row >= h or col < 0 or col + n > w:
        raise OutsideOfPlane(f"row {row}, columns {col}..{col + n - 1} of a {w} x {h} plane")


def overlay_literal(canvas, layer, alpha, dx, dy):
    """HeifPixelImage::overlay on canvas = [R, G, B] (modified in place), layer = [R, G, B], alpha = plane or None"""
    has_alpha = alpha is not None
    for ch in range(3):  # (std::set order R, G, B; the canvas has no alpha channel)
        in_p, out_p = layer[ch], canvas[ch]
        in_h, in_w = in_p.shape
        out_h, out_w = out_p.shape
        if dx > 0 and dx >= out_w:
            return
        elif dx < 0 and in_w <= _negate_negative_int32(dx):
            return
        if dx < 0:
            in_x0 = _negate_negative_int32(dx)
            out_x0 = 0
            in_w = in_w - in_x0
        else:
            in_x0 = 0
            out_x0 = dx
        if (dx & U32) > U32 - in_w or ((dx + in_w) & U32) > out_w:
            in_w = (out_w - (dx & U32)) & U32
        if dy > 0 and dy >= out_h:
            return
        elif dy < 0 and in_h <= _negate_negative_int32(dy):
            return
        if dy < 0:
            in_y0 = _negate_negative_int32(dy)
            out_y0 = 0
            in_h = in_h - in_y0
        else:
            in_y0 = 0
            out_y0 = dy
        if (dy & U32) > U32 - in_h or ((dy + in_h) & U32) > out_h:
            in_h = (out_h - (dy & U32)) & U32
        for y in range(in_y0, in_h):
            orow = out_y0 + y - in_y0
            if not has_alpha:
                n = (in_w - in_x0) & U32
                if n > (1 << 20):
                    raise OutsideOfPlane(f"memcpy of {n} bytes")
                if n == 0:
                    continue
                _check(out_p, orow, out_x0, n)
                _check(in_p, y, in_x0, n)
                out_p[orow, out_x0:out_x0 + n] = in_p[y, in_x0:in_x0 + n]
            else:
                for x in range(in_x0, in_w):
                    _check(out_p, orow, out_x0 + x)
                    _check(in_p, y, in_x0 + x)
                    _check(alpha, y, in_x0 + x)
                    in_val = int(in_p[y, in_x0 + x])
                    a = int(alpha[y, in_x0 + x])
                    out_p[orow, out_x0 + x] = (in_val * a + int(out_p[orow, out_x0 + x]) * (255 - a)) // 255


def overlay_clipped(canvas, layer, alpha, dx, dy):
    """the layer clipped to the canvas, copied (no alpha) or blended with the same integer formula"""
    out_h, out_w = canvas[0].shape
    in_h, in_w = layer[0].shape
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + in_w, out_w), min(dy + in_h, out_h)
    if x0 >= x1 or y0 >= y1:
        return
    for ch in range(3):
        src = layer[ch][y0 - dy:y1 - dy, x0 - dx:x1 - dx].astype(np.int64)
        if alpha is None:
            canvas[ch][y0:y1, x0:x1] = src
        else:
            a = alpha[y0 - dy:y1 - dy, x0 - dx:x1 - dx].astype(np.int64)
            dst = canvas[ch][y0:y1, x0:x1].astype(np.int64)
            canvas[ch][y0:y1, x0:x1] = (src * a + dst * (255 - a)) // 255


def reference_defined(cw, ch, w, h, dx, dy, has_alpha):
    """hm::reference_defined (csrc/hm_overlay_plan.h) restated: the placements on which overlay() stays inside both images"""
    if dx > 0 and dx >= cw:
        return True
    if dx < 0 and w <= -dx:
        return True
    if dy > 0 and dy >= ch:
        return True
    if dy < 0 and h <= -dy:
        return True
    if dx < 0 and (has_alpha or w + dx < cw):
        return False
    if dy < 0 and h + dy < ch:
        return False
    return True


def compose(canvas_size, background, layers, literal_where_defined=True):
    """layers: [(rgb planes, alpha or None, dx, dy)] bottom first -> (R, G, B, every_layer_defined).
    A layer inside the Q20 domain goes through the literal transcription, the others through the clipping composer."""
    w, h = canvas_size
    canvas = fill_rgb_16bit(w, h, background)
    all_defined = True
    for rgb, alpha, dx, dy in layers:
        lh, lw = rgb[0].shape
        if literal_where_defined and reference_defined(w, h, lw, lh, dx, dy, alpha is not None):
            overlay_literal(canvas, rgb, alpha, dx, dy)
        else:
            all_defined = False
            overlay_clipped(canvas, rgb, alpha, dx, dy)
    return canvas[0], canvas[1], canvas[2], all_defined


def layer_rgb(planes, chroma, seen):
    """planes: [Y] or [Y, Cb, Cr] uint8 arrays of a decoded 8-bit child; seen = (has_nclx, matrix, primaries, full_range) of the image
    Op_YCbCr_to_RGB<uint8_t> is handed -> [R, G, B]"""
    y = np.asarray(planes[0], dtype=np.uint8)
    if chroma == 0:  # Op_mono_to_YCbCr420: neutral chroma planes
        hh, ww = y.shape
        cb = np.full(((hh + 1) // 2, (ww + 1) // 2), 128, dtype=np.uint8)
        return list(planar_ref.op_ycbcr_to_rgb(y, cb, cb, 8, 1, seen))
    return list(planar_ref.op_ycbcr_to_rgb(y, np.asarray(planes[1], dtype=np.uint8), np.asarray(planes[2], dtype=np.uint8), 8, chroma, seen))


def interleave(r, g, b, with_alpha):
    """Op_RGB_to_RGB24_32: alpha 255"""
    planes = [r, g, b] + ([np.full_like(r, 255)] if with_alpha else [])
    return np.stack(planes, axis=-1).astype(np.uint8)
