"""CPU: the numpy restatement of the reference's overlay code (tests/overlay_ref.py) against itself - the literal transcription of
HeifPixelImage::overlay equals the clipping composer wherever it stays inside its planes, and leaves them exactly where DESIGN Q20's
predicate says - and the payload parser against hand-written byte strings."""
import numpy as np
import pytest

import overlay_ref
from overlaywriter import iovl_payload

CANVAS = (7, 6)
BKG = (0x20FF, 0x8000, 0xE0AB, 0x1234)


def _layer(w, h, alpha, seed):
    rng = np.random.default_rng(seed)
    rgb = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    a = None
    if alpha:
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        a.flat[:6] = [0, 1, 127, 128, 254, 255]
    return rgb, a


@pytest.mark.parametrize("w,h", [(5, 3), (8, 8)])
@pytest.mark.parametrize("alpha", [False, True])
def test_literal_equals_clipped_inside_and_raises_outside(w, h, alpha):
    cw, ch = CANVAS
    rgb, a = _layer(w, h, alpha, 7 * w + h + alpha)
    n_inside = n_outside = 0
    for dy in range(-(h + 1), ch + 2):
        for dx in range(-(w + 1), cw + 2):
            lit = overlay_ref.fill_rgb_16bit(cw, ch, BKG)
            clip = overlay_ref.fill_rgb_16bit(cw, ch, BKG)
            overlay_ref.overlay_clipped(clip, rgb, a, dx, dy)
            defined = overlay_ref.reference_defined(cw, ch, w, h, dx, dy, alpha)
            if defined:
                overlay_ref.overlay_literal(lit, rgb, a, dx, dy)
                for c in range(3):
                    assert np.array_equal(lit[c], clip[c]), (dx, dy, c)
                n_inside += 1
            else:
                with pytest.raises(overlay_ref.OutsideOfPlane):
                    overlay_ref.overlay_literal(lit, rgb, a, dx, dy)
                n_outside += 1
    assert n_inside > 0 and n_outside > 0


def test_background_is_the_high_byte_and_alpha_is_ignored():
    r, g, b = overlay_ref.fill_rgb_16bit(3, 2, BKG)
    assert r.shape == (2, 3) and int(r[0, 0]) == 0x20 and int(g[1, 2]) == 0x80 and int(b[0, 1]) == 0xE0


def test_blend_is_the_truncating_quotient():
    canvas = [np.full((1, 6), 200, dtype=np.uint8) for _ in range(3)]
    layer = [np.full((1, 6), 10, dtype=np.uint8) for _ in range(3)]
    a = np.array([[0, 1, 127, 128, 254, 255]], dtype=np.uint8)
    overlay_ref.overlay_literal(canvas, layer, a, 0, 0)
    assert canvas[0].tolist() == [[(10 * k + 200 * (255 - k)) // 255 for k in (0, 1, 127, 128, 254, 255)]]


@pytest.mark.parametrize("wide", [False, True])
def test_payload_parser(wide):
    offs = [(-(1 << 31), (1 << 31) - 1), (-1, 0), (7, -70000)] if wide else [(-32768, 32767), (-1, 0), (7, -300)]
    data = iovl_payload(offs, (70000 if wide else 96, 80), BKG, wide)
    # by hand: version, flags, four 16-bit values, two sizes, then the offsets
    fl = 4 if wide else 2
    assert data[:2] == bytes([0, 1 if wide else 0]) and data[2:10] == bytes([0x20, 0xFF, 0x80, 0x00, 0xE0, 0xAB, 0x12, 0x34])
    assert len(data) == 10 + 2 * fl + 3 * 2 * fl
    if not wide:
        assert data[10:14] == bytes([0, 96, 0, 80]) and data[14:18] == bytes([0x80, 0x00, 0x7F, 0xFF]) and data[18:22] == bytes([0xFF, 0xFF, 0, 0])
    else:
        assert data[10:18] == bytes([0, 1, 0x11, 0x70, 0, 0, 0, 80]) and data[18:26] == bytes([0x80, 0, 0, 0, 0x7F, 0xFF, 0xFF, 0xFF])
    p = overlay_ref.parse_overlay(3, data)
    assert p["background"] == list(BKG) and (p["width"], p["height"]) == (70000 if wide else 96, 80) and p["offsets"] == offs
    for n in range(len(data)):  # truncation at every length
        with pytest.raises(overlay_ref.OverlayError) as e:
            overlay_ref.parse_overlay(3, data[:n])
        assert e.value.kind == "invalid"
    assert overlay_ref.parse_overlay(1, data)["offsets"] == offs[:1] and overlay_ref.parse_overlay(0, data)["offsets"] == []
    with pytest.raises(overlay_ref.OverlayError) as e:
        overlay_ref.parse_overlay(3, bytes([1]) + data[1:])
    assert e.value.kind == "version"
    for canvas in ((0, 80), (96, 0)):
        with pytest.raises(overlay_ref.OverlayError) as e:
            overlay_ref.parse_overlay(3, iovl_payload(offs, canvas, BKG, wide))
        assert e.value.kind == "invalid"
