"""csrc/hm_overlay_plan.h ('iovl' payload parser, layer clipping, start-layer search, the division by 255 as multiply and shift,
the Q20 predicate) in a stand-alone host program (tests/host/overlay_plan_check.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: no GPU, no library, nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    out = str(tmp_path_factory.mktemp("overlay_plan") / "overlay_plan_check")
    src = os.path.join(ROOT, "tests", "host", "overlay_plan_check.cpp")
    inc = os.path.join(ROOT, "heif-decoder-lib_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", inc, src, "-o", out], check=True)
    return out


def test_overlay_plan_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "overlay plan: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("w,h", [(5, 3), (8, 8)])
@pytest.mark.parametrize("alpha", [0, 1])
def test_reference_defined_is_where_the_transcription_stays_inside(exe, w, h, alpha):
    """hm::reference_defined (the C++ the product documents Q20 with) against the literal transcription of HeifPixelImage::overlay:
    the transcription leaves a plane exactly on the placements the predicate excludes - dx, dy over -(w+1) .. canvas+1 on a 7 x 6 canvas"""
    cw, ch = 7, 6
    r = subprocess.run([exe, "defined", str(cw), str(ch), str(w), str(h), str(alpha)], capture_output=True, text=True, check=True)
    rows = r.stdout.split()
    rng = np.random.default_rng(w * 100 + h * 10 + alpha)
    layer = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    a = rng.integers(0, 256, (h, w), dtype=np.uint8) if alpha else None
    assert len(rows) == ch + h + 3
    for j, dy in enumerate(range(-(h + 1), ch + 2)):
        assert len(rows[j]) == cw + w + 3
        for i, dx in enumerate(range(-(w + 1), cw + 2)):
            canvas = overlay_ref.fill_rgb_16bit(cw, ch, (0x2000, 0x8000, 0xE000, 0))
            try:
                overlay_ref.overlay_literal(canvas, layer, a, dx, dy)
                inside = True
            except overlay_ref.OutsideOfPlane:
                inside = False
            assert (rows[j][i] == "1") == inside, (dx, dy)
            assert overlay_ref.reference_defined(cw, ch, w, h, dx, dy, bool(alpha)) == inside, (dx, dy)
