"""Writes profiles/icc_lcms_crosscheck.txt: the model of the ICC reading (tests/icc_ref.py) against littleCMS 2 (Pillow's ImageCms) on
the 17^3 cube of 8-bit colours of three writer-made profiles, rendered to 8-bit sRGB - the histogram of the differences in codes and
their maximum, from which tests/test_icc_host.py takes its bound (the maximum plus one code).  CPU only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_icc_host  # noqa: E402


def main():
    import PIL
    from PIL import ImageCms
    hist, worst = test_icc_host.crosscheck()
    lines = ["The model of the ICC reading (tests/icc_ref.py: curves, Bradford-adapted matrix to BT.709 primaries, sRGB encoding) against",
             "littleCMS through Pillow's ImageCms (relative colorimetric, the CMM's own sRGB profile as the destination), on the 17^3 cube",
             "of 8-bit colours of three writer-made profiles: Display P3 with one parametric sRGB curve, P3 with three distinct curves",
             "(para 0 / para 3 / a 1024-entry curv that is not monotone), P3 with that curv alone.",
             f"Pillow {PIL.__version__}, littleCMS {getattr(ImageCms.core, 'littlecms_version', '?')}",
             "", "|model - CMM| in 8-bit codes : samples"]
    lines += [f"  {d} : {n}" for d, n in hist.items()]
    lines += [f"maximum {worst}", "",
              "A difference of one code is the CMM's 8-bit path (its curves and matrix run in fixed point); the adaptation and the curves agree.",
              f"tests/test_icc_host.py asserts at most {worst} + 1 = {worst + 1} codes."]
    with open(os.path.join(ROOT, "profiles", "icc_lcms_crosscheck.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
