"""The index arithmetic of a multi-view write (csrc/hm_view_multi.h: grouping key, block layout, the cut of blockIdx.y by running sums,
the chunk cut) in a stand-alone host program (tests/host/view_multi_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
no GPU, no library, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_multi_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "view_multi_check")
    src = os.path.join(ROOT, "tests", "host", "view_multi_check.cpp")
    inc = os.path.join(ROOT, "heif-decoder-lib_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", inc, src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "view multi arithmetic: ok" in r.stdout, r.stdout + r.stderr
