"""GPU: k_residual with its constant tables loaded as one image, two CTB rows of a chain kind per wave at full load and the block
map written in pairs of cells - every picture bit-exact against the oracle (stage 0: reconstruction, stage 1: + deblocking from the
block map, stage 3 where SAO is comparable), in the shapes at which each of them can go wrong; and k_chain, which consumes what
k_residual writes, in every cut it can be forced into on a small picture.  One helper process decodes all cases
(residual_fixed_costs_check.py: the cut knobs are hooks of the test library); the tests below read its verdicts and the launchers'
debug lines.

Not among the cases: a picture of 68 x 36 (a block map of odd width).  No such picture exists - width and height are multiples of
MinCbSizeY >= 8 (the synthesiser refuses it, the parser and stream_check.cpp too) -, so the map's width is always even and the
kernel has one path for it."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_BYTES = 4352


@pytest.fixture(scope="module")
def check():
    """-> ({case: verdict}, {case: [the stderr behind each of its "[case]" lines]})"""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, os.path.join(HERE, "residual_fixed_costs_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    logs, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            cur = logs.setdefault(line.split()[1], [])
            cur.append("")
        elif cur is not None:
            cur[-1] += line + "\n"
    return json.loads(r.stdout.strip().splitlines()[-1]), logs


def _residual_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("[k_residual] ")]


@pytest.mark.parametrize("case", ["one_ctb", "three_rows", "two_rows_wide", "mixed_few", "ragged_ctb16", "ragged_ctb32", "ctb64", "ten_bit_420", "ten_bit_422",
                                  "eight_bit_422", "mono", "big_blocks_at_the_edges", "slices_deblock_per_slice"])
def test_pictures_equal_the_oracle(check, case):
    verdicts, logs = check
    assert verdicts[case] == "ok", verdicts[case]
    assert all(_residual_lines(text) for text in logs[case]), "k_residual did not run"
    # few pictures: a wave per row (in segments)
    assert all("1 rows of a kind per wave" in ln for text in logs[case] for ln in _residual_lines(text)), logs[case]


def test_two_rows_per_wave_above_the_threshold(check):
    """one batch of 32x32 (one row: its wave has no second), 96x96 (three: the last wave of a kind has one) and 128x64 pictures, enough
    of them to cross the launcher's threshold - and the same three sizes below it (mixed_few above)"""
    verdicts, logs = check
    assert verdicts["mixed_two_rows_per_wave"] == "ok", verdicts["mixed_two_rows_per_wave"]
    lines = [ln for text in logs["mixed_two_rows_per_wave"] for ln in _residual_lines(text)]
    assert lines and all("in 1 segments, 2 rows of a kind per wave" in ln for ln in lines), lines


def test_forced_segments_keep_a_wave_per_row(check):
    """resid_segs 1, 2, 3 on the 96x96 batch: all three the oracle's pictures (so equal), each with the forced count and a wave per row"""
    verdicts, logs = check
    assert verdicts["three_rows"] == "ok", verdicts["three_rows"]
    texts = logs["three_rows"]
    assert len(texts) == 4
    for segs, text in zip((1, 2, 3), texts[1:]):
        lines = _residual_lines(text)
        assert lines and all(f"in {segs} segments, 1 rows of a kind per wave" in ln for ln in lines), (segs, lines)


@pytest.mark.parametrize("case", ["forced_cuts", "forced_cuts_422_ctb64"])
def test_every_forced_cut_of_the_chains(check, case):
    verdicts, logs = check
    assert verdicts[case] == "ok", verdicts[case]
    if case == "forced_cuts":  # (4 x 3 CTUs of 32: every forced cut fits; a forced share falls to a wave per row pair, handing over through HBM)
        text = "".join(logs[case])
        for want in ("(one per picture)", "(one per pair of CTU rows)", "(one per CTU row)", "(one per chain of a CTU row)", "handed over through LDS in a ring",
                     "a CTU starts when the CTU above it is done"):
            assert want in text, (want, text[-3000:])


def test_block_map_under_the_fused_tail_and_the_separate_kernels(check):
    verdicts, _ = check
    assert verdicts["fused_tail"] == "ok", verdicts["fused_tail"]


def test_the_device_holds_the_host_built_tables(hm_hooks):
    """the image k_residual copies into LDS, read back from the device, is the one the host compiler worked out
    (test_residual_tables.py holds that one to the formulas)"""
    hm_hooks.hm_debug_residual_tables.argtypes = [C.c_int, C.c_void_p, C.c_int]
    host, dev = (C.c_uint8 * RT_BYTES)(), (C.c_uint8 * RT_BYTES)()
    assert hm_hooks.hm_debug_residual_tables(0, host, RT_BYTES) == RT_BYTES
    assert hm_hooks.hm_debug_residual_tables(1, dev, RT_BYTES) == RT_BYTES, hm_hooks.hm_last_error().decode()
    assert np.array_equal(np.frombuffer(bytes(host), np.uint8), np.frombuffer(bytes(dev), np.uint8))


def test_the_kernels_keep_their_registers(hm_hooks):
    """k_residual seven waves per SIMD (72 registers), the wave per picture of the headline class five (96), neither with scratch"""
    hm_hooks.hm_debug_kernel_regs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int * 2)]
    out = (C.c_int * 2)()
    assert hm_hooks.hm_debug_kernel_regs(0, 0, 0, 0, C.byref(out)) == 0
    assert out[0] <= 72 and out[1] == 0, ("k_residual", out[0], out[1])
    assert hm_hooks.hm_debug_kernel_regs(2, 5, 1, 0, C.byref(out)) == 0
    assert out[0] <= 96 and out[1] == 0, ("k_chain<uint8_t, 5, 0>", out[0], out[1])
