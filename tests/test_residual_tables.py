"""k_residual's constant tables (csrc/residual_tables.h) are one 4 352-byte image the compiler works out and the kernel copies
into LDS.  Here the image - as the test hook hm_debug_residual_tables hands it out, without a GPU - is rebuilt in numpy from the
formulas of the prologue the kernel had before (residual.hip built dct, tab[0..92), w8, mt16, mt32 in LDS per workgroup) and
compared byte for byte, padding included."""
import ctypes as C

import numpy as np

RT_BYTES = 4352
DCT_MAG = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0]
LEVEL_SCALE = [40, 45, 51, 57, 64, 72]
DST = [[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]]


def expected_image():
    # dct[i], i = 32 k + n (the first loop of the old prologue)
    dct = np.zeros(1024, dtype=np.int8)
    for i in range(1024):
        k, n = i >> 5, i & 31
        m = (k * (2 * n + 1)) & 127
        if k == 0:
            v = 64
        elif m <= 32:
            v = DCT_MAG[m]
        elif m <= 64:
            v = -DCT_MAG[64 - m]
        elif m <= 96:
            v = -DCT_MAG[m - 64]
        else:
            v = DCT_MAG[128 - m]
        dct[i] = v
    # tab: [70, 76) level scale, [76, 92) DST; 128 entries reserved
    tab = np.zeros(128, dtype=np.int16)
    for i in range(92):
        if 70 <= i < 76:
            tab[i] = LEVEL_SCALE[i - 70]
        elif i >= 76:
            tab[i] = DST[(i - 76) >> 2][(i - 76) & 3]
    # w8[t], t = 4 i + k: dct[4 (2 k)][i] | dct[4 (2 k + 1)][i] << 16
    w8 = np.zeros(32, dtype=np.uint32)
    for t in range(32):
        i, k = t >> 2, t & 3
        lo = int(dct[(4 * (2 * k)) * 32 + i]) & 0xFFFF
        hi = int(dct[(4 * (2 * k + 1)) * 32 + i]) & 0xFFFF
        w8[t] = lo | (hi << 16)
    # mt16[i][j] = dct[2 j][i], rows of 20; mt32[i][j] = dct[j][i], rows of 36
    mt16 = np.zeros((16, 20), dtype=np.int16)
    mt32 = np.zeros((32, 36), dtype=np.int16)
    for i in range(16):
        for j in range(16):
            mt16[i, j] = dct[(2 * j) * 32 + i]
    for i in range(32):
        for j in range(32):
            mt32[i, j] = dct[j * 32 + i]
    parts = [dct.tobytes(), tab.astype("<i2").tobytes(), w8.astype("<u4").tobytes(), mt16.astype("<i2").tobytes(), mt32.astype("<i2").tobytes()]
    return np.frombuffer(b"".join(parts), dtype=np.uint8)


def host_image(hm_hooks):
    hm_hooks.hm_debug_residual_tables.argtypes = [C.c_int, C.c_void_p, C.c_int]
    buf = (C.c_uint8 * RT_BYTES)()
    assert hm_hooks.hm_debug_residual_tables(0, buf, RT_BYTES) == RT_BYTES
    return np.frombuffer(bytes(buf), dtype=np.uint8)


def test_the_image_is_what_the_prologue_built(hm_hooks):
    exp = expected_image()
    assert exp.size == RT_BYTES
    got = host_image(hm_hooks)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} bytes differ, first at offset {bad[0]}: {got[bad[0]]} instead of {exp[bad[0]]}"


def test_the_basis_is_the_standard_s(hm_hooks):
    """independent of the folding formula: the 32-point basis is round(64 sqrt(2) cos((2 n + 1) k pi / 64)) up to the standard's
    hand-tuned entries (at most 1 off), its first row 64, and the DST rows are the standard's"""
    got = host_image(hm_hooks)
    dct = got[:1024].view(np.int8).reshape(32, 32).astype(np.int32)
    k, n = np.mgrid[0:32, 0:32]
    ideal = 64 * np.sqrt(2) * np.cos((2 * n + 1) * k * np.pi / 64)
    ideal[0, :] = 64
    assert np.abs(dct - ideal).max() < 1.5
    assert (dct[0] == 64).all()
    tab = got[1024:1280].view("<i2")
    assert tab[70:76].tolist() == LEVEL_SCALE and tab[76:92].reshape(4, 4).tolist() == DST
    assert not tab[:70].any() and not tab[92:].any()


def test_too_small_a_buffer_is_refused(hm_hooks):
    hm_hooks.hm_debug_residual_tables.argtypes = [C.c_int, C.c_void_p, C.c_int]
    buf = (C.c_uint8 * 16)()
    assert hm_hooks.hm_debug_residual_tables(0, buf, 16) < 0
