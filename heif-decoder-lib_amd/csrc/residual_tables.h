// residual_tables.h - the constant tables of k_residual (residual.hip) as ONE image, worked out by the compiler.
//
// Every workgroup of k_residual used to rebuild these 4 352 bytes in LDS from c_dct_mag / c_level_scale / c_dst (index
// arithmetic, two stages, three barriers) although they depend on nothing but constants.  The image is now a constant of the
// code object: the kernel copies it into LDS 16 bytes per thread, the test hook (test_hooks.cpp) hands the same bytes to
// tests/test_residual_tables.py, which rebuilds them from the formulas.  The formulas live here and nowhere else for this
// kernel; recon.hip and chain.hip keep their own tables in constant memory (recon_common.h).
//
// Layout (bytes, little endian; everything not named is zero):
//   [   0, 1024)  dct   int8 [32][32]   the 32-point inverse-DCT basis, dct[k][n] (fallback-dct.cc:592-733: mat_dct)
//   [1024, 1280)  tab   int16[128]      [70, 76) level scale (transform.cc:496-502), [76, 92) DST-VII rows (fallback-dct.cc:311-449)
//   [1280, 1408)  w8    uint32[8][4]    8-point basis as pairs of consecutive inputs: M[j][i] = dct[4 j][i], j = 2k | 2k + 1 << 16
//   [1408, 2048)  mt16  int16[16][20]   16-point basis as rows mt[i][j] = M[j][i] = dct[2 j][i], 4 int16 of padding per row
//   [2048, 4352)  mt32  int16[32][36]   32-point basis, mt[i][j] = dct[j][i], 4 int16 of padding per row
#ifndef HM_RESIDUAL_TABLES_H
#define HM_RESIDUAL_TABLES_H

#include <cstdint>

constexpr int HM_RT_DCT = 0, HM_RT_TAB = 1024, HM_RT_W8 = 1024 + 256, HM_RT_MT16 = 1024 + 256 + 128;
constexpr int HM_RT_MT16_STRIDE = 16 + 4, HM_RT_MT32_STRIDE = 32 + 4; // int16 per row (residual.hip: BigGeom::MT_STRIDE)
constexpr int HM_RT_MT32 = HM_RT_MT16 + 16 * HM_RT_MT16_STRIDE * 2;
constexpr int HM_RT_BYTES = HM_RT_MT32 + 32 * HM_RT_MT32_STRIDE * 2;
static_assert(HM_RT_BYTES == 4352 && HM_RT_BYTES % 16 == 0, "copied 16 bytes per thread");

struct alignas(16) hm_residual_tables {
  uint8_t b[HM_RT_BYTES];
};

constexpr hm_residual_tables hm_make_residual_tables()
{
  // magnitudes of the inverse-DCT basis by angle index, level scale, DST-VII: the values of recon_common.h's constant tables
  constexpr int mag[33] = {64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64,
                           61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0};
  constexpr int level_scale[6] = {40, 45, 51, 57, 64, 72};
  constexpr int dst[4][4] = {{29, 55, 74, 84}, {74, 74, 0, -74}, {84, -29, -74, 55}, {55, -84, 74, -29}};
  hm_residual_tables t{};
  int dct[32][32] = {};
  for (int k = 0; k < 32; k++)
    for (int n = 0; n < 32; n++) {
      const int m = (k * (2 * n + 1)) & 127; // angle index of cos((2 n + 1) k pi / 64), folded into a quarter period
      int v = 0;
      if (k == 0) v = 64;
      else if (m <= 32) v = mag[m];
      else if (m <= 64) v = -mag[64 - m];
      else if (m <= 96) v = -mag[m - 64];
      else v = mag[128 - m];
      dct[k][n] = v;
      t.b[HM_RT_DCT + k * 32 + n] = (uint8_t)(int8_t)v;
    }
  auto put16 = [&t](int at, int v) {
    t.b[at] = (uint8_t)((unsigned)v & 0xFF);
    t.b[at + 1] = (uint8_t)(((unsigned)v >> 8) & 0xFF);
  };
  for (int i = 0; i < 6; i++) put16(HM_RT_TAB + 2 * (70 + i), level_scale[i]);
  for (int i = 0; i < 16; i++) put16(HM_RT_TAB + 2 * (76 + i), dst[i >> 2][i & 3]);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) {
      put16(HM_RT_W8 + 4 * (i * 4 + k), dct[4 * (2 * k)][i]);
      put16(HM_RT_W8 + 4 * (i * 4 + k) + 2, dct[4 * (2 * k + 1)][i]);
    }
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++) put16(HM_RT_MT16 + 2 * (i * HM_RT_MT16_STRIDE + j), dct[2 * j][i]);
  for (int i = 0; i < 32; i++)
    for (int j = 0; j < 32; j++) put16(HM_RT_MT32 + 2 * (i * HM_RT_MT32_STRIDE + j), dct[j][i]);
  return t;
}

#endif
