// hm_icc.h — internal: an ICC.1 matrix/TRC profile (versions 2.x and 4.x) read on the host (icc.cpp: no device code).  The rules - what
// is accepted, how a curve is evaluated, how the matrix is derived - are stated in include/heif_mi355x.h ("ICC"); the exported
// functions (hm_icc_parse, hm_icc_table, hm_icc_matrix) are declared there.  This is what devdest.cpp's plan works on.
#ifndef HM_ICC_H
#define HM_ICC_H

#include <cstddef>
#include <cstdint>

#include "heif_mi355x.h"

namespace hm_icc {

// one TRC tag: hm_icc_curve's fields, and for HM_ICC_CURVE_TABLE its `count` big-endian u16 entries inside the profile's bytes (the
// profile must outlive the curve)
struct Curve {
  int kind = HM_ICC_CURVE_IDENTITY, count = 0;
  double p[7] = {0, 0, 0, 0, 0, 0, 0};
  const uint8_t* table = nullptr;
};

struct Profile {
  int major = 0, minor = 0;
  int space = 0;              // HM_ICC_RGB / HM_ICC_GRAY
  bool same_curves = false;   // one tag data for r, g and b
  bool has_cicp = false, cicp_known = false;
  int cicp[4] = {0, 0, 0, 0}; // primaries, transfer, matrix, full range
  double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // the colorants, row-major (column k: r / g / b); GRAY: 0
  Curve curve[3];
};

// HM_OK, or the refusal (hm_fail: HM_ERR_UNSUPPORTED for lack of support, HM_ERR_BITSTREAM for a malformed profile)
int parse(const uint8_t* icc, size_t size, Profile* out);
// Y of the curve at X in [0, 1], clamped to [0, 1]
double eval(const Curve& c, double x);
// lin[v] = (float)(g * eval(c, v / peak)), v = 0 .. peak = (1 << bits) - 1
void fill_table(const Curve& c, int bits, double g, float* out);
// (A T)^-1 M rounded to float32 (to_primaries: a code hm_light::primaries_known); GRAY: the identity
void matrix_to(const Profile& p, int to_primaries, float m[9]);

} // namespace hm_icc

#endif
