// hm_primaries.h — internal: the H.273 codes the light step knows and the RGB -> XYZ matrix of a set of primaries, in double (host
// only, no device code).  Stated once for devdest.cpp (hm_light_matrix, hm_ootf_luma) and icc.cpp (hm_icc_matrix).
#ifndef HM_PRIMARIES_H
#define HM_PRIMARIES_H

#include <cstring>

namespace hm_light {

inline bool transfer_known(int t) { return t == 1 || t == 4 || t == 5 || t == 6 || t == 8 || t == 13 || t == 14 || t == 15 || t == 16 || t == 18; }
inline bool primaries_known(int p) { return p == 1 || p == 5 || p == 6 || p == 7 || p == 9 || p == 12; }

// RGB -> XYZ of a set of primaries (H.273 chromaticities, D65 white), row-major
inline bool primaries_to_xyz(int code, double M[9])
{
  double x[3], y[3];
  switch (code) {
    case 1: x[0] = 0.640; y[0] = 0.330; x[1] = 0.300; y[1] = 0.600; x[2] = 0.150; y[2] = 0.060; break;
    case 5: x[0] = 0.640; y[0] = 0.330; x[1] = 0.290; y[1] = 0.600; x[2] = 0.150; y[2] = 0.060; break;
    case 6: case 7: x[0] = 0.630; y[0] = 0.340; x[1] = 0.310; y[1] = 0.595; x[2] = 0.155; y[2] = 0.070; break;
    case 9: x[0] = 0.708; y[0] = 0.292; x[1] = 0.170; y[1] = 0.797; x[2] = 0.131; y[2] = 0.046; break;
    case 12: x[0] = 0.680; y[0] = 0.320; x[1] = 0.265; y[1] = 0.690; x[2] = 0.150; y[2] = 0.060; break;
    default: return false;
  }
  const double xw = 0.3127, yw = 0.3290;
  double P[9]; // columns: the primaries' XYZ at Y = 1
  for (int k = 0; k < 3; k++) { P[k] = x[k] / y[k]; P[3 + k] = 1.0; P[6 + k] = (1.0 - x[k] - y[k]) / y[k]; }
  const double W[3] = {xw / yw, 1.0, (1.0 - xw - yw) / yw};
  // S = P^-1 W by Cramer's rule
  auto det3 = [](const double* a) { return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]); };
  const double d = det3(P);
  for (int k = 0; k < 3; k++) {
    double Q[9];
    std::memcpy(Q, P, sizeof(Q));
    for (int r = 0; r < 3; r++) Q[3 * r + k] = W[r];
    const double S = det3(Q) / d;
    for (int r = 0; r < 3; r++) M[3 * r + k] = P[3 * r + k] * S;
  }
  return true;
}

inline void invert3(const double a[9], double inv[9])
{
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double d = a[0] * c00 + a[1] * c01 + a[2] * c02;
  inv[0] = c00 / d; inv[1] = (a[2] * a[7] - a[1] * a[8]) / d; inv[2] = (a[1] * a[5] - a[2] * a[4]) / d;
  inv[3] = c01 / d; inv[4] = (a[0] * a[8] - a[2] * a[6]) / d; inv[5] = (a[2] * a[3] - a[0] * a[5]) / d;
  inv[6] = c02 / d; inv[7] = (a[1] * a[6] - a[0] * a[7]) / d; inv[8] = (a[0] * a[4] - a[1] * a[3]) / d;
}

} // namespace hm_light

#endif
