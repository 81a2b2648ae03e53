// icc.cpp — the ICC profile reader of the light step (hm_icc.h; the rules: include/heif_mi355x.h, "ICC").  Host arithmetic only.
// Every read goes through Bytes, which knows the profile's own size: nothing outside [0, size) is touched.
#include <cmath>
#include <cstring>

#include "hm_icc.h"
#include "hm_internal.h"
#include "hm_primaries.h"

namespace hm_icc {

namespace {

constexpr uint32_t sig(char a, char b, char c, char d) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d; }

// the profile's bytes; the callers have checked every offset they pass against n
struct Bytes {
  const uint8_t* p; size_t n;
  uint32_t u32(size_t o) const { return ((uint32_t)p[o] << 24) | ((uint32_t)p[o + 1] << 16) | ((uint32_t)p[o + 2] << 8) | (uint32_t)p[o + 3]; }
  uint32_t u16(size_t o) const { return ((uint32_t)p[o] << 8) | (uint32_t)p[o + 1]; }
  double s15f16(size_t o) const { return (double)(int32_t)u32(o) / 65536.0; }
};

struct Tag { uint32_t off = 0, size = 0; bool present = false; };

const char* sig_text(uint32_t s, char out[5])
{
  for (int i = 0; i < 4; i++) { const int c = (int)((s >> (24 - 8 * i)) & 0xFF); out[i] = c >= 32 && c < 127 ? (char)c : '?'; }
  out[4] = 0;
  return out;
}

int read_xyz(const Bytes& b, const Tag& t, const char* name, double out[3])
{
  char txt[5];
  if (!t.present) return hm_fail(HM_ERR_BITSTREAM, "icc: no %s tag", name);
  if (t.size < 8) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s tag holds %u bytes", name, t.size);
  if (b.u32(t.off) != sig('X', 'Y', 'Z', ' ')) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s tag has type '%s', not 'XYZ '", name, sig_text(b.u32(t.off), txt));
  if (t.size < 20) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s tag holds %u bytes, an XYZ number takes 20", name, t.size);
  for (int k = 0; k < 3; k++) out[k] = b.s15f16(t.off + 8 + 4 * (size_t)k);
  return HM_OK;
}

int read_curve(const Bytes& b, const Tag& t, const char* name, Curve* c)
{
  char txt[5];
  *c = Curve();
  if (!t.present) return hm_fail(HM_ERR_BITSTREAM, "icc: no %s tag", name);
  if (t.size < 12) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s tag holds %u bytes", name, t.size);
  const uint32_t type = b.u32(t.off);
  if (type == sig('c', 'u', 'r', 'v')) {
    const uint32_t n = b.u32(t.off + 8);
    if ((uint64_t)12 + 2 * (uint64_t)n > t.size) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve of %u entries runs past its tag of %u bytes", name, n, t.size);
    if (n > 0x7FFFFFFFu) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve has %u entries", name, n);
    c->count = (int)n;
    if (n == 0) c->kind = HM_ICC_CURVE_IDENTITY;
    else if (n == 1) { c->kind = HM_ICC_CURVE_GAMMA; c->p[0] = (double)b.u16(t.off + 12) / 256.0; }
    else { c->kind = HM_ICC_CURVE_TABLE; c->table = b.p + t.off + 12; }
    return HM_OK;
  }
  if (type == sig('p', 'a', 'r', 'a')) {
    const uint32_t f = b.u16(t.off + 8);
    static const int params[5] = {1, 3, 4, 5, 7};
    if (f > 4) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve has the parametric function type %u (0 .. 4 exist)", name, f);
    if ((uint32_t)(12 + 4 * params[f]) > t.size) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve of function type %u runs past its tag of %u bytes", name, f, t.size);
    c->kind = HM_ICC_CURVE_PARA; c->count = (int)f;
    for (int k = 0; k < params[f]; k++) c->p[k] = b.s15f16(t.off + 12 + 4 * (size_t)k);
    if (!(c->p[0] > 0.0)) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve has the exponent g = %g (it must be above 0)", name, c->p[0]);
    if ((f == 1 || f == 2) && c->p[1] == 0.0) return hm_fail(HM_ERR_BITSTREAM, "icc: the %s curve of function type %u has a = 0", name, f);
    return HM_OK;
  }
  return hm_fail(HM_ERR_BITSTREAM, "icc: the %s tag has type '%s', not 'curv' or 'para'", name, sig_text(type, txt));
}

} // namespace

int parse(const uint8_t* icc, size_t size, Profile* out)
{
  char txt[5];
  *out = Profile();
  if (size < 132) return hm_fail(HM_ERR_BITSTREAM, "icc: %zu bytes are less than a header and a tag count", size);
  Bytes b{icc, size};
  const uint32_t declared = b.u32(0);
  if (declared > size) return hm_fail(HM_ERR_BITSTREAM, "icc: the size field says %u bytes, %zu were given", declared, size);
  if (declared < 132) return hm_fail(HM_ERR_BITSTREAM, "icc: the size field says %u bytes, less than a header and a tag count", declared);
  b.n = declared; // (what lies behind the profile's own size is not the profile)
  if (b.u32(36) != sig('a', 'c', 's', 'p')) return hm_fail(HM_ERR_BITSTREAM, "icc: the header signature is '%s', not 'acsp'", sig_text(b.u32(36), txt));
  out->major = icc[8]; out->minor = icc[9] >> 4;
  if (out->major == 5) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a version 5 profile (iccMAX) is not supported");
  if (out->major != 2 && out->major != 4) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a version %d profile is not supported (2.x and 4.x are)", out->major);
  const uint32_t cls = b.u32(12), space = b.u32(16), pcs = b.u32(20);
  if (cls == sig('l', 'i', 'n', 'k')) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a device link profile is not supported");
  if (cls == sig('a', 'b', 's', 't')) return hm_fail(HM_ERR_UNSUPPORTED, "icc: an abstract profile is not supported");
  if (cls == sig('n', 'm', 'c', 'l')) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a named-colour profile is not supported");
  if (cls != sig('m', 'n', 't', 'r') && cls != sig('s', 'c', 'n', 'r') && cls != sig('s', 'p', 'a', 'c'))
    return hm_fail(HM_ERR_UNSUPPORTED, "icc: a profile of class '%s' is not supported ('mntr', 'scnr' and 'spac' are)", sig_text(cls, txt));
  if (space != sig('R', 'G', 'B', ' ') && space != sig('G', 'R', 'A', 'Y'))
    return hm_fail(HM_ERR_UNSUPPORTED, "icc: the data colour space '%s' is not supported ('RGB ' and 'GRAY' are)", sig_text(space, txt));
  if (pcs == sig('L', 'a', 'b', ' ')) return hm_fail(HM_ERR_UNSUPPORTED, "icc: the connection space Lab is not supported ('XYZ ' is)");
  if (pcs != sig('X', 'Y', 'Z', ' ')) return hm_fail(HM_ERR_UNSUPPORTED, "icc: the connection space '%s' is not supported ('XYZ ' is)", sig_text(pcs, txt));
  out->space = space == sig('R', 'G', 'B', ' ') ? HM_ICC_RGB : HM_ICC_GRAY;

  const uint32_t count = b.u32(128);
  const uint64_t table_end = 132 + 12 * (uint64_t)count;
  if (table_end > b.n) return hm_fail(HM_ERR_BITSTREAM, "icc: the tag table of %u tags runs past the profile's %zu bytes", count, b.n);
  Tag rXYZ, gXYZ, bXYZ, rTRC, gTRC, bTRC, kTRC, cicp;
  bool lut = false;
  for (uint32_t i = 0; i < count; i++) {
    const size_t e = 132 + 12 * (size_t)i;
    const uint32_t s = b.u32(e), off = b.u32(e + 4), sz = b.u32(e + 8);
    if ((uint64_t)off < table_end) return hm_fail(HM_ERR_BITSTREAM, "icc: the '%s' tag at offset %u overlaps the header or the tag table", sig_text(s, txt), off);
    if ((uint64_t)off + sz > b.n) return hm_fail(HM_ERR_BITSTREAM, "icc: the '%s' tag (offset %u, %u bytes) runs past the profile's %zu bytes", sig_text(s, txt), off, sz, b.n);
    Tag* t = s == sig('r', 'X', 'Y', 'Z')   ? &rXYZ
             : s == sig('g', 'X', 'Y', 'Z') ? &gXYZ
             : s == sig('b', 'X', 'Y', 'Z') ? &bXYZ
             : s == sig('r', 'T', 'R', 'C') ? &rTRC
             : s == sig('g', 'T', 'R', 'C') ? &gTRC
             : s == sig('b', 'T', 'R', 'C') ? &bTRC
             : s == sig('k', 'T', 'R', 'C') ? &kTRC
             : s == sig('c', 'i', 'c', 'p') ? &cicp
                                            : nullptr;
    if (s == sig('A', '2', 'B', '0') || s == sig('A', '2', 'B', '1') || s == sig('A', '2', 'B', '2') || s == sig('B', '2', 'A', '0')) lut = true;
    if (t && !t->present) { t->off = off; t->size = sz; t->present = true; } // (a signature listed twice: the first one counts)
  }

  int rc;
  if (cicp.present) {
    if (cicp.size < 12) return hm_fail(HM_ERR_BITSTREAM, "icc: the cicp tag holds %u bytes, it takes 12", cicp.size);
    if (b.u32(cicp.off) != sig('c', 'i', 'c', 'p')) return hm_fail(HM_ERR_BITSTREAM, "icc: the cicp tag has type '%s', not 'cicp'", sig_text(b.u32(cicp.off), txt));
    out->has_cicp = true;
    for (int k = 0; k < 4; k++) out->cicp[k] = icc[cicp.off + 8 + k];
    out->cicp_known = hm_light::primaries_known(out->cicp[0]) && hm_light::transfer_known(out->cicp[1]);
  }
  if (out->space == HM_ICC_GRAY) {
    if (!kTRC.present && lut) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a profile with lookup tables (A2B0) and no kTRC curve is not supported");
    if ((rc = read_curve(b, kTRC, "kTRC", &out->curve[0]))) return rc;
    out->curve[1] = out->curve[2] = out->curve[0];
    out->same_curves = true;
    return HM_OK;
  }
  const bool any = rXYZ.present || gXYZ.present || bXYZ.present || rTRC.present || gTRC.present || bTRC.present;
  if (!any && lut) return hm_fail(HM_ERR_UNSUPPORTED, "icc: a profile with lookup tables (A2B0) and no matrix/TRC set is not supported");
  const Tag* xyz[3] = {&rXYZ, &gXYZ, &bXYZ};
  const Tag* trc[3] = {&rTRC, &gTRC, &bTRC};
  static const char* const xyz_name[3] = {"rXYZ", "gXYZ", "bXYZ"};
  static const char* const trc_name[3] = {"rTRC", "gTRC", "bTRC"};
  for (int k = 0; k < 3; k++) {
    double col[3];
    if ((rc = read_xyz(b, *xyz[k], xyz_name[k], col))) return rc;
    for (int r = 0; r < 3; r++) out->M[3 * r + k] = col[r];
  }
  for (int k = 0; k < 3; k++)
    if ((rc = read_curve(b, *trc[k], trc_name[k], &out->curve[k]))) return rc;
  auto same = [&](const Tag& x, const Tag& y) { return x.size == y.size && (x.off == y.off || std::memcmp(b.p + x.off, b.p + y.off, x.size) == 0); };
  out->same_curves = same(rTRC, gTRC) && same(rTRC, bTRC);
  return HM_OK;
}

double eval(const Curve& c, double x)
{
  double y = x;
  if (c.kind == HM_ICC_CURVE_GAMMA) y = std::pow(x, c.p[0]);
  else if (c.kind == HM_ICC_CURVE_TABLE) {
    const int n = c.count;
    const double pos = x * (double)(n - 1);
    int i = (int)pos;
    if (i > n - 2) i = n - 2;
    if (i < 0) i = 0;
    const double t0 = (double)(((unsigned)c.table[2 * (size_t)i] << 8) | c.table[2 * (size_t)i + 1]) / 65535.0;
    const double t1 = (double)(((unsigned)c.table[2 * (size_t)i + 2] << 8) | c.table[2 * (size_t)i + 3]) / 65535.0;
    y = t0 + (pos - (double)i) * (t1 - t0);
  }
  else if (c.kind == HM_ICC_CURVE_PARA) {
    const double g = c.p[0], a = c.p[1], bb = c.p[2], cc = c.p[3], d = c.p[4], e = c.p[5], f = c.p[6];
    auto P = [&](double X) { const double base = a * X + bb; return std::pow(base > 0.0 ? base : 0.0, g); };
    switch (c.count) {
      case 0: y = std::pow(x, g); break;
      case 1: y = x >= -bb / a ? P(x) : 0.0; break;
      case 2: y = x >= -bb / a ? P(x) + cc : cc; break;
      case 3: y = x >= d ? P(x) : cc * x; break;
      default: y = x >= d ? P(x) + e : cc * x + f; break;
    }
  }
  return y >= 1.0 ? 1.0 : y > 0.0 ? y : 0.0; // (a NaN cannot arise: finite parameters, g > 0)
}

void fill_table(const Curve& c, int bits, double g, float* out)
{
  const int n = 1 << bits;
  const double peak = (double)(n - 1);
  for (int v = 0; v < n; v++) out[v] = (float)(g * eval(c, (double)v / peak));
}

void matrix_to(const Profile& p, int to_primaries, float m[9])
{
  if (p.space == HM_ICC_GRAY) { for (int i = 0; i < 9; i++) m[i] = i % 4 == 0 ? 1.0f : 0.0f; return; }
  static const double B[9] = {0.8951, 0.2664, -0.1614, -0.7502, 1.7135, 0.0367, 0.0389, -0.0685, 1.0296};
  const double xw = 0.3127, yw = 0.3290;
  const double W[3] = {xw / yw, 1.0, (1.0 - xw - yw) / yw};
  const double I[3] = {(double)0xF6D6 / 65536.0, 1.0, (double)0xD32D / 65536.0};
  auto mul = [](const double* a, const double* b, double* o) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
  };
  double Bi[9], D[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, DB[9], A[9], T[9], AT[9], ATi[9];
  hm_light::invert3(B, Bi);
  for (int k = 0; k < 3; k++) {
    const double ci = B[3 * k] * I[0] + B[3 * k + 1] * I[1] + B[3 * k + 2] * I[2], cw = B[3 * k] * W[0] + B[3 * k + 1] * W[1] + B[3 * k + 2] * W[2];
    D[4 * k] = ci / cw;
  }
  mul(D, B, DB);
  mul(Bi, DB, A);
  hm_light::primaries_to_xyz(to_primaries, T);
  mul(A, T, AT);
  hm_light::invert3(AT, ATi);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) m[3 * r + c] = (float)(ATi[3 * r] * p.M[c] + ATi[3 * r + 1] * p.M[3 + c] + ATi[3 * r + 2] * p.M[6 + c]);
}

} // namespace hm_icc

extern "C" {

int hm_icc_parse(const uint8_t* icc, size_t size, hm_icc_info* out)
{
  if (!icc || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  std::memset(out, 0, sizeof(*out));
  hm_icc::Profile p;
  const int rc = hm_icc::parse(icc, size, &p);
  if (rc) return rc;
  out->version_major = p.major; out->version_minor = p.minor; out->colour_space = p.space; out->same_curves = p.same_curves ? 1 : 0;
  out->has_cicp = p.has_cicp ? 1 : 0; out->cicp_known = p.cicp_known ? 1 : 0;
  for (int k = 0; k < 4; k++) out->cicp[k] = p.cicp[k];
  for (int k = 0; k < 9; k++) out->colorant[k] = p.M[k];
  for (int c = 0; c < 3; c++) {
    out->curve[c].kind = p.curve[c].kind; out->curve[c].count = p.curve[c].count;
    for (int k = 0; k < 7; k++) out->curve[c].p[k] = p.curve[c].p[k];
  }
  return HM_OK;
}

int hm_icc_table(const uint8_t* icc, size_t size, int channel, int bits, float gain, float* out)
{
  if (!icc || !out) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (channel < 0 || channel > 2) return hm_fail(HM_ERR_INVALID_ARG, "icc: channel %d is not 0 .. 2", channel);
  if (bits < 8 || bits > 12) return hm_fail(HM_ERR_UNSUPPORTED, "light: samples of %d bits (8 .. 12 are supported)", bits);
  if (!std::isfinite(gain) || !(gain > 0.0f)) return hm_fail(HM_ERR_INVALID_ARG, "light: gain %g is not finite and above 0", (double)gain);
  hm_icc::Profile p;
  const int rc = hm_icc::parse(icc, size, &p);
  if (rc) return rc;
  hm_icc::fill_table(p.curve[channel], bits, (double)gain, out);
  return 1 << bits;
}

int hm_icc_matrix(const uint8_t* icc, size_t size, int to_primaries, float m[9])
{
  if (!icc || !m) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (!hm_light::primaries_known(to_primaries)) return hm_fail(HM_ERR_UNSUPPORTED, "light: colour primaries %d are not supported", to_primaries);
  hm_icc::Profile p;
  const int rc = hm_icc::parse(icc, size, &p);
  if (rc) return rc;
  hm_icc::matrix_to(p, to_primaries, m);
  return HM_OK;
}

} // extern "C"
