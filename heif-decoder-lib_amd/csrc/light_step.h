// light_step.h — the per-pixel rules of the light step (hm_device_light) and of the tone step inside it, stated once (included by
// light.hip and alpha.hip; HIP only; the element rules behind them are out_elem.h's):
//   fill_tables  the step's tables from global memory into LDS, once per workgroup
//   encode_of    the re-encoding: a count of thresholds by binary search
//   gamut        the 3 x 3 matrix on one pixel's linear light
//   tone_map     the tone step on one pixel's linear light
//   ootf_map     the OOTF step (hm_device_ootf) on one pixel's linear light, in front of the matrix
//   colour_out   linear light of a colour channel to an element of the destination
// Every product and sum is rounded on its own (-ffp-contract=off, __fmul_rn / __fadd_rn).
#ifndef HM_LIGHT_STEP_H
#define HM_LIGHT_STEP_H

#include "hm_devdest.h"
#include "out_elem.h"

// ebits: of the codes of enc (bits, or 8 under the 8-bit finish); tone: thr[TONE_STEPS], then sg[TONE_STEPS] (NULL: no tone step);
// ootf: thr[OOTF_STEPS], then sg[OOTF_STEPS] (NULL: no OOTF step), y: the luminance weights of the source primaries
struct Light { const float* lin; const float* enc; const float* tone; const float* ootf; int bits, ebits, encode, matrix; float m[9]; float y[3]; };
constexpr int TONE_STEPS = HM_TONE_STEPS;
constexpr int OOTF_STEPS = HM_OOTF_STEPS;

// a[na], b[nb], c[nc], d[nd] (each may be NULL: nothing is copied, its place stays) -> lds, one behind the other; every thread of the
// workgroup comes here
__device__ __forceinline__ void fill_tables(float* lds, const float* __restrict__ a, int na, const float* __restrict__ b, int nb, const float* __restrict__ c, int nc,
                                            const float* __restrict__ d = nullptr, int nd = 0)
{
  if (a) for (int i = threadIdx.x; i < na; i += 256) lds[i] = a[i];
  if (b) for (int i = threadIdx.x; i < nb; i += 256) lds[na + i] = b[i];
  if (c) for (int i = threadIdx.x; i < nc; i += 256) lds[na + nb + i] = c[i];
  if (d) for (int i = threadIdx.x; i < nd; i += 256) lds[na + nb + nc + i] = d[i];
  __syncthreads();
}

// |{c in 1 .. peak : enc[c] <= r}|: enc rises, so the count is the largest c whose threshold r has reached (0: none; a NaN: none)
__device__ __forceinline__ unsigned encode_of(const float* enc, int bits, float r)
{
  int code = 0;
  for (int step = 1 << (bits - 1); step; step >>= 1) { // (code + step <= peak: the steps sum to it)
    const int t = code + step;
    if (enc[t] <= r) code = t;
  }
  return (unsigned)code;
}

__device__ __forceinline__ void gamut(const Light& L, float r[3])
{
  if (!L.matrix) return;
  const float R = r[0], G = r[1], B = r[2];
  r[0] = __fadd_rn(__fadd_rn(__fmul_rn(L.m[0], R), __fmul_rn(L.m[1], G)), __fmul_rn(L.m[2], B));
  r[1] = __fadd_rn(__fadd_rn(__fmul_rn(L.m[3], R), __fmul_rn(L.m[4], G)), __fmul_rn(L.m[5], B));
  r[2] = __fadd_rn(__fadd_rn(__fmul_rn(L.m[6], R), __fmul_rn(L.m[7], G)), __fmul_rn(L.m[8], B));
}

// the tone step on one pixel's linear light; tl: thr, then sg, in LDS
__device__ __forceinline__ void tone_map(const float* tl, float r[3])
{
  const float N = fmaxf(fmaxf(r[0], r[1]), r[2]);
  int k = 0;
  for (int step = TONE_STEPS >> 1; step; step >>= 1) { // (k + step <= TONE_STEPS - 1: the steps sum to it)
    const int t = k + step;
    if (tl[t] <= N) k = t;
  }
  const float g = tl[TONE_STEPS + k];
  r[0] = __fmul_rn(r[0], g); r[1] = __fmul_rn(r[1], g); r[2] = __fmul_rn(r[2], g);
}

// the OOTF step on one pixel's linear light (scene light), in front of the matrix; ol: thr, then sg, in LDS (behind the tone step's
// tables where there are any); a negative or NaN Ys counts no threshold
__device__ __forceinline__ void ootf_map(const Light& L, const float* ol, float r[3])
{
  const float Ys = __fadd_rn(__fadd_rn(__fmul_rn(L.y[0], r[0]), __fmul_rn(L.y[1], r[1])), __fmul_rn(L.y[2], r[2]));
  int k = 0;
  for (int step = OOTF_STEPS >> 1; step; step >>= 1) { // (k + step <= OOTF_STEPS - 1: the steps sum to it)
    const int t = k + step;
    if (ol[t] <= Ys) k = t;
  }
  const float g = ol[OOTF_STEPS + k];
  r[0] = __fmul_rn(r[0], g); r[1] = __fmul_rn(r[1], g); r[2] = __fmul_rn(r[2], g);
}
// where the OOTF tables sit behind enc (vl: enc, then thr and sg of the tone step, then those of the OOTF step)
__device__ __forceinline__ const float* ootf_tables(const Light& L, const float* vl) { return vl + (L.encode ? 1 << L.ebits : 0) + (L.tone ? 2 * TONE_STEPS : 0); }

// linear light r of a colour channel to an element of the destination; enc: the threshold table in LDS
template <typename OutT> __device__ __forceinline__ OutT colour_out(const Light& L, const float* enc, float r, float sc, float bi)
{
  if (L.encode) return moved<OutT>(encode_of(enc, L.ebits, r), sc, bi);
  return linear_out<OutT>(r, sc, bi);
}

// ---- host ----
static inline Light light_of(const hm_light_args* la)
{
  Light L;
  L.lin = la->lin; L.enc = la->enc; L.tone = la->tone; L.ootf = la->ootf; L.bits = la->bits; L.ebits = la->enc_bits; L.encode = la->encode; L.matrix = la->matrix;
  for (int i = 0; i < 9; i++) L.m[i] = la->m[i];
  for (int i = 0; i < 3; i++) L.y[i] = la->y[i];
  return L;
}
// the dynamic LDS of a launch: the pointwise and nearest kernels hold lin, enc, the tone and the OOTF tables, a horizontal pass lin, a
// vertical pass enc, the tone and the OOTF tables - at most 16 + 16 + 16 + 8 = 56 KB
static inline size_t light_tone_bytes(const hm_light_args* la) { return la->tone ? 2 * (size_t)TONE_STEPS * sizeof(float) : 0; }
static inline size_t light_ootf_bytes(const hm_light_args* la) { return la->ootf ? 2 * (size_t)OOTF_STEPS * sizeof(float) : 0; }
static inline size_t light_h_bytes(const hm_light_args* la) { return (size_t)4 << la->bits; }
static inline size_t light_v_bytes(const hm_light_args* la) { return (la->encode ? (size_t)4 << la->enc_bits : 0) + light_tone_bytes(la) + light_ootf_bytes(la); }
static inline size_t light_tables_bytes(const hm_light_args* la) { return light_h_bytes(la) + light_v_bytes(la); }

#endif
