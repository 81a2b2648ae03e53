// light_step.h — the per-pixel rules of the light step (hm_device_light) and of the tone and OOTF steps inside it, stated once (included
// by light.hip, alpha.hip and gain.hip; HIP only; the element rules behind them are out_elem.h's):
//   light_layout where each of the step's tables sits in LDS (host and device: what a launch asks for is what a kernel lays out)
//   fill_tables  tables from global memory into LDS, once per workgroup; fill_light: the step's own, by their layout
//   encode_of    the re-encoding: a count of thresholds by binary search
//   gamut        the 3 x 3 matrix on one pixel's linear light
//   tone_map     the tone step on one pixel's linear light
//   ootf_map     the OOTF step (hm_device_ootf) on one pixel's linear light, in front of the matrix
//   colour_out   linear light of a colour channel to an element of the destination
//   light_in     one pixel's colour samples to linear light
//   light_out    one pixel's linear light to its three colour elements: OOTF step, matrix, tone step, colour_out
// Behind them, on the host: light_of, the dynamic LDS of a launch, and the one check of hm_light_args against a destination plan.
// Every product and sum is rounded on its own (-ffp-contract=off, __fmul_rn / __fadd_rn).
#ifndef HM_LIGHT_STEP_H
#define HM_LIGHT_STEP_H

#include "hm_devdest.h"
#include "out_elem.h"

// ebits: of the codes of enc (bits, or 8 under the 8-bit finish); tone: thr[TONE_STEPS], then sg[TONE_STEPS] (NULL: no tone step);
// ootf: thr[OOTF_STEPS], then sg[OOTF_STEPS] (NULL: no OOTF step), y: the luminance weights of the source primaries;
// lin3: lin is three tables of 1 << bits entries, one per colour channel (an ICC profile with distinct curves), not one
struct Light { const float* lin; const float* enc; const float* tone; const float* ootf; int bits, ebits, encode, matrix; float m[9]; float y[3]; int lin3; };
constexpr int TONE_STEPS = HM_TONE_STEPS;
constexpr int OOTF_STEPS = HM_OOTF_STEPS;

// The step's tables lie in LDS one behind the other: lin[1 << bits] (lin3: three of them, red, green, blue; with_lin: a vertical pass has
// none - its sums are of light already), enc[1 << ebits] when re-encoding, thr and sg of the tone step, thr and sg of the OOTF step.  Offsets in floats; end: all of them.
// thr_only: the statistics pass (stats.hip) searches the tone step's thr and scales by nothing - sg is not laid out (and it never re-encodes).
struct LightLayout { int enc, tone, ootf, end; };
__host__ __device__ inline LightLayout light_layout(bool with_lin, int bits, int ebits, bool encode, bool tone, bool ootf, bool lin3, bool thr_only = false)
{
  LightLayout o;
  o.enc = with_lin ? (lin3 ? 3 : 1) << bits : 0;
  o.tone = o.enc + (encode ? 1 << ebits : 0);
  o.ootf = o.tone + (tone ? (thr_only ? 1 : 2) * TONE_STEPS : 0);
  o.end = o.ootf + (ootf ? 2 * OOTF_STEPS : 0);
  return o;
}
// ... as a kernel sees them: the base in LDS and which layout; a table's place is worked out where the table is used (scalars; a table
// the step does not have is not looked at), as the kernels did before they shared this.  Taken up front as pointers, k_light_v waits
// once more on its kernel arguments: 14.8 against 14.1 us (profiles/step_kernels_refactor.txt).
struct LightTables {
  const float* lds; bool with_lin; bool thr_only = false;
  __device__ __forceinline__ LightLayout at(const Light& L) const { return light_layout(with_lin, L.bits, L.ebits, L.encode, L.tone, L.ootf, L.lin3, thr_only); }
  __device__ __forceinline__ const float* lin() const { return lds; }
  __device__ __forceinline__ const float* enc(const Light& L) const { return lds + at(L).enc; }
  __device__ __forceinline__ const float* tone(const Light& L) const { return lds + at(L).tone; }
  __device__ __forceinline__ const float* ootf(const Light& L) const { return lds + at(L).ootf; }
};

// a[na], b[nb], c[nc], d[nd] (each may be NULL: nothing is copied, its place stays) -> lds, one behind the other; every thread of the
// workgroup comes here
__device__ __forceinline__ void fill_tables(float* lds, const float* __restrict__ a, int na, const float* __restrict__ b = nullptr, int nb = 0,
                                            const float* __restrict__ c = nullptr, int nc = 0, const float* __restrict__ d = nullptr, int nd = 0)
{
  if (a) for (int i = threadIdx.x; i < na; i += 256) lds[i] = a[i];
  if (b) for (int i = threadIdx.x; i < nb; i += 256) lds[na + i] = b[i];
  if (c) for (int i = threadIdx.x; i < nc; i += 256) lds[na + nb + i] = c[i];
  if (d) for (int i = threadIdx.x; i < nd; i += 256) lds[na + nb + nc + i] = d[i];
  __syncthreads();
}

// the step's tables into LDS by light_layout, every one or (no lin) a vertical pass's; every thread of the workgroup comes here
// thr_only (the statistics pass; with_lin): of the tone step thr alone - sg lies behind it in global memory and is not loaded
__device__ __forceinline__ LightTables fill_light(float* lds, const Light& L, bool with_lin, bool thr_only = false)
{
  const int ne = L.encode ? 1 << L.ebits : 0, nt = L.tone ? (thr_only ? 1 : 2) * TONE_STEPS : 0;
  if (with_lin) fill_tables(lds, L.lin, (L.lin3 ? 3 : 1) << L.bits, L.enc, ne, L.tone, nt, L.ootf, 2 * OOTF_STEPS);
  else if (L.encode || L.tone || L.ootf) fill_tables(lds, L.enc, ne, L.tone, nt, L.ootf, 2 * OOTF_STEPS); // (uniform: the barrier inside is met by every thread or by none)
  return LightTables{lds, with_lin, thr_only};
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

// linear light r of a colour channel to an element of the destination; enc: the threshold table in LDS
template <typename OutT> __device__ __forceinline__ OutT colour_out(const Light& L, const float* enc, float r, float sc, float bi)
{
  if (L.encode) return moved<OutT>(encode_of(enc, L.ebits, r), sc, bi);
  return linear_out<OutT>(r, sc, bi);
}

// a pixel's colour samples to linear light: lin at the sample, clamped to the table; lin3 (wave-uniform, as the step's other options
// are): channel c in its own table, lin[(c << bits) + min(v, peak)]
template <typename Tables> __device__ __forceinline__ void light_in(const Light& L, const Tables& T, const unsigned v[3], float r[3])
{
  const unsigned peak = (1u << L.bits) - 1u;
  if (L.lin3) {
    r[0] = T.lin()[min(v[0], peak)]; r[1] = T.lin()[(1u << L.bits) + min(v[1], peak)]; r[2] = T.lin()[(2u << L.bits) + min(v[2], peak)];
    return;
  }
  r[0] = T.lin()[min(v[0], peak)]; r[1] = T.lin()[min(v[1], peak)]; r[2] = T.lin()[min(v[2], peak)];
}

// the sample-to-float step of a horizontal pass (k_light_h, k_alpha_h), which holds lin alone: the colour channels through lin (in LDS)
struct LinLookup {
  const float* lin; unsigned peak;
  __device__ __forceinline__ float colour(unsigned v, int) const { return lin[min(v, peak)]; }
  __device__ __forceinline__ float operator()(unsigned v, int c) const { return c < 3 ? colour(v, c) : (float)v; } // (alpha: converted as it is)
};
// ... with a table per channel
struct LinLookup3 {
  const float* lin; unsigned peak; int bits;
  __device__ __forceinline__ float colour(unsigned v, int c) const { return lin[((unsigned)c << bits) + min(v, peak)]; }
  __device__ __forceinline__ float operator()(unsigned v, int c) const { return c < 3 ? colour(v, c) : (float)v; }
};

// one pixel's linear light r (changed in place) to its three colour elements: what every kernel of the step does behind its lookups or
// its sums, each part a wave-uniform branch on a kernel argument.  OOTF false: a kernel that never meets the OOTF step (the gain step's:
// the host refuses the two together) does not carry its search.  Tables: LightTables, or whatever else answers enc(L), tone(L) and ootf(L).
template <bool OOTF = true, typename Tables, typename OutT> __device__ __forceinline__ void light_out(const Light& L, const Tables& T, float r[3], const Affine& a, OutT o[3])
{
  if (OOTF && L.ootf) ootf_map(L, T.ootf(L), r);
  gamut(L, r);
  if (L.tone) tone_map(T.tone(L), r);
#pragma unroll
  for (int c = 0; c < 3; c++) o[c] = colour_out<OutT>(L, T.enc(L), r[c], a.scale[c], a.bias[c]);
}

// ---- host ----
static inline Light light_of(const hm_light_args* la)
{
  Light L;
  L.lin = la->lin; L.enc = la->enc; L.tone = la->tone; L.ootf = la->ootf; L.bits = la->bits; L.ebits = la->enc_bits; L.encode = la->encode; L.matrix = la->matrix; L.lin3 = la->lin3;
  for (int i = 0; i < 9; i++) L.m[i] = la->m[i];
  for (int i = 0; i < 3; i++) L.y[i] = la->y[i];
  return L;
}
// the dynamic LDS of a launch: the pointwise and nearest kernels hold lin, enc, the tone and the OOTF tables, a horizontal pass lin, a
// vertical pass enc, the tone and the OOTF tables - with one lin at most 16 + 16 + 16 + 8 = 56 KB; with three, what check_light_lds lets pass
static inline size_t light_layout_bytes(const hm_light_args* la, bool with_lin)
{
  return (size_t)light_layout(with_lin, la->bits, la->enc_bits, la->encode != 0, la->tone != nullptr, la->ootf != nullptr, la->lin3 != 0).end * sizeof(float);
}
static inline size_t light_h_bytes(const hm_light_args* la) { return (size_t)(la->lin3 ? 12 : 4) << la->bits; }
static inline size_t light_v_bytes(const hm_light_args* la) { return light_layout_bytes(la, false); }
static inline size_t light_tables_bytes(const hm_light_args* la) { return light_layout_bytes(la, true); }
// the statistics pass: lin, thr of the tone step, the OOTF tables; behind them its histogram and the word of its maximum (padded to 16 bytes)
enum { LIGHT_STATS_WORDS = HM_LIGHT_STATS_BINS + 4 };
static inline size_t light_stats_bytes(const hm_light_args* la)
{
  return ((size_t)light_layout(true, la->bits, la->enc_bits, false, true, la->ootf != nullptr, la->lin3 != 0, true).end + LIGHT_STATS_WORDS) * sizeof(float);
}

// What a launch may ask for as dynamic LDS: 64 KB, what a workgroup gets without the launch opting in to more (the CU has 160 KB; no
// launch here opts in).  Only three lin tables reach it: 12-bit samples with a 12-bit re-encoding and a tone step are 48 + 16 + 16 KB.
// The one host check of it - the plan asks before anything is queued (hm_light_lds_check), every launcher asks again.
// pass 0: k_*_tensor / k_*_nearest, 1: a horizontal pass, 2: a vertical pass, 3: the statistics pass (k_light_stats: whatever la says of enc
// and the tone step, it holds lin, thr, the OOTF tables and its histogram - 12-bit samples through three curves are 48 + 8 + 8 KB and a word)
enum { LIGHT_LDS_MOST = 64 * 1024 };
static inline size_t light_pass_bytes(const hm_light_args* la, int pass)
{
  return pass == 0 ? light_tables_bytes(la) : pass == 1 ? light_h_bytes(la) : pass == 2 ? light_v_bytes(la) : light_stats_bytes(la);
}
static inline int check_light_lds(const hm_light_args* la, int pass)
{
  const size_t bytes = light_pass_bytes(la, pass);
  if (bytes <= (size_t)LIGHT_LDS_MOST) return HM_OK;
  if (pass == 3)
    return hm_fail(HM_ERR_UNSUPPORTED, "light statistics: %d-bit samples through %s with%s in one kernel need %zu bytes of local memory for their tables and the histogram (%d fit): not supported",
                   la->bits, la->lin3 ? "three distinct curves of the ICC profile" : "one curve", la->ootf ? " an OOTF step" : " no OOTF step", bytes, (int)LIGHT_LDS_MOST);
  return hm_fail(HM_ERR_UNSUPPORTED, "light: %d-bit samples through %s with%s%s%s in one kernel need %zu bytes of local memory for their tables (%d fit): not supported", la->bits,
                 la->lin3 ? "three distinct curves of the ICC profile" : "one curve", la->encode ? (la->enc_bits == 8 ? " a re-encoding to 8-bit codes," : " a re-encoding,") : "",
                 la->tone ? " a tone step," : "", la->ootf ? " an OOTF step," : " no OOTF step,", bytes, (int)LIGHT_LDS_MOST);
}

// hm_light_args against p, the plan of the target the destination is written as (under the 8-bit finish its samples are bytes, the
// source's are not); k: the kernel family, for the message
static inline int check_light_args(const char* k, const hm_dest_plan* p, const hm_light_args* la)
{
  if (!la->lin || (la->encode && !la->enc) || la->bits < 8 || la->bits > 12 || (la->lin3 != 0 && la->lin3 != 1)) return hm_fail(HM_ERR_INTERNAL, "%s: tables of %d bits", k, la->bits);
  if (la->enc_bits != la->bits && la->enc_bits != 8) return hm_fail(HM_ERR_INTERNAL, "%s: codes of %d bits from tables of %d", k, la->enc_bits, la->bits);
  if (la->src_bytes != (la->bits > 8 ? 2 : 1)) return hm_fail(HM_ERR_INTERNAL, "%s: %d-byte samples of %d bits", k, la->src_bytes, la->bits);
  if (p->channels != 3 && p->channels != 4) return hm_fail(HM_ERR_INTERNAL, "%s: %d channels", k, p->channels);
  if (p->sample_bytes != (la->enc_bits > 8 ? 2 : 1) || (p->sample_bytes != la->src_bytes && p->channels != 3))
    return hm_fail(HM_ERR_INTERNAL, "%s: a %d-byte target of %d channels from %d-byte samples, codes of %d bits", k, p->sample_bytes, p->channels, la->src_bytes, la->enc_bits);
  const bool integer = p->dtype == HM_DEV_U8 || p->dtype == HM_DEV_U16;
  if (integer && (!la->encode || p->dtype != (p->sample_bytes == 1 ? HM_DEV_U8 : HM_DEV_U16)))
    return hm_fail(HM_ERR_INTERNAL, "%s: integer dtype %d on %d-byte samples, %s", k, p->dtype, p->sample_bytes, la->encode ? "re-encoded" : "linear");
  return HM_OK;
}

#endif
