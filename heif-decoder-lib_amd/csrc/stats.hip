// stats.hip — the light statistics (hm_light_stats, include/heif_mi355x.h "Light statistics") of interleaved pixels (gfx950): the one
// kernel here that reduces a picture to numbers.  Every pixel of a rectangle goes through the light step's own rules up to the tone
// step's search - light_in, ootf_map, gamut, the max of R, G and B, the count of thresholds in thr[] (light_step.h, unchanged) - and is
// counted in the bin of its code; beside the histogram the largest norm is kept by its bit pattern (a float above 0 orders like the
// unsigned word it is stored as).
//   k_light_stats<SB, C, VEC>  ONE launch.  Workgroups of 4 waves are persistent: the rectangle is cut into tasks of 64 consecutive pixel
//                    groups of ONE row (the pointwise kernels' row shape: a lane's group is 8 pixels, loaded with 16-byte loads - 8-byte
//                    ones for three 8-bit channels - where pointer and stride allow, the scalar instance otherwise), and wave i of the
//                    launch takes tasks i, i + waves, ... - the grid comes from the device's CU count (hm_launch_light_stats), not
//                    from the picture, so the number of flushes is bounded whatever the size.
// LDS: lin (three of them under lin3), thr of the tone step - sg and enc are not loaded: light_layout's thr_only -, the OOTF tables, then
// 2048 counters and the word of the workgroup's maximum; at most 64 KB (check_light_lds, pass 3).  A pixel is one ds_add_u32 without
// return.  Lanes of a wave that meet the same bin serialise in the LDS atomic unit, yet a flat picture is the FAST case: its table reads
// and its search are broadcasts, where noise meets bank conflicts in both - 70.7 against 96.8 us at 12 MP (profiles/light_stats.txt) -, so
// equal bins of a wave are not aggregated.  The maximum is kept per lane over all of a wave's tasks,
// reduced across the wave once, and costs one LDS atomicMax per wave.  At the end of the workgroup the non-zero bins go to the global
// histogram with device-scope integer atomicAdd and the maximum with one atomicMax: integer sums and a maximum, no result depends on
// the order of arrival.
#include <algorithm>

#include "hm_devdest.h"
#include "light_step.h"
#include "out_launch.h"

namespace {

constexpr int STATS_P = 8; // pixels of a lane's group

// one pixel: its code is counted, its norm is folded into the lane's maximum
template <int C> __device__ __forceinline__ void measure(const Light& L, const LightTables& T, const unsigned (&v)[C], unsigned* hist, unsigned& most)
{
  float r[3];
  light_in(L, T, v, r);
  if (L.ootf) ootf_map(L, T.ootf(L), r);
  gamut(L, r);
  const float N = fmaxf(fmaxf(r[0], r[1]), r[2]);
  const float* thr = T.tone(L);
  int k = 0;
  for (int step = TONE_STEPS >> 1; step; step >>= 1) { // tone_map's search (k + step <= TONE_STEPS - 1: the steps sum to it)
    const int t = k + step;
    if (thr[t] <= N) k = t;
  }
  atomicAdd(&hist[k], 1u);
  if (N > 0.0f) most = max(most, __float_as_uint(N)); // (a negative or NaN N: nothing)
}

// src: the rectangle's origin; w x h: its size in pixels; out: HM_LIGHT_STATS_BINS counters, then the maximum's word (zeroed on the stream
// in front of the launch).  grid: x = workgroups, any number; dynamic LDS: the tables, then LIGHT_STATS_WORDS words.
template <int SB, int C, bool VEC>
__global__ __launch_bounds__(256) void k_light_stats(const uint8_t* __restrict__ src, int src_stride, int w, int h, Light L, unsigned* __restrict__ out)
{
  typedef typename std::conditional<SB == 1, uint8_t, uint16_t>::type InT;
  constexpr int P = STATS_P, NB = P * C * SB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  unsigned* hist = reinterpret_cast<unsigned*>(lds + light_layout(true, L.bits, L.ebits, false, true, L.ootf != nullptr, L.lin3 != 0, true).end);
  for (int i = threadIdx.x; i < LIGHT_STATS_WORDS; i += 256) hist[i] = 0u;
  const LightTables T = fill_light(lds, L, true, true); // (its barrier covers the counters too)
  const int lane = threadIdx.x & 63;
  const int chunks = ((w + P - 1) / P + 63) / 64; // tasks of a row
  const long long tasks = (long long)h * chunks, waves = (long long)gridDim.x * 4;
  unsigned most = 0u;
  for (long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); task < tasks; task += waves) {
    const int y = (int)(task / chunks), chunk = (int)(task - (long long)y * chunks);
    const uint8_t* row = src + (size_t)y * src_stride;
    if (!VEC) { // one pixel per lane and step
      const InT* irow = reinterpret_cast<const InT*>(row);
#pragma unroll 1
      for (int i = 0; i < P; i++) {
        const int x = (chunk * P + i) * 64 + lane;
        if (x >= w) break;
        unsigned v[C];
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = irow[(size_t)x * C + c];
        measure<C>(L, T, v, hist, most);
      }
      continue;
    }
    const int x0 = (chunk * 64 + lane) * P;
    if (x0 >= w) continue;
    const uint8_t* in = row + (size_t)x0 * (C * SB);
    if (x0 + P <= w) {
      typedef typename LoadWord<(NB % 16 == 0) ? 16 : 8>::type LW; // (NB = 24: three 8-bit channels)
      constexpr int NL = NB / (int)sizeof(LW);
      LW lw[NL];
#pragma unroll
      for (int k = 0; k < NL; k++) lw[k] = reinterpret_cast<const LW*>(in)[k];
      InT smp[P * C];
      __builtin_memcpy(smp, lw, NB);
#pragma unroll
      for (int i = 0; i < P; i++) {
        unsigned v[C];
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = smp[i * C + c];
        measure<C>(L, T, v, hist, most);
      }
      continue;
    }
    const InT* ip = reinterpret_cast<const InT*>(in); // the ragged last group: element by element
#pragma unroll 1
    for (int i = 0; i < w - x0; i++) {
      unsigned v[C];
#pragma unroll
      for (int c = 0; c < C; c++) v[c] = ip[i * C + c];
      measure<C>(L, T, v, hist, most);
    }
  }
  for (int o = 32; o; o >>= 1) most = max(most, (unsigned)__shfl_xor((int)most, o));
  if (lane == 0 && most) atomicMax(&hist[HM_LIGHT_STATS_BINS], most);
  __syncthreads();
  for (int i = threadIdx.x; i < HM_LIGHT_STATS_BINS; i += 256) {
    const unsigned n = hist[i];
    if (n) atomicAdd(&out[i], n);
  }
  if (threadIdx.x == 0 && hist[HM_LIGHT_STATS_BINS]) atomicMax(&out[HM_LIGHT_STATS_BINS], hist[HM_LIGHT_STATS_BINS]);
}

// every instance the launcher below can pick (hm_debug_kernel_regs)
const void* const g_instances[] = {
  (const void*)k_light_stats<1, 3, true>, (const void*)k_light_stats<1, 3, false>, (const void*)k_light_stats<1, 4, true>, (const void*)k_light_stats<1, 4, false>,
  (const void*)k_light_stats<2, 3, true>, (const void*)k_light_stats<2, 3, false>, (const void*)k_light_stats<2, 4, true>, (const void*)k_light_stats<2, 4, false>,
};

template <int SB, int C>
void launch(bool vec, int groups, size_t lds, const uint8_t* src, int src_stride, int w, int h, const Light& L, unsigned* out, hipStream_t s)
{
  if (vec) hipLaunchKernelGGL((k_light_stats<SB, C, true>), dim3((unsigned)groups), dim3(256), lds, s, src, src_stride, w, h, L, out);
  else hipLaunchKernelGGL((k_light_stats<SB, C, false>), dim3((unsigned)groups), dim3(256), lds, s, src, src_stride, w, h, L, out);
}

} // namespace

extern "C" const void* hm_stats_kernel_of(int index) // (test_hooks.cpp: hm_debug_kernel_regs)
{
  return index >= 0 && index < (int)(sizeof(g_instances) / sizeof(g_instances[0])) ? g_instances[index] : nullptr;
}

// The workgroups of a launch: as many as the device keeps resident - per CU what its 160 KB of LDS hold of this launch's request, at
// most 8 (32 waves) - and no more than the rectangle has tasks for; knob stats_groups > 0: that many (tests: few workgroups on a small
// picture, so that every wave loops).
static int stats_groups(size_t lds, int w, int h)
{
  const long long tasks = (long long)h * (((w + STATS_P - 1) / STATS_P + 63) / 64);
  const int forced = hm_knob(HM_KNOB_STATS_GROUPS);
  if (forced > 0) return forced;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
  const long long per_cu = std::min<long long>(8, std::max<long long>(1, (long long)(160 * 1024) / (long long)lds));
  return (int)std::max<long long>(1, std::min<long long>(cus * per_cu, (tasks + 3) / 4));
}

// the w x h pixels at `src` (the rectangle's origin) counted into out[HM_LIGHT_STATS_BINS + 1] (zeroed on `s` by the caller); la: lin,
// tone = thr of the tone step (sg is not read), ootf; enc and encode are not looked at.  channels: 3 / 4.  Asynchronous on `s`.
extern "C" int hm_launch_light_stats_kernel(const hm_light_args* la, int channels, const void* src, int src_stride, int w, int h, unsigned* out, hipStream_t s)
{
  if (w <= 0 || h <= 0) return HM_OK;
  if (!la->lin || !la->tone || la->bits < 8 || la->bits > 12 || (la->lin3 != 0 && la->lin3 != 1)) return hm_fail(HM_ERR_INTERNAL, "k_light_stats: tables of %d bits", la->bits);
  if (la->src_bytes != (la->bits > 8 ? 2 : 1)) return hm_fail(HM_ERR_INTERNAL, "k_light_stats: %d-byte samples of %d bits", la->src_bytes, la->bits);
  if (channels != 3 && channels != 4) return hm_fail(HM_ERR_INTERNAL, "k_light_stats: %d channels", channels);
  const int rc = check_light_lds(la, 3);
  if (rc) return rc;
  Light L = light_of(la);
  L.enc = nullptr; L.encode = 0; L.ebits = L.bits; // (the pass never re-encodes)
  const size_t lds = light_stats_bytes(la);
  const bool vec = ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0;
  const int groups = stats_groups(lds, w, h);
  with_flags(la->src_bytes == 2, channels == 4, [&](auto wide, auto four) {
    launch<wide.value ? 2 : 1, four.value ? 4 : 3>(vec, groups, lds, (const uint8_t*)src, src_stride, w, h, L, out, s);
  });
  return hm_check_hip(hipGetLastError(), "k_light_stats launch");
}
