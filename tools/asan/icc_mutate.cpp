// icc_mutate.cpp — the ICC reader (csrc/icc.cpp) under ASan + UBSan, CPU only: every seed profile given on the command line, then a few
// thousand variants of each - bytes flipped, fields of the header and the tag table overwritten with edge values, the buffer cut
// short - through hm_icc_parse, hm_icc_table and hm_icc_matrix.  Each variant sits in a heap block of exactly its size, so a read
// behind it is a finding.  Built and run by tools/asan/run_icc_mutate.sh; prints how many variants parsed and how many were refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "heif_mi355x.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}

static long g_ok = 0, g_refused = 0;

static void run(const std::vector<uint8_t>& v)
{
  uint8_t* p = (uint8_t*)std::malloc(v.size() ? v.size() : 1); // (exactly the bytes: ASan guards the rest)
  if (!p) std::abort();
  if (!v.empty()) std::memcpy(p, v.data(), v.size());
  hm_icc_info info;
  const int rc = hm_icc_parse(p, v.size(), &info);
  static float table[4096];
  float m[9];
  for (int bits = 8; bits <= 12; bits += 2)
    for (int c = 0; c < 3; c++) {
      const int n = hm_icc_table(p, v.size(), c, bits, 1.5f, table);
      if ((rc == 0) != (n == 1 << bits)) { std::fprintf(stderr, "parse says %d, table says %d\n", rc, n); std::abort(); }
      for (int i = 0; i < n; i++)
        if (!(table[i] >= 0.0f && table[i] <= 1.5f)) { std::fprintf(stderr, "table entry %d = %g\n", i, (double)table[i]); std::abort(); }
    }
  static const int prim[6] = {1, 5, 6, 7, 9, 12};
  for (int k = 0; k < 6; k++)
    if ((hm_icc_matrix(p, v.size(), prim[k], m) == 0) != (rc == 0)) { std::fprintf(stderr, "parse says %d, matrix disagrees\n", rc); std::abort(); }
  (rc == 0 ? g_ok : g_refused)++;
  std::free(p);
}

int main(int argc, char** argv)
{
  const int rounds = 3000;
  static const uint32_t edge[] = {0, 1, 2, 3, 4, 12, 127, 128, 131, 132, 133, 255, 256, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000u, 0xFFFFFFF0u, 0xFFFFFFFFu};
  for (int a = 1; a < argc; a++) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> seed;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) seed.insert(seed.end(), buf, buf + n);
    std::fclose(f);
    run(seed);
    for (size_t cut = 0; cut < seed.size(); cut += (cut < 200 ? 1 : 7)) run(std::vector<uint8_t>(seed.begin(), seed.begin() + cut)); // truncated
    for (int r = 0; r < rounds; r++) {
      std::vector<uint8_t> v = seed;
      const int flips = 1 + (int)(rnd() % 4);
      for (int k = 0; k < flips; k++) {
        const uint32_t kind = rnd() % 4;
        // the header and the tag table decide where the reader looks: most mutations go there
        const size_t head = v.size() < 300 ? v.size() : 300;
        const size_t pos = (kind == 0 ? rnd() % v.size() : rnd() % head);
        if (kind <= 1) v[pos] ^= (uint8_t)(1u << (rnd() % 8));
        else if (kind == 2) v[pos] = (uint8_t)rnd();
        else if (pos + 4 <= v.size()) { // a 32-bit field at a multiple of four gets an edge value, or one near the size
          const size_t at = pos & ~(size_t)3;
          uint32_t val = edge[rnd() % (sizeof(edge) / sizeof(edge[0]))];
          if (rnd() % 3 == 0) val = (uint32_t)v.size() - 2 + rnd() % 5;
          v[at] = (uint8_t)(val >> 24); v[at + 1] = (uint8_t)(val >> 16); v[at + 2] = (uint8_t)(val >> 8); v[at + 3] = (uint8_t)val;
        }
      }
      if (rnd() % 8 == 0) v.resize(rnd() % (v.size() + 1));
      run(v);
    }
  }
  std::printf("icc_mutate: %ld variants parsed, %ld refused\n", g_ok, g_refused);
  return g_ok > 0 && g_refused > 0 ? 0 : 1;
}
