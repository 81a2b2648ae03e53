// AddressSanitizer / UBSan walk of the region-item reader (CPU only, a program of its own - nothing here is loaded into Python): a small
// HEIF file with a mask item ('mski' + mskC), and a region item ('rgan') that holds every geometry type and references the mask, is
// written in memory; mutated copies of it - the 'rgan' payload truncated at every length, with random bytes, with random field values
// in both field sizes, and single bytes flipped anywhere in the file - go through hm_file_open, hm_file_item_kind,
// hm_file_top_level_images, hm_file_image_info, hm_file_region_items, hm_file_region_item_info, hm_file_region, hm_file_region_points
// and hm_file_region_inline_mask.  What the reader hands out for the seed is checked, and every point and bit string it hands out is read.
// Build and run from the repository's root:
//   S=heif-decoder-lib_amd/csrc; g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//     -Iinclude -I$S -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/asan/region_fuzz.cpp $S/hm_image.cpp $S/heif_file.cpp $S/unci_layout.cpp \
//     $S/devdest.cpp $S/devpool.cpp $S/colour_host.cpp $S/common.cpp -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//     -Wl,--unresolved-symbols=ignore-all -lpthread -o /tmp/hm_region_fuzz && ASAN_OPTIONS=detect_leaks=0 /tmp/hm_region_fuzz
// (the launchers of the .hip files and the decode are left out: no call here gets to them, the linker lets them pass).
// HM_FUZZ_ITER: random mutations (default 20000).  Exit status 0: every call returned, the seed's answers are right, no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "heif_mi355x.h"

extern "C" void hm_chain_test_knobs(int, int) {}

typedef std::vector<uint8_t> Bytes;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static void be(Bytes& b, uint64_t v, int n) { for (int i = n - 1; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i))); }
static void put(Bytes& b, const Bytes& x) { b.insert(b.end(), x.begin(), x.end()); }
static void put(Bytes& b, const char* s) { b.insert(b.end(), s, s + std::strlen(s)); }
static Bytes box(const char* type, const Bytes& body)
{
  Bytes b;
  be(b, 8 + body.size(), 4); put(b, type); put(b, body);
  return b;
}
static Bytes full(const char* type, int version, uint32_t flags, const Bytes& body)
{
  Bytes b;
  be(b, (uint64_t)version << 24 | flags, 4); put(b, body);
  return box(type, b);
}

// every geometry type once; fb: bytes per field
static Bytes seed_payload(int fb)
{
  Bytes p;
  be(p, 0, 1); be(p, fb == 4 ? 1 : 0, 1); be(p, 64, fb); be(p, 48, fb); be(p, 7, 1);
  be(p, 0, 1); be(p, (uint64_t)-4, fb); be(p, 9, fb);                                    // point
  be(p, 1, 1); be(p, (uint64_t)-10, fb); be(p, 3, fb); be(p, 20, fb); be(p, 7, fb);       // rectangle
  be(p, 2, 1); be(p, 30, fb); be(p, (uint64_t)-2, fb); be(p, 11, fb); be(p, 0, fb);       // ellipse
  be(p, 3, 1); be(p, 3, fb); for (int v : {-3, 5, 40, -7, 12, 30}) be(p, (uint64_t)v, fb); // polygon
  be(p, 4, 1); be(p, (uint64_t)-2, fb); be(p, 1, fb); be(p, 0, fb); be(p, 0, fb);         // referenced mask
  be(p, 5, 1); be(p, (uint64_t)-5, fb); be(p, 2, fb); be(p, 13, fb); be(p, 5, fb); be(p, 0, 1); // inline mask: 65 bits, 9 bytes
  for (int i = 0; i < 9; i++) be(p, 0xA0 + i, 1);
  be(p, 6, 1); be(p, 2, fb); for (int v : {-3, 5, 40, -7}) be(p, (uint64_t)v, fb);       // polyline
  return p;
}

// item 1: 'mski' 4 x 3, item 2: 'rgan'; cdsc 2 -> 1, mask 2 -> 1
static Bytes file_of(const Bytes& rgan, size_t* payload_at = nullptr)
{
  Bytes mask(12, 0x80);
  Bytes ispe; be(ispe, 4, 4); be(ispe, 3, 4);
  Bytes ipco; put(ipco, full("ispe", 0, 0, ispe)); put(ipco, full("mskC", 0, 0, Bytes{8}));
  Bytes ipma; be(ipma, 1, 4); be(ipma, 1, 2); be(ipma, 2, 1); be(ipma, 1, 1); be(ipma, 0x82, 1);
  Bytes iprp; put(iprp, box("ipco", ipco)); put(iprp, full("ipma", 0, 0, ipma));
  Bytes iinf; be(iinf, 2, 2);
  for (int i = 1; i <= 2; i++) { Bytes e; be(e, (uint64_t)i, 2); be(e, 0, 2); put(e, i == 1 ? "mski" : "rgan"); be(e, 0, 1); put(iinf, full("infe", 2, 0, e)); }
  Bytes iref;
  for (const char* t : {"cdsc", "mask"}) { Bytes r; be(r, 2, 2); be(r, 1, 2); be(r, 1, 2); put(iref, box(t, r)); }
  Bytes pitm; be(pitm, 1, 2);
  Bytes hdlr; be(hdlr, 0, 4); put(hdlr, "pict"); hdlr.resize(hdlr.size() + 13, 0);
  Bytes ftyp; put(ftyp, "heic"); be(ftyp, 0, 4); put(ftyp, "mif1heic");
  Bytes out;
  for (int pass = 0; pass < 2; pass++) { // (the second pass knows where the mdat starts)
    const size_t mdat_at = pass ? out.size() - mask.size() - rgan.size() : 0;
    Bytes iloc; be(iloc, 0x44, 1); be(iloc, 0, 1); be(iloc, 2, 2);
    be(iloc, 1, 2); be(iloc, 0, 2); be(iloc, 1, 2); be(iloc, mdat_at, 4); be(iloc, mask.size(), 4);
    be(iloc, 2, 2); be(iloc, 0, 2); be(iloc, 1, 2); be(iloc, mdat_at + mask.size(), 4); be(iloc, rgan.size(), 4);
    Bytes meta; put(meta, full("hdlr", 0, 0, hdlr)); put(meta, full("pitm", 0, 0, pitm)); put(meta, full("iloc", 0, 0, iloc)); put(meta, full("iinf", 0, 0, iinf));
    put(meta, full("iref", 0, 0, iref)); put(meta, box("iprp", iprp));
    Bytes data = mask; put(data, rgan);
    out.clear();
    put(out, box("ftyp", ftyp)); put(out, full("meta", 0, 0, meta)); put(out, box("mdat", data));
    if (payload_at) *payload_at = out.size() - rgan.size();
  }
  return out;
}

static long refused_open = 0, refused_item = 0, read_ok = 0;

// every call on every item; every point and bit handed out is read
static int walk(const Bytes& file)
{
  hm_file* f = nullptr;
  if (hm_file_open(file.data(), file.size(), &f) != HM_OK) { refused_open++; return 0; }
  uint32_t ids[8];
  (void)hm_file_top_level_images(f, ids, 8);
  volatile uint64_t sink = 0;
  for (uint32_t id = 0; id <= 3; id++) {
    (void)hm_file_item_kind(f, id);
    hm_image_info ii;
    (void)hm_file_image_info(f, id, &ii);
    uint32_t items[4];
    (void)hm_file_region_items(f, id, items, 4);
    hm_region_item_info info;
    if (hm_file_region_item_info(f, id, &info) != HM_OK) { refused_item++; continue; }
    read_ok++;
    if (info.n_regions < 0 || info.n_regions > 255) { std::fprintf(stderr, "%d regions\n", info.n_regions); return 1; }
    for (int k = -1; k <= info.n_regions; k++) {
      hm_region g;
      const int rc = hm_file_region(f, id, k, &g);
      if ((rc == HM_OK) != (k >= 0 && k < info.n_regions)) { std::fprintf(stderr, "region %d of %d: status %d\n", k, info.n_regions, rc); return 1; }
      if (rc != HM_OK) continue;
      std::vector<int32_t> xy(2 * (size_t)g.n_points + 2);
      const int n = hm_file_region_points(f, id, k, xy.data(), (int)g.n_points);
      if (n != (int)g.n_points) { std::fprintf(stderr, "points: %d of %u\n", n, g.n_points); return 1; }
      for (size_t i = 0; i < 2 * (size_t)g.n_points; i++) {
        if (xy[i] < -HM_REGION_COORD_LIMIT || xy[i] >= HM_REGION_COORD_LIMIT) { std::fprintf(stderr, "a point beyond the limit was handed out\n"); return 1; }
        sink = sink + (uint64_t)xy[i];
      }
      const uint8_t* bits = nullptr;
      size_t len = 0;
      const int rb = hm_file_region_inline_mask(f, id, k, &bits, &len);
      if ((rb == HM_OK) != (g.type == HM_REGION_INLINE_MASK)) { std::fprintf(stderr, "inline mask of a region of type %d: status %d\n", g.type, rb); return 1; }
      if (rb == HM_OK) {
        if (len != ((uint64_t)g.w * g.h + 7) / 8 || len != g.mask_bytes) { std::fprintf(stderr, "inline mask of %u x %u with %zu bytes\n", g.w, g.h, len); return 1; }
        for (size_t i = 0; i < len; i++) sink = sink + bits[i];
      }
      if (g.type == HM_REGION_ELLIPSE && (g.w > HM_REGION_MAX_RADIUS || g.h > HM_REGION_MAX_RADIUS)) { std::fprintf(stderr, "a radius beyond the limit was handed out\n"); return 1; }
    }
  }
  hm_file_close(f);
  return 0;
}

static int check_seed(int fb)
{
  const Bytes file = file_of(seed_payload(fb));
  hm_file* f = nullptr;
  if (hm_file_open(file.data(), file.size(), &f) != HM_OK) { std::fprintf(stderr, "the seed does not open: %s\n", hm_last_error()); return 1; }
  uint32_t items[4] = {0, 0, 0, 0};
  hm_region_item_info info;
  hm_region g;
  bool bad = hm_file_item_kind(f, 1) != HM_ITEM_MSKI || hm_file_region_items(f, 1, items, 4) != 1 || items[0] != 2;
  bad |= hm_file_top_level_images(f, items, 4) != 0; // (the mask of a region is no image of its own)
  bad |= hm_file_region_item_info(f, 2, &info) != HM_OK || info.reference_width != 64 || info.reference_height != 48 || info.n_regions != 7 || info.field_bits != 8 * fb;
  bad |= hm_file_region(f, 2, 4, &g) != HM_OK || g.type != HM_REGION_REFERENCED_MASK || g.x != -2 || g.w != 4 || g.h != 3 || g.mask_item != 1 || g.mask_bytes != 12;
  bad |= hm_file_region(f, 2, 5, &g) != HM_OK || g.type != HM_REGION_INLINE_MASK || g.x != -5 || g.w != 13 || g.mask_bytes != 9;
  int32_t xy[6];
  bad |= hm_file_region_points(f, 2, 3, xy, 3) != 3 || xy[0] != -3 || xy[3] != -7 || xy[5] != 30;
  bad |= hm_file_region(f, 2, 6, &g) != HM_OK || g.type != HM_REGION_POLYLINE || g.n_points != 2;
  hm_file_close(f);
  if (bad) std::fprintf(stderr, "the seed's answers are wrong (%d-byte fields): %s\n", fb, hm_last_error());
  return bad ? 1 : 0;
}

int main()
{
  const char* env = std::getenv("HM_FUZZ_ITER");
  const long iters = env ? std::atol(env) : 20000;
  if (check_seed(2) || check_seed(4)) return 1;
  for (int fb : {2, 4}) { // every truncation of the payload
    const Bytes p = seed_payload(fb);
    for (size_t n = 0; n <= p.size(); n++)
      if (walk(file_of(Bytes(p.begin(), p.begin() + n)))) return 1;
  }
  for (long it = 0; it < iters; it++) {
    const int fb = rnd() & 1 ? 4 : 2;
    Bytes p = seed_payload(fb);
    size_t at = 0;
    Bytes file;
    switch (rnd() % 4) {
      case 0: // random bytes in the payload
        for (int k = 1 + (int)(rnd() % 4); k > 0; k--) p[rnd() % p.size()] = (uint8_t)rnd();
        file = file_of(p);
        break;
      case 1: // a payload of random bytes behind a plausible header
        p.resize(4 + 2 * (size_t)fb + rnd() % 64);
        for (size_t i = 2 + 2 * (size_t)fb; i < p.size(); i++) p[i] = (uint8_t)(rnd() % 3 ? rnd() % 8 : rnd());
        file = file_of(p);
        break;
      case 2: // extreme values in a whole field
        file = file_of(p, &at);
        for (int k = 0; k < fb; k++) file[at + 2 + (rnd() % (p.size() - 2 - (size_t)fb)) ] = rnd() & 1 ? 0xFF : 0x7F;
        break;
      default: // a byte anywhere in the file
        file = file_of(p);
        file[rnd() % file.size()] ^= (uint8_t)(1u << (rnd() % 8));
    }
    if (walk(file)) { std::fprintf(stderr, "iteration %ld\n", it); return 1; }
  }
  std::printf("region reader: %ld mutated files, %ld refused at open, region items read %ld times and refused %ld times; no finding\n", iters, refused_open, read_ok,
              refused_item);
  return 0;
}
