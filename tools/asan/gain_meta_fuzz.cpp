// AddressSanitizer / UBSan walk of the 'tmap' metadata reader (CPU only, a program of its own - nothing here is loaded into Python):
// a small HEIF file with a base image item, a gain-map item, an auxiliary image and a 'tmap' item is written in memory, and mutated
// copies of it - the 'tmap' payload, the 'dimg' / 'auxl' reference lists, the property boxes, single bytes anywhere, truncations - go
// through hm_file_open, hm_file_item_kind, hm_file_top_level_images, hm_file_gain_map_of, hm_file_gain_map_info,
// hm_file_item_aux_type and the refusals of hm_decode_item_to_device_gain (which end at the device probe at the latest: no picture is
// looked at).  Well-formed payloads with extreme fractions are walked too, and what the reader hands out for the seed is checked.
// Build and run from the repository's root:
//   S=heif-decoder-lib_amd/csrc; g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//     -Iinclude -I$S -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/asan/gain_meta_fuzz.cpp $S/hm_image.cpp $S/heif_file.cpp $S/devdest.cpp \
//     $S/devpool.cpp $S/colour_host.cpp $S/common.cpp -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -Wl,--unresolved-symbols=ignore-all \
//     -lpthread -o /tmp/hm_gain_meta_fuzz && ASAN_OPTIONS=detect_leaks=0 /tmp/hm_gain_meta_fuzz
// (the launchers of the .hip files and the decode behind the refusals are left out: no call here gets to them, the linker lets them pass).
// HM_FUZZ_ITER: mutations (default 20000).  Exit status 0: every call returned, the seed's answers are right, no sanitizer report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "heif_mi355x.h"

// (common.cpp's test hooks reach into the device side of the library, which this host-only build leaves out)
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

struct Fraction { int64_t n; uint32_t d; };
struct Channel { Fraction min, max, gamma, base_offset, alternate_offset; };

static Bytes tmap_payload(int version, int minimum, int flags, Fraction hb, Fraction ha, const std::vector<Channel>& ch)
{
  Bytes p;
  be(p, (uint64_t)version, 1); be(p, (uint64_t)minimum, 2); be(p, 0, 2); be(p, (uint64_t)flags, 1);
  be(p, (uint64_t)hb.n, 4); be(p, hb.d, 4); be(p, (uint64_t)ha.n, 4); be(p, ha.d, 4);
  for (const Channel& c : ch)
    for (const Fraction* f : {&c.min, &c.max, &c.gamma, &c.base_offset, &c.alternate_offset}) { be(p, (uint64_t)f->n, 4); be(p, f->d, 4); }
  return p;
}

// where the mutations aim: the 'tmap' payload, the reference box, the property container
struct Seed { Bytes file; size_t payload_at, payload_n, iref_at, iref_n, iprp_at, iprp_n; };

// items: 1 base (hvc1), 2 gain map (hvc1, hidden), 3 auxiliary image of 1 with a vendor URN, 4 'tmap' over (1, 2)
static Seed make_file(const Bytes& payload, const std::vector<uint16_t>& tmap_refs)
{
  const char* types[4] = {"hvc1", "hvc1", "hvc1", "tmap"};
  const Bytes pictures[3] = {Bytes(24, 0x11), Bytes(16, 0x22), Bytes(16, 0x33)};
  Bytes ispe64, ispe32, colr, clli, auxc, hvcc(23, 0);
  be(ispe64, 64, 4); be(ispe64, 64, 4); be(ispe32, 32, 4); be(ispe32, 32, 4);
  put(colr, "nclx"); be(colr, 9, 2); be(colr, 16, 2); be(colr, 0, 2); be(colr, 0x80, 1);
  be(clli, 1000, 2); be(clli, 400, 2);
  put(auxc, "urn:com:example:hdr:aux:hdrgainmap"); auxc.push_back(0);
  hvcc[0] = 1;
  Bytes ipco;
  put(ipco, box("hvcC", hvcc)); put(ipco, full("ispe", 0, 0, ispe64)); put(ipco, full("ispe", 0, 0, ispe32)); put(ipco, box("colr", colr));
  put(ipco, box("clli", clli)); put(ipco, full("auxC", 0, 0, auxc));
  const std::vector<std::vector<uint8_t>> assoc = {{0x81, 2}, {0x81, 3}, {0x81, 3, 0x86}, {2, 4, 5}};
  Bytes ipma;
  be(ipma, assoc.size(), 4);
  for (size_t i = 0; i < assoc.size(); i++) { be(ipma, i + 1, 2); be(ipma, assoc[i].size(), 1); put(ipma, assoc[i]); }
  Bytes iprp_body;
  put(iprp_body, box("ipco", ipco)); put(iprp_body, full("ipma", 0, 0, ipma));
  const Bytes iprp = box("iprp", iprp_body);
  Bytes dimg, auxl, iref_body;
  be(dimg, 4, 2); be(dimg, tmap_refs.size(), 2);
  for (uint16_t t : tmap_refs) be(dimg, t, 2);
  be(auxl, 3, 2); be(auxl, 1, 2); be(auxl, 1, 2);
  put(iref_body, box("dimg", dimg)); put(iref_body, box("auxl", auxl));
  const Bytes iref = full("iref", 0, 0, iref_body);
  Bytes iinf_body;
  be(iinf_body, 4, 2);
  for (int i = 0; i < 4; i++) {
    Bytes infe;
    be(infe, (uint64_t)i + 1, 2); be(infe, 0, 2); put(infe, types[i]); infe.push_back(0);
    put(iinf_body, full("infe", 2, i == 1 ? 1 : 0, infe));
  }
  Bytes hdlr_body, pitm_body, ftyp_body;
  be(hdlr_body, 0, 4); put(hdlr_body, "pict"); hdlr_body.insert(hdlr_body.end(), 13, 0);
  be(pitm_body, 1, 2);
  put(ftyp_body, "heic"); be(ftyp_body, 0, 4); put(ftyp_body, "mif1heic");
  const Bytes ftyp = box("ftyp", ftyp_body), hdlr = full("hdlr", 0, 0, hdlr_body), pitm = full("pitm", 0, 0, pitm_body), iinf = full("iinf", 0, 0, iinf_body);
  const size_t sizes[4] = {pictures[0].size(), pictures[1].size(), pictures[2].size(), payload.size()};
  auto meta_with = [&](size_t first, size_t* iref_at, size_t* iprp_at) {
    Bytes iloc_body, body;
    be(iloc_body, 0x44, 1); be(iloc_body, 0, 1); be(iloc_body, 4, 2);
    size_t off = first;
    for (int i = 0; i < 4; i++) { be(iloc_body, (uint64_t)i + 1, 2); be(iloc_body, 0, 2); be(iloc_body, 1, 2); be(iloc_body, off, 4); be(iloc_body, sizes[i], 4); off += sizes[i]; }
    put(body, hdlr); put(body, pitm); put(body, full("iloc", 0, 0, iloc_body)); put(body, iinf);
    if (iref_at) *iref_at = 12 + body.size();
    put(body, iref);
    if (iprp_at) *iprp_at = 12 + body.size();
    put(body, iprp);
    return full("meta", 0, 0, body);
  };
  Seed s;
  const size_t first = ftyp.size() + meta_with(0, nullptr, nullptr).size() + 8;
  size_t iref_at = 0, iprp_at = 0;
  const Bytes meta = meta_with(first, &iref_at, &iprp_at);
  Bytes mdat_body;
  for (const Bytes& p : pictures) put(mdat_body, p);
  put(mdat_body, payload);
  put(s.file, ftyp); put(s.file, meta); put(s.file, box("mdat", mdat_body));
  s.payload_at = first + sizes[0] + sizes[1] + sizes[2]; s.payload_n = payload.size();
  s.iref_at = ftyp.size() + iref_at; s.iref_n = iref.size();
  s.iprp_at = ftyp.size() + iprp_at; s.iprp_n = iprp.size();
  return s;
}

static long opened = 0, refused_open = 0, infos_ok = 0, infos_refused = 0, decodes = 0;

// every answer of the file layer about a (possibly damaged) file, and the decode's refusals on top of them
static int walk(const Bytes& file)
{
  hm_file* f = nullptr;
  if (hm_file_open(file.data(), file.size(), &f) != HM_OK) { refused_open++; return 0; }
  opened++;
  uint32_t ids[16];
  const int n = hm_file_top_level_images(f, ids, 16);
  if (n < 0 || n > 8) { std::fprintf(stderr, "%d top-level images\n", n); return 1; }
  for (uint32_t id = 0; id <= 6; id++) {
    const int kind = hm_file_item_kind(f, id);
    char urn[24];
    (void)hm_file_item_aux_type(f, id, urn, (int)sizeof(urn));
    (void)hm_file_item_aux_type(f, id, nullptr, 0);
    (void)hm_file_gain_map_of(f, id);
    hm_gain_map_info info;
    const int rc = hm_file_gain_map_info(f, id, &info);
    if (rc == HM_OK) {
      infos_ok++;
      if (kind != HM_ITEM_TMAP || !info.base_item || !info.map_item) { std::fprintf(stderr, "gain map info of item %u of kind %d: base %u, map %u\n", id, kind, info.base_item, info.map_item); return 1; }
      for (int c = 0; c < 3; c++)
        if (!(info.params.gamma[c] > 0.0) || !std::isfinite(info.params.map_min[c]) || !std::isfinite(info.params.map_max[c])) { std::fprintf(stderr, "bad parameters handed out\n"); return 1; }
    }
    else infos_refused++;
    // the decode's refusals (a destination that is never written: everything ends at the device probe at the latest)
    hm_decode_params prm = {};
    prm.out_format = HM_OUT_RGB; prm.host_threads = 1;
    hm_device_light light = {};
    light.to_transfer = HM_LIGHT_LINEAR; light.gain = 1.0f;
    hm_device_view view = {2 * (int32_t)(rnd() % 3), (int32_t)(rnd() % 5), 16, 16, (int32_t)(rnd() % 2) * 8, (int32_t)(rnd() % 2) * 8, (int32_t)(rnd() % 2)};
    if (view.out_w != view.out_h) view.out_h = view.out_w;
    hm_device_gain gain = {};
    gain.headroom = (rnd() % 4) ? 1.5f : std::numeric_limits<float>::infinity();
    if (rnd() % 4 == 0) { gain.map_item = 1 + rnd() % 5; gain.params.alternate_headroom = 2.0; for (int c = 0; c < 3; c++) { gain.params.map_max[c] = 2.0; gain.params.gamma[c] = 1.0; } }
    hm_device_dest d = {};
    d.ptr = (void*)(uintptr_t)0x10000000; d.len = 64 * 64 * 12; d.layout = HM_DEV_LAYOUT_CHW; d.dtype = HM_DEV_F32;
    for (int c = 0; c < 4; c++) d.scale[c] = 1.0f;
    hm_decoded out;
    const int drc = hm_decode_item_to_device_gain(f, id, &prm, rnd() % 2 ? &view : nullptr, &light, nullptr, &gain, &d, &out);
    decodes++;
    if (drc >= 0) { std::fprintf(stderr, "a decode to a fake pointer returned %d\n", drc); return 1; }
  }
  hm_file_close(f);
  return 0;
}

static int check_seed(const Seed& s)
{
  hm_file* f = nullptr;
  if (hm_file_open(s.file.data(), s.file.size(), &f) != HM_OK) { std::fprintf(stderr, "the seed does not open: %s\n", hm_last_error()); return 1; }
  uint32_t ids[8];
  hm_gain_map_info info;
  char urn[64];
  int bad = 0;
  bad |= hm_file_top_level_images(f, ids, 8) != 1 || ids[0] != 1;
  bad |= hm_file_item_kind(f, 4) != HM_ITEM_TMAP || hm_file_gain_map_of(f, 1) != 4 || hm_file_gain_map_of(f, 2) != 0;
  bad |= hm_file_gain_map_info(f, 4, &info) != HM_OK || info.base_item != 1 || info.map_item != 2 || info.alt_primaries != 9 || info.alt_transfer != 16;
  bad |= info.params.base_headroom != 0.0 || info.params.alternate_headroom != 2.5 || info.params.map_min[2] != -0.75 || info.params.gamma[1] != 2.2 ||
         info.params.use_base_primaries != 1;
  bad |= hm_file_item_aux_type(f, 3, urn, 64) != 34 || std::strcmp(urn, "urn:com:example:hdr:aux:hdrgainmap") != 0;
  if (bad) std::fprintf(stderr, "the seed's answers are wrong (%s)\n", hm_last_error());
  hm_file_close(f);
  return bad;
}

int main()
{
  int iterations = 20000;
  if (const char* e = std::getenv("HM_FUZZ_ITER")) iterations = std::atoi(e);
  const std::vector<Channel> one = {{{-3, 4}, {5, 2}, {22, 10}, {1, 64}, {1, 64}}};
  const Seed seed = make_file(tmap_payload(0, 0, 0x40, {0, 1}, {5, 2}, one), {1, 2});
  if (check_seed(seed)) return 1;
  // well-formed payloads at the ends of the fractions' ranges, and the reference lists a 'tmap' item may not have
  const Fraction ends[] = {{0, 1}, {-2147483647 - 1, 1}, {2147483647, 1}, {1, 4294967295u}, {4294967295ll, 4294967295u}, {-1, 4294967295u}, {1, 0}, {0, 0}};
  for (const Fraction& a : ends)
    for (const Fraction& b : ends) {
      const std::vector<Channel> three = {{a, b, {22, 10}, a, b}, {b, a, b, {1, 64}, a}, {a, a, a, b, b}};
      for (int flags : {0x00, 0x40, 0x80, 0xC0, 0xFF})
        if (walk(make_file(tmap_payload(0, 0, flags, a, b, (flags & 0x80) ? three : std::vector<Channel>{three[rnd() % 3]}), {1, 2}).file)) return 1;
    }
  for (const std::vector<uint16_t>& refs : std::vector<std::vector<uint16_t>>{{}, {1}, {1, 2, 3}, {4, 4}, {1, 1}, {2, 1}, {9, 2}, {1, 9}, {3, 2}, {1, 4}})
    if (walk(make_file(tmap_payload(0, 0, 0, {0, 1}, {5, 2}, one), refs).file)) return 1;
  for (int version = 0; version < 3; version++)
    for (int minimum = 0; minimum < 3; minimum++)
      if (walk(make_file(tmap_payload(version, minimum, 0, {0, 1}, {5, 2}, one), {1, 2}).file)) return 1;
  const long structured = opened + refused_open;
  // mutations: aimed at the payload, the references or the properties, or anywhere; sometimes a truncated payload
  for (int it = 0; it < iterations; it++) {
    Bytes payload = tmap_payload(0, 0, (rnd() % 2 ? 0x80 : 0) | (rnd() % 2 ? 0x40 : 0), {0, 1}, {5, 2}, std::vector<Channel>(3, one[0]));
    if (rnd() % 4 == 0) payload.resize(rnd() % payload.size() + 1); // (a length of 0 in 'iloc' means "to the end of the file")
    Seed s = make_file(payload, {1, 2});
    Bytes& b = s.file;
    const int n = 1 + rnd() % 4;
    for (int k = 0; k < n; k++) {
      size_t at, span;
      switch (rnd() % 4) {
        case 0: at = s.payload_at; span = s.payload_n; break;
        case 1: at = s.iref_at; span = s.iref_n; break;
        case 2: at = s.iprp_at; span = s.iprp_n; break;
        default: at = 0; span = b.size(); break;
      }
      if (at >= b.size()) continue;
      if (at + span > b.size()) span = b.size() - at;
      const size_t p = at + rnd() % span;
      switch (rnd() % 5) {
        case 0: b[p] ^= (uint8_t)(1u << (rnd() % 8)); break;
        case 1: b[p] = (uint8_t)rnd(); break;
        case 2: if (p + 4 <= b.size()) { const uint32_t v = rnd() % 3 ? (rnd() % 2 ? 0xFFFFFFFFu : 0u) : rnd(); std::memcpy(&b[p], &v, 4); } break;
        case 3: b[p] = 0; break;
        default: if (rnd() % 8 == 0) b.resize(p + 1); break;
      }
    }
    if (walk(b)) return 1;
  }
  std::printf("gain_meta_fuzz: %ld structured files, %d mutations; opened %ld, refused at open %ld; gain map infos %ld answered, %ld refused; %ld decode requests, all refused\n",
              structured, iterations, opened, refused_open, infos_ok, infos_refused, decodes);
  return 0;
}
