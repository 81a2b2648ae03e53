// AddressSanitizer / UBSan walk of the stand-alone device-write entries' refusals (CPU only): devdest.cpp's host code, built with the
// sanitizers, takes every tensor_* request of tests/target_cases.py (one per line on stdin: tools/asan/target_walk.py) through
// hm_to_tensor, hm_resample_to_tensor, hm_light_to_tensor, hm_tone_to_tensor and hm_alpha_to_tensor.  Every one of them is refused before
// a device is looked for; the status and message go to stdout.  Build + run: tools/asan/run_target_walk.sh
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "heif_mi355x.h"

// (common.cpp's test hooks reach into the device side of the library, which this host-only build leaves out - as it leaves out the
// launchers of the .hip files, which no request of the walk gets to: run_target_walk.sh lets the linker pass them)
extern "C" void hm_chain_test_knobs(int, int) {}

static std::vector<double> group(std::istringstream& in)
{
  int n = 0;
  in >> n;
  std::vector<double> v((size_t)n);
  for (double& x : v) { std::string tok; in >> tok; x = std::strtod(tok.c_str(), nullptr); }
  return v;
}

int main()
{
  std::string text;
  int lines = 0, bad = 0;
  while (std::getline(std::cin, text)) {
    const size_t bar = text.find(" | ");
    if (bar == std::string::npos) continue;
    std::istringstream in(text.substr(0, bar));
    std::string family;
    int fmt, bits, w, h, stride;
    in >> family >> fmt >> bits >> w >> h >> stride;
    const std::vector<double> v = group(in), l = group(in), t = group(in), a = group(in);
    hm_device_view view = {};
    hm_device_light light = {};
    hm_device_tone tone = {};
    hm_device_alpha alpha = {};
    if (v.size() == 7) { view.crop_x = (int)v[0]; view.crop_y = (int)v[1]; view.crop_w = (int)v[2]; view.crop_h = (int)v[3]; view.out_w = (int)v[4]; view.out_h = (int)v[5]; view.filter = (int)v[6]; }
    if (l.size() == 5) { light.from_transfer = (int)l[0]; light.from_primaries = (int)l[1]; light.to_transfer = (int)l[2]; light.to_primaries = (int)l[3]; light.gain = (float)l[4]; }
    if (t.size() == 6) { tone.curve = (int)t[0]; tone.out_bits = (int)t[1]; tone.src_peak = (float)t[2]; tone.dst_peak = (float)t[3]; tone.unit_nits = (float)t[4]; tone.out_unit_nits = (float)t[5]; }
    if (a.size() == 8) { alpha.mode = (int)a[0]; for (int c = 0; c < 4; c++) alpha.background[c] = (uint16_t)a[1 + c]; for (int c = 0; c < 3; c++) alpha.reserved[c] = (int)a[5 + c]; }
    hm_device_dest d = {};
    unsigned long long ptr, len;
    long long row_pitch, plane_pitch;
    in >> d.layout >> d.dtype >> ptr >> len >> row_pitch >> plane_pitch;
    if (!in) { std::printf("unreadable line: %s\n", text.c_str()); bad++; continue; }
    d.ptr = (void*)(uintptr_t)ptr; d.len = len; d.row_pitch = row_pitch; d.plane_pitch = plane_pitch;
    for (int c = 0; c < 4; c++) { d.scale[c] = 1.0f; d.bias[c] = 0.0f; }
    const void* src = (const void*)(uintptr_t)0x10000000;
    const hm_device_view* pv = v.empty() ? nullptr : &view;
    const hm_device_light* pl = l.empty() ? nullptr : &light;
    const hm_device_tone* pt = t.empty() ? nullptr : &tone;
    int rc = 1;
    if (family == "tensor_dest") rc = hm_to_tensor(fmt, w, h, src, stride, &d, nullptr);
    else if (family == "tensor_view") rc = hm_resample_to_tensor(fmt, w, h, src, stride, pv, &d, nullptr);
    else if (family == "tensor_light") rc = hm_light_to_tensor(fmt, bits, w, h, src, stride, pv, pl, &d, nullptr);
    else if (family == "tensor_tone") rc = hm_tone_to_tensor(fmt, bits, w, h, src, stride, pv, pl, pt, &d, nullptr);
    else if (family == "tensor_alpha") rc = hm_alpha_to_tensor(fmt, bits, w, h, src, stride, pv, pl, pt, &alpha, &d, nullptr);
    std::printf("%s: %d %s\n", text.substr(bar + 3).c_str(), rc, rc ? hm_last_error() : "");
    lines++;
    if (rc >= 0 || rc == HM_ERR_NO_DEVICE) bad++; // (not refused, or only by the device probe)
  }
  std::fprintf(stderr, "%d requests, %d not refused before the device probe\n", lines, bad);
  return lines == 0 || bad ? 1 : 0;
}
