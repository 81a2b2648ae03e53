// test_hooks.cpp - the setters and probes the tests and measurement scripts use, kept OUT of the library that ships (r06).
//
// libheif_mi355x.so exports nothing that changes a decode's behaviour from outside the API: hm_knob_set (common.cpp) and
// the kernel getters below are hidden symbols.  This file is linked only into libheif_mi355x_test.so - every object of
// the shipping library plus this one (csrc/Makefile) -, so the tests that need a forced cut, a fault injection or the
// register counts of a kernel run the same object code as production, and code that merely shares a process with the
// production library cannot shorten a chain wave's wait bound or make batches refuse a width.
#include <hip/hip_runtime.h>

#include <cstring>

#include "hm_internal.h"
#include "hm_overlay.h"
#include "residual_tables.h"

extern "C" const void* hm_chain_kernel_of(int log2_ctb, int bytes_per_sample, int mode); // chain.hip
extern "C" const void* hm_residual_kernel();                                             // residual.hip
extern "C" int hm_residual_tables_read(void* out);                                       // ... the table image in the current device's memory
extern "C" const void* hm_tail420_kernel();                                              // filters.hip
extern "C" const void* hm_tail420_kernel16();
extern "C" const void* hm_resample_kernel_of(int index);                                    // resample.hip: NULL behind the last instance
extern "C" const void* hm_resample_staged_kernel_of(int index);                             // ... the instances of k_resample_h_staged
extern "C" const void* hm_resample_batch_kernel_of(int index);                              // ... the batched forms of all three passes
extern "C" const void* hm_resample_multi_kernel_of(int index);                              // ... the multi forms of all three passes
extern "C" const void* hm_planes_view_kernel_of(int index);                                 // planes_view.hip: NULL behind the last instance
extern "C" const void* hm_overlay_kernel_of(int index);                                     // overlay.hip: NULL behind the last instance
extern "C" const void* hm_light_kernel_of(int index);                                       // light.hip: NULL behind the last instance
extern "C" const void* hm_light_finish8_kernel_of(int index);                               // ... the instances of the 8-bit finish from 16-bit samples
extern "C" const void* hm_alpha_kernel_of(int index);                                       // alpha.hip: NULL behind the last instance
extern "C" const void* hm_gain_kernel_of(int index);                                        // gain.hip: NULL behind the last instance
extern "C" const void* hm_stats_kernel_of(int index);                                       // stats.hip: NULL behind the last instance
extern "C" long long hm_light_lds_bytes(int bits, int enc_bits, int encode, int tone, int pass); // ... the dynamic LDS its launchers ask for

extern "C" {

__attribute__((visibility("default"))) int hm_debug_set(const char* name, int value) { return hm_knob_set(name, value); }

// groups of the batch's last hm_batch_execute (1: the single stream) and the image index behind the first of them (hm_overlap_plan.h)
__attribute__((visibility("default"))) int hm_debug_batch_groups(const hm_batch* b, int* first_cut) { return hm_batch_last_groups(b, first_cut); }

// the fused tail of the batch (-1 none, 0 the integer 4:2:0 chain, 1 the float chain) and, in *kernel, the kernel the last launch of a fused tail
// since the previous call picked: 0 none, 1 / 2 k_tail420 on 8- / 16-bit samples, 3 + 2 * (CF - 1) + (16-bit samples) k_tailf<Pix, CF> (the float chain of 9..11-bit 4:2:0 to
// RGB24 / RGBA32 runs on k_tail420's 16-bit instantiation: hm_launch_tailf)
__attribute__((visibility("default"))) int hm_debug_batch_tail(const hm_batch* b, int* kernel)
{
  if (kernel) *kernel = hm_tail_last_launch();
  return hm_batch_tail_kind(b);
}

// registers and scratch of a hot-path kernel as the loaded code object has them (hm_internal.h)
__attribute__((visibility("default"))) int hm_debug_kernel_regs(int which, int a, int b, int c, int out[2])
{
  const void* fn = nullptr;
  if (which == 0) fn = hm_residual_kernel();
  else if (which == 1) fn = hm_tail420_kernel();
  else if (which == 2) fn = hm_chain_kernel_of(a, b, c);
  else if (which == 3) fn = hm_tail420_kernel16();
  else if (which == 4) fn = hm_resample_kernel_of(a); // (the view kernels: a = 0, 1, ... until the call fails)
  else if (which == 5) fn = hm_resample_staged_kernel_of(a); // (k_resample_h_staged; out[1] counts scratch, not LDS)
  else if (which == 6) fn = hm_resample_batch_kernel_of(a); // (k_resample_h_batch, k_resample_h_staged_batch, k_resample_v_batch)
  else if (which == 7) fn = hm_planes_view_kernel_of(a); // (k_planes_resample_h, k_planes_resample_v, k_planes_view_nearest)
  else if (which == 8) fn = hm_overlay_kernel_of(a); // (k_overlay: RGB24, RGBA32, planes)
  else if (which == 9) fn = hm_light_kernel_of(a); // (k_light_tensor, k_light_nearest, k_light_h, k_light_v; out[1] counts scratch, not LDS)
  else if (which == 10) fn = hm_light_finish8_kernel_of(a); // (k_light_tensor<2, 3, uint8_t, ...>, k_light_nearest<uint16_t, 3, uint8_t>)
  else if (which == 11) fn = hm_alpha_kernel_of(a); // (k_alpha_tensor, k_alpha_nearest, k_alpha_h, k_alpha_v; out[1] counts scratch, not LDS)
  else if (which == 12) fn = hm_gain_kernel_of(a); // (k_gain_tensor, k_gain_nearest, k_gain_map_h, k_gain_map_v, k_gain_v; out[1] counts scratch, not LDS)
  else if (which == 13) fn = hm_stats_kernel_of(a); // (k_light_stats; out[1] counts scratch, not LDS)
  else if (which == 14) fn = hm_resample_multi_kernel_of(a); // (k_resample_h_multi, k_resample_h_staged_multi, k_resample_v_multi; out[1] counts scratch, not LDS)
  hipFuncAttributes fa;
  if (!fn || !out || hipFuncGetAttributes(&fa, fn) != hipSuccess) return -1;
  out[0] = fa.numRegs;
  out[1] = (int)fa.localSizeBytes;
  return 0;
}

// the dynamic LDS, in bytes, a launch of the light kernels asks for with tables of (bits, enc_bits), re-encoding or not, with a tone step or
// not (tone: bit 0 the tone step, bit 1 the OOTF step); pass 0: the pointwise and nearest kernels, 1: k_light_h, 2: k_light_v
// (hipFuncGetAttributes does not see dynamic LDS)
__attribute__((visibility("default"))) long long hm_debug_light_lds(int bits, int enc_bits, int encode, int tone, int pass)
{
  return hm_light_lds_bytes(bits, enc_bits, encode, tone, pass);
}

// k_overlay on its own (measurement scripts: tools/bench_overlay.py): the layer table is uploaded and the kernel queued on `stream`;
// *pinned / *device are the table's blocks, handed back through hm_debug_overlay_release once the stream has drained
__attribute__((visibility("default"))) int hm_debug_overlay_launch(const hm_overlay_job* job, const hm_overlay_layer* layers, int n, void** pinned, void** device, void* stream)
{
  return hm_launch_overlay(job, layers, n, pinned, device, (hipStream_t)stream);
}
__attribute__((visibility("default"))) void hm_debug_overlay_release(void* pinned, void* device)
{
  if (pinned) hm_pool_pinned_free(pinned);
  if (device) hm_pool_device_free(device);
}

// k_residual's constant tables (residual_tables.h), HM_RT_BYTES bytes into `out`: from_device = 0 the image as the host compiler
// worked it out (no HIP call: tests/test_residual_tables.py runs without a GPU), 1 the bytes the kernel reads on the current device
// -> the size, or < 0
__attribute__((visibility("default"))) int hm_debug_residual_tables(int from_device, uint8_t* out, int capacity)
{
  if (!out || capacity < HM_RT_BYTES) return -1;
  if (from_device) {
    const int rc = hm_residual_tables_read(out);
    return rc < 0 ? rc : HM_RT_BYTES;
  }
  static constexpr hm_residual_tables image = hm_make_residual_tables();
  std::memcpy(out, image.b, HM_RT_BYTES);
  return HM_RT_BYTES;
}

} // extern "C"
