// out_launch.h - host side of the output kernels' launchers: a run-time dtype, layout or channel count becomes a template argument in
// one place, and so do the grid of a wave per row, the test for 16-byte accesses and the rule which instances exist.
#ifndef HM_OUT_LAUNCH_H
#define HM_OUT_LAUNCH_H

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <type_traits>

#include "hm_devdest.h"

// A run-time dtype (HM_DEV_*) becomes a type here and nowhere else: with_dtype answers f(TypeTag<T>()), T the destination's element
// type.  Which instances exist for a type stays with the launcher (if constexpr on the tag's type): f answers the status of its
// launch, or NO_KERNEL_INSTANCE where it has none - as with_dtype does for a dtype it does not know -, and the launcher's own refusal follows.
enum { NO_KERNEL_INSTANCE = 1 }; // (never a status: those are <= 0)
template <typename T> struct TypeTag { typedef T type; };
template <typename F> int with_dtype(int dtype, F&& f)
{
  switch (dtype) {
    case HM_DEV_U8: return f(TypeTag<uint8_t>());
    case HM_DEV_U16: return f(TypeTag<uint16_t>());
    case HM_DEV_F16: return f(TypeTag<__half>());
    case HM_DEV_F32: return f(TypeTag<float>());
  }
  return NO_KERNEL_INSTANCE;
}

// Two run-time choices between two values each become template arguments: f(std::bool_constant<a>(), std::bool_constant<b>()), for the
// layout (CHW or not) beside the channels (4 or 3), and for the sample width (2 bytes or 1) beside the channels.
template <typename F> auto with_flags(bool a, bool b, F&& f)
{
  if (a) return b ? f(std::true_type(), std::true_type()) : f(std::true_type(), std::false_type());
  return b ? f(std::false_type(), std::true_type()) : f(std::false_type(), std::false_type());
}

// Is there an instance of a step's pointwise and nearest kernels for elements of OutT from samples of SB bytes, OC channels written,
// LIT: with a light step?  A float type; the integer type of the samples' own width; with a light step, bytes from a deeper
// three-channel image (the 8-bit finish, hm_device_tone.out_bits == 8); nothing else.
template <typename OutT, int SB, int OC, bool LIT> constexpr bool has_instance()
{
  if (!std::is_integral<OutT>::value || sizeof(OutT) == SB) return true;
  return sizeof(OutT) == 1 && SB == 2 && OC == 3 && LIT;
}

// the grid of the kernels whose wave takes 64 columns (pixels, or pixel groups) of ONE row: workgroups of 4 waves, z for planes
static inline dim3 grid_64x4(int columns, int rows, int planes = 1) { return dim3((unsigned)((columns + 63) / 64), (unsigned)((rows + 3) / 4), (unsigned)planes); }

// may a streaming kernel take 16-byte accesses on both sides (its VEC instance)?
static inline bool aligned16(const void* src, int src_stride, const void* dst, const hm_dest_plan* p)
{
  return ((uintptr_t)src % 16) == 0 && (src_stride % 16) == 0 && ((uintptr_t)dst % 16) == 0 && (p->row_pitch % 16) == 0 &&
         (p->layout != HM_DEV_LAYOUT_CHW || (p->plane_pitch % 16) == 0);
}

#endif
