// out_launch.h - host side of the output kernels' launchers: a run-time dtype becomes a type in one place.
#ifndef HM_OUT_LAUNCH_H
#define HM_OUT_LAUNCH_H

#include <hip/hip_fp16.h>
#include <stdint.h>

#include "hm_internal.h"

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

#endif
