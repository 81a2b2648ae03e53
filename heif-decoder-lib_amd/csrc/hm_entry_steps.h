// hm_entry_steps.h — internal: which step pointers a device entry point takes.  The exported entries of the four families (item, frames,
// pipeline, stand-alone tensor) differ in the arguments that are no steps; what they ask of the steps is stated here, once.
// Not part of the C ABI.
#ifndef HM_ENTRY_STEPS_H
#define HM_ENTRY_STEPS_H

#include "hm_devdest.h"

// the entry a request came through: the suffix of its name (dest: none)
enum hm_entry_kind { HM_ENTRY_DEST, HM_ENTRY_VIEW, HM_ENTRY_LIGHT, HM_ENTRY_TONE, HM_ENTRY_ALPHA, HM_ENTRY_OOTF, HM_ENTRY_GAIN, HM_ENTRY_PLANES, HM_ENTRY_PLANES_VIEW,
                     HM_ENTRY_ICC /* hm_icc_to_tensor: the light step, with a profile as its source */,
                     HM_ENTRY_STATS /* the light statistics: a light step, no destination of the caller's */,
                     HM_ENTRY_MEASURED /* hm_decode_item_to_device_measured: light and tone steps, the peak measured */,
                     HM_ENTRY_VIEWS /* hm_decode_item_to_device_views: many views of one item; every step may be NULL */ };

// st: the step pointers the caller passed (those the entry does not have: NULL).  HM_OK, or the refusal:
//   - the step the entry is named after must be given ("null argument"); every other step may be NULL.  An _ootf entry without an OOTF
//     step is the same call without the step: the _alpha entry's rule if an alpha step is given, else the _tone entry's.
//     The statistics entries are named after the light step; the measured entry needs the tone step beside it.
//     The _views entry is named after its arrays, which it judges itself: it takes the steps as the _ootf entry does, each of them optional.
//     view_may_be_null: the family's _view entry takes a NULL view (the frames family: it has no plain entry); a _planes_view entry never does.
//   - a tone, gain or OOTF step needs a light step ("<step>: null light step", the OOTF step's before the tone step's).
//     light_judged_later: the family leaves that to hm_out_check_static, which says it behind the alpha step's own refusals (the
//     stand-alone tensor entries).
inline int hm_entry_steps(int kind, const hm_out_steps& st, bool view_may_be_null = false, bool light_judged_later = false)
{
  if (kind == HM_ENTRY_OOTF && !st.ootf) kind = st.alpha ? HM_ENTRY_ALPHA : HM_ENTRY_TONE;
  const bool given = kind == HM_ENTRY_VIEW          ? st.view || view_may_be_null
                     : kind == HM_ENTRY_PLANES_VIEW ? st.view != nullptr
                     : kind == HM_ENTRY_LIGHT       ? st.light != nullptr
                     : kind == HM_ENTRY_ICC         ? st.light != nullptr && st.icc != nullptr
                     : kind == HM_ENTRY_TONE        ? st.tone != nullptr
                     : kind == HM_ENTRY_ALPHA       ? st.alpha != nullptr
                     : kind == HM_ENTRY_GAIN        ? st.gain != nullptr
                     : kind == HM_ENTRY_STATS       ? st.light != nullptr
                     : kind == HM_ENTRY_MEASURED    ? st.light != nullptr && st.tone != nullptr
                     : kind == HM_ENTRY_VIEWS       ? !st.view && !st.gain
                                                    : true;
  if (!given) return hm_fail(HM_ERR_INVALID_ARG, "null argument");
  if (st.light || light_judged_later) return HM_OK;
  const char* needs_light = st.ootf ? "ootf" : st.gain ? "gain" : st.tone ? "tone" : nullptr;
  return needs_light ? hm_fail(HM_ERR_INVALID_ARG, "%s: null light step", needs_light) : (int)HM_OK;
}

// HM_LIGHT_FROM_ICC in a light step's from_transfer / from_primaries: in one field only it is refused everywhere; in both, by the
// entries that have no profile to read - no_profile names why (the frames family, the stand-alone forms), NULL: the entry reads one
inline bool hm_light_from_icc(const hm_device_light* l) { return l && l->from_transfer == HM_LIGHT_FROM_ICC && l->from_primaries == HM_LIGHT_FROM_ICC; }
inline int hm_entry_icc(const hm_out_steps& st, const char* no_profile)
{
  const hm_device_light* l = st.light;
  if (!l || (l->from_transfer != HM_LIGHT_FROM_ICC && l->from_primaries != HM_LIGHT_FROM_ICC)) return HM_OK;
  if (!hm_light_from_icc(l)) return hm_fail(HM_ERR_INVALID_ARG, "light: HM_LIGHT_FROM_ICC must be set in both from_transfer and from_primaries (they are %d and %d)", l->from_transfer, l->from_primaries);
  return no_profile ? hm_fail(HM_ERR_UNSUPPORTED, "light: HM_LIGHT_FROM_ICC %s", no_profile) : (int)HM_OK;
}

#endif
