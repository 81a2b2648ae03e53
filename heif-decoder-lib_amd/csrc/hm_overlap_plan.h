// hm_overlap_plan.h - how hm_batch_execute cuts a step's images into groups that run on streams of their own (batch.cpp), as a
// pure function: no HIP types, nothing read from anywhere else, so that a stand-alone host program can walk it
// (tests/host/overlap_plan_check.cpp).
//
// Why groups: the fused tail of one group fills the issue slots that the chain kernel of another leaves while it drains (a wave
// per picture: the last pictures of a launch run on an emptying device).  Why so few: every group adds a drain of its own, and a
// group that is not a whole number of chain rounds ends in a partial round (chain.hip: hm_launch_chain).
#ifndef HM_OVERLAP_PLAN_H
#define HM_OVERLAP_PLAN_H

#include <initializer_list>

#define HM_OVERLAP_MAX_GROUPS 8
// the automatic schedule engages from this many rounds of resident chain waves on (profiles/batch_overlap.txt: below two rounds
// a second group costs more in its own drain than it fills of the first's)
#define HM_OVERLAP_MIN_ROUNDS 2

struct hm_overlap_in {
  int n_images;         // images of the batch, queued one after the other
  int per_image;        // pictures of every image
  long resident;        // chain waves the device holds at once (chain.hip: ChainPlan.resident; 0: not known)
  int per_picture;      // the chain launcher would take a wave per picture for the whole batch
  int split_fraction;   // chain.hip's split_round_fraction: a launch of k x resident + r pictures gives its last r a launch of their
                        //   own if split_fraction x k x r <= resident (0: never)
  int eligible;         // the batch runs the fused tail on one class with colour attached
  int requested;        // hm_batch_set_concurrency: 0 automatic, 1 one stream, 2..8 that many equal groups
  long min_pics;        // knob overlap_min_pics: > 0 replaces the load criterion of the automatic schedule (a wave per picture,
                        //   HM_OVERLAP_MIN_ROUNDS x resident pictures, no partial-round launch) by "at least this many pictures"
  int forced_cut;       // knob overlap_cut: > 0 the image index of the automatic schedule's cut
};

// group g holds the images [bound[g], bound[g + 1]); bound[0] = 0, bound[groups] = n_images
struct hm_overlap_plan {
  int groups;
  int bound[HM_OVERLAP_MAX_GROUPS + 1];
};

// would the chain launcher give the partial last round of a launch of `pics` pictures a launch of its own (chain.hip: hm_launch_chain)?
static inline int hm_overlap_partial_round(long long pics, long resident, int split_fraction)
{
  if (resident <= 0 || split_fraction <= 0 || pics <= resident) return 0;
  const long long rounds = pics / resident, r = pics % resident;
  return r > 0 && split_fraction * rounds * r <= resident;
}

static inline hm_overlap_plan hm_plan_groups(const hm_overlap_in& in)
{
  hm_overlap_plan p;
  p.groups = 1;
  for (int g = 0; g <= HM_OVERLAP_MAX_GROUPS; g++) p.bound[g] = 0;
  const int n = in.n_images > 0 ? in.n_images : 0;
  p.bound[1] = n;
  if (!in.eligible || in.per_image <= 0 || n < 2 || in.requested == 1) return p;
  if (in.requested >= 2) { // the explicit count: equal groups of whole images, if there is an image for each
    const int k = in.requested > HM_OVERLAP_MAX_GROUPS ? HM_OVERLAP_MAX_GROUPS : in.requested;
    if (n < k) return p;
    p.groups = k;
    for (int g = 0; g <= k; g++) p.bound[g] = (int)((long long)n * g / k);
    return p;
  }
  // automatic: two groups once the batch is several rounds of a wave per picture (fewer pictures take finer cuts, whose waves
  // fill the device without any help - and the single-image paths must stay what they are)
  const long long pics = (long long)n * in.per_image;
  int cut = 0;
  if (in.min_pics > 0) {
    if (pics < in.min_pics) return p;
    cut = n / 2;
  }
  else {
    if (!in.per_picture || in.resident <= 0 || pics < (long long)HM_OVERLAP_MIN_ROUNDS * in.resident) return p;
    // Where the cut goes (profiles/batch_overlap.txt: 200 ... 512 images of 48 pictures, every whole-round cut and the halves).
    // The cuts that measured slower than one stream were those with a group whose count ends in a partial round small enough
    // for the launcher to give it a launch of its own beside the full rounds (that launch then shares the device with the
    // other group's kernels too), and those that leave the second group less than a round.  So: equal halves if neither half
    // is such a count; else the last image boundary at which the first group is still whole chain rounds (the count of rounds
    // nearest to half of the batch: the second group is then a round or more), under the same condition; else one stream.
    const int halves = n / 2;
    long long rounds = (pics / 2 + in.resident / 2) / in.resident;
    if (rounds < 1) rounds = 1;
    const long long whole = rounds * in.resident / in.per_image;
    for (const long long c : {(long long)halves, whole}) {
      if (c < 1 || c > n - 1) continue;
      if (hm_overlap_partial_round(c * in.per_image, in.resident, in.split_fraction) || hm_overlap_partial_round(pics - c * in.per_image, in.resident, in.split_fraction)) continue;
      cut = (int)c;
      break;
    }
    if (!cut && in.forced_cut <= 0) return p;
  }
  if (in.forced_cut > 0) cut = in.forced_cut;
  if (cut < 1) cut = 1;
  if (cut > n - 1) cut = n - 1;
  p.groups = 2;
  p.bound[1] = cut;
  p.bound[2] = n;
  return p;
}

#endif
