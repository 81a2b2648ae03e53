// overlap_plan_check.cpp - a stand-alone host program over the schedule of hm_batch_execute's overlapped groups
// (csrc/hm_overlap_plan.h: hm_plan_groups).  Built with -fsanitize=address,undefined by tests/test_overlap_plan_host.py.  It walks
// every image count 0..400 with SAMPLED pictures per image (14 values of 1..64) and resident wave counts (16 values of 1..8192,
// the edges and the neighbours of 5120 among them) through the automatic schedule, the explicit
// counts and the two knobs, and holds every plan to: boundaries that are strictly increasing image indices from 0 to the image
// count (every image in exactly one group, no group empty), one group below the threshold, one group wherever a condition of the
// automatic schedule fails, no group whose partial last round the chain launcher would launch on its own (that condition spelt out
// here).  Which of the two candidate cuts is taken is recomputed with the header's own formula - that part pins the rule, it is no
// second opinion; the independent expectations are the structural properties and the hand-written cases at the end.
#include <cstdio>
#include <vector>

#include "hm_overlap_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s (images %d, per image %d, resident %ld, requested %d, min_pics %ld, cut %d)\n", __FILE__, __LINE__, #c, \
                                                in.n_images, in.per_image, in.resident, in.requested, in.min_pics, in.forced_cut); return 1; } } while (0)

// the properties every plan has; the groups it holds
static int well_formed(const hm_overlap_in& in, const hm_overlap_plan& p)
{
  const int n = in.n_images > 0 ? in.n_images : 0;
  CHECK(p.groups >= 1 && p.groups <= HM_OVERLAP_MAX_GROUPS);
  CHECK(p.bound[0] == 0 && p.bound[p.groups] == n);
  std::vector<int> seen((size_t)n, 0);
  for (int g = 0; g < p.groups; g++) {
    if (p.groups > 1) CHECK(p.bound[g] < p.bound[g + 1]); // strictly increasing: no group is empty
    CHECK(p.bound[g] <= p.bound[g + 1]);
    for (int i = p.bound[g]; i < p.bound[g + 1]; i++) seen[(size_t)i]++;
  }
  for (int v : seen) CHECK(v == 1); // every image exactly once
  return 0;
}

int main()
{
  static const long residents[] = {1, 2, 3, 47, 48, 64, 255, 256, 1000, 2560, 4096, 5119, 5120, 5121, 8191, 8192};
  static const int per_images[] = {1, 2, 3, 4, 5, 7, 8, 16, 31, 47, 48, 49, 63, 64};
  long plans = 0, split = 0;
  for (int n = 0; n <= 400; n++) {
    for (int per : per_images) {
      for (long resident : residents) {
        hm_overlap_in in{};
        in.n_images = n; in.per_image = per; in.resident = resident; in.per_picture = 1; in.eligible = 1; in.split_fraction = 4;
        const long long pics = (long long)n * per;
        // ---- automatic ----
        hm_overlap_plan p = hm_plan_groups(in);
        if (well_formed(in, p)) return 1;
        plans++;
        const bool above = n >= 2 && pics >= (long long)HM_OVERLAP_MIN_ROUNDS * resident;
        if (!above) CHECK(p.groups == 1); // one group below the threshold
        // the two cuts the schedule considers: equal halves, then the last image boundary in front of a whole number of rounds
        // (less than an image short of it, never a picture into the next round); neither group may be a count whose partial
        // last round the chain launcher would give a launch of its own
        long long rounds = (pics / 2 + resident / 2) / resident;
        if (rounds < 1) rounds = 1;
        const long long cand[2] = {n / 2, rounds * resident / per};
        int want = 0;
        for (int k = 0; k < 2 && !want && above; k++) {
          const long long c = cand[k];
          if (c < 1 || c > n - 1) continue;
          if (k == 1) CHECK(rounds * resident - c * per >= 0 && rounds * resident - c * per < per);
          if (!hm_overlap_partial_round(c * per, resident, in.split_fraction) && !hm_overlap_partial_round(pics - c * per, resident, in.split_fraction)) want = (int)c;
        }
        CHECK(p.groups == (want ? 2 : 1));
        if (p.groups == 2) {
          split++;
          CHECK(p.bound[1] == want);
          for (int g = 0; g < 2; g++) {
            const long long m = (long long)(p.bound[g + 1] - p.bound[g]) * per, r = m % resident;
            CHECK(!(m > resident && r > 0 && 4 * (m / resident) * r <= resident)); // (chain.hip: hm_launch_chain's condition, spelt out)
          }
        }
        // ... and one group wherever one of its conditions fails
        for (int which = 0; which < 4; which++) {
          hm_overlap_in off = in;
          if (which == 0) off.eligible = 0;
          if (which == 1) off.per_picture = 0;
          if (which == 2) off.resident = 0;
          if (which == 3) off.requested = 1;
          const hm_overlap_plan q = hm_plan_groups(off);
          if (well_formed(off, q)) return 1;
          CHECK(q.groups == 1);
        }
        // ---- the knobs: the threshold in pictures, the cut's image index (clamped into the batch) ----
        for (long min_pics : {1L, 20L, 1000L}) {
          for (int cut : {0, 1, 2, 4, n - 1, n, n + 7}) {
            hm_overlap_in k = in;
            k.min_pics = min_pics; k.forced_cut = cut;
            k.per_picture = (n + per) & 1; // (the knob replaces the load criterion)
            const hm_overlap_plan q = hm_plan_groups(k);
            if (well_formed(k, q)) return 1;
            plans++;
            CHECK(q.groups == (n >= 2 && pics >= min_pics ? 2 : 1));
            if (q.groups == 2 && cut >= 1 && cut <= n - 1) CHECK(q.bound[1] == cut);
          }
        }
      }
    }
    // ---- explicit counts: equal groups, one stream where there is no image for each ----
    for (int k = 2; k <= 8; k++) {
      hm_overlap_in in{};
      in.n_images = n; in.per_image = 4; in.eligible = 1; in.requested = k;
      const hm_overlap_plan p = hm_plan_groups(in);
      if (well_formed(in, p)) return 1;
      CHECK(p.groups == (n >= k ? k : 1));
      for (int g = 0; g < p.groups && p.groups > 1; g++) {
        const int m = p.bound[g + 1] - p.bound[g];
        CHECK(m == n / k || m == n / k + 1);
      }
      in.eligible = 0;
      CHECK(hm_plan_groups(in).groups == 1);
    }
  }
  {
    // the headline batch: 384 images of 48 pictures on 5120 resident waves - 3.6 rounds, equal halves of 1.8 rounds
    hm_overlap_in in{};
    in.n_images = 384; in.per_image = 48; in.resident = 5120; in.per_picture = 1; in.eligible = 1; in.split_fraction = 4;
    hm_overlap_plan p = hm_plan_groups(in);
    CHECK(p.groups == 2 && p.bound[1] == 192 && p.bound[2] == 384);
    in.n_images = 448; // halves of 2.1 rounds would each end in a partial-round launch: the cut behind two rounds
    p = hm_plan_groups(in);
    CHECK(p.groups == 2 && p.bound[1] == 213);
    in.n_images = 256; // 2.4 rounds: halves of 1.2 no, one round + 1.4 rounds
    p = hm_plan_groups(in);
    CHECK(p.groups == 2 && p.bound[1] == 106);
    in.n_images = 224; // 2.1 rounds: neither cut leaves both groups without a partial-round launch
    CHECK(hm_plan_groups(in).groups == 1);
    in.n_images = 192; // 1.8 rounds, and BASELINE config 3 on one GPU (128 images, 1.2 rounds): one stream
    CHECK(hm_plan_groups(in).groups == 1);
    in.n_images = 128;
    CHECK(hm_plan_groups(in).groups == 1);
    in.split_fraction = 0; in.n_images = 224; // (the launcher never splits: nothing to avoid)
    CHECK(hm_plan_groups(in).groups == 2 && hm_plan_groups(in).bound[1] == 112);
    in.n_images = -3; in.per_image = 0;
    CHECK(hm_plan_groups(in).groups == 1 && hm_plan_groups(in).bound[1] == 0);
  }
  std::printf("overlap plan: ok (%ld plans, %ld of the automatic ones in two groups)\n", plans, split);
  return 0;
}
