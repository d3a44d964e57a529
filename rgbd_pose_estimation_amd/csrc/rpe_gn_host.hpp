// The host side of a Gauss-Newton solve, stated once for every loop of the library: the step (solve the 6x6 system, left-multiply the
// pose by exp(delta), measure |delta|), the round loop around it, and the coarse-to-fine walk over pyramid levels.  Where a round's
// record comes from -- a launch and a host wait, a resident grid, the ranks' exchange -- is the caller's callable; so is every message.
// This header includes no HIP header and no rpe_host.hpp: RPE_OK and RPE_MAX_LEVELS are the includer's (include/rgbd_pose_hip.h in the
// library, two enumerators in tests/cpp/gn_host.cpp).
#pragma once
#include "../include/rpe/linalg.hpp"
#include <cstdint>

namespace rpeh __attribute__((visibility("hidden"))) {

// One step on the record ne (H upper triangle 21 | g 6 | ...): pose12 <- exp(delta) pose12, *step = |delta|.  false, and pose12
// untouched, where the solve refuses the system (a pivot at or below rel_floor x its diagonal entry: rpe::pivot_floor)
inline bool gn_update(const double* ne, double rel_floor, double* pose12, double* step) {
  double d[6];
  if (!rpe::solve_normal_eq6(ne, d, rel_floor)) return false;
  rpe::se3_left_update(d, pose12);
  *step = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  return true;
}

// internal, never returned through the C ABI (beside kResidentLost ... of rpe_host.hpp): the solve refused a round's system
constexpr int kGnRefused = -1003;
// where a loop stands: whole rounds done, the last |delta|, cost (record word 27 x the caller's scale) and weight (word 28) of the last record
struct GnRun {
  int it = 0; double step = 0, cost = 0, weight = 0;
  // ... into whichever of its outputs the entry point was given
  void report(int* iters_out, double* last_step, double* final_cost, int64_t* matched = nullptr) const {
    if (iters_out) *iters_out = it;
    if (last_step) *last_step = step;
    if (final_cost) *final_cost = cost;
    if (matched) *matched = (int64_t)weight;
  }
};

// Rounds run->it .. max_iter - 1 (a loop that a lost resident grid left after `it` whole rounds goes on from there): round(pose12, ne)
// fills the round's 32-double record or returns its own non-zero code, which ends the loop at once.  A refused system ends it with
// kGnRefused, run->it the refused round and run's cost / weight that record's; the caller words the failure.  A step under tol ends it
// with that round counted.
template <class Round>
inline int gn_host_rounds(Round round, double rel_floor, double cost_scale, int max_iter, double tol, double* pose12, GnRun* run) {
  for (; run->it < max_iter; run->it++) {
    double ne[32];
    if (int rc = round(pose12, ne)) return rc;
    run->cost = cost_scale * ne[27]; run->weight = ne[28];
    if (!gn_update(ne, rel_floor, pose12, &run->step)) return kGnRefused;
    if (run->step < tol) { run->it++; break; }
  }
  return RPE_OK;
}

// ---- coarse to fine: iters_per_level[l] rounds and the gate dist_thr_per_level[l] (null: one default gate) at level l, 0 = finest
enum PyramidArg { kPyramidOk = 0, kPyramidLevels, kPyramidRounds, kPyramidGate };
// which complaint a call deserves: levels outside 1 .. RPE_MAX_LEVELS (or no round counts at all), the first level whose round count
// is negative (0 at the finest) or whose gate is not >= 0 (*bad_level).  The entry point words it
inline PyramidArg pyramid_args(int levels, const int* iters_per_level, const double* dist_thr_per_level, int* bad_level) {
  if (!iters_per_level || levels < 1 || levels > RPE_MAX_LEVELS) return kPyramidLevels;
  for (int l = 0; l < levels; l++) {
    *bad_level = l;
    if (iters_per_level[l] < (l == 0 ? 1 : 0)) return kPyramidRounds;
    if (dist_thr_per_level && !(dist_thr_per_level[l] >= 0)) return kPyramidGate;
  }
  return kPyramidOk;
}
// the walk from the coarsest level down: level_fn(l, rounds, gate, fine, &it) for every level with rounds to run (fine: l == 0, the
// level whose figures the caller reports), iters_out[l] = it (0 for a skipped level), THEN the return on the first non-zero code
template <class LevelFn>
inline int coarse_to_fine(int levels, const int* iters_per_level, const double* dist_thr_per_level, double default_gate, int* iters_out,
                          LevelFn level_fn) {
  for (int l = levels - 1; l >= 0; l--) {
    int it = 0, rc = RPE_OK;
    if (iters_per_level[l] > 0)
      rc = level_fn(l, iters_per_level[l], dist_thr_per_level ? dist_thr_per_level[l] : default_gate, l == 0, &it);
    if (iters_out) iters_out[l] = it;
    if (rc) return rc;
  }
  return RPE_OK;
}

}  // namespace rpeh
