// The host side of a Gauss-Newton solve, stated once for every loop of the library: the step (solve the 6x6 system, left-multiply the
// pose by exp(delta), measure |delta|), the round loop around it, the driver of one level of the loops whose round is one launch, and
// the coarse-to-fine walk over pyramid levels.  Where a round's
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

// ---- one level of a host-driven loop whose round is one launch (rpe_icp_rgbd, the volume term, the volume colour term and their
// coarse-to-fine forms).  Where an entry point wants a level's figures, any of them null; cost2 / matched2 are the second term's, for a
// round that carries one
struct GnOut {
  int* iters = nullptr; double* step = nullptr; double* cost = nullptr; int64_t* matched = nullptr;
  double* cost2 = nullptr; int64_t* matched2 = nullptr;
  // what a level of a coarse_to_fine walk reports: its rounds into `it`, everything else at the finest level only
  GnOut at_level(bool fine, int* it) const {
    GnOut o = fine ? *this : GnOut{};
    o.iters = it;
    return o;
  }
};
// gn_host_rounds from round 0 over round(pose12, ne, second): second[0 .. 1] is the second term's cost and rows of the record, the
// driver's own words, zero until a round writes them.  A refused system: out.iters = the refused round, nothing else is written, and
// refused(round, weight, second term's rows) words the failure and gives the code.  A round's own non-zero code comes back with nothing
// written.  Otherwise the figures of the last round run go into whichever outputs are there.
template <class Round, class Refused>
inline int gn_host_level(Round round, double rel_floor, int max_iter, double tol, double* pose12, const GnOut& out, Refused refused) {
  GnRun run;
  double second[2] = {0, 0};
  const int rc = gn_host_rounds([&](const double* pose, double* ne) { return round(pose, ne, second); }, rel_floor, 1.0, max_iter, tol, pose12,
                                &run);
  if (rc == kGnRefused) {
    if (out.iters) *out.iters = run.it;
    return refused(run.it, run.weight, second[1]);
  }
  if (rc) return rc;
  run.report(out.iters, out.step, out.cost, out.matched);
  if (out.cost2) *out.cost2 = second[0];
  if (out.matched2) *out.matched2 = (int64_t)second[1];
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
