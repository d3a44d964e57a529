// CPU: the host side of every Gauss-Newton loop of the library (csrc/rpe_gn_host.hpp) on scripted rounds -- lambdas that hand out canned
// 32-double records -- and the coarse-to-fine walk on scripted levels.  The header includes no HIP header, so the two names it takes
// from the C header are defined here.  Built with -fsanitize=address,undefined: nothing here links the library or the HIP runtime.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

enum { RPE_OK = 0, RPE_MAX_LEVELS = 4 };
#include "../../rgbd_pose_estimation_amd/csrc/rpe_gn_host.hpp"
using namespace rpeh;

#define CHECK(x) do { if (!(x)) { std::printf("gn_host: FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static const int kDiag[6] = {0, 6, 11, 15, 18, 20};   // where the diagonal of H sits in the packed upper triangle
static const double kFloor = 1e-12;
static const double kStart[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.2, 0.3};

// H = 2 I, g = -0.2 10^-k (1 .. 6): delta = 0.1 10^-k (1 .. 6), |delta| = 0.954 10^-k; cost 10 + k, weight 100 + k
static void shrinking(int k, double* ne) {
  for (int i = 0; i < 32; i++) ne[i] = 0;
  for (int i = 0; i < 6; i++) { ne[kDiag[i]] = 2.0; ne[21 + i] = -0.2 * std::pow(10.0, -k) * (i + 1); }
  ne[27] = 10 + k; ne[28] = 100 + k;
}
// the three primitives by hand
static bool by_hand(const double* ne, double* pose, double* step) {
  double d[6];
  if (!rpe::solve_normal_eq6(ne, d, kFloor)) return false;
  rpe::se3_left_update(d, pose);
  *step = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  return true;
}
static bool same(const double* a, const double* b, int n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
  // ---- gn_update: bitwise the three primitives; a zero record is refused and nothing is written
  {
    double ne[32], p[12], q[12], s = -1, t = -1;
    for (int i = 0; i < 32; i++) ne[i] = 0.01 * ((i * 7) % 5 - 2);                // a full system: small off-diagonals ...
    for (int i = 0; i < 6; i++) ne[kDiag[i]] = 3.0 + i;                            // ... under a dominant diagonal
    for (int i = 0; i < 6; i++) ne[21 + i] = 0.05 * (i - 2.5);
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    CHECK(gn_update(ne, kFloor, p, &s) && by_hand(ne, q, &t));
    CHECK(same(p, q, 12) && same(&s, &t, 1) && s > 0 && !same(p, kStart, 12));
    double zero[32] = {0};
    s = -1;
    CHECK(!gn_update(zero, kFloor, p, &s) && same(p, q, 12) && s == -1);
  }
  // ---- round count: the round that goes under tol is counted; figures of the last record; the pose of four steps by hand
  {
    double p[12], q[12], t = 0;
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    int calls = 0;
    GnRun run;
    const int rc = gn_host_rounds([&](const double* pose, double* ne) { CHECK(pose == p); shrinking(calls++, ne); return 0; }, kFloor, 1.0, 50,
                                  1e-3, p, &run);
    CHECK(rc == RPE_OK && run.it == 4 && calls == 4 && run.cost == 13 && run.weight == 103);
    for (int k = 0; k < 4; k++) { double ne[32]; shrinking(k, ne); CHECK(by_hand(ne, q, &t)); }
    CHECK(same(p, q, 12) && same(&run.step, &t, 1) && run.step < 1e-3 && run.step > 9e-4);
  }
  // ---- limits: max_iter is reached exactly; a loop taken up at round 3 of 5 makes two calls; nothing left to do: no call
  {
    double p[12];
    std::memcpy(p, kStart, sizeof p);
    int calls = 0;
    auto round = [&](const double*, double* ne) { calls++; shrinking(0, ne); return 0; };
    GnRun run;
    CHECK(gn_host_rounds(round, kFloor, 1.0, 5, 0.0, p, &run) == RPE_OK && run.it == 5 && calls == 5);
    GnRun taken_up;
    taken_up.it = 3; calls = 0;
    CHECK(gn_host_rounds(round, kFloor, 1.0, 5, 0.0, p, &taken_up) == RPE_OK && taken_up.it == 5 && calls == 2);
    GnRun done;
    done.it = 5; done.step = 0.25; done.cost = 4; done.weight = 8; calls = 0;
    CHECK(gn_host_rounds(round, kFloor, 1.0, 5, 0.0, p, &done) == RPE_OK && calls == 0);
    CHECK(done.it == 5 && done.step == 0.25 && done.cost == 4 && done.weight == 8);
  }
  // ---- a system refused at round 2: the sentinel, it == 2, that record's cost and weight, pose and step as after round 1
  {
    double p[12], q[12], t = 0;
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    int calls = 0;
    GnRun run;
    const int rc = gn_host_rounds([&](const double*, double* ne) {
      shrinking(calls, ne);
      if (calls++ == 2) { for (int i = 0; i < 27; i++) ne[i] = 0; ne[27] = 7; ne[28] = 9; }
      return 0;
    }, kFloor, 1.0, 50, 0.0, p, &run);
    CHECK(rc == kGnRefused && rc != RPE_OK && run.it == 2 && calls == 3 && run.cost == 7 && run.weight == 9);
    for (int k = 0; k < 2; k++) { double ne[32]; shrinking(k, ne); CHECK(by_hand(ne, q, &t)); }
    CHECK(same(p, q, 12) && same(&run.step, &t, 1));
  }
  // ---- a round's own error at round 2 comes back as it is, at once: it == 2, the figures of round 1
  {
    double p[12];
    std::memcpy(p, kStart, sizeof p);
    int calls = 0;
    GnRun run;
    const int rc = gn_host_rounds([&](const double*, double* ne) { shrinking(calls, ne); return calls++ == 2 ? -77 : 0; }, kFloor, 1.0, 50, 0.0,
                                  p, &run);
    CHECK(rc == -77 && run.it == 2 && calls == 3 && run.cost == 11 && run.weight == 101);
  }
  // ---- cost_scale multiplies the cost only
  {
    double p[12], q[12];
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    int calls = 0;
    auto round = [&](const double*, double* ne) { shrinking(calls++, ne); return 0; };
    GnRun plain, scaled;
    CHECK(gn_host_rounds(round, kFloor, 1.0, 3, 0.0, p, &plain) == RPE_OK);
    calls = 0;
    CHECK(gn_host_rounds(round, kFloor, 2.5, 3, 0.0, q, &scaled) == RPE_OK);
    CHECK(plain.cost == 12 && scaled.cost == 2.5 * 12 && scaled.weight == plain.weight && scaled.it == plain.it);
    CHECK(same(&scaled.step, &plain.step, 1) && same(p, q, 12));
  }
  // ---- gn_host_level: the level driver on the same scripted rounds, whose second term is cost 20 + k and rows 200 + k at round k
  {
    struct Words { int it = -1; double step = -1, cost = -1, cost2 = -1; int64_t matched = -1, matched2 = -1; };
    auto all = [](Words& w) { return GnOut{&w.it, &w.step, &w.cost, &w.matched, &w.cost2, &w.matched2}; };
    auto untouched = [](const Words& w) { return w.step == -1 && w.cost == -1 && w.cost2 == -1 && w.matched == -1 && w.matched2 == -1; };
    int calls = 0, refusals = 0;
    auto round = [&](const double*, double* ne, double* second) { shrinking(calls, ne); second[0] = 20 + calls; second[1] = 200 + calls; calls++; return 0; };
    auto never = [&](int, double, double) { refusals++; return -9; };
    double p[12], q[12], t = 0;
    // a tol stop in round 3: every figure is that round's, the pose that of gn_host_rounds
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    Words w;
    CHECK(gn_host_level(round, kFloor, 50, 1e-3, p, all(w), never) == RPE_OK && calls == 4 && refusals == 0);
    for (int k = 0; k < 4; k++) { double ne[32]; shrinking(k, ne); CHECK(by_hand(ne, q, &t)); }
    CHECK(same(p, q, 12) && w.it == 4 && same(&w.step, &t, 1) && w.cost == 13 && w.matched == 103 && w.cost2 == 23 && w.matched2 == 203);
    // outputs are written only where there is one: none at all; the rounds alone (a coarser level of a walk); all but the second term's
    calls = 0;
    CHECK(gn_host_level(round, kFloor, 2, 0.0, p, GnOut{}, never) == RPE_OK && calls == 2);
    Words coarse, geo;
    int it = -1;
    calls = 0;
    CHECK(gn_host_level(round, kFloor, 2, 0.0, p, all(coarse).at_level(false, &it), never) == RPE_OK && it == 2 && coarse.it == -1 && untouched(coarse));
    calls = 0;
    CHECK(gn_host_level(round, kFloor, 2, 0.0, p, GnOut{&geo.it, &geo.step, &geo.cost, &geo.matched}, never) == RPE_OK);
    CHECK(geo.it == 2 && geo.step > 0 && geo.cost == 11 && geo.matched == 101 && geo.cost2 == -1 && geo.matched2 == -1);
    Words fine;
    calls = 0;
    CHECK(gn_host_level(round, kFloor, 2, 0.0, p, all(fine).at_level(true, &it), never) == RPE_OK && it == 2 && fine.it == -1);
    CHECK(fine.cost == 11 && fine.matched == 101 && fine.cost2 == 21 && fine.matched2 == 201);
    // a round without a second term leaves the driver's zeros
    Words plain;
    calls = 0;
    CHECK(gn_host_level([&](const double*, double* ne, double*) { shrinking(calls++, ne); return 0; }, kFloor, 2, 0.0, p, all(plain), never) == RPE_OK);
    CHECK(plain.cost == 11 && plain.cost2 == 0 && plain.matched2 == 0);
    // a system refused at round 2: iters = 2, no other output, and the hook has that round's weight and second-term rows; its code comes back
    Words r;
    int r_it = -1;
    double r_weight = -1, r_rows2 = -1;
    calls = 0;
    std::memcpy(p, kStart, sizeof p); std::memcpy(q, kStart, sizeof q);
    const int rc = gn_host_level([&](const double*, double* ne, double* second) {
      shrinking(calls, ne);
      second[0] = 20 + calls; second[1] = 200 + calls;
      if (calls++ == 2) { for (int i = 0; i < 27; i++) ne[i] = 0; ne[27] = 7; ne[28] = 9; }
      return 0;
    }, kFloor, 50, 0.0, p, all(r), [&](int at, double weight, double rows2) { r_it = at; r_weight = weight; r_rows2 = rows2; return -42; });
    CHECK(rc == -42 && calls == 3 && r.it == 2 && untouched(r) && r_it == 2 && r_weight == 9 && r_rows2 == 202);
    for (int k = 0; k < 2; k++) { double ne[32]; shrinking(k, ne); CHECK(by_hand(ne, q, &t)); }
    CHECK(same(p, q, 12));
    CHECK(gn_host_level([&](const double*, double* ne, double*) { for (int i = 0; i < 32; i++) ne[i] = 0; return 0; }, kFloor, 5, 0.0, p, GnOut{},
                        [&](int at, double, double) { return -40 - at; }) == -40);   // refused at once, nowhere to write: the hook's code still
    // a round's own code at round 2 passes through: nothing reported, not even the rounds, and the hook is not asked
    Words e;
    calls = 0;
    CHECK(gn_host_level([&](const double*, double* ne, double* second) { shrinking(calls, ne); second[0] = 1; second[1] = 2; return calls++ == 2 ? -77 : 0; },
                        kFloor, 50, 0.0, p, all(e), never) == -77);
    CHECK(calls == 3 && e.it == -1 && untouched(e) && refusals == 0);
  }
  // ---- coarse_to_fine: coarsest first, a level without rounds skipped with a 0, per-level gates or the default, fine at level 0 only
  {
    struct Visit { int l, rounds; double gate; bool fine; };
    std::vector<Visit> seen;
    auto level = [&](int l, int rounds, double gate, bool fine, int* it) { seen.push_back({l, rounds, gate, fine}); *it = rounds - 1; return 0; };
    const int iters[3] = {2, 0, 3};
    const double gates[3] = {0.1, 0.2, 0.3};
    int out[3] = {-1, -1, -1};
    CHECK(coarse_to_fine(3, iters, gates, 0.5, out, level) == RPE_OK);
    CHECK(seen.size() == 2 && seen[0].l == 2 && seen[0].rounds == 3 && seen[1].l == 0 && seen[1].rounds == 2);
    CHECK(out[0] == 1 && out[1] == 0 && out[2] == 2);
    CHECK(seen[0].gate == 0.3 && seen[1].gate == 0.1 && !seen[0].fine && seen[1].fine);
    seen.clear();
    CHECK(coarse_to_fine(3, iters, nullptr, 0.5, nullptr, level) == RPE_OK);   // no gates: the default; no iters_out: none written
    CHECK(seen.size() == 2 && seen[0].gate == 0.5 && seen[1].gate == 0.5);
    const int all[3] = {2, 2, 2};
    seen.clear();
    CHECK(coarse_to_fine(3, all, nullptr, 0.5, nullptr, level) == RPE_OK);
    CHECK(seen.size() == 3 && !seen[0].fine && !seen[1].fine && seen[2].fine && seen[2].l == 0);
    // an error at level 1: its count is written BEFORE the return, level 0 is neither visited nor written
    int part[3] = {-1, -1, -1};
    seen.clear();
    auto failing = [&](int l, int rounds, double gate, bool fine, int* it) {
      seen.push_back({l, rounds, gate, fine});
      *it = l == 1 ? 1 : rounds;
      return l == 1 ? -5 : 0;
    };
    CHECK(coarse_to_fine(3, all, nullptr, 0.5, part, failing) == -5);
    CHECK(seen.size() == 2 && part[2] == 2 && part[1] == 1 && part[0] == -1);
  }
  // ---- pyramid_args: which of the three complaints, and at which level
  {
    const int ok[4] = {1, 0, 0, 2};
    int bad = -1;
    CHECK(pyramid_args(4, ok, nullptr, &bad) == kPyramidOk && pyramid_args(1, ok, nullptr, &bad) == kPyramidOk);
    CHECK(pyramid_args(0, ok, nullptr, &bad) == kPyramidLevels && pyramid_args(RPE_MAX_LEVELS + 1, ok, nullptr, &bad) == kPyramidLevels);
    CHECK(pyramid_args(-1, ok, nullptr, &bad) == kPyramidLevels && pyramid_args(2, nullptr, nullptr, &bad) == kPyramidLevels);
    const int finest0[2] = {0, 3};
    CHECK(pyramid_args(2, finest0, nullptr, &bad) == kPyramidRounds && bad == 0);
    const int coarser[3] = {3, 0, -1};
    CHECK(pyramid_args(3, coarser, nullptr, &bad) == kPyramidRounds && bad == 2);
    CHECK(pyramid_args(2, coarser, nullptr, &bad) == kPyramidOk);
    const double nan_gate[3] = {0.1, std::numeric_limits<double>::quiet_NaN(), 0.1}, neg_gate[3] = {-0.1, 0.1, 0.1}, zero_gate[3] = {0, 0, 0};
    CHECK(pyramid_args(3, ok, nan_gate, &bad) == kPyramidGate && bad == 1);
    CHECK(pyramid_args(3, ok, neg_gate, &bad) == kPyramidGate && bad == 0);
    CHECK(pyramid_args(3, ok, zero_gate, &bad) == kPyramidOk);
    CHECK(pyramid_args(3, finest0, neg_gate, &bad) == kPyramidRounds && bad == 0);   // a level's rounds before its gate, as the entry points had it
  }
  std::printf("gn_host: ok\n");
  return 0;
}
