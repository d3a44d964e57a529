// rpe_graph_solve (csrc/library.cpp: host code, no GPU) under AddressSanitizer / UndefinedBehaviorSanitizer: compiled TOGETHER with
// library.cpp by tests/test_graph_oracle.py and run there.  A chain of K keyframes with a loop edge, records made of random full-rank
// rows J_j, J_i and residuals (so that H = sum J^T J, g = sum J^T r exactly as a round leaves them): the solution must satisfy the
// assembled system; fixed keyframes, a keyframe on no edge, two components, K = 256 (the largest system) and a rank-deficient
// record are covered.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/rgbd_pose_hip.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0 - 0.5; }

// one edge's record from `rows` random residual rows; rank_one: every row the same direction (not positive definite)
static void make_record(int rows, bool rank_one, double* rec) {
  for (int k = 0; k < RPE_GRAPH_RECORD; k++) rec[k] = 0.0;
  double Hjj[36] = {0}, Hii[36] = {0}, Hji[36] = {0}, base[12];
  for (int k = 0; k < 12; k++) base[k] = rnd();
  for (int n = 0; n < rows; n++) {
    double J[12], r = rnd();
    for (int k = 0; k < 12; k++) J[k] = rank_one ? base[k] * (1.0 + n) : rnd();
    rec[0] += 1; rec[1] += r * r;
    for (int a = 0; a < 6; a++) {
      rec[2 + a] += J[a] * r; rec[8 + a] += J[6 + a] * r;
      for (int b = 0; b < 6; b++) { Hjj[6 * a + b] += J[a] * J[b]; Hii[6 * a + b] += J[6 + a] * J[6 + b]; Hji[6 * a + b] += J[a] * J[6 + b]; }
    }
  }
  int k = 14;
  for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) rec[k++] = Hjj[6 * a + b];
  for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) rec[k++] = Hii[6 * a + b];
  for (int m = 0; m < 36; m++) rec[k++] = Hji[m];
}

// | H delta + g | over the rows of the keyframes in `free`, assembled here from the records
static double residual(int K, const std::vector<int32_t>& ji, const std::vector<double>& rec, const std::vector<double>& d, const std::vector<uint8_t>& fixed) {
  std::vector<double> out((size_t)6 * K, 0.0);
  std::vector<char> on(K, 0);
  for (size_t e = 0; e < ji.size() / 2; e++) {
    const int j = ji[2 * e], i = ji[2 * e + 1];
    const double* R = &rec[e * RPE_GRAPH_RECORD];
    on[j] = on[i] = 1;
    double Hjj[36], Hii[36];
    int k = 14;
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { Hjj[6 * a + b] = Hjj[6 * b + a] = R[k++]; }
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { Hii[6 * a + b] = Hii[6 * b + a] = R[k++]; }
    for (int a = 0; a < 6; a++) {
      out[6 * j + a] += R[2 + a]; out[6 * i + a] += R[8 + a];
      for (int b = 0; b < 6; b++) {
        out[6 * j + a] += Hjj[6 * a + b] * d[6 * j + b] + R[56 + 6 * a + b] * d[6 * i + b];
        out[6 * i + a] += Hii[6 * a + b] * d[6 * i + b] + R[56 + 6 * b + a] * d[6 * j + b];
      }
    }
  }
  double worst = 0;
  for (int k = 0; k < K; k++) if (on[k] && !fixed[k]) for (int a = 0; a < 6; a++) worst = std::fmax(worst, std::fabs(out[6 * k + a]));
  return worst;
}

static void chain(int K, int skip) {
  std::vector<int32_t> ji;
  for (int j = 1; j < K; j++) { if (j == skip) continue; ji.push_back(j); ji.push_back(j - 1 == skip ? j - 2 : j - 1); }
  if (K > 3) { ji.push_back(K - 1); ji.push_back(0); }                                 // the loop
  const int E = (int)ji.size() / 2;
  std::vector<double> rec((size_t)E * RPE_GRAPH_RECORD), d((size_t)6 * K, 7.0);
  for (int e = 0; e < E; e++) make_record(40, false, &rec[(size_t)e * RPE_GRAPH_RECORD]);
  std::vector<uint8_t> fixed(K, 0);
  fixed[K / 2] = 1;
  CHECK(rpe_graph_solve(K, E, ji.data(), rec.data(), fixed.data(), d.data()) == RPE_OK);
  bool moved = false;
  for (int k = 0; k < K; k++) for (int a = 0; a < 6; a++) {
    if (k == K / 2 || k == skip) CHECK(d[6 * k + a] == 0.0); else moved = moved || d[6 * k + a] != 0.0;
  }
  const double res = residual(K, ji, rec, d, fixed);
  std::printf("K %d, %d edges: |H delta + g| = %.2e\n", K, E, res);
  CHECK(moved && res < 1e-8);
}

int main() {
  chain(2, -1);
  chain(8, -1);
  chain(9, 4);          // keyframe 4 is on no edge: it has no equation and keeps delta = 0
  chain(256, -1);       // the largest system: 1530 unknowns
  {                     // two components, each with its own fixed keyframe; then one of them free: not positive definite
    const std::vector<int32_t> ji = {1, 0, 3, 2};
    std::vector<double> rec(2 * RPE_GRAPH_RECORD), d(24);
    make_record(30, false, &rec[0]); make_record(30, false, &rec[RPE_GRAPH_RECORD]);
    std::vector<uint8_t> fixed = {1, 0, 1, 0};
    CHECK(rpe_graph_solve(4, 2, ji.data(), rec.data(), fixed.data(), d.data()) == RPE_OK && residual(4, ji, rec, d, fixed) < 1e-9);
    make_record(30, true, &rec[RPE_GRAPH_RECORD]);
    CHECK(rpe_graph_solve(4, 2, ji.data(), rec.data(), fixed.data(), d.data()) == RPE_ERR_DEGENERATE);
    CHECK(rpe_graph_solve(4, 2, ji.data(), rec.data(), nullptr, d.data()) == RPE_ERR_DEGENERATE);
  }
  {
    const int32_t bad[2] = {2, 0};
    double rec[RPE_GRAPH_RECORD] = {0}, d[12];
    CHECK(rpe_graph_solve(2, 1, bad, rec, nullptr, d) == RPE_ERR_ARG);
    CHECK(rpe_graph_solve(0, 0, nullptr, nullptr, nullptr, d) == RPE_ERR_ARG && rpe_graph_solve(2, 1, nullptr, rec, nullptr, d) == RPE_ERR_ARG);
    CHECK(rpe_graph_solve(2, 0, nullptr, nullptr, nullptr, d) == RPE_OK && d[0] == 0.0 && d[11] == 0.0);
  }
  std::printf(fails ? "graph_solve_host: %d failure(s)\n" : "graph_solve_host: ok\n", fails);
  return fails ? 1 : 0;
}
