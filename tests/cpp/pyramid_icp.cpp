// Coarse-to-fine ICP through the C++ front end (compiled and run by tests/test_gpu_pyramid.py): two depth frames of a box room
// rendered on the host, a 3-level pyramid of each, DepthFrontEnd::icpPyramid recovering the motion between them; a one-level
// pyramid reproduces DepthFrontEnd::icp bit for bit; the level maps have the level sizes.
#include <cmath>
#include <cstdio>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// inside of a box: walls x = -1.5 / 1.8, ceiling y = -1.2, floor y = 1.2, back wall z = 4; camera Xc = R Xw + t
static std::vector<float> render(const double R[9], const double t[3], const rpe::PinholeCamera& k) {
  const double nrm[5][3] = {{1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 1, 0}, {0, 0, 1}};
  const double off[5] = {-1.5, 1.8, -1.2, 1.2, 4.0};
  double O[3];
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  std::vector<float> d((size_t)k.width * k.height);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const double c[3] = {(u - k.cx) / k.fx, (v - k.cy) / k.fy, 1.0};
      double D[3];
      for (int i = 0; i < 3; i++) D[i] = R[i] * c[0] + R[3 + i] * c[1] + R[6 + i] * c[2];
      double best = 1e30;
      for (int p = 0; p < 5; p++) {
        const double nd = nrm[p][0] * D[0] + nrm[p][1] * D[1] + nrm[p][2] * D[2];
        if (std::fabs(nd) < 1e-12) continue;
        const double s = (off[p] - (nrm[p][0] * O[0] + nrm[p][1] * O[1] + nrm[p][2] * O[2])) / nd;
        if (s > 0 && s < best) best = s;
      }
      d[(size_t)v * k.width + u] = (float)best;
    }
  return d;
}

int main() {
  rpe::PinholeCamera cam;   // 640 x 480, f = 585
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0, 0, 0};
  const double a = 0.03, ca = std::cos(a), sa = std::sin(a);
  const double RB[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca}, tB[3] = {0.04, -0.03, 0.05};
  const std::vector<float> dA = render(I, t0, cam), dB = render(RB, tB, cam);
  double pA[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, pB[12];
  for (int i = 0; i < 9; i++) pB[i] = RB[i];
  for (int i = 0; i < 3; i++) pB[9 + i] = tB[i];
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};

  rpe::DepthFrontEnd fe;
  fe.setDepthPyramid(dA.data(), cam, 3, range);
  fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(pA));
  fe.setDepthPyramid(dB.data(), cam, 3, range);
  CHECK(fe.map(RPE_MAP_DEPTH, 2).cols() == 160 * 120 && fe.map(RPE_MAP_VERTEX, 1).cols() == 320 * 240);
  CHECK(fe.map(RPE_MAP_MODEL_NORMAL, 2).rows() == 3 && fe.map(RPE_MAP_MODEL_NORMAL, 2).cols() == 160 * 120);

  rpe::IcpOptions o;
  o.tol = 1e-7; o.cos_thr = 0.8;
  for (int fused = 0; fused < 2; fused++) {
    o.fused = fused == 1;
    rpe::DepthFrontEnd::Pose T = rpe::DepthFrontEnd::pose_of(pA);
    const rpe::PyramidIcpResult r = fe.icpPyramid(T, {6, 4, 10}, {0.1, 0.2, 0.3}, o);
    double p[12];
    rpe::DepthFrontEnd::pose12(T, p);
    double err = 0;
    for (int i = 0; i < 12; i++) err = std::fmax(err, std::fabs(p[i] - pB[i]));
    std::printf("fused=%d levels 0/1/2: %d/%d/%d rounds, %lld pairs, max |pose - truth| %.3g\n", fused, r.level_iterations[0],
                r.level_iterations[1], r.level_iterations[2], r.pairs, err);
    CHECK(err < 1e-4);
    CHECK(r.level_iterations[2] >= 1 && r.level_iterations[0] >= 1 && r.pairs > 200000);
    CHECK(r.iterations == r.level_iterations[0] + r.level_iterations[1] + r.level_iterations[2]);
  }

  // one level: the pyramid call is rpe_icp
  o.fused = false; o.max_iter = 5; o.tol = 0.0;
  rpe::DepthFrontEnd::Pose T1 = rpe::DepthFrontEnd::pose_of(pA), T2 = T1;
  const rpe::IcpResult r1 = fe.icp(T1, o);
  const rpe::PyramidIcpResult r2 = fe.icpPyramid(T2, {5}, {}, o);
  double p1[12], p2[12];
  rpe::DepthFrontEnd::pose12(T1, p1);
  rpe::DepthFrontEnd::pose12(T2, p2);
  bool same = r1.iterations == r2.iterations && r1.cost == r2.cost && r1.pairs == r2.pairs;
  for (int i = 0; i < 12; i++) same = same && p1[i] == p2[i];
  CHECK(same);

  bool threw = false;
  try { rpe::DepthFrontEnd::Pose T = T1; fe.icpPyramid(T, {3, 3, 3, 3}); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);   // the frame has 3 levels
  if (fails) { std::printf("pyramid_icp: %d failures\n", fails); return 1; }
  std::printf("pyramid_icp: ok\n");
  return 0;
}
