// The robust volume terms through the C++ front end (compiled by tests/test_sdf_robust_oracle.py, run by tests/test_gpu_sdf_robust.py):
// a box room rendered on the host and fused from one pose; a second frame in which a block of the depth -- an intruder -- stands 8 cm
// in front of the room, tracked with DepthFrontEnd::icpPyramidVolume without a weight and with setVolumeRobust(RPE_ROBUST_TUKEY);
// volumeRobust reads the setting back and volumeRobustWeights shows the weights.
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

static double pose_error(const rpe::DepthFrontEnd::Pose& T, const double truth[12]) {
  double p[12], err = 0;
  rpe::DepthFrontEnd::pose12(T, p);
  for (int i = 0; i < 12; i++) err = std::fmax(err, std::fabs(p[i] - truth[i]));
  return err;
}

static int run() {
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;   // volume_sdf_track.cpp's
  const size_t n = (size_t)cam.width * cam.height;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc vd;   // the box with a margin, 4 cm voxels
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  const double eye[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  const double a = 0.012, ca = std::cos(a), sa = std::sin(a);
  const double truth[12] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca, 0.015, -0.01, 0.02};
  rpe::DepthFrontEnd fe;
  rpe::IcpOptions o;
  o.cos_thr = 0.8;

  // the setting: off at first, refused values leave it as it was, a good one reads back
  CHECK(fe.volumeRobust().kind == RPE_ROBUST_NONE);
  int refused = 0;
  try { fe.setVolumeRobust(RPE_ROBUST_CAUCHY, 0.05); } catch (const rpe::DeviceError&) { refused++; }
  try { fe.setVolumeRobust(RPE_ROBUST_TUKEY, 1e-9); } catch (const rpe::DeviceError&) { refused++; }
  try { fe.setVolumeRobust(RPE_ROBUST_HUBER, 0.05, -1.0); } catch (const rpe::DeviceError&) { refused++; }
  CHECK(refused == 3 && fe.volumeRobust().kind == RPE_ROBUST_NONE);

  fe.setDepthPyramid(render(eye, eye + 9, cam).data(), cam, 3, range);
  fe.initVolume(vd);
  fe.integrate(rpe::DepthFrontEnd::pose_of(eye));

  // the second frame with the intruder: rows 60 .. 199, columns 40 .. 159 (22 % of the frame) closer by 8 cm
  std::vector<float> d = render(truth, truth + 9, cam);
  for (int v = 60; v < 200; v++)
    for (int u = 40; u < 160; u++) d[(size_t)v * cam.width + u] -= 0.08f;
  fe.setDepthPyramid(d.data(), cam, 3, range);

  rpe::DepthFrontEnd::Pose plain = rpe::DepthFrontEnd::pose_of(eye);
  fe.icpPyramidVolume(plain, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
  const double e_plain = pose_error(plain, truth);

  fe.setVolumeRobust(RPE_ROBUST_TUKEY, 0.05);
  const rpe::DepthFrontEnd::VolumeRobust set = fe.volumeRobust();
  CHECK(set.kind == RPE_ROBUST_TUKEY && set.k == 0.05 && set.photo_k == 0.0);
  rpe::DepthFrontEnd::Pose robust = rpe::DepthFrontEnd::pose_of(eye);
  const rpe::PyramidIcpResult r = fe.icpPyramidVolume(robust, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
  const double e_robust = pose_error(robust, truth);
  std::printf("max |pose - truth|: unweighted %.3g, Tukey 50 mm %.3g (%lld rows)\n", e_plain, e_robust, r.pairs);
  // a direction only: the room's bounds come from the oracle in the Python tests (tests/sdf_robust_cases.py)
  CHECK(e_robust < e_plain && r.pairs > 20000);

  // the weights at the tracked pose: in [0, 1] where there is a row; the intruder's rows, 8 cm off, have weight 0 under k = 5 cm
  const std::vector<float> w = fe.volumeRobustWeights(robust, 0, o);
  const std::vector<float> res = fe.volumeResiduals(robust, 0, o);
  size_t rows = 0, zero = 0, bad = 0;
  for (size_t i = 0; i < n; i++) {
    if (std::isnan(w[i]) != std::isnan(res[i])) bad++;
    if (std::isnan(w[i])) continue;
    rows++;
    if (!(w[i] >= 0.0f && w[i] <= 1.0f) || (w[i] == 0.0f) != (std::fabs(res[i]) >= 0.05f)) bad++;
    zero += w[i] == 0.0f ? 1 : 0;
  }
  std::printf("%zu rows, %zu of weight 0\n", rows, zero);
  CHECK(w.size() == n && bad == 0 && rows > 20000 && zero > 2000);

  // off again: every row has weight 1
  fe.setVolumeRobust(RPE_ROBUST_NONE);
  CHECK(fe.volumeRobust().kind == RPE_ROBUST_NONE && fe.volumeRobust().k == 0.0);
  const std::vector<float> one = fe.volumeRobustWeights(robust, 0, o);
  size_t other = 0;
  for (size_t i = 0; i < n; i++) other += std::isnan(one[i]) ? (std::isnan(res[i]) ? 0 : 1) : (one[i] == 1.0f ? 0 : 1);
  CHECK(other == 0);
  if (fails) { std::printf("volume_sdf_robust_track: %d failures\n", fails); return 1; }
  std::printf("volume_sdf_robust_track: ok\n");
  return 0;
}

int main() {
  try { return run(); }
  catch (const rpe::DeviceError& e) { std::printf("volume_sdf_robust_track: %s\n", e.what()); return 1; }   // (no abort on a refused call)
}
