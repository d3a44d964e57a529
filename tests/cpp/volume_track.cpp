// Frame-to-model tracking through the C++ front end (compiled and run by tests/test_gpu_volume.py): depth frames of a box room
// rendered on the host along a short path, DepthFrontEnd::initVolume / integrate / raycast / icpPyramid tracking it; the raycast of
// the first frame's volume from its own pose reproduces that frame's depth; the volume comes back with the voxels the frames saw.
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
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1}, ray{1.0, 0.1, 6.0, 0.1};
  rpe::VolumeDesc vd;   // the box [-1.5, 1.8] x [-1.2, 1.2] x [.., 4] with a margin, 4 cm voxels
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  rpe::DepthFrontEnd fe;
  fe.initVolume(vd);
  const int frames = 6;
  double truth[frames][12];
  for (int f = 0; f < frames; f++) {
    const double a = 0.012 * f, ca = std::cos(a), sa = std::sin(a);
    const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    for (int i = 0; i < 9; i++) truth[f][i] = R[i];
    truth[f][9] = 0.015 * f; truth[f][10] = -0.01 * f; truth[f][11] = 0.02 * f;
  }
  rpe::DepthFrontEnd::Pose T = rpe::DepthFrontEnd::pose_of(truth[0]);
  {
    const std::vector<float> d = render(truth[0], truth[0] + 9, cam);
    fe.setDepthPyramid(d.data(), cam, 3, range);
    fe.integrate(T);
    fe.raycast(T, cam, ray);   // the first frame's own view: its depth again, to within the voxel interpolation
    const rpe::MatrixX<float> mv = fe.map(RPE_MAP_MODEL_VERTEX);
    int hits = 0, close = 0;
    for (int i = 0; i < cam.width * cam.height; i++) {
      if (std::isnan(mv(2, i))) continue;
      hits++;
      close += std::fabs(mv(2, i) - d[i]) < 0.01 ? 1 : 0;   // pose 0 is the identity: world z = camera z
    }
    std::printf("raycast of frame 0: %d hits, %d within 1 cm\n", hits, close);
    CHECK(hits > 0.9 * cam.width * cam.height && close > 0.95 * hits);
  }
  rpe::IcpOptions o;
  o.cos_thr = 0.8;
  double err = 0;
  for (int f = 1; f < frames; f++) {
    const std::vector<float> d = render(truth[f], truth[f] + 9, cam);
    fe.setDepthPyramid(d.data(), cam, 3, range);
    fe.raycast(T, cam, ray, 3);
    const rpe::PyramidIcpResult r = fe.icpPyramid(T, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
    fe.integrate(T);
    double p[12];
    rpe::DepthFrontEnd::pose12(T, p);
    err = 0;
    for (int i = 0; i < 12; i++) err = std::fmax(err, std::fabs(p[i] - truth[f][i]));
    std::printf("frame %d: %d rounds, %lld pairs, max |pose - truth| %.3g\n", f, r.iterations, r.pairs, err);
    // an exercise of the C++ path: the five planes of the box constrain the pose more weakly than the room of the Python tests, whose
    // bounds come from the oracle (tests/volume_cases.py)
    CHECK(err < 3e-2 && r.pairs > 30000);
  }
  const rpe::MatrixX<float> vol = fe.volume();
  long long seen = 0;
  for (long long i = 0; i < (long long)vol.cols(); i++) {
    seen += vol(1, i) > 0 ? 1 : 0;
    if (vol(1, i) > (float)frames || vol(0, i) > 1.0f || vol(0, i) < -1.0f) { CHECK(false); break; }
  }
  std::printf("volume: %lld of %lld voxels observed\n", seen, (long long)vol.cols());
  CHECK(vol.rows() == 2 && vol.cols() == 90 * 72 * 120 && seen > 10000);
  bool threw = false;
  try { rpe::VolumeDesc bad = vd; bad.dim[1] = 1; fe.initVolume(bad); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  if (fails) { std::printf("volume_track: %d failures\n", fails); return 1; }
  std::printf("volume_track: ok\n");
  return 0;
}
