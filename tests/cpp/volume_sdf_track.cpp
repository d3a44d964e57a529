// Tracking against the TSDF volume itself through the C++ front end (compiled by tests/test_sdf_oracle.py, run and replayed by
// tests/test_gpu_sdf.py): depth frames of a box room rendered on the host along a short path; DepthFrontEnd::initVolume / integrate /
// icpPyramidVolume track it with no raycast and no model; volumeResiduals is the residual image.  With a directory as argument the
// first two frames and the first tracked pose are left there for the replay.
#include <cmath>
#include <cstdio>
#include <string>
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

static void dump(const std::string& dir, const char* name, const void* data, size_t bytes) {
  if (dir.empty()) return;
  std::FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f || std::fwrite(data, 1, bytes, f) != bytes) { std::printf("FAIL cannot write %s\n", name); fails++; }
  if (f) std::fclose(f);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "";
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const size_t n = (size_t)cam.width * cam.height;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc vd;   // the box [-1.5, 1.8] x [-1.2, 1.2] x [.., 4] with a margin, 4 cm voxels
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  rpe::DepthFrontEnd fe;
  const int frames = 6;
  double truth[frames][12];
  for (int f = 0; f < frames; f++) {
    const double a = 0.012 * f, ca = std::cos(a), sa = std::sin(a);
    const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    for (int i = 0; i < 9; i++) truth[f][i] = R[i];
    truth[f][9] = 0.015 * f; truth[f][10] = -0.01 * f; truth[f][11] = 0.02 * f;
  }
  rpe::DepthFrontEnd::Pose T = rpe::DepthFrontEnd::pose_of(truth[0]);
  rpe::IcpOptions o;
  o.cos_thr = 0.8;
  // no volume yet: the term has nothing to read
  {
    const std::vector<float> d = render(truth[0], truth[0] + 9, cam);
    fe.setDepthPyramid(d.data(), cam, 3, range);
    bool threw = false;
    try { fe.icpVolume(T, o); } catch (const rpe::DeviceError&) { threw = true; }
    CHECK(threw);
    fe.initVolume(vd);
    fe.integrate(T);
    dump(dir, "depth0.bin", d.data(), n * sizeof(float));
    // the frame in its own volume: nearly every pixel has a row, and the residual is the interpolation error
    const std::vector<float> r = fe.volumeResiduals(T, 0, o);
    size_t rows = 0, small = 0;
    for (size_t i = 0; i < n; i++) if (!std::isnan(r[i])) { rows++; small += std::fabs(r[i]) < 0.02f ? 1 : 0; }
    std::printf("frame 0 in its own volume: %zu rows of %zu pixels, %zu within 2 cm\n", rows, n, small);
    CHECK(r.size() == n && rows > 0.8 * n && small > 0.95 * rows);
  }
  for (int f = 1; f < frames; f++) {
    const std::vector<float> d = render(truth[f], truth[f] + 9, cam);
    fe.setDepthPyramid(d.data(), cam, 3, range);
    const rpe::PyramidIcpResult r = fe.icpPyramidVolume(T, {6, 4, 3}, {0.1, 0.15, 0.2}, o);   // no raycast, no model
    double p[12];
    rpe::DepthFrontEnd::pose12(T, p);
    if (f == 1) { dump(dir, "depth1.bin", d.data(), n * sizeof(float)); dump(dir, "result.bin", p, sizeof(p)); }
    fe.integrate(T);
    double err = 0;
    for (int i = 0; i < 12; i++) err = std::fmax(err, std::fabs(p[i] - truth[f][i]));
    std::printf("frame %d: %d rounds (%d %d %d), %lld rows, max |pose - truth| %.3g\n", f, r.iterations, r.level_iterations[0],
                r.level_iterations[1], r.level_iterations[2], r.pairs, err);
    // an exercise of the C++ path: the five planes of the box constrain the pose more weakly than the room of the Python tests, whose
    // bounds come from the oracle (tests/sdf_cases.py)
    CHECK(err < 3e-2 && r.pairs > 30000 && r.iterations >= 3 && r.iterations <= 13);
  }
  {
    rpe::DepthFrontEnd::Pose one = T;
    rpe::IcpOptions single = o;
    single.max_iter = 1;
    const rpe::IcpResult r = fe.icpVolume(one, single);
    CHECK(r.iterations == 1 && r.pairs > 30000 && r.cost > 0 && r.last_step < 1e-2);
    bool threw = false;
    single.device_resident = true;
    try { fe.icpVolume(one, single); } catch (const rpe::DeviceError&) { threw = true; }
    CHECK(threw);
  }
  if (fails) { std::printf("volume_sdf_track: %d failures\n", fails); return 1; }
  std::printf("volume_sdf_track: ok\n");
  return 0;
}
