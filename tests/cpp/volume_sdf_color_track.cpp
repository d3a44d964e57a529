// Tracking against the TSDF and the colour volume themselves through the C++ front end (compiled by tests/test_sdf_photo_oracle.py, run
// by tests/test_gpu_sdf_photo.py): a textured WALL rendered on the host along a path that slides in the wall's plane.  The volume term
// alone has nothing to hold that motion with; DepthFrontEnd::icpPyramidVolumeColor holds it, with no raycast, no model and no
// preparePhoto; volumeColorResiduals is the residual image.
#include <cmath>
#include <cstdio>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// the wall z = 3 seen from Xc = Xw + t (no rotation: the path slides), with a smooth texture of a few waves per metre
static void render(const double t[3], const rpe::PinholeCamera& k, std::vector<float>& d, std::vector<uint8_t>& rgb) {
  d.resize((size_t)k.width * k.height);
  rgb.resize(d.size() * 3);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const size_t i = (size_t)v * k.width + u;
      const double z = 3.0 + t[2], x = (u - k.cx) / k.fx * z - t[0], y = (v - k.cy) / k.fy * z - t[1];
      d[i] = (float)z;
      rgb[3 * i] = (uint8_t)std::lround(128 + 90 * std::sin(3.1 * x) * std::cos(2.3 * y));
      rgb[3 * i + 1] = (uint8_t)std::lround(128 + 90 * std::sin(2.2 * x + 1.7 * y));
      rgb[3 * i + 2] = (uint8_t)std::lround(128 + 90 * std::cos(1.3 * x - 2.9 * y));
    }
}

int main() {
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const size_t n = (size_t)cam.width * cam.height;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc vd;   // a slab of 4 cm voxels around the part of the wall the path sees
  vd.dim[0] = 128; vd.dim[1] = 96; vd.dim[2] = 20; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -2.5; vd.origin[1] = -1.9; vd.origin[2] = 2.6;
  rpe::DepthFrontEnd fe;
  const int frames = 4;
  double truth[frames][12];
  for (int f = 0; f < frames; f++) {
    for (int i = 0; i < 9; i++) truth[f][i] = i % 4 == 0 ? 1.0 : 0.0;
    truth[f][9] = 0.03 * f; truth[f][10] = -0.02 * f; truth[f][11] = 0.0;
  }
  rpe::DepthFrontEnd::Pose T = rpe::DepthFrontEnd::pose_of(truth[0]);
  rpe::IcpOptions o;
  o.cos_thr = 0.8;
  std::vector<float> d;
  std::vector<uint8_t> rgb;
  render(truth[0] + 9, cam, d, rgb);
  fe.setDepthPyramid(d.data(), cam, 3, range);
  fe.initVolume(vd);
  {
    // no frame colour, then no colour volume: the term has nothing to read
    bool threw = false;
    try { fe.icpVolumeColor(T, 0.01, o); } catch (const rpe::DeviceError&) { threw = true; }
    CHECK(threw);
    fe.setColor(rgb.data());
    threw = false;
    try { fe.icpVolumeColor(T, 0.01, o); } catch (const rpe::DeviceError&) { threw = true; }
    CHECK(threw);
  }
  fe.integrateColor(T);
  {
    // the frame in its own volume: most pixels have a row, and the residual is the voxel blend's error
    const std::vector<float> r = fe.volumeColorResiduals(T, 0, 0.1);
    size_t rows = 0, small = 0;
    for (size_t i = 0; i < n; i++) if (!std::isnan(r[i])) { rows++; small += std::fabs(r[i]) < 8.f ? 1 : 0; }
    std::printf("frame 0 in its own volume: %zu rows of %zu pixels, %zu within 8 levels\n", rows, n, small);
    CHECK(r.size() == n && rows > 0.8 * n && small > 0.9 * rows);
  }
  for (int f = 1; f < frames; f++) {
    render(truth[f] + 9, cam, d, rgb);
    fe.setDepthPyramid(d.data(), cam, 3, range);
    fe.setColor(rgb.data());
    const rpe::RgbdIcpResult r = fe.icpPyramidVolumeColor(T, 0.01, {6, 4, 3}, {0.1, 0.15, 0.2}, o);   // no raycast, no model, no preparePhoto
    double p[12];
    rpe::DepthFrontEnd::pose12(T, p);
    fe.integrateColor(T);
    double err = 0;
    for (int i = 0; i < 12; i++) err = std::fmax(err, std::fabs(p[i] - truth[f][i]));
    std::printf("frame %d: %d rounds (%d %d %d), %lld + %lld rows, max |pose - truth| %.3g\n", f, r.iterations, r.level_iterations[0],
                r.level_iterations[1], r.level_iterations[2], r.pairs, r.photo_pairs, err);
    // an exercise of the C++ path (the bounds of the Python tests come from the oracle, tests/sdf_photo_cases.py): the slide of 36 mm a
    // frame is followed to well under a voxel
    CHECK(err < 1e-2 && r.pairs > 30000 && r.photo_pairs > 30000 && r.iterations >= 3 && r.iterations <= 13);
  }
  {
    rpe::DepthFrontEnd::Pose one = T;
    rpe::IcpOptions single = o;
    single.max_iter = 1;
    const rpe::RgbdIcpResult r = fe.icpVolumeColor(one, 0.01, single);
    CHECK(r.iterations == 1 && r.pairs > 30000 && r.photo_pairs > 30000 && r.photo_cost > 0);
    bool threw = false;
    try { fe.icpVolumeColor(one, 0.0, single); } catch (const rpe::DeviceError&) { threw = true; }
    CHECK(threw);
  }
  if (fails) { std::printf("volume_sdf_color_track: %d failures\n", fails); return 1; }
  std::printf("volume_sdf_color_track: ok\n");
  return 0;
}
