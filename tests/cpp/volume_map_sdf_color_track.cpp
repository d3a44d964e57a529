// Tracking with colour against the whole map through the C++ front end (compiled by tests/test_mapsdf_photo_oracle.py, run by
// tests/test_gpu_mapsdf_photo.py): a textured WALL fused with its colour into a window that then moves on with the archive on, so that
// half of the wall in view lies in archived bricks.  The frame is tracked from an in-plane offset against the map's geometry alone
// (icpPyramidMap: a plane holds no in-plane motion) and against its geometry and colour (icpPyramidMapColor, which holds it);
// mapColorResiduals is the residual image, and with the window's extent for a box all of it is the window term's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// the wall z = 3 seen from the identity pose, with a smooth texture of a few waves per metre
static void render(const rpe::PinholeCamera& k, std::vector<float>& d, std::vector<uint8_t>& rgb) {
  d.resize((size_t)k.width * k.height);
  rgb.resize(d.size() * 3);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const size_t i = (size_t)v * k.width + u;
      const double z = 3.0, x = (u - k.cx) / k.fx * z, y = (v - k.cy) / k.fy * z;
      d[i] = (float)z;
      rgb[3 * i] = (uint8_t)std::lround(128 + 90 * std::sin(3.1 * x) * std::cos(2.3 * y));
      rgb[3 * i + 1] = (uint8_t)std::lround(128 + 90 * std::sin(2.2 * x + 1.7 * y));
      rgb[3 * i + 2] = (uint8_t)std::lround(128 + 90 * std::cos(1.3 * x - 2.9 * y));
    }
}

static size_t count(const std::vector<float>& r) {
  size_t n = 0;
  for (float x : r) n += std::isnan(x) ? 0 : 1;
  return n;
}

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const size_t n = (size_t)k.width * k.height;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc desc;   // a slab of 4 cm voxels around the wall, wider than the view
  desc.dim[0] = 96; desc.dim[1] = 64; desc.dim[2] = 24;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -1.92; desc.origin[1] = -1.28; desc.origin[2] = 2.52;
  std::vector<float> depth;
  std::vector<uint8_t> rgb;
  render(k, depth, rgb);
  try {
    rpe::DepthFrontEnd fe;
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const double off[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.03, -0.02, 0.01};   // 36 mm in the wall's plane, 10 mm off it
    const auto T = rpe::DepthFrontEnd::pose_of(I);
    rpe::IcpOptions o;
    o.cos_thr = 0.8;
    fe.setDepthPyramid(depth.data(), k, 3, range);
    fe.setColor(rgb.data());
    fe.initVolume(desc);
    bool threw = false;                                            // no colour volume yet
    try { rpe::DepthFrontEnd::Pose p = T; fe.icpMapColor(p, 0.01, o); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    fe.integrateColor(T);
    const std::vector<float> whole = fe.volumeColorResiduals(T, 0, 0.1);
    CHECK(count(fe.mapColorResiduals(T, 0, 0.1)) == count(whole));   // the archive is off: the map is the window

    fe.archiveVolume(256);
    const int32_t out[3] = {48, 0, 0};
    fe.shiftVolume(out);
    const std::vector<float> rw = fe.volumeColorResiduals(T, 0, 0.1), rm = fe.mapColorResiduals(T, 0, 0.1);
    std::printf("photometric rows at the true pose: %zu before the shift, %zu in the window after it, %zu in the map\n", count(whole), count(rw),
                count(rm));
    CHECK(count(whole) > 0.8 * n && count(rw) < 0.8 * count(whole) && count(rm) > count(rw));
    CHECK(rm.size() == n && std::memcmp(rm.data(), whole.data(), n * sizeof(float)) == 0);   // the box has the first window's origin
    const int64_t wlo[3] = {48, 0, 0}, whi[3] = {144, 64, 24};
    const std::vector<float> re = fe.mapColorResiduals(T, 0, 0.1, wlo, whi);
    CHECK(std::memcmp(re.data(), rw.data(), n * sizeof(float)) == 0);                         // the window's extent: the window term

    rpe::DepthFrontEnd::Pose pg = rpe::DepthFrontEnd::pose_of(off), pc = pg, p1 = pg;
    // geometry alone: a perfect plane leaves the in-plane offset where it was, or the round has no solution at all
    double g12[12], c12[12], eg = 0, ec = 0;
    bool lost = false;
    try {
      const rpe::PyramidIcpResult a = fe.icpPyramidMap(pg, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
      rpe::DepthFrontEnd::pose12(pg, g12);
      for (int i = 0; i < 12; i++) eg = std::fmax(eg, std::fabs(g12[i] - I[i]));
      std::printf("map term: %lld rows, max |pose - truth| %.3g\n", a.pairs, eg);
    } catch (const rpe::DeviceError& e) { lost = e.code == RPE_ERR_DEGENERATE; }
    CHECK(lost || eg > 0.015);
    const rpe::RgbdIcpResult b = fe.icpPyramidMapColor(pc, 0.01, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
    rpe::DepthFrontEnd::pose12(pc, c12);
    for (int i = 0; i < 12; i++) ec = std::fmax(ec, std::fabs(c12[i] - I[i]));
    std::printf("map term with colour: %lld + %lld rows, max |pose - truth| %.3g\n", b.pairs, b.photo_pairs, ec);
    // an exercise of the C++ path (the bounds of the Python tests come from the oracle, tests/mapsdf_photo_cases.py): the colour brings
    // the offset to well under a voxel, with rows the window alone does not have
    CHECK(ec < 5e-3 && b.pairs > 0.8 * n && b.photo_pairs > 0.8 * n && b.photo_pairs > (long long)count(rw));
    CHECK(b.iterations >= 3 && b.iterations <= 13 && b.photo_cost > 0);

    rpe::IcpOptions single = o;
    single.max_iter = 1;
    const rpe::RgbdIcpResult r = fe.icpMapColor(p1, 0.01, single);
    CHECK(r.iterations == 1 && r.pairs > 0.8 * n && r.photo_pairs > 0.8 * n && r.last_step > 1e-3);
    threw = false;
    try { fe.icpMapColor(p1, 0.0, single); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
    threw = false;
    single.device_resident = true;
    try { fe.icpMapColor(p1, 0.01, single); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
    const int64_t odd[3] = {4, 0, 0};
    threw = false;
    try { fe.mapColorResiduals(T, 0, 0.1, odd, whi); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_map_sdf_color_track: %d failure(s)\n" : "volume_map_sdf_color_track: ok\n", fails);
  return fails ? 1 : 0;
}
