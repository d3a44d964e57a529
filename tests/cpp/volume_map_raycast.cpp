// The map raycast through the C++ front end (compiled by tests/test_mapray_oracle.py, run by tests/test_gpu_mapray.py): a wall fused
// into a 64 x 48 x 24 window that then moves two bricks along +x with the archive on.  raycastMap is held once to the C call it wraps;
// over the bounds the model shows the slab that left -- bit for bit the model the window gave before it moved, the box having that
// window's origin --, over the window's extent it is the window's own raycast, and the flags, the pyramid and the errors behave.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

struct Model { rpe::MatrixX<float> v, n; };
static Model model(const rpe::DepthFrontEnd& fe) { return Model{fe.map(RPE_MAP_MODEL_VERTEX, 0), fe.map(RPE_MAP_MODEL_NORMAL, 0)}; }
static bool same(const Model& a, const Model& b) {
  return a.v.cols() == b.v.cols() && std::memcmp(a.v.data(), b.v.data(), sizeof(float) * 3 * (size_t)a.v.cols()) == 0 &&
         std::memcmp(a.n.data(), b.n.data(), sizeof(float) * 3 * (size_t)a.n.cols()) == 0;
}
static long hits(const Model& m) {
  long n = 0;
  for (long i = 0; i < (long)m.v.cols(); i++) n += m.v.data()[3 * i] == m.v.data()[3 * i] ? 1 : 0;
  return n;
}

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc desc;
  desc.dim[0] = 64; desc.dim[1] = 48; desc.dim[2] = 24;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -1.28; desc.origin[1] = -0.96; desc.origin[2] = 2.52;
  std::vector<float> depth((size_t)k.width * k.height);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) depth[(size_t)v * k.width + u] = (float)(3.0 + 0.1 * std::cos(u / 25.0));
  try {
    rpe::DepthFrontEnd fe;
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const auto T = rpe::DepthFrontEnd::pose_of(I);
    bool threw = false;                                            // no volume yet
    try { fe.raycastMap(T, k, range); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    fe.initVolume(desc);
    fe.setDepth(depth.data(), k, range);
    fe.integrate(T);
    fe.raycast(T, k, range);
    const Model first = model(fe);
    fe.raycastMap(T, k, range);                                    // the archive is off: the map is the window
    CHECK(hits(first) > 5000 && same(model(fe), first));

    fe.archiveVolume(256);
    const int32_t out[3] = {16, 0, 0};
    fe.shiftVolume(out);
    fe.raycast(T, k, range);
    const Model window = model(fe);
    fe.raycastMap(T, k, range);
    const Model map = model(fe);
    CHECK(hits(map) > hits(window) && same(map, first));           // the slab that left is in the model again
    const rpe_camera kc = {k.fx, k.fy, k.cx, k.cy, k.width, k.height};
    CHECK(rpe_volume_map_raycast(fe.context(), I, &kc, range.dmin, range.dmax, nullptr, nullptr, 0) == RPE_OK && same(model(fe), map));   // with the pre-pass
    const int64_t wlo[3] = {16, 0, 0}, whi[3] = {80, 48, 24};
    fe.raycastMap(T, k, range, 1, wlo, whi);
    CHECK(same(model(fe), window));
    fe.raycastMap(T, k, range, 3);                                 // the model pyramid
    CHECK(fe.map(RPE_MAP_MODEL_VERTEX, 2).cols() == (k.width / 4) * (k.height / 4) && same(model(fe), map));
    threw = false;                                                 // no colour anywhere
    try { fe.raycastMap(T, k, range, 1, nullptr, nullptr, RPE_MAPRAY_COLOR); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    threw = false;
    try { fe.modelColorMap(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    const int64_t odd[3] = {4, 0, 0};
    threw = false;
    try { fe.raycastMap(T, k, range, 1, odd, whi); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw && same(model(fe), map));                          // the model is as before
    std::printf("%ld hits in the map, %ld in the window\n", hits(map), hits(window));
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_map_raycast: %d failure(s)\n" : "volume_map_raycast: ok\n", fails);
  return fails ? 1 : 0;
}
