// The map mesh through the C++ front end (compiled by tests/test_mapmesh_oracle.py, run by tests/test_gpu_mapmesh.py): a wall fused into
// a 64 x 48 x 24 window that then moves two bricks along +x.  mapBounds and meshMap are each held once to the C call they wrap; the
// whole map shows the slab that left, the window's extent is the window's own mesh, triangle for triangle.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// every triangle as its nine position words, sorted
static std::vector<std::array<uint32_t, 9>> words(const rpe::Mesh& M) {
  std::vector<std::array<uint32_t, 9>> out(M.triangles.size() / 3);
  for (size_t t = 0; t < out.size(); t++)
    for (int k = 0; k < 3; k++) std::memcpy(&out[t][3 * k], M.vertices.data() + 3 * (size_t)M.triangles[3 * t + k], 12);
  std::sort(out.begin(), out.end());
  return out;
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
    int64_t lo[3], hi[3], lo_c[3], hi_c[3];
    bool threw = false;                                            // no volume yet
    try { fe.meshMap(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    fe.initVolume(desc);
    fe.setDepth(depth.data(), k, range);
    fe.integrate(rpe::DepthFrontEnd::pose_of(I));
    const rpe::Mesh whole = fe.mesh(1);
    fe.mapBounds(lo, hi);                                          // the archive is off: the window
    CHECK(lo[0] == 0 && lo[1] == 0 && lo[2] == 0 && hi[0] == 64 && hi[1] == 48 && hi[2] == 24);
    const rpe::Mesh same = fe.meshMap(1);
    CHECK(whole.triangles.size() > 3000 && words(same) == words(whole));

    fe.archiveVolume(256);
    const int32_t out[3] = {16, 0, 0};
    fe.shiftVolume(out);
    fe.mapBounds(lo, hi);
    CHECK(rpe_volume_map_bounds(fe.context(), lo_c, hi_c) == RPE_OK && std::memcmp(lo, lo_c, sizeof(lo)) == 0 && std::memcmp(hi, hi_c, sizeof(hi)) == 0);
    CHECK(lo[0] == 0 && hi[0] == 80 && lo[1] >= 0 && hi[1] <= 48 && lo[2] >= 0 && hi[2] <= 24);
    const rpe::Mesh map = fe.meshMap(1);
    int64_t nv = -1, nt = -1;
    CHECK(rpe_volume_map_mesh(fe.context(), 1, nullptr, nullptr, &nv, &nt) == RPE_OK && nv == map.vertices.cols() && (size_t)nt * 3 == map.triangles.size());
    const rpe::Mesh window = fe.mesh(1);
    const int64_t wlo[3] = {16, 0, 0}, whi[3] = {80, 48, 24};
    const rpe::Mesh boxed = fe.meshMap(1, wlo, whi);
    CHECK(words(boxed) == words(window));
    // the slab that left is in the map and not in the window; the map has every triangle the fixed window had (the wall ends at x = 64)
    CHECK(map.triangles.size() > window.triangles.size() && words(map) == words(whole));
    threw = false;                                                 // no colour anywhere
    try { fe.meshColors(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    const int64_t odd[3] = {4, 0, 0};
    threw = false;
    try { fe.meshMap(1, odd, whi); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
    std::printf("%zu triangles in the map, %zu in the window\n", map.triangles.size() / 3, window.triangles.size() / 3);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_map_mesh: %d failure(s)\n" : "volume_map_mesh: ok\n", fails);
  return fails ? 1 : 0;
}
