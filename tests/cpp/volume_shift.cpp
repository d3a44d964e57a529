// The moving volume through the C++ front end (compiled by tests/test_shift_oracle.py, run by tests/test_gpu_shift_cpp.py): a wall at
// z = 3 fused from a camera that then steps 0.8 m along it.  followShift proposes the shift, mesh(min_weight, lo, hi) keeps the slab
// that leaves, shiftVolume moves the window; each DepthFrontEnd method is held once to the C call it wraps, the moved volume to the
// old one voxel by voxel, and the triangles of the leaving slab plus the new window's to the mesh before the shift.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc desc;                                            // 2.6 x 2.0 x 0.96 m around the wall, 4 cm voxels, an odd row
  desc.dim[0] = 65; desc.dim[1] = 50; desc.dim[2] = 24;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -1.3; desc.origin[1] = -1.0; desc.origin[2] = 2.52;
  std::vector<float> depth((size_t)k.width * k.height);
  for (int v = 0; v < k.height; v++)                               // a gently curved wall: z = 3 + 0.1 cos(u / 25)
    for (int u = 0; u < k.width; u++) depth[(size_t)v * k.width + u] = (float)(3.0 + 0.1 * std::cos(u / 25.0));
  try {
    rpe::DepthFrontEnd fe;
    int32_t d[3] = {1, 0, 0};
    bool threw = false;                                            // no volume yet
    try { fe.shiftVolume(d); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);

    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    fe.initVolume(desc);
    fe.setDepth(depth.data(), k, range);
    fe.integrate(rpe::DepthFrontEnd::pose_of(I));
    fe.integrate(rpe::DepthFrontEnd::pose_of(I));
    const rpe::MatrixX<float> before = fe.volume();
    const rpe::Mesh whole = fe.mesh();
    CHECK(whole.triangles.size() > 3000);

    // the camera 0.8 m further along +x: Xc = Xw - (0.8, 0, 0); the target 3 m ahead is 20 voxels off the centre
    const double P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -0.8, 0, 0};
    fe.followShift(rpe::DepthFrontEnd::pose_of(P), 3.0, 8, d);
    int32_t dc[3] = {0, 0, 0};
    CHECK(rpe_volume_follow(fe.context(), P, 3.0, 8, dc) == RPE_OK && std::memcmp(d, dc, sizeof(d)) == 0);
    CHECK(d[0] == 16 && d[1] == 0 && d[2] == 0);

    // what leaves: the cubes with i < 16
    const int32_t lo[3] = {0, 0, 0}, hi[3] = {d[0], desc.dim[1] - 1, desc.dim[2] - 1};
    const rpe::Mesh gone = fe.mesh(1.0, lo, hi);
    int64_t nv = 0, nt = 0;
    CHECK(rpe_volume_mesh_box(fe.context(), 1.0, lo, hi, &nv, &nt) == RPE_OK && nv == gone.vertices.cols() && 3 * nt == (int64_t)gone.triangles.size());
    CHECK(!gone.triangles.empty() && gone.triangles.size() < whole.triangles.size());
    float xmax = -1e30f;
    for (int v = 0; v < gone.vertices.cols(); v++) xmax = std::max(xmax, gone.vertices(0, v));
    CHECK(xmax <= (float)(desc.origin[0] + (d[0] + 0.5) * desc.voxel_size) + 1e-4f);   // nothing beyond the cut's far corners

    fe.shiftVolume(d);
    threw = false;                                                 // the shift dropped the mesh
    try { (void)fe.meshColors(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    int64_t total[3] = {0, 0, 0}, totalc[3] = {0, 0, 0};
    const rpe::VolumeDesc now = fe.volumeGeometry(total);
    rpe_volume_desc vc;
    CHECK(rpe_volume_geometry(fe.context(), &vc, totalc) == RPE_OK && std::memcmp(total, totalc, sizeof(total)) == 0);
    CHECK(total[0] == 16 && total[1] == 0 && total[2] == 0);
    CHECK(now.origin[0] == desc.origin[0] + 16.0 * desc.voxel_size && now.origin[0] == vc.origin[0] && now.origin[1] == desc.origin[1]
          && now.origin[2] == desc.origin[2] && now.dim[0] == desc.dim[0] && now.voxel_size == desc.voxel_size);

    // voxel by voxel: new (i, j, k) = old (i + 16, j, k), zero where that was outside
    const rpe::MatrixX<float> after = fe.volume();
    size_t bad = 0, moved = 0;
    for (int kk = 0; kk < desc.dim[2]; kk++)
      for (int j = 0; j < desc.dim[1]; j++)
        for (int i = 0; i < desc.dim[0]; i++) {
          const int v = (kk * desc.dim[1] + j) * desc.dim[0] + i;
          float want[2] = {0.f, 0.f};
          if (i + d[0] < desc.dim[0]) { want[0] = before(0, v + d[0]); want[1] = before(1, v + d[0]); moved += want[1] > 0; }
          const float got[2] = {after(0, v), after(1, v)};
          bad += std::memcmp(want, got, sizeof(want)) != 0;
        }
    CHECK(bad == 0 && moved > 1000);

    // no triangle lost or doubled: the leaving slab's and the new window's add up to the mesh before the shift
    const rpe::Mesh stays = fe.mesh();
    CHECK(gone.triangles.size() + stays.triangles.size() == whole.triangles.size());
    std::printf("whole %d triangles = leaving %d + staying %d; window at x = %.2f after %lld voxels\n", (int)whole.triangles.size() / 3,
                (int)gone.triangles.size() / 3, (int)stays.triangles.size() / 3, now.origin[0], (long long)total[0]);

    // the window is an ordinary volume: raycast from the new pose finds the wall
    fe.raycast(rpe::DepthFrontEnd::pose_of(P), k, range);
    const int32_t back[3] = {-16, 0, 0}, none[3] = {0, 0, 0};
    fe.shiftVolume(back);
    fe.shiftVolume(none);
    (void)fe.volumeGeometry(total);
    CHECK(total[0] == 0 && fe.volumeGeometry().origin[0] == desc.origin[0]);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_shift: %d failure(s)\n" : "volume_shift: ok\n", fails);
  return fails ? 1 : 0;
}
