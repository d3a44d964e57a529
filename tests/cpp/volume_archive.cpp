// The volume archive through the C++ front end (compiled by tests/test_archive_oracle.py, run by tests/test_gpu_archive_cpp.py): a wall
// fused into a 64 x 48 x 24 window that then moves two bricks along +x and back.  archiveVolume / archiveHeld / archiveDownload /
// archiveClear are each held once to the C call they wrap, the returned window to the one before the walk, bit for bit.
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
  rpe::VolumeDesc desc;
  desc.dim[0] = 64; desc.dim[1] = 48; desc.dim[2] = 24;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -1.28; desc.origin[1] = -0.96; desc.origin[2] = 2.52;
  std::vector<float> depth((size_t)k.width * k.height);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) depth[(size_t)v * k.width + u] = (float)(3.0 + 0.1 * std::cos(u / 25.0));
  try {
    rpe::DepthFrontEnd fe;
    bool threw = false;                                            // no volume yet
    try { fe.archiveVolume(64); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    fe.initVolume(desc);
    fe.setDepth(depth.data(), k, range);
    fe.integrate(rpe::DepthFrontEnd::pose_of(I));
    const rpe::MatrixX<float> before = fe.volume();
    int64_t cap = -1, held_c = -1, cap_c = -1;
    CHECK(fe.archiveHeld(&cap) == 0 && cap == 0);                  // off
    fe.archiveVolume(256);
    CHECK(fe.archiveHeld(&cap) == 0 && cap == 256);
    CHECK(rpe_volume_archive_info(fe.context(), &held_c, &cap_c) == RPE_OK && held_c == 0 && cap_c == 256);

    const int32_t odd[3] = {4, 0, 0}, out[3] = {16, 0, 0}, back[3] = {-16, 0, 0};
    threw = false;                                                 // not a multiple of 8
    try { fe.shiftVolume(odd); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
    fe.shiftVolume(out);
    const int64_t held = fe.archiveHeld();
    CHECK(held > 0 && held <= 2 * 6 * 3);                          // of the 2 x 6 x 3 bricks that left, those the wall touches
    std::vector<int64_t> coords, coords_c;
    std::vector<float> tsdf, tsdf_c;
    std::vector<uint16_t> colour;
    CHECK(fe.archiveDownload(coords, tsdf, &colour) == held && coords.size() == (size_t)held * 3 && tsdf.size() == (size_t)held * 1024);
    coords_c.assign(coords.size(), -7); tsdf_c.assign(tsdf.size(), -1.f);
    CHECK(rpe_volume_archive_download(fe.context(), coords_c.data(), tsdf_c.data(), nullptr) == RPE_OK);
    CHECK(coords == coords_c && std::memcmp(tsdf.data(), tsdf_c.data(), tsdf.size() * sizeof(float)) == 0);
    bool sorted = true, inside = true, zero = true;
    for (int64_t n = 0; n < held; n++) {
      const int64_t* b = &coords[3 * n];
      inside = inside && b[0] >= 0 && b[0] < 2 && b[1] >= 0 && b[1] < 6 && b[2] >= 0 && b[2] < 3;
      if (n) { const int64_t* a = b - 3; sorted = sorted && (a[2] < b[2] || (a[2] == b[2] && (a[1] < b[1] || (a[1] == b[1] && a[0] < b[0])))); }
    }
    for (uint16_t c : colour) zero = zero && c == 0;
    CHECK(sorted && inside && zero);
    // the first brick's first voxel is the window's voxel at 8 x its coordinates before the shift
    const int64_t* b0 = &coords[0];
    const size_t v0 = ((size_t)(8 * b0[2]) * desc.dim[1] + 8 * b0[1]) * desc.dim[0] + 8 * b0[0];
    CHECK(std::memcmp(&tsdf[0], before.data() + 2 * v0, 2 * sizeof(float)) == 0);

    fe.shiftVolume(back);
    CHECK(fe.archiveHeld() == 0);
    const rpe::MatrixX<float> after = fe.volume();
    CHECK(after.cols() == before.cols() && std::memcmp(after.data(), before.data(), sizeof(float) * 2 * (size_t)before.cols()) == 0);
    std::printf("%lld bricks left and returned; the window is what it was\n", (long long)held);

    fe.shiftVolume(out);
    CHECK(fe.archiveHeld() == held);
    fe.archiveClear();
    CHECK(fe.archiveHeld(&cap) == 0 && cap == 256);
    fe.archiveVolume(0);
    CHECK(fe.archiveHeld(&cap) == 0 && cap == 0);
    fe.shiftVolume(odd);                                           // off: any shift again
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_archive: %d failure(s)\n" : "volume_archive: ok\n", fails);
  return fails ? 1 : 0;
}
