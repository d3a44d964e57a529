// The map volume term through the C++ front end (compiled by tests/test_mapsdf_oracle.py, run and replayed by
// tests/test_gpu_mapsdf.py): a rippled wall fused into a 64 x 48 x 24 window that then moves two bricks along +x with the archive on.
// The frame is tracked from an offset pose against the window alone (icpPyramidVolume) and against the whole map (icpPyramidMap): the
// map term has the rows of the slab that left.  mapResiduals over the window's extent is volumeResiduals, bit for bit; the errors
// behave.  With a directory as argument the frame and the map term's pose are left there for the replay.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void dump(const std::string& dir, const char* name, const void* data, size_t bytes) {
  if (dir.empty()) return;
  std::FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f || std::fwrite(data, 1, bytes, f) != bytes) { std::printf("FAIL cannot write %s\n", name); fails++; }
  if (f) std::fclose(f);
}
static size_t count(const std::vector<float>& r) {
  size_t n = 0;
  for (float x : r) n += std::isnan(x) ? 0 : 1;
  return n;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "";
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const size_t n = (size_t)k.width * k.height;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc desc;
  desc.dim[0] = 64; desc.dim[1] = 48; desc.dim[2] = 24;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -1.28; desc.origin[1] = -0.96; desc.origin[2] = 2.52;
  std::vector<float> depth(n);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) depth[(size_t)v * k.width + u] = (float)(3.0 + 0.1 * std::cos(u / 25.0) + 0.08 * std::sin(v / 20.0));
  try {
    rpe::DepthFrontEnd fe;
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const double off[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.02, -0.015, 0.02};
    const auto T = rpe::DepthFrontEnd::pose_of(I);
    rpe::IcpOptions o;
    o.cos_thr = 0.8;
    fe.setDepthPyramid(depth.data(), k, 3, range);
    bool threw = false;                                            // no volume yet
    try { rpe::DepthFrontEnd::Pose p = T; fe.icpMap(p, o); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    fe.initVolume(desc);
    fe.integrate(T);
    const std::vector<float> whole = fe.volumeResiduals(T, 0, o);
    CHECK(count(fe.mapResiduals(T, 0, o)) == count(whole));         // the archive is off: the map is the window

    fe.archiveVolume(256);
    const int32_t out[3] = {16, 0, 0};
    fe.shiftVolume(out);
    const std::vector<float> rw = fe.volumeResiduals(T, 0, o), rm = fe.mapResiduals(T, 0, o);
    std::printf("rows at the true pose: %zu before the shift, %zu in the window after it, %zu in the map\n", count(whole), count(rw), count(rm));
    CHECK(count(whole) > 0.5 * n && count(rw) < 0.9 * count(whole) && count(rm) > count(rw));
    CHECK(rm.size() == n && std::memcmp(rm.data(), whole.data(), n * sizeof(float)) == 0);   // the box has the first window's origin
    const int64_t wlo[3] = {16, 0, 0}, whi[3] = {80, 48, 24};
    const std::vector<float> re = fe.mapResiduals(T, 0, o, wlo, whi);
    CHECK(std::memcmp(re.data(), rw.data(), n * sizeof(float)) == 0);                         // the window's extent: the window term

    rpe::DepthFrontEnd::Pose pw = rpe::DepthFrontEnd::pose_of(off), pm = pw, pe = pw, p1 = pw;
    const rpe::PyramidIcpResult a = fe.icpPyramidVolume(pw, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
    const rpe::PyramidIcpResult b = fe.icpPyramidMap(pm, {6, 4, 3}, {0.1, 0.15, 0.2}, o);
    double w12[12], m12[12], e12[12];
    rpe::DepthFrontEnd::pose12(pw, w12);
    rpe::DepthFrontEnd::pose12(pm, m12);
    double ew = 0, em = 0;
    for (int i = 0; i < 12; i++) { ew = std::fmax(ew, std::fabs(w12[i] - I[i])); em = std::fmax(em, std::fabs(m12[i] - I[i])); }
    std::printf("window term: %lld rows, max |pose - truth| %.3g; map term: %lld rows, %.3g\n", a.pairs, ew, b.pairs, em);
    CHECK(b.pairs > a.pairs && b.pairs > 0.5 * n && em < 5e-3 && b.iterations >= 3 && b.iterations <= 13);
    dump(dir, "depth.bin", depth.data(), n * sizeof(float));
    dump(dir, "result.bin", m12, sizeof(m12));
    fe.icpPyramidMap(pe, {6, 4, 3}, {0.1, 0.15, 0.2}, o, wlo, whi);
    rpe::DepthFrontEnd::pose12(pe, e12);
    for (int i = 0; i < 12; i++) CHECK(std::fabs(e12[i] - w12[i]) < 1e-4);   // (the map form's sums round otherwise: close, not equal)

    rpe::IcpOptions single = o;
    single.max_iter = 1;
    const rpe::IcpResult r = fe.icpMap(p1, single);
    CHECK(r.iterations == 1 && r.pairs > 0.5 * n && r.cost > 0 && r.last_step > 1e-3);
    threw = false;
    single.device_resident = true;
    try { fe.icpMap(p1, single); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
    const int64_t odd[3] = {4, 0, 0};
    threw = false;
    try { fe.mapResiduals(T, 0, o, odd, whi); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_map_sdf_track: %d failure(s)\n" : "volume_map_sdf_track: ok\n", fails);
  return fails ? 1 : 0;
}
