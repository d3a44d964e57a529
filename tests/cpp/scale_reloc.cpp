// Relocalisation of a camera that has walked UP TO the wall it mapped, through the C++ front end (compiled by
// tests/test_scale_oracle.py, run by tests/test_gpu_scale.py): feature_reloc.cpp's wall at 3 m seen by the 160 x 120 camera, and again
// from 1.5 m closer, where everything is twice as large.  With the default, one scale level the frame is not found; after setLevels(4)
// relocalize returns its pose.  featureScale gives the level and the level pixel of every keypoint, level 0 throughout with one level.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static const double kWallZ = 3.0, kCell = 0.12;

// a byte per lattice cell and channel
static unsigned hash(int i, int j, int c) {
  unsigned h = (unsigned)i * 73856093u ^ (unsigned)j * 19349663u ^ (unsigned)(c + 1) * 0x9E3779B1u;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h & 255u;
}
static double noise(unsigned& s) { s = s * 1664525u + 1013904223u; return 0.002 * (((s >> 8) & 0xffff) / 32768.0 - 1.0); }

// the plane z = kWallZ seen by the camera Xc = R Xw + t
static void render(const double p[12], const rpe::PinholeCamera& k, unsigned seed, std::vector<float>& d, std::vector<uint8_t>& rgb) {
  const double *R = p, *t = p + 9;
  double O[3];
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  d.assign((size_t)k.width * k.height, 0.f);
  rgb.assign((size_t)k.width * k.height * 3, 128);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const double c[3] = {(u - k.cx) / k.fx, (v - k.cy) / k.fy, 1.0};
      double D[3];
      for (int i = 0; i < 3; i++) D[i] = R[i] * c[0] + R[3 + i] * c[1] + R[6 + i] * c[2];
      const double s = (kWallZ - O[2]) / D[2];
      const size_t i = (size_t)v * k.width + u;
      d[i] = (float)(s + noise(seed));
      const int ci = (int)std::floor((O[0] + s * D[0]) / kCell), cj = (int)std::floor((O[1] + s * D[1]) / kCell);
      for (int ch = 0; ch < 3; ch++) rgb[3 * i + ch] = (uint8_t)hash(ci, cj, ch);
    }
}

static void pose_error(const double a[12], const double b[12], double* ang, double* pos) {
  double tr = 0, ca[3], cb[3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) tr += a[3 * i + j] * b[3 * i + j];
  *ang = std::acos(std::min(1.0, std::max(-1.0, (tr - 1) / 2)));
  for (int i = 0; i < 3; i++) {
    ca[i] = -(a[i] * a[9] + a[3 + i] * a[10] + a[6 + i] * a[11]);
    cb[i] = -(b[i] * b[9] + b[3 + i] * b[10] + b[6 + i] * b[11]);
  }
  *pos = std::sqrt((ca[0] - cb[0]) * (ca[0] - cb[0]) + (ca[1] - cb[1]) * (ca[1] - cb[1]) + (ca[2] - cb[2]) * (ca[2] - cb[2]));
}

// feature_reloc.cpp's rule: found = within the solver's own resolution of the truth (5 cm at the wall's 3 m is 0.017 rad)
static bool found(const double P[12], const double truth[12], double* ang, double* pos) {
  pose_error(P, truth, ang, pos);
  return *ang < 0.02 && *pos < 0.05;
}

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  const double A[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  const double B[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.05, -1.5};          // 1.5 m towards the wall and a slide
  std::vector<float> dA, dB;
  std::vector<uint8_t> cA, cB;
  render(A, k, 1u, dA, cA);
  render(B, k, 2u, dB, cB);
  try {
    rpe::DepthFrontEnd fe;
    fe.setDepth(dA.data(), k, range);
    fe.setColor(cA.data());
    fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(A));
    fe.modelColorFromFrame();
    fe.setDepth(dB.data(), k, range);
    fe.setColor(cB.data());
    double P[12], ang = 0, pos = 0;
    std::vector<int32_t> level, lxy;

    CHECK(fe.levels() == 1);
    const rpe::RelocResult one = fe.relocalize(6 /* shinji_kneip_prosac */, 0.05, 3.0, 0.1, 200, 0.99, 7, 1 /* shinji_ls */);
    rpe::DepthFrontEnd::pose12(one.pose, P);
    const bool one_found = one.ok && found(P, B, &ang, &pos);
    std::printf("1 level: ok %d, matches %d, votes %d, found %d\n", (int)one.ok, one.matches, one.votes, (int)one_found);
    CHECK(!one_found);
    fe.featureScale(RPE_FEAT_FRAME, level, lxy);
    const size_t at_one = level.size();
    CHECK(at_one > 20 && lxy.size() == 2 * at_one && std::all_of(level.begin(), level.end(), [](int32_t l) { return l == 0; }));

    fe.setLevels(4);
    CHECK(fe.levels() == 4);
    bool dropped = false;                                                     // the one-level features went with the setting
    try { fe.featureScale(RPE_FEAT_FRAME, level, lxy); } catch (const rpe::DeviceError& e) { dropped = e.code == RPE_ERR_STATE; }
    CHECK(dropped);
    const rpe::RelocResult r = fe.relocalize(6, 0.05, 3.0, 0.1, 200, 0.99, 7, 1);
    rpe::DepthFrontEnd::pose12(r.pose, P);
    const bool reloc_found = found(P, B, &ang, &pos);
    std::printf("4 levels: ok %d, matches %d, votes %d, Iter %d, %.2e rad / %.2e m from the truth\n", (int)r.ok, r.matches, r.votes,
                r.iterations, ang, pos);
    CHECK(r.ok && r.matches >= 40 && r.votes > 20 && r.masks.size() == (size_t)3 * r.matches);
    CHECK(reloc_found);
    fe.featureScale(RPE_FEAT_FRAME, level, lxy);
    CHECK(level.size() > at_one && lxy.size() == 2 * level.size());           // level 0 finds what it found, the others add theirs
    CHECK(std::is_sorted(level.begin(), level.end()) && level.front() == 0 && level.back() >= 2);
    CHECK((size_t)std::count(level.begin(), level.end(), 0) == at_one);
    bool inside = true;                                                       // a level pixel lies 16 inside its level
    const int P4[4] = {1, 2, 1, 1}, Q4[4] = {1, 3, 2, 3};
    for (size_t i = 0; i < level.size(); i++) {
      const int l = level[i], wl = k.width * P4[l] / Q4[l], hl = k.height * P4[l] / Q4[l];
      inside = inside && lxy[2 * i] >= 16 && lxy[2 * i] < wl - 16 && lxy[2 * i + 1] >= 16 && lxy[2 * i + 1] < hl - 16;
    }
    CHECK(inside);

    bool threw = false;
    try { fe.setLevels(5); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw && fe.levels() == 4);
    threw = false;
    try { fe.setLevels(0); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw && fe.levels() == 4);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "scale_reloc: %d failure(s)\n" : "scale_reloc: ok\n", fails);
  return fails ? 1 : 0;
}
