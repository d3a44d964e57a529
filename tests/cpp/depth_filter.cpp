// The depth filter through the C++ front end (compiled by tests/test_filter_oracle.py, run by tests/test_gpu_filter.py): a wall 3 m
// away seen with a depth sensor's noise (2 cm at that range, millimetre steps).  Raw, the frame's normals are mostly noise; after
// setDepthFilter(DepthFilter()) they point at the camera again.  The setting is read back, a bad one is refused and leaves it alone,
// and turning the filter off gives the bits of the frame that never had it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// a sum of twelve uniforms: near enough a standard normal
static double gauss(unsigned& s) {
  double a = -6.0;
  for (int i = 0; i < 12; i++) { s = s * 1664525u + 1013904223u; a += ((s >> 8) & 0xffff) / 65536.0; }
  return a;
}

// median angle (degrees) between the frame's normals and the wall's (0, 0, -1), and how many pixels have a normal
static double median_angle(const rpe::MatrixX<float>& N, int* count) {
  std::vector<double> ang;
  for (int i = 0; i < N.cols(); i++) {
    const float* n = N.data() + 3 * (size_t)i;
    if (n[0] == n[0]) ang.push_back(std::acos(std::min(1.0, std::max(-1.0, -(double)n[2]))) * 180.0 / 3.14159265358979323846);
  }
  *count = (int)ang.size();
  if (ang.empty()) return 180.0;
  std::nth_element(ang.begin(), ang.begin() + ang.size() / 2, ang.end());
  return ang[ang.size() / 2];
}

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 146.25; k.cx = 80; k.cy = 60; k.width = 160; k.height = 120;
  const size_t n = (size_t)k.width * k.height;
  std::vector<unsigned short> depth(n);
  unsigned seed = 11u;
  const double z = 3.0, sigma = 0.0012 + 0.0019 * (z - 0.4) * (z - 0.4);
  for (size_t i = 0; i < n; i++) depth[i] = (unsigned short)std::lround((z + sigma * gauss(seed)) * 1000.0);
  try {
    rpe::DepthFrontEnd fe;
    CHECK(fe.depthFilter().radius == 0);                                       // off by default
    fe.setDepth(depth.data(), k);
    const rpe::MatrixX<float> raw = fe.map(RPE_MAP_NORMAL), raw_v = fe.map(RPE_MAP_VERTEX);
    int raw_count = 0, fil_count = 0;
    const double raw_deg = median_angle(raw, &raw_count);

    fe.setDepthFilter(rpe::DepthFilter());
    const rpe::DepthFilter f = fe.depthFilter();
    CHECK(f.radius == 3 && f.sigma_space == 2.0 && f.depth_cut == 0.01 && f.depth_cut_z2 == 0.02);
    const rpe::MatrixX<float> same = fe.map(RPE_MAP_NORMAL);                   // the setting does not touch the current frame
    CHECK(std::memcmp(same.data(), raw.data(), sizeof(float) * 3 * n) == 0);
    fe.setDepth(depth.data(), k);
    const double fil_deg = median_angle(fe.map(RPE_MAP_NORMAL), &fil_count);
    std::printf("median angle to the wall's normal: raw %.1f deg over %d pixels, filtered %.1f deg over %d\n", raw_deg, raw_count,
                fil_deg, fil_count);
    CHECK(fil_deg * 3 <= raw_deg && fil_count >= raw_count);

    bool threw = false;
    rpe::DepthFilter bad;
    bad.radius = RPE_FILTER_MAX_RADIUS + 1;
    try { fe.setDepthFilter(bad); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw && fe.depthFilter().radius == 3);
    threw = false;
    bad = rpe::DepthFilter();
    bad.depth_cut = 0.0;
    try { fe.setDepthFilter(bad); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_ARG; }
    CHECK(threw && fe.depthFilter().depth_cut == 0.01);

    fe.setDepthFilter(rpe::DepthFilter::off());
    CHECK(fe.depthFilter().radius == 0);
    fe.setDepth(depth.data(), k);
    const rpe::MatrixX<float> again = fe.map(RPE_MAP_NORMAL), again_v = fe.map(RPE_MAP_VERTEX);
    CHECK(std::memcmp(again.data(), raw.data(), sizeof(float) * 3 * n) == 0);
    CHECK(std::memcmp(again_v.data(), raw_v.data(), sizeof(float) * 3 * n) == 0);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "depth_filter: %d failure(s)\n" : "depth_filter: ok\n", fails);
  return fails ? 1 : 0;
}
