// Loop closing through the C++ front end (compiled by tests/test_graph_oracle.py, run by tests/test_gpu_graph.py): a wall with a blocky
// hashed texture is seen from three keyframe poses a metre and a half apart along it.  The tracker that stored them had DRIFTED: each
// keyframe is added at a pose that is off by more than the one before, so its world points sit where that pose puts them.  A frame
// near the last keyframe relocalised against this store is found where the drifted keyframe says, not where it is.  linkKeyframes
// links the keyframes by their own matches, optimizeKeyframes refines all poses with keyframe 0 as the anchor and rewrites the store;
// afterwards every keyframe pose is close to the truth and the same frame relocalises to its true pose.
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
static void render(const double p[12], const rpe::PinholeCamera& k, unsigned seed, bool flat, std::vector<float>& d, std::vector<uint8_t>& rgb) {
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
      if (flat) continue;
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

// A pose counts as FOUND when it is within the solver's own resolution of the truth: the consensus was voted with a 3-D threshold of
// 5 cm, so a pose it supports cannot place the wall further off than that, and 5 cm across at the wall's 3 m is 0.017 rad.  Tracking
// that starts from a found pose must stay found; tracking from the stale pose must not get there.
static bool found(const double P[12], const double truth[12], double* ang, double* pos) {
  pose_error(P, truth, ang, pos);
  return *ang < 0.02 && *pos < 0.05;
}

// d followed after p: Xc = Rd (R Xw + t) + td, Rd a roll by `a`
static void drifted(const double p[12], double a, double x, double y, double z, double out[12]) {
  const double c = std::cos(a), s = std::sin(a), Rd[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, td[3] = {x, y, z};
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) out[3 * r + q] = Rd[3 * r] * p[q] + Rd[3 * r + 1] * p[3 + q] + Rd[3 * r + 2] * p[6 + q];
    out[9 + r] = Rd[3 * r] * p[9] + Rd[3 * r + 1] * p[10] + Rd[3 * r + 2] * p[11] + td[r];
  }
}

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 292.5; k.cx = 160; k.cy = 120; k.width = 320; k.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  const int K = 3;
  double KF[K][12], DR[K][12];
  for (int i = 0; i < K; i++) {
    const double p[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -1.5 * i, 0, 0};         // the camera 1.5 m further along the wall each time
    std::copy(p, p + 12, KF[i]);
    drifted(p, 0.02 * i, 0.05 * i, -0.03 * i, 0.02 * i, DR[i]);                // ... and the tracker's pose further off each time
  }
  const double cr = std::cos(0.1), sr = std::sin(0.1);
  const double B[12] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1, 0.3 - 3.0 * cr, -0.15 - 3.0 * sr, 0.1};   // keyframe 2's view rolled, slid, stepped back
  std::vector<float> d;
  std::vector<uint8_t> c;
  try {
    rpe::DepthFrontEnd fe;
    for (int i = 0; i < K; i++) {
      render(KF[i], k, 1u + i, false, d, c);
      fe.setDepth(d.data(), k, range);
      fe.setColor(c.data());
      fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(DR[i]));
      fe.modelColorFromFrame();
      fe.detectFeatures(RPE_FEAT_MODEL);
      const int id = fe.addKeyframe();
      const int edges = fe.linkKeyframes(id);                                  // each new keyframe against the older ones
      std::printf("keyframe %d: %d edge(s)\n", id, edges);
      CHECK(id == i && edges >= (i > 0 ? i : 0));
    }
    double P[12], ang = 0, pos = 0;
    render(B, k, 9u, false, d, c);
    fe.setDepth(d.data(), k, range);
    fe.setColor(c.data());
    rpe::KeyframeRelocResult r = fe.relocalizeKeyframes(6 /* shinji_kneip_prosac */, 0.05, 3.0, 0.1, 3, 200, 0.99, 7, 1 /* shinji_ls */);
    rpe::DepthFrontEnd::pose12(r.pose, P);
    const bool before = found(P, B, &ang, &pos);
    std::printf("drifted store: ok %d, keyframe %d, %.2e rad / %.2e m from the truth\n", (int)r.ok, r.keyframe, ang, pos);
    CHECK(r.ok && r.keyframe == 2 && !before);

    const std::vector<double> gates = {0.3, 0.15, 0.1, 0.05, 0.05, 0.05};
    const rpe::GraphResult dry = fe.optimizeKeyframes(gates, 0, 0.0, false);
    rpe::DepthFrontEnd::pose12(fe.keyframePose(2), P);
    CHECK(dry.ok && dry.poses.size() == (size_t)K && dry.pairs.size() == gates.size());
    CHECK(std::equal(P, P + 12, DR[2]));                                       // apply = false: the store is what it was
    const rpe::GraphResult g = fe.optimizeKeyframes(gates);
    CHECK(g.ok && g.poses.size() == (size_t)K && g.pairs.size() == gates.size() && g.pairs.back() >= 50 && g.step.back() < g.step.front());
    for (int i = 0; i < K; i++) {
      double e0a, e0p;
      pose_error(DR[i], KF[i], &e0a, &e0p);
      rpe::DepthFrontEnd::pose12(fe.keyframePose(i), P);
      pose_error(P, KF[i], &ang, &pos);
      std::printf("keyframe %d: %.2e rad / %.2e m -> %.2e rad / %.2e m from the truth (%lld pairs in the last round)\n", i, e0a, e0p, ang, pos,
                  (long long)g.pairs.back());
      if (i == 0) CHECK(std::equal(P, P + 12, DR[0]));                         // the anchor stays
      else CHECK(ang < e0a / 3 && pos < e0p / 3);
    }
    r = fe.relocalizeKeyframes(6, 0.05, 3.0, 0.1, 3, 200, 0.99, 7, 1);
    rpe::DepthFrontEnd::pose12(r.pose, P);
    const bool after = found(P, B, &ang, &pos);
    std::printf("corrected store: ok %d, keyframe %d, %.2e rad / %.2e m from the truth\n", (int)r.ok, r.keyframe, ang, pos);
    CHECK(r.ok && r.keyframe == 2 && after);

    fe.clearKeyframes();                                                       // the graph goes with the store
    bool threw = false;
    try { fe.optimizeKeyframes(gates); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    threw = false;
    try { fe.linkKeyframes(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "graph_optimize: %d failure(s)\n" : "graph_optimize: ok\n", fails);
  return fails ? 1 : 0;
}
