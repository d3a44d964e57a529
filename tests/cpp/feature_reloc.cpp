// Relocalisation through the C++ front end (compiled by tests/test_feature_oracle.py, run by tests/test_gpu_feature.py): a wall with a
// blocky hashed texture is seen from two poses 0.1 rad of roll and 0.35 m apart -- far outside ICP's basin.  Frame A becomes the model
// (setModelFromFrame + modelColorFromFrame), frame B is relocalised against it with no pose guess: detectFeatures / matchFeatures
// count keypoints and matches, relocalize returns B's pose, icp from it ends on B; icp from A's pose does not.  A frame of one colour
// is a result with ok = false, not an exception.
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

int main() {
  rpe::PinholeCamera k;
  k.fx = k.fy = 292.5; k.cx = 160; k.cy = 120; k.width = 320; k.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  const double A[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  const double cr = std::cos(0.1), sr = std::sin(0.1);
  const double B[12] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1, 0.3, -0.15, 0.1};     // roll about the optical axis, a slide and a step back
  std::vector<float> dA, dB;
  std::vector<uint8_t> cA, cB;
  render(A, k, 1u, false, dA, cA);
  render(B, k, 2u, false, dB, cB);
  try {
    rpe::DepthFrontEnd fe;
    fe.setDepth(dA.data(), k, range);
    fe.setColor(cA.data());
    fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(A));
    fe.modelColorFromFrame();
    fe.setDepth(dB.data(), k, range);
    fe.setColor(cB.data());
    const int nf = fe.detectFeatures(RPE_FEAT_FRAME), nm = fe.detectFeatures(RPE_FEAT_MODEL);
    const int m = fe.matchFeatures();
    std::printf("keypoints %d / %d, matches %d\n", nf, nm, m);
    CHECK(nf > 200 && nm > 200 && m >= 50 && m <= nf);
    rpe::MatchOptions cross;
    cross.cross_check = true;
    CHECK(fe.matchFeatures(cross) <= m);

    const rpe::RelocResult r = fe.relocalize(6 /* shinji_kneip_prosac */, 0.05, 3.0, 0.1, 200, 0.99, 7, 1 /* shinji_ls */);
    double P[12], ang = 0, pos = 0;
    rpe::DepthFrontEnd::pose12(r.pose, P);
    const bool reloc_found = found(P, B, &ang, &pos);
    std::printf("relocalised: ok %d, matches %d, votes %d, Iter %d, %.2e rad / %.2e m from the truth\n", (int)r.ok, r.matches, r.votes,
                r.iterations, ang, pos);
    CHECK(r.ok && r.matches == m && r.votes > 20 && r.masks.size() == (size_t)3 * r.matches);
    CHECK(reloc_found);
    // ICP from the relocalised pose stays on B; from A's pose it does not get there
    rpe::IcpOptions o;
    o.max_iter = 15; o.cos_thr = 0.8;
    rpe::DepthFrontEnd::Pose T = r.pose;
    fe.preparePhoto(1);
    fe.icpRgbd(T, 0.01, o);
    rpe::DepthFrontEnd::pose12(T, P);
    const bool kept = found(P, B, &ang, &pos);
    std::printf("ICP after relocalisation: %.2e rad / %.2e m\n", ang, pos);
    CHECK(kept);
    T = rpe::DepthFrontEnd::pose_of(A);
    bool lost = false;
    try {
      fe.icpRgbd(T, 0.01, o);
      rpe::DepthFrontEnd::pose12(T, P);
      lost = !found(P, B, &ang, &pos);
    } catch (const rpe::DeviceError&) { lost = true; }
    std::printf("ICP from the stale pose: %s\n", lost ? "lost" : "found it");
    CHECK(lost);

    // a frame of one colour: too few matches is a result
    render(B, k, 3u, true, dB, cB);
    fe.setDepth(dB.data(), k, range);
    fe.setColor(cB.data());
    const rpe::RelocResult none = fe.relocalize(6, 0.05, 3.0, 0.1);
    CHECK(!none.ok && none.matches == 0 && none.masks.empty());
    // ... and no model colour is an error
    fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(B));
    bool threw = false;
    try { fe.relocalize(6, 0.05, 3.0, 0.1); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "feature_reloc: %d failure(s)\n" : "feature_reloc: ok\n", fails);
  return fails ? 1 : 0;
}
