// Relocalisation against a keyframe store through the C++ front end (compiled by tests/test_keyframe_oracle.py, run by
// tests/test_gpu_keyframes.py): a wall with a blocky hashed texture is seen from three keyframe poses a metre and a half apart along
// it, each added to the store from the tracked frame (setModelFromFrame + modelColorFromFrame + detectFeatures + addKeyframe).  A frame
// near the LAST keyframe is then relocalised with no pose guess and no hint which keyframe it sees: queryKeyframes ranks that keyframe
// first, matchKeyframe gives the count the query announced, relocalizeKeyframes returns the frame's pose and the keyframe it chose.  The
// store survives the new frames and models in between; a frame of one colour is a result with ok = false; an empty store is an error.
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
  const int K = 3;
  double KF[K][12];
  for (int i = 0; i < K; i++) {
    const double p[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, -1.5 * i, 0, 0};         // the camera 1.5 m further along the wall each time
    std::copy(p, p + 12, KF[i]);
  }
  const double cr = std::cos(0.1), sr = std::sin(0.1);
  const double B[12] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1, 0.3 - 3.0 * cr, -0.15 - 3.0 * sr, 0.1};   // keyframe 2's view rolled, slid, stepped back
  std::vector<float> d;
  std::vector<uint8_t> c;
  try {
    rpe::DepthFrontEnd fe;
    int kp[K];
    for (int i = 0; i < K; i++) {
      render(KF[i], k, 1u + i, false, d, c);
      fe.setDepth(d.data(), k, range);
      fe.setColor(c.data());
      fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(KF[i]));
      fe.modelColorFromFrame();
      kp[i] = fe.detectFeatures(RPE_FEAT_MODEL);
      CHECK(fe.addKeyframe() == i && kp[i] > 200);
    }
    CHECK(fe.keyframes() == K);
    render(B, k, 9u, false, d, c);
    fe.setDepth(d.data(), k, range);
    fe.setColor(c.data());
    const int nf = fe.detectFeatures(RPE_FEAT_FRAME);
    const rpe::KeyframeRanking q = fe.queryKeyframes();
    std::printf("keypoints %d against %d / %d / %d, counts %d / %d / %d, best %d\n", nf, kp[0], kp[1], kp[2], q.counts[0], q.counts[1],
                q.counts[2], q.order[0]);
    CHECK(q.counts.size() == (size_t)K && q.order[0] == 2 && q.counts[2] >= 50 && q.counts[2] > q.counts[1] && q.counts[1] > q.counts[0]);
    CHECK(fe.matchKeyframe(2) == q.counts[2] && fe.matchKeyframe(0) == q.counts[0]);
    rpe::MatchOptions cross;
    cross.cross_check = true;
    CHECK(fe.matchKeyframe(2, cross) <= q.counts[2]);

    const rpe::KeyframeRelocResult r = fe.relocalizeKeyframes(6 /* shinji_kneip_prosac */, 0.05, 3.0, 0.1, 3, 200, 0.99, 7, 1 /* shinji_ls */);
    double P[12], ang = 0, pos = 0;
    rpe::DepthFrontEnd::pose12(r.pose, P);
    const bool reloc_found = found(P, B, &ang, &pos);
    std::printf("relocalised: ok %d, keyframe %d, matches %d, votes %d, Iter %d, %.2e rad / %.2e m from the truth\n", (int)r.ok, r.keyframe,
                r.matches, r.votes, r.iterations, ang, pos);
    CHECK(r.ok && r.keyframe == 2 && r.matches == q.counts[2] && r.votes > 20 && r.masks.size() == (size_t)3 * r.matches);
    CHECK(reloc_found);

    // a frame of one colour: no keyframe with enough matches is a result, and it names the best-ranked keyframe
    render(B, k, 3u, true, d, c);
    fe.setDepth(d.data(), k, range);
    fe.setColor(c.data());
    const rpe::KeyframeRelocResult none = fe.relocalizeKeyframes(6, 0.05, 3.0, 0.1);
    CHECK(!none.ok && none.matches == 0 && none.keyframe == 0 && none.masks.empty());
    CHECK(fe.keyframes() == K);
    fe.clearKeyframes();
    CHECK(fe.keyframes() == 0);
    bool threw = false;
    try { fe.queryKeyframes(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
    threw = false;
    try { fe.relocalizeKeyframes(6, 0.05, 3.0, 0.1); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "keyframe_reloc: %d failure(s)\n" : "keyframe_reloc: ok\n", fails);
  return fails ? 1 : 0;
}
