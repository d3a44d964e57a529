// The photometric term through the C++ front end (compiled by tests/test_photo_oracle.py, run by tests/test_gpu_photo.py): a textured
// WALL -- one plane in view -- is seen from two poses 10 mrad of roll and 50 mm of in-plane slide apart.  Frame A becomes the model
// (setModelFromFrame + modelColorFromFrame), frame B is tracked from A's pose: icp alone stays where it started (the plane holds
// neither the slide nor the roll), icpRgbd finds B.  Also: the residual image shrinks, and a new depth drops the prepared maps.  With
// an output directory as argument, the frames, poses and the result are written there so that the Python path can replay the same
// calls and compare the bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static const double kWallZ = 3.0;
// texture: channel c = 127.5 + 120 sin(k_c . P + phi_c), wavelengths of about 1.3 m
static const double kTexK[3][3] = {{1.0, 5.0, 0.6}, {1.5, 0.0, 3.7}, {0.0, 2.0, 4.5}};
static const double kTexPhi[3] = {0.3, 1.2, 2.0};

static double texture(const double P[3], int c) {
  return 127.5 + 120.0 * std::sin(kTexK[c][0] * P[0] + kTexK[c][1] * P[1] + kTexK[c][2] * P[2] + kTexPhi[c]);
}
// depth noise of +-2 mm, a fixed sequence
static double noise(unsigned& s) { s = s * 1664525u + 1013904223u; return 0.002 * (((s >> 8) & 0xffff) / 32768.0 - 1.0); }

// the plane z = kWallZ seen by the camera Xc = R Xw + t
static void render(const double p[12], const rpe::PinholeCamera& k, unsigned seed, std::vector<float>& d, std::vector<uint8_t>& rgb) {
  const double *R = p, *t = p + 9;
  double O[3];
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  d.assign((size_t)k.width * k.height, 0.f);
  rgb.assign((size_t)k.width * k.height * 3, 0);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const double c[3] = {(u - k.cx) / k.fx, (v - k.cy) / k.fy, 1.0};
      double D[3];
      for (int i = 0; i < 3; i++) D[i] = R[i] * c[0] + R[3 + i] * c[1] + R[6 + i] * c[2];
      const double s = (kWallZ - O[2]) / D[2];     // camera depth of the hit (c[2] = 1)
      const size_t i = (size_t)v * k.width + u;
      d[i] = (float)(s + noise(seed));
      const double P[3] = {O[0] + s * D[0], O[1] + s * D[1], O[2] + s * D[2]};
      for (int ch = 0; ch < 3; ch++) rgb[3 * i + ch] = (uint8_t)std::min(255.0, std::max(0.0, std::nearbyint(texture(P, ch))));
    }
}

template <class T> static void dump(const std::string& dir, const char* name, const T* p, size_t n) {
  if (dir.empty()) return;
  FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f) { std::printf("FAIL cannot write %s\n", name); fails++; return; }
  if (n) std::fwrite(p, sizeof(T), n, f);
  std::fclose(f);
}

// (rotation angle, distance of the camera centres) between two poses
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

static double median_abs(std::vector<float> r, size_t* pairs) {
  r.erase(std::remove_if(r.begin(), r.end(), [](float x) { return std::isnan(x); }), r.end());
  *pairs = r.size();
  if (r.empty()) return 1e30;
  for (float& x : r) x = std::fabs(x);
  std::nth_element(r.begin(), r.begin() + r.size() / 2, r.end());
  return r[r.size() / 2];
}

int main(int argc, char** argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  const double a = 0.01, ca = std::cos(a), sa = std::sin(a);
  const double pA[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  const double pB[12] = {ca, -sa, 0, sa, ca, 0, 0, 0, 1, 0.04, -0.03, 0};
  std::vector<float> dA, dB;
  std::vector<uint8_t> cA, cB;
  render(pA, cam, 1u, dA, cA);
  render(pB, cam, 2u, dB, cB);
  dump(out, "depthA.bin", dA.data(), dA.size()); dump(out, "rgbA.bin", cA.data(), cA.size());
  dump(out, "depthB.bin", dB.data(), dB.size()); dump(out, "rgbB.bin", cB.data(), cB.size());
  dump(out, "poses.bin", pA, 12);

  rpe::DepthFrontEnd fe;
  bool threw = false;
  fe.setDepth(dA.data(), cam, range);
  try { fe.modelColorFromFrame(); } catch (const rpe::DeviceError&) { threw = true; }   // no model, no colour yet
  CHECK(threw);
  fe.setColor(cA.data());
  fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(pA));
  fe.modelColorFromFrame();
  fe.setDepth(dB.data(), cam, range);
  threw = false;
  try { fe.preparePhoto(1); } catch (const rpe::DeviceError&) { threw = true; }         // the new depth dropped the frame colour
  CHECK(threw);
  fe.setColor(cB.data());
  fe.preparePhoto(1);

  rpe::IcpOptions o;
  o.max_iter = 12; o.tol = 0; o.cos_thr = 0.8;
  double start_ang, start_pos, ang, pos, p[12];
  pose_error(pA, pB, &start_ang, &start_pos);
  // ICP alone: the wall holds neither the slide nor the roll -- it reports a singular system or ends about where it started
  rpe::DepthFrontEnd::Pose T = rpe::DepthFrontEnd::pose_of(pA);
  bool degenerate = false;
  o.fused = false;
  try { fe.icp(T, o); } catch (const rpe::DeviceError&) { degenerate = true; }
  rpe::DepthFrontEnd::pose12(T, p);
  pose_error(p, pB, &ang, &pos);
  std::printf("icp alone: %s, %.2e rad / %.2e m from the truth (start %.2e / %.2e)\n", degenerate ? "degenerate" : "ran", ang, pos, start_ang,
              start_pos);
  CHECK(degenerate || (ang > start_ang / 2 && pos > start_pos / 2));
  // with the photometric term
  T = rpe::DepthFrontEnd::pose_of(pA);
  size_t pairs0 = 0, pairs1 = 0;
  const double med0 = median_abs(fe.photoResiduals(T), &pairs0);
  const rpe::RgbdIcpResult r = fe.icpRgbd(T, 0.01, o);
  const double med1 = median_abs(fe.photoResiduals(T), &pairs1);
  rpe::DepthFrontEnd::pose12(T, p);
  pose_error(p, pB, &ang, &pos);
  std::printf("icp + photometric: %d rounds, %.2e rad / %.2e m from the truth; %lld geometric and %lld photometric pairs; median |r| %.2f -> "
              "%.2f levels\n", r.iterations, ang, pos, r.pairs, r.photo_pairs, med0, med1);
  CHECK(r.iterations == 12 && ang < 5e-4 && pos < 1e-3);
  CHECK(r.photo_pairs > 0.8 * cam.width * cam.height && r.pairs > 0.8 * cam.width * cam.height && r.photo_cost > 0);
  CHECK(pairs0 > 0.8 * dA.size() && pairs1 > 0.8 * dA.size() && med1 < 0.5 * med0 && med1 < 1.0);
  dump(out, "result.bin", p, 12);
  // refused: the resident forms, point-to-point
  rpe::IcpOptions bad = o;
  bad.device_resident = true;
  threw = false;
  try { fe.icpRgbd(T, 0.01, bad); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  bad = o; bad.kind = RPE_RES_P2P;
  threw = false;
  try { fe.icpRgbd(T, 0.01, bad); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  // a new depth drops the prepared maps
  fe.setDepth(dB.data(), cam, range);
  threw = false;
  try { fe.icpRgbd(T, 0.01, o); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  if (fails) { std::printf("photo_track: %d failures\n", fails); return 1; }
  std::printf("photo_track: ok\n");
  return 0;
}
