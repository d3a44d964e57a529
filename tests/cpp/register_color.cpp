// Colour registration through the C++ front end (compiled by tests/test_register_oracle.py, run by tests/test_gpu_register.py): a depth
// frame of a textured box room and the image of a SEPARATE colour camera -- 400 x 300 pixels, 5 cm beside the depth camera, with radial
// distortion -- are rendered on the host; DepthFrontEnd::registerColor brings the colour onto the depth frame, and the result is checked
// for sanity: nearly every depth pixel has a colour, close to the texture at its vertex, and the count equals the A = 255 pixels.  The
// frame is then fused with integrateColor.  With an output directory as argument, the inputs and results are written there so that
// the Python path can replay the same calls and compare the bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// inside of a box: walls x = -1.5 / 1.8, ceiling y = -1.2, floor y = 1.2, back wall z = 4; the depth camera is the world frame
static const double kNrm[5][3] = {{1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 1, 0}, {0, 0, 1}};
static const double kOff[5] = {-1.5, 1.8, -1.2, 1.2, 4.0};
static const double kTexK[3][3] = {{1.0, 5.0, 0.6}, {1.5, 0.0, 3.7}, {0.0, 2.0, 4.5}};
static const double kTexPhi[3] = {0.3, 1.2, 2.0};

static double texture(const double P[3], int c) {
  return 127.5 + 120.0 * std::sin(kTexK[c][0] * P[0] + kTexK[c][1] * P[1] + kTexK[c][2] * P[2] + kTexPhi[c]);
}

// first hit of the ray O + s D with the box, s > 0
static double hit(const double O[3], const double D[3]) {
  double best = 1e30;
  for (int p = 0; p < 5; p++) {
    const double nd = kNrm[p][0] * D[0] + kNrm[p][1] * D[1] + kNrm[p][2] * D[2];
    if (std::fabs(nd) < 1e-12) continue;
    const double s = (kOff[p] - (kNrm[p][0] * O[0] + kNrm[p][1] * O[1] + kNrm[p][2] * O[2])) / nd;
    if (s > 0 && s < best) best = s;
  }
  return best;
}

template <class T> static void dump(const std::string& dir, const char* name, const T* p, size_t n) {
  if (dir.empty()) return;
  FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
  if (!f) { std::printf("FAIL cannot write %s\n", name); fails++; return; }
  if (n) std::fwrite(p, sizeof(T), n, f);
  std::fclose(f);
}

int main(int argc, char** argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  rpe::ColorRig rig;
  rig.cam.fx = rig.cam.fy = 365.0; rig.cam.cx = 200; rig.cam.cy = 150; rig.cam.width = 400; rig.cam.height = 300;
  rig.dist[0] = -0.1;                                        // k1
  rig.T_kd.translation()[0] = -0.05;                         // the colour camera 5 cm to the right, axes parallel
  const double Ok[3] = {0.05, 0, 0}, Od[3] = {0, 0, 0};
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};

  std::vector<float> d((size_t)cam.width * cam.height);
  for (int v = 0; v < cam.height; v++)
    for (int u = 0; u < cam.width; u++) {
      const double D[3] = {(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, 1.0};
      d[(size_t)v * cam.width + u] = (float)hit(Od, D);
    }
  std::vector<uint8_t> rgb((size_t)rig.cam.width * rig.cam.height * 3);
  for (int v = 0; v < rig.cam.height; v++)
    for (int u = 0; u < rig.cam.width; u++) {
      // the ray of a distorted pixel: x <- xd / (1 + k1 r^2), iterated
      const double xd = (u - rig.cam.cx) / rig.cam.fx, yd = (v - rig.cam.cy) / rig.cam.fy;
      double x = xd, y = yd;
      for (int it = 0; it < 30; it++) { const double rad = 1.0 + rig.dist[0] * (x * x + y * y); x = xd / rad; y = yd / rad; }
      const double D[3] = {x, y, 1.0};
      const double s = hit(Ok, D);
      const double P[3] = {Ok[0] + s * D[0], Ok[1] + s * D[1], Ok[2] + s * D[2]};
      for (int ch = 0; ch < 3; ch++)
        rgb[3 * ((size_t)v * rig.cam.width + u) + ch] = (uint8_t)std::min(255.0, std::max(0.0, std::nearbyint(texture(P, ch))));
    }

  rpe::VolumeDesc vd;
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  rpe::DepthFrontEnd fe;
  fe.initVolume(vd);
  bool threw = false;
  try { fe.registerColor(rgb.data(), rig); } catch (const rpe::DeviceError&) { threw = true; }   // no frame yet
  CHECK(threw);
  fe.setDepth(d.data(), cam, range);
  CHECK(fe.registerColor(rgb.data(), rig) == -1);
  const int64_t known = fe.registerColor(rgb.data(), rig, RPE_COLOR_RGB8, true);
  const size_t n = (size_t)cam.width * cam.height;
  std::vector<uint8_t> rgba(4 * n);
  CHECK(rpe_color_download(fe.context(), RPE_COLOR_FRAME, rgba.data()) == RPE_OK);
  const rpe::MatrixX<float> V = fe.map(RPE_MAP_VERTEX);
  size_t got = 0;
  std::vector<double> err;
  for (size_t i = 0; i < n; i++) {
    if (rgba[4 * i + 3] != 255) { CHECK(rgba[4 * i] == 0 && rgba[4 * i + 1] == 0 && rgba[4 * i + 2] == 0 && rgba[4 * i + 3] == 0); continue; }
    got++;
    const double P[3] = {V(0, (int)i), V(1, (int)i), V(2, (int)i)};
    for (int c = 0; c < 3; c++) err.push_back(std::fabs(rgba[4 * i + c] - texture(P, c)));
  }
  std::nth_element(err.begin(), err.begin() + err.size() / 2, err.end());
  const double med = err.empty() ? 1e30 : err[err.size() / 2];
  std::printf("registered colour: %zu of %zu pixels, median error %.3f levels\n", got, n, med);
  CHECK((int64_t)got == known && got > 0.85 * n && med < 1.0);
  fe.integrateColor(rpe::DepthFrontEnd::Pose());
  std::vector<uint16_t> cv((size_t)vd.dim[0] * vd.dim[1] * vd.dim[2] * 4);
  CHECK(rpe_volume_color_download(fe.context(), cv.data()) == RPE_OK);
  // a bad rig is refused and the frame colour stays
  rpe::ColorRig bad = rig;
  bad.cell = 17;
  threw = false;
  try { fe.registerColor(rgb.data(), bad); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  std::vector<uint8_t> again(4 * n);
  CHECK(rpe_color_download(fe.context(), RPE_COLOR_FRAME, again.data()) == RPE_OK && again == rgba);
  dump(out, "depth.bin", d.data(), d.size());
  dump(out, "rgb.bin", rgb.data(), rgb.size());
  dump(out, "rgba.bin", rgba.data(), rgba.size());
  dump(out, "color_volume.bin", cv.data(), cv.size());
  if (fails) { std::printf("register_color: %d failures\n", fails); return 1; }
  std::printf("register_color: ok\n");
  return 0;
}
