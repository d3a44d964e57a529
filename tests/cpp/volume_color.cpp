// Colour through the C++ front end (compiled by tests/test_color_oracle.py, run by tests/test_gpu_color.py): depth and colour frames of
// a textured box room rendered on the host are fused by DepthFrontEnd::setColor / integrateColor, the model colour of a raycast and the
// colours of the mesh are taken out, and checked for sanity: most hits and vertices have a known colour close to the texture there, and
// the mesh has one colour per vertex.  Frame 1 is passed in BGR order.  With an output directory as argument, the frames, poses and
// results are written there so that the Python path can replay the same calls and compare the bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// inside of a box: walls x = -1.5 / 1.8, ceiling y = -1.2, floor y = 1.2, back wall z = 4; camera Xc = R Xw + t
static const double kNrm[5][3] = {{1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 1, 0}, {0, 0, 1}};
static const double kOff[5] = {-1.5, 1.8, -1.2, 1.2, 4.0};
// texture: channel c = 127.5 + 120 sin(k_c . P + phi_c), wavelengths of about 1.3 m
static const double kTexK[3][3] = {{1.0, 5.0, 0.6}, {1.5, 0.0, 3.7}, {0.0, 2.0, 4.5}};
static const double kTexPhi[3] = {0.3, 1.2, 2.0};

static double texture(const double P[3], int c) {
  return 127.5 + 120.0 * std::sin(kTexK[c][0] * P[0] + kTexK[c][1] * P[1] + kTexK[c][2] * P[2] + kTexPhi[c]);
}

static void render(const double R[9], const double t[3], const rpe::PinholeCamera& k, std::vector<float>& d, std::vector<uint8_t>& rgb) {
  double O[3];
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  d.assign((size_t)k.width * k.height, 0.f);
  rgb.assign((size_t)k.width * k.height * 3, 0);
  for (int v = 0; v < k.height; v++)
    for (int u = 0; u < k.width; u++) {
      const double c[3] = {(u - k.cx) / k.fx, (v - k.cy) / k.fy, 1.0};
      double D[3];
      for (int i = 0; i < 3; i++) D[i] = R[i] * c[0] + R[3 + i] * c[1] + R[6 + i] * c[2];
      double best = 1e30;
      for (int p = 0; p < 5; p++) {
        const double nd = kNrm[p][0] * D[0] + kNrm[p][1] * D[1] + kNrm[p][2] * D[2];
        if (std::fabs(nd) < 1e-12) continue;
        const double s = (kOff[p] - (kNrm[p][0] * O[0] + kNrm[p][1] * O[1] + kNrm[p][2] * O[2])) / nd;
        if (s > 0 && s < best) best = s;
      }
      const size_t i = (size_t)v * k.width + u;
      d[i] = (float)best;
      const double P[3] = {O[0] + best * D[0], O[1] + best * D[1], O[2] + best * D[2]};
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

// median of |colour - texture at the point| over the known colours (A = 255), and how many are known
static double colour_error(const std::vector<uint8_t>& rgba, const float* pts, size_t n, size_t* known) {
  std::vector<double> err;
  for (size_t i = 0; i < n; i++) {
    if (rgba[4 * i + 3] != 255) continue;
    const double P[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    for (int c = 0; c < 3; c++) err.push_back(std::fabs(rgba[4 * i + c] - texture(P, c)));
  }
  *known = err.size() / 3;
  if (err.empty()) return 1e30;
  std::nth_element(err.begin(), err.begin() + err.size() / 2, err.end());
  return err[err.size() / 2];
}

int main(int argc, char** argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc vd;   // the box [-1.5, 1.8] x [-1.2, 1.2] x [.., 4] with a margin, 4 cm voxels
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  rpe::DepthFrontEnd fe;
  fe.initVolume(vd);
  bool threw = false;
  try { fe.integrateColor(rpe::DepthFrontEnd::Pose()); } catch (const rpe::DeviceError&) { threw = true; }   // no frame yet
  CHECK(threw);
  double poses[3][12];
  std::vector<float> d;
  std::vector<uint8_t> rgb;
  for (int f = 0; f < 3; f++) {
    const double a = 0.05 * f, ca = std::cos(a), sa = std::sin(a);
    const double p[12] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca, 0.05 * f, 0, 0};
    std::copy(p, p + 12, poses[f]);
    render(p, p + 9, cam, d, rgb);
    const std::string tag = std::to_string(f);
    dump(out, ("depth" + tag + ".bin").c_str(), d.data(), d.size());
    dump(out, ("rgb" + tag + ".bin").c_str(), rgb.data(), rgb.size());
    fe.setDepth(d.data(), cam, range);
    if (f == 1) {
      for (size_t i = 0; i < rgb.size(); i += 3) std::swap(rgb[i], rgb[i + 2]);
      fe.setColor(rgb.data(), RPE_COLOR_BGR8);
    } else {
      fe.setColor(rgb.data());
    }
    fe.integrateColor(rpe::DepthFrontEnd::pose_of(p));
  }
  dump(out, "poses.bin", &poses[0][0], 36);
  fe.raycast(rpe::DepthFrontEnd::pose_of(poses[1]), cam, range);
  const std::vector<uint8_t> mc = fe.modelColor();
  const rpe::MatrixX<float> mv = fe.map(RPE_MAP_MODEL_VERTEX);
  size_t hits = 0, known = 0;
  for (int i = 0; i < mv.cols(); i++) hits += std::isnan(mv(0, i)) ? 0 : 1;
  const double med = colour_error(mc, mv.data(), (size_t)mv.cols(), &known);
  std::printf("model colour: %zu of %zu hits known, median error %.3f levels\n", known, hits, med);
  CHECK(mc.size() == (size_t)cam.width * cam.height * 4 && hits > 0.9 * mv.cols() && known > 0.9 * hits && med < 2.0);
  const rpe::Mesh m = fe.mesh();
  const std::vector<uint8_t> vc = fe.meshColors();
  size_t vknown = 0;
  const double vmed = colour_error(vc, m.vertices.data(), (size_t)m.vertices.cols(), &vknown);
  std::printf("mesh colours: %zu of %d vertices known, median error %.3f levels\n", vknown, (int)m.vertices.cols(), vmed);
  CHECK(vc.size() == (size_t)m.vertices.cols() * 4 && m.vertices.cols() > 10000 && vknown > 0.9 * m.vertices.cols() && vmed < 2.0);
  std::vector<uint16_t> cv((size_t)vd.dim[0] * vd.dim[1] * vd.dim[2] * 4);
  CHECK(rpe_volume_color_download(fe.context(), cv.data()) == RPE_OK);
  dump(out, "model_color.bin", mc.data(), mc.size());
  dump(out, "mesh_vertices.bin", m.vertices.data(), (size_t)m.vertices.cols() * 3);
  dump(out, "mesh_colors.bin", vc.data(), vc.size());
  dump(out, "color_volume.bin", cv.data(), cv.size());
  // a new depth drops the frame colour
  fe.setDepth(d.data(), cam, range);
  threw = false;
  try { fe.integrateColor(rpe::DepthFrontEnd::pose_of(poses[2])); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  if (fails) { std::printf("volume_color: %d failures\n", fails); return 1; }
  std::printf("volume_color: ok\n");
  return 0;
}
