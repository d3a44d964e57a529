// The map rebuilt after a loop closure, through the C++ front end (compiled by tests/test_rebuild_oracle.py, run by
// tests/test_gpu_rebuild.py): the textured wall of graph_optimize.cpp seen from three keyframe poses whose tracker had drifted.  Each
// keyframe keeps its depth and colour (attachFrame).  Fused at the drifted poses the wall comes out bent; after linkKeyframes +
// optimizeKeyframes, fuseKeyframes rebuilds the volume at the corrected poses in one launch -- the same bits as initVolume and one
// integrateColor per keyframe -- and the mesh of it lies on the wall.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static const double kWallZ = 3.0, kCell = 0.12;

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

// d followed after p: Xc = Rd (R Xw + t) + td, Rd a roll by `a`
static void drifted(const double p[12], double a, double x, double y, double z, double out[12]) {
  const double c = std::cos(a), s = std::sin(a), Rd[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, td[3] = {x, y, z};
  for (int r = 0; r < 3; r++) {
    for (int q = 0; q < 3; q++) out[3 * r + q] = Rd[3 * r] * p[q] + Rd[3 * r + 1] * p[3 + q] + Rd[3 * r + 2] * p[6 + q];
    out[9 + r] = Rd[3 * r] * p[9] + Rd[3 * r + 1] * p[10] + Rd[3 * r + 2] * p[11] + td[r];
  }
}

// mean and largest distance of the mesh's vertices from the wall
static void wall_error(const rpe::Mesh& m, double* mean, double* worst) {
  *mean = *worst = 0;
  for (int v = 0; v < m.vertices.cols(); v++) {
    const double e = std::fabs((double)m.vertices(2, v) - kWallZ);
    *mean += e; *worst = std::max(*worst, e);
  }
  if (m.vertices.cols() > 0) *mean /= m.vertices.cols();
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
    drifted(p, 0.02 * i, 0.05 * i, -0.03 * i, 0.02 * i, DR[i]);               // ... and the tracker's pose further off each time
  }
  rpe::VolumeDesc desc;                                                        // 7.0 x 3.2 x 0.8 m around the wall, 4 cm voxels
  desc.dim[0] = 175; desc.dim[1] = 80; desc.dim[2] = 20;
  desc.voxel_size = 0.04; desc.trunc = 0.12; desc.max_weight = 64;
  desc.origin[0] = -2.0; desc.origin[1] = -1.6; desc.origin[2] = 2.6;
  std::vector<std::vector<float> > depth(K);
  std::vector<std::vector<uint8_t> > rgb(K);
  try {
    rpe::DepthFrontEnd fe;
    for (int i = 0; i < K; i++) {
      render(KF[i], k, 1u + i, depth[i], rgb[i]);
      fe.setDepth(depth[i].data(), k, range);
      fe.setColor(rgb[i].data());
      fe.setModelFromFrame(rpe::DepthFrontEnd::pose_of(DR[i]));
      fe.modelColorFromFrame();
      fe.detectFeatures(RPE_FEAT_MODEL);
      const int id = fe.addKeyframe();
      CHECK(!fe.keyframeAttachment(id).depth);
      fe.attachFrame(id);                                                      // the keyframe keeps its depth and colour
      fe.linkKeyframes(id);
    }
    const rpe::KeyframeAttachment a = fe.keyframeAttachment(1);
    CHECK(a.depth && a.color && a.cam.width == k.width && a.cam.height == k.height && a.z.size() == depth[1].size());
    size_t valid = 0, other = 0;                                                // a valid pixel's z is the metric depth it was given
    for (size_t i = 0; i < a.z.size(); i++) if (a.z[i] == a.z[i]) { valid++; other += a.z[i] != depth[1][i]; }
    CHECK(valid > a.z.size() / 2 && other == 0);

    bool threw = false;                                                        // no volume yet
    try { fe.fuseKeyframes(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);

    // the map as the drifted tracker made it
    fe.initVolume(desc);
    fe.fuseKeyframes({}, {}, true, true);
    double mean0 = 0, worst0 = 0, mean1 = 0, worst1 = 0;
    const rpe::Mesh bent = fe.mesh();
    wall_error(bent, &mean0, &worst0);

    const std::vector<double> gates = {0.3, 0.15, 0.1, 0.05, 0.05, 0.05};
    const rpe::GraphResult g = fe.optimizeKeyframes(gates);
    CHECK(g.ok);
    fe.fuseKeyframes({}, {}, true, true);                                      // ... and rebuilt at the corrected poses
    const rpe::MatrixX<float> rebuilt = fe.volume();
    const rpe::Mesh flat = fe.mesh();
    wall_error(flat, &mean1, &worst1);
    const std::vector<uint8_t> colors = fe.meshColors();
    std::printf("mesh at the drifted poses: %d vertices, %.4f m mean / %.4f m worst from the wall; rebuilt: %d vertices, %.4f / %.4f\n",
                (int)bent.vertices.cols(), mean0, worst0, (int)flat.vertices.cols(), mean1, worst1);
    CHECK(bent.vertices.cols() > 1000 && flat.vertices.cols() > 1000 && colors.size() == (size_t)4 * flat.vertices.cols());
    CHECK(mean1 < 0.01 && 3 * mean1 < mean0);

    // the same bits as the frame-by-frame route at the poses the store now holds
    fe.initVolume(desc);
    for (int i = 0; i < K; i++) {
      fe.setDepth(depth[i].data(), k, range);
      fe.setColor(rgb[i].data());
      fe.integrateColor(fe.keyframePose(i));
    }
    const rpe::MatrixX<float> sequential = fe.volume();
    CHECK(rebuilt.cols() == sequential.cols() && std::memcmp(rebuilt.data(), sequential.data(), sizeof(float) * 2 * (size_t)rebuilt.cols()) == 0);

    fe.clearKeyframes();                                                       // the attachments go with the store
    threw = false;
    try { fe.fuseKeyframes(); } catch (const rpe::DeviceError& e) { threw = e.code == RPE_ERR_STATE; }
    CHECK(threw);
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    fails++;
  }
  std::printf(fails ? "volume_rebuild: %d failure(s)\n" : "volume_rebuild: ok\n", fails);
  return fails ? 1 : 0;
}
