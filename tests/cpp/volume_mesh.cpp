// Mesh extraction through the C++ front end (compiled by tests/test_mesh_oracle.py, run by tests/test_gpu_mesh.py): depth frames of a
// box room rendered on the host are fused by DepthFrontEnd::integrate, DepthFrontEnd::mesh extracts the surface, and the mesh is
// checked for sanity: ids in range, the vertices on the walls, faces wound towards the camera side, the vertex normals agreeing with
// the faces; the volume uploaded back gives the same mesh; a bad min_weight throws.
#include <cmath>
#include <cstdio>
#include <vector>
#include "DepthFrontEnd.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// inside of a box: walls x = -1.5 / 1.8, ceiling y = -1.2, floor y = 1.2, back wall z = 4; camera Xc = R Xw + t
static const double kNrm[5][3] = {{1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 1, 0}, {0, 0, 1}};
static const double kOff[5] = {-1.5, 1.8, -1.2, 1.2, 4.0};

static std::vector<float> render(const double R[9], const double t[3], const rpe::PinholeCamera& k) {
  double O[3];
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  std::vector<float> d((size_t)k.width * k.height);
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
      d[(size_t)v * k.width + u] = (float)best;
    }
  return d;
}

int main() {
  rpe::PinholeCamera cam;
  cam.fx = cam.fy = 292.5; cam.cx = 160; cam.cy = 120; cam.width = 320; cam.height = 240;
  const rpe::DepthRange range{1.0, 0.1, 10.0, 0.1};
  rpe::VolumeDesc vd;   // the box [-1.5, 1.8] x [-1.2, 1.2] x [.., 4] with a margin, 4 cm voxels
  vd.dim[0] = 90; vd.dim[1] = 72; vd.dim[2] = 120; vd.voxel_size = 0.04; vd.trunc = 0.12;
  vd.origin[0] = -1.7; vd.origin[1] = -1.4; vd.origin[2] = -0.5;
  rpe::DepthFrontEnd fe;
  fe.initVolume(vd);
  for (int f = 0; f < 3; f++) {
    const double a = 0.05 * f, ca = std::cos(a), sa = std::sin(a);
    const double p[12] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca, 0.05 * f, 0, 0};
    const std::vector<float> d = render(p, p + 9, cam);
    fe.setDepth(d.data(), cam, range);
    fe.integrate(rpe::DepthFrontEnd::pose_of(p));
  }
  const rpe::Mesh m = fe.mesh();
  const int nv = m.vertices.cols();
  const long long nt = (long long)m.triangles.size() / 3;
  std::printf("mesh: %d vertices, %lld triangles\n", nv, nt);
  CHECK(nv > 10000 && nt > 20000 && m.normals.cols() == nv && (long long)m.triangles.size() == 3 * nt);
  bool ids_ok = true;
  for (int32_t id : m.triangles) ids_ok = ids_ok && id >= 0 && id < nv;
  CHECK(ids_ok);
  // the vertices lie on the walls: within a voxel of the nearest one
  int on_wall = 0;
  for (int i = 0; i < nv; i++) {
    double best = 1e30;
    for (int p = 0; p < 5; p++)
      best = std::fmin(best, std::fabs(kNrm[p][0] * m.vertices(0, i) + kNrm[p][1] * m.vertices(1, i) + kNrm[p][2] * m.vertices(2, i) - kOff[p]));
    on_wall += best < 0.04 ? 1 : 0;
  }
  std::printf("mesh: %d of %d vertices within a voxel of a wall\n", on_wall, nv);
  CHECK(on_wall > 0.99 * nv);
  // faces point to the free side (into the room, where the camera is) and agree with the vertex normals there
  long long inward = 0, agree = 0, with_normal = 0;
  for (long long t = 0; t < nt; t++) {
    const int32_t* v = &m.triangles[3 * t];
    double e1[3], e2[3], c[3], n[3];
    for (int a = 0; a < 3; a++) {
      e1[a] = m.vertices(a, v[1]) - m.vertices(a, v[0]);
      e2[a] = m.vertices(a, v[2]) - m.vertices(a, v[0]);
      c[a] = (m.vertices(a, v[0]) + m.vertices(a, v[1]) + m.vertices(a, v[2])) / 3;
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    inward += (n[0] * (0.1 - c[0]) + n[1] * (0.0 - c[1]) + n[2] * (1.0 - c[2])) > 0 ? 1 : 0;   // (0.1, 0, 1): inside the room
    const double dn = n[0] * m.normals(0, v[0]) + n[1] * m.normals(1, v[0]) + n[2] * m.normals(2, v[0]);
    if (!std::isnan(dn)) { with_normal++; agree += dn > 0 ? 1 : 0; }
  }
  std::printf("mesh: %lld of %lld faces towards the room, %lld of %lld agree with their vertex normal\n", inward, nt, agree, with_normal);
  CHECK(inward > 0.99 * nt && with_normal > 0.5 * nt && agree > 0.99 * with_normal);
  // the volume uploaded back (after a re-init) gives the same mesh bits
  const rpe::MatrixX<float> vol = fe.volume();
  fe.initVolume(vd);
  fe.uploadVolume(vol);
  const rpe::Mesh m2 = fe.mesh();
  bool same = m2.vertices.cols() == nv && m2.triangles == m.triangles;
  for (int i = 0; same && i < 3 * nv; i++) same = m2.vertices.data()[i] == m.vertices.data()[i];
  CHECK(same);
  bool threw = false;
  try { (void)fe.mesh(0.0); } catch (const rpe::DeviceError&) { threw = true; }
  CHECK(threw);
  if (fails) { std::printf("volume_mesh: %d failures\n", fails); return 1; }
  std::printf("volume_mesh: ok\n");
  return 0;
}
