// Part 3 of include/rgbd_pose_hip.h: the mesh of the TSDF volume (kernels in rpe_mesh.hip).  Marching cubes over the context's volume
// into device buffers the context owns: three launches, one host wait for the totals, two launches; the download copies them out.
// rpe_volume_mesh_box is the same extraction over the cubes of a box only (the whole volume is still swept).
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

namespace {

// lo / hi = nullptr: every cube (rpe_volume_mesh)
int mesh_of_box(rpe_context* c, const char* who, double min_weight, const int32_t* lo, const int32_t* hi, bool boxed, int64_t* n_vertices,
                int64_t* n_triangles) {
  session_end(c);
  if (c) c->vol.have_mesh = c->vol.mesh_is_map = false;   // the last mesh lives until this call, whatever it returns
  if (!c || !n_vertices || !n_triangles || (boxed && (!lo || !hi))) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  const float wmin = (float)min_weight;
  if (!(min_weight > 0) || !std::isfinite(min_weight) || !(wmin > 0))
    return fail(RPE_ERR_ARG, "%s: min_weight must be finite and > 0, also in fp32 (got %g)", who, min_weight);
  rpe::MeshBox B;
  for (int a = 0; a < 3; a++) {
    B.lo[a] = boxed ? lo[a] : 0; B.hi[a] = boxed ? hi[a] : V.g.dim[a] - 1;
    if (B.lo[a] < 0 || B.lo[a] > B.hi[a] || B.hi[a] > V.g.dim[a] - 1)
      return fail(RPE_ERR_ARG, "%s: need 0 <= lo[%d] <= hi[%d] <= dim - 1 = %d (got %d, %d)", who, a, a, V.g.dim[a] - 1, B.lo[a], B.hi[a]);
  }
  HIP_TRY(hipSetDevice(c->device));
  const int64_t nvox = (int64_t)V.g.dim[0] * V.g.dim[1] * V.g.dim[2];
  const size_t ws = rpe::mesh_workspace_bytes(nvox);
  int rc;
  if ((rc = V.ws.reserve(c, ws))) return rc;
  const rpe::MeshWorkspace W = rpe::mesh_workspace(V.ws, nvox);
  HIP_TRY(rpe::launch_mesh_count(V.d, V.g, wmin, B, W, c->stream));
  long long tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, W.totals, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (tot[0] >= ((long long)1 << 31))
    return fail(RPE_ERR_ARG, "%s: %lld vertices; the int32 triangle ids hold fewer than 2^31", who, tot[0]);
  const size_t vb = (size_t)tot[0] * 3 * sizeof(float), tb = (size_t)tot[1] * 3 * sizeof(int32_t);
  if (vb && ((rc = V.mv.reserve(c, vb)) || (rc = V.mn.reserve(c, vb)))) return rc;   // (an empty mesh asks for nothing)
  if (tb && (rc = V.mt.reserve(c, tb))) return rc;
  if (tot[0] > 0) HIP_TRY(rpe::launch_mesh_emit(V.d, V.g, W, V.mv, V.mn, V.mt, c->stream));
  V.nv = tot[0]; V.nt = tot[1];
  V.have_mesh = true;
  *n_vertices = V.nv; *n_triangles = V.nt;
  return RPE_OK;
}

}  // namespace

extern "C" {

int rpe_volume_mesh(rpe_context* c, double min_weight, int64_t* n_vertices, int64_t* n_triangles) {
  return mesh_of_box(c, "rpe_volume_mesh", min_weight, nullptr, nullptr, false, n_vertices, n_triangles);
}

int rpe_volume_mesh_box(rpe_context* c, double min_weight, const int32_t lo[3], const int32_t hi[3], int64_t* n_vertices,
                        int64_t* n_triangles) {
  return mesh_of_box(c, "rpe_volume_mesh_box", min_weight, lo, hi, true, n_vertices, n_triangles);
}

int rpe_volume_mesh_download(rpe_context* c, float* vertices, float* normals, int32_t* triangles) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_mesh_download: bad argument");
  const auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!V.have_mesh) return fail(RPE_ERR_STATE, "no mesh: call rpe_volume_mesh first (rpe_volume_init drops the mesh)");
  if ((V.nv > 0 && !vertices) || (V.nt > 0 && !triangles)) return fail(RPE_ERR_ARG, "rpe_volume_mesh_download: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  const size_t vb = (size_t)V.nv * 3 * sizeof(float), tb = (size_t)V.nt * 3 * sizeof(int32_t);
  if (vb) HIP_TRY(hipMemcpyAsync(vertices, V.mv, vb, hipMemcpyDeviceToHost, c->stream));
  if (vb && normals) HIP_TRY(hipMemcpyAsync(normals, V.mn, vb, hipMemcpyDeviceToHost, c->stream));
  if (tb) HIP_TRY(hipMemcpyAsync(triangles, V.mt, tb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

}  // extern "C"
