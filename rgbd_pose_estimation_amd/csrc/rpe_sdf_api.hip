// Part 3 of include/rgbd_pose_hip.h: the volume term (kernels in rpe_frontend.hip, rule in rpe_sdf_rule.hpp).  A frame tracked against
// the TSDF volume itself: per-pixel rows, the normal equations of one level, and the loops -- per round ONE launch, one host wait, the
// host solve and left update of rpe_icp.  Reads the frame's maps and the volume; the model, the solver slots and the prepared
// photometric maps are neither read nor replaced.
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

namespace {
// one level of what a round reads: frame vertex / normal, pixels
struct SdfLevel { const float *fv, *fn; int64_t n; };
SdfLevel sdf_level(rpe_context* c, int l) {
  auto& F = c->fe;
  SdfLevel L;
  L.fv = F.fmap[0] + 3 * F.fgeo.off[l]; L.fn = F.fmap[1] + 3 * F.fgeo.off[l];
  L.n = (int64_t)F.fgeo.cam[l].width * F.fgeo.cam[l].height;
  return L;
}
int sdf_ready(rpe_context* c, int levels, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!c->fe.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (c->fe.fgeo.levels < levels)
    return fail(RPE_ERR_STATE, "%s: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)", who, c->fe.fgeo.levels, levels);
  return RPE_OK;
}
// one round: launch, wait, the 32-double record (H | g | sum r^2 | rows | pivot floor)
int sdf_round(rpe_context* c, const SdfLevel& lv, double dist_thr, double cos_thr, int use_normals, const double* pose12, double* ne) {
  HIP_TRY(rpe::launch_icp_sdf(lv.fv, lv.fn, lv.n, c->vol.d, c->vol.g, (float)dist_thr, (float)cos_thr, use_normals, pose12,
                              collect_target(c), c->stream));
  int rc = wait_host(c, rpe::kNeLd);
  if (rc) return rc;
  for (int i = 0; i < 32; i++) ne[i] = i < 29 ? c->h_out[i] : 0.0;
  ne[29] = rpe::pivot_floor(false);   // the rows' products are fp32
  return RPE_OK;
}
// rpe_icp's host rounds on one level
int sdf_rounds(rpe_context* c, const rpe_icp_options* o, int l, int max_iter, double dist_thr, double* pose12, int* iters_out,
               double* last_step, double* final_cost, int64_t* matched) {
  const SdfLevel lv = sdf_level(c, l);
  int it = 0, rc;
  double step = 0, cost = 0, rows = 0;
  for (; it < max_iter; it++) {
    double ne[32], d[6];
    if ((rc = sdf_round(c, lv, dist_thr, o->cos_thr, o->use_normals, pose12, ne))) return rc;
    cost = ne[27]; rows = ne[28];
    if (!rpe::solve_normal_eq6(ne, d, rpe::pivot_floor(false))) {
      if (iters_out) *iters_out = it;
      return fail(RPE_ERR_DEGENERATE, "volume term: normal equations are not positive definite at iteration %d (%g rows)", it, rows);
    }
    rpe::se3_left_update(d, pose12);
    step = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    if (step < o->tol) { it++; break; }
  }
  if (iters_out) *iters_out = it;
  if (last_step) *last_step = step;
  if (final_cost) *final_cost = cost;
  if (matched) *matched = (int64_t)rows;
  return RPE_OK;
}
int sdf_options(const rpe_icp_options* o, const double* pose12, const char* who) {
  if (!o || !pose12 || !(o->dist_thr >= 0)) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if (o->device_resident) return fail(RPE_ERR_ARG, "%s: host-driven only (device_resident must be 0)", who);
  return RPE_OK;
}
}  // namespace

extern "C" {

int rpe_sdf_rows(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, float* rows) {
  session_end(c);
  if (!c || !pose12 || !rows || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0))
    return fail(RPE_ERR_ARG, "rpe_sdf_rows: bad argument (level 0 .. %d, dist_thr >= 0)", RPE_MAX_LEVELS - 1);
  int rc = sdf_ready(c, level + 1, "rpe_sdf_rows");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const SdfLevel lv = sdf_level(c, level);
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, (size_t)lv.n * 7 * sizeof(float)))) return rc;
  hipError_t e = rpe::launch_sdf_rows(lv.fv, lv.fn, lv.n, c->vol.d, c->vol.g, (float)dist_thr, (float)cos_thr, use_normals != 0, pose12,
                                      d_rows, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, d_rows, (size_t)lv.n * 7 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "rpe_sdf_rows: %s", hipGetErrorString(e));
  return RPE_OK;
}

int rpe_sdf_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, double* out32) {
  session_end(c);
  if (!c || !pose12 || !out32 || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0))
    return fail(RPE_ERR_ARG, "rpe_sdf_normal_eq: bad argument (level 0 .. %d, dist_thr >= 0)", RPE_MAX_LEVELS - 1);
  int rc = sdf_ready(c, level + 1, "rpe_sdf_normal_eq");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return sdf_round(c, sdf_level(c, level), dist_thr, cos_thr, use_normals != 0, pose12, out32);
}

int rpe_icp_sdf(rpe_context* c, const rpe_icp_options* o, double* pose12, int* iters_out, double* last_step, double* final_cost,
                int64_t* matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = sdf_options(o, pose12, "rpe_icp_sdf");
  if (rc) return rc;
  if (o->max_iter < 1) return fail(RPE_ERR_ARG, "rpe_icp_sdf: max_iter >= 1");
  if ((rc = sdf_ready(c, 1, "rpe_icp_sdf"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return sdf_rounds(c, o, 0, o->max_iter, o->dist_thr, pose12, iters_out, last_step, final_cost, matched);
}

int rpe_icp_pyramid_sdf(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level, const double* dist_thr_per_level,
                        double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = sdf_options(o, pose12, "rpe_icp_pyramid_sdf");
  if (rc) return rc;
  if (!iters_per_level || levels < 1 || levels > RPE_MAX_LEVELS)
    return fail(RPE_ERR_ARG, "rpe_icp_pyramid_sdf: levels must be 1 .. %d (got %d)", RPE_MAX_LEVELS, levels);
  for (int l = 0; l < levels; l++) {
    if (iters_per_level[l] < (l == 0 ? 1 : 0))
      return fail(RPE_ERR_ARG, "rpe_icp_pyramid_sdf: level %d needs %s rounds (got %d)", l, l == 0 ? ">= 1" : ">= 0", iters_per_level[l]);
    if (dist_thr_per_level && !(dist_thr_per_level[l] >= 0))
      return fail(RPE_ERR_ARG, "rpe_icp_pyramid_sdf: bad distance gate at level %d", l);
  }
  if ((rc = sdf_ready(c, levels, "rpe_icp_pyramid_sdf"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  for (int l = levels - 1; l >= 0; l--) {
    int it = 0;
    const bool fine = l == 0;
    if (iters_per_level[l] > 0)
      rc = sdf_rounds(c, o, l, iters_per_level[l], dist_thr_per_level ? dist_thr_per_level[l] : o->dist_thr, pose12, &it,
                      fine ? last_step : nullptr, fine ? final_cost : nullptr, fine ? matched : nullptr);
    if (iters_out) iters_out[l] = it;
    if (rc) return rc;
  }
  return RPE_OK;
}

}  // extern "C"
