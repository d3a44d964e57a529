// Part 3 of include/rgbd_pose_hip.h: the volume term (kernels in rpe_frontend.hip, rule in rpe_sdf_rule.hpp).  A frame tracked against
// the TSDF volume itself: per-pixel rows, the normal equations of one level, and the loops -- per round ONE launch, one host wait, the
// host solve and left update of rpe_icp.  Reads the frame's maps and the volume; the model, the solver slots and the prepared
// photometric maps are neither read nor replaced.  The MAP form of each call reads the virtual volume of a box of the map -- the window
// plus the archived bricks -- through the brick grid of the map raycast (rpe_mapmesh_api.hip builds it): the grid is built and
// uploaded once per call, into the volume's map list, and every round of the call reads it.
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

namespace {
int sdf_ready(rpe_context* c, int levels, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!c->fe.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (c->fe.fgeo.levels < levels)
    return fail(RPE_ERR_STATE, "%s: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)", who, c->fe.fgeo.levels, levels);
  return RPE_OK;
}
// where a call reads the field: the dense window (map = false), or the virtual volume g of a box of the map through the grid of M
struct Field { bool map = false; rpe::VolumeGeometry g; rpe::MapRayView M{}; };
Field window_field(rpe_context* c) {
  Field f;
  f.g = c->vol.g;
  return f;
}
// the map's field inside the box (rpe_frontend_host.hpp map_field, in rpe_mapmesh_api.hip: rules, grid, upload)
int map_field(rpe_context* c, const char* who, const int64_t* lo, const int64_t* hi, Field& f) {
  const int rc = rpeh::map_field(c, who, lo, hi, f.g, f.M);
  f.map = rc == RPE_OK;
  return rc;
}
// one round: launch, wait, the 32-double record (H | g | sum r^2 | rows | pivot floor)
int sdf_round(rpe_context* c, const Field& f, const Level& lv, double dist_thr, double cos_thr, int use_normals, const double* pose12,
              double* ne) {
  if (f.map)
    HIP_TRY(rpe::launch_icp_map_sdf(lv.f[0], lv.f[1], lv.n, f.M, f.g, (float)dist_thr, (float)cos_thr, use_normals, pose12,
                                    collect_target(c), c->stream));
  else
    HIP_TRY(rpe::launch_icp_sdf(lv.f[0], lv.f[1], lv.n, c->vol.d, f.g, (float)dist_thr, (float)cos_thr, use_normals, pose12,
                                collect_target(c), c->stream));
  int rc = wait_host(c, rpe::kNeLd);
  if (rc) return rc;
  for (int i = 0; i < 32; i++) ne[i] = i < 29 ? c->h_out[i] : 0.0;
  ne[29] = rpe::pivot_floor(false);   // the rows' products are fp32
  return RPE_OK;
}
// rpe_icp's host rounds on one level
int sdf_rounds(rpe_context* c, const Field& f, const rpe_icp_options* o, int l, int max_iter, double dist_thr, double* pose12, int* iters_out,
               double* last_step, double* final_cost, int64_t* matched) {
  const Level lv = level_of(c, l);   // the frame's side only
  GnRun run;   // run.weight: the rows
  const int rc = gn_host_rounds([&](const double* pose, double* ne) { return sdf_round(c, f, lv, dist_thr, o->cos_thr, o->use_normals, pose, ne); },
                                rpe::pivot_floor(false), 1.0, max_iter, o->tol, pose12, &run);
  if (rc == kGnRefused) {
    if (iters_out) *iters_out = run.it;
    return fail(RPE_ERR_DEGENERATE, "volume term: normal equations are not positive definite at iteration %d (%g rows)", run.it, run.weight);
  }
  if (rc) return rc;
  run.report(iters_out, last_step, final_cost, matched);
  return RPE_OK;
}
int sdf_options(const rpe_icp_options* o, const double* pose12, const char* who) {
  if (!o || !pose12 || !(o->dist_thr >= 0)) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if (o->device_resident) return fail(RPE_ERR_ARG, "%s: host-driven only (device_resident must be 0)", who);
  return RPE_OK;
}

// ---- the four calls, on the window (box = false) or on a box of the map
int rows_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, int level, const double* pose12, double dist_thr,
              double cos_thr, int use_normals, float* rows) {
  session_end(c);
  if (!c || !pose12 || !rows || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", who, RPE_MAX_LEVELS - 1);
  int rc = sdf_ready(c, level + 1, who);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  Field f = window_field(c);
  if (box && (rc = map_field(c, who, lo, hi, f))) return rc;
  const Level lv = level_of(c, level);
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, (size_t)lv.n * 7 * sizeof(float)))) return rc;
  hipError_t e = f.map ? rpe::launch_map_sdf_rows(lv.f[0], lv.f[1], lv.n, f.M, f.g, (float)dist_thr, (float)cos_thr, use_normals != 0, pose12,
                                                  d_rows, c->stream)
                       : rpe::launch_sdf_rows(lv.f[0], lv.f[1], lv.n, c->vol.d, f.g, (float)dist_thr, (float)cos_thr, use_normals != 0, pose12,
                                              d_rows, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, d_rows, (size_t)lv.n * 7 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return RPE_OK;
}

int normal_eq_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, int level, const double* pose12,
                   double dist_thr, double cos_thr, int use_normals, double* out32) {
  session_end(c);
  if (!c || !pose12 || !out32 || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", who, RPE_MAX_LEVELS - 1);
  int rc = sdf_ready(c, level + 1, who);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  Field f = window_field(c);
  if (box && (rc = map_field(c, who, lo, hi, f))) return rc;
  return sdf_round(c, f, level_of(c, level), dist_thr, cos_thr, use_normals != 0, pose12, out32);
}

int icp_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, double* pose12,
             int* iters_out, double* last_step, double* final_cost, int64_t* matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = sdf_options(o, pose12, who);
  if (rc) return rc;
  if (o->max_iter < 1) return fail(RPE_ERR_ARG, "%s: max_iter >= 1", who);
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if ((rc = sdf_ready(c, 1, who))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  Field f = window_field(c);
  if (box && (rc = map_field(c, who, lo, hi, f))) return rc;
  return sdf_rounds(c, f, o, 0, o->max_iter, o->dist_thr, pose12, iters_out, last_step, final_cost, matched);
}

int pyramid_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, int levels,
                 const int* iters_per_level, const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step,
                 double* final_cost, int64_t* matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = sdf_options(o, pose12, who);
  if (rc) return rc;
  if ((rc = pyramid_complaint(who, levels, iters_per_level, dist_thr_per_level))) return rc;
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if ((rc = sdf_ready(c, levels, who))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  Field f = window_field(c);
  if (box && (rc = map_field(c, who, lo, hi, f))) return rc;
  return coarse_to_fine(levels, iters_per_level, dist_thr_per_level, o->dist_thr, iters_out,
                        [&](int l, int rounds, double gate, bool fine, int* it) {
    return sdf_rounds(c, f, o, l, rounds, gate, pose12, it, fine ? last_step : nullptr, fine ? final_cost : nullptr, fine ? matched : nullptr);
  });
}
}  // namespace

extern "C" {

int rpe_sdf_rows(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, float* rows) {
  return rows_call(c, "rpe_sdf_rows", false, nullptr, nullptr, level, pose12, dist_thr, cos_thr, use_normals, rows);
}
int rpe_sdf_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, double* out32) {
  return normal_eq_call(c, "rpe_sdf_normal_eq", false, nullptr, nullptr, level, pose12, dist_thr, cos_thr, use_normals, out32);
}
int rpe_icp_sdf(rpe_context* c, const rpe_icp_options* o, double* pose12, int* iters_out, double* last_step, double* final_cost,
                int64_t* matched) {
  return icp_call(c, "rpe_icp_sdf", false, nullptr, nullptr, o, pose12, iters_out, last_step, final_cost, matched);
}
int rpe_icp_pyramid_sdf(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level, const double* dist_thr_per_level,
                        double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched) {
  return pyramid_call(c, "rpe_icp_pyramid_sdf", false, nullptr, nullptr, o, levels, iters_per_level, dist_thr_per_level, pose12, iters_out,
                      last_step, final_cost, matched);
}

int rpe_map_sdf_rows(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, const int64_t lo[3],
                     const int64_t hi[3], float* rows) {
  return rows_call(c, "rpe_map_sdf_rows", true, lo, hi, level, pose12, dist_thr, cos_thr, use_normals, rows);
}
int rpe_map_sdf_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals,
                          const int64_t lo[3], const int64_t hi[3], double* out32) {
  return normal_eq_call(c, "rpe_map_sdf_normal_eq", true, lo, hi, level, pose12, dist_thr, cos_thr, use_normals, out32);
}
int rpe_icp_map_sdf(rpe_context* c, const rpe_icp_options* o, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                    double* last_step, double* final_cost, int64_t* matched) {
  return icp_call(c, "rpe_icp_map_sdf", true, lo, hi, o, pose12, iters_out, last_step, final_cost, matched);
}
int rpe_icp_pyramid_map_sdf(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level,
                            const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                            double* last_step, double* final_cost, int64_t* matched) {
  return pyramid_call(c, "rpe_icp_pyramid_map_sdf", true, lo, hi, o, levels, iters_per_level, dist_thr_per_level, pose12, iters_out,
                      last_step, final_cost, matched);
}

}  // extern "C"
