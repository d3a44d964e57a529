// Part 3 of include/rgbd_pose_hip.h: the volume colour term (kernels in rpe_sdf_photo.hpp, compiled into rpe_frontend.hip).  A frame
// tracked against the TSDF volume AND the colour volume beside it: the photometric rows, their normal equations, and the loops of the
// volume term with the photometric rows beside the geometric ones -- per round ONE launch, one host wait, the host solve and left update
// of rpe_gn_host.hpp.  Reads the frame's maps and colour and both volumes.  The model, the model colour, the prepared photometric maps,
// the solver slots, the volumes and the archive are neither read nor replaced: the frame's intensity pyramid is the calls' own
// (c->fe.sint), built with one launch of the photometric term's frame_intensity_kernel and kept until the frame's depth or colour goes.
// The MAP form of each call (kernels in rpe_map_sdf_photo.hpp) reads the virtual volume and the virtual colour volume of a box of the
// map -- the window plus the archived bricks -- through the brick grid of map_field (rpe_frontend_host.hpp): built and uploaded once
// per call, into the volume's map list, for both fetches and every round.
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

namespace {
// what every call needs, and the intensity pyramid of all the frame's levels if the current frame has none yet
int photo_ready(rpe_context* c, int levels, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!F.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!c->vol.have_color) return fail(RPE_ERR_STATE, "no colour volume: call rpe_volume_integrate_color or rpe_volume_color_upload first");
  if (F.fgeo.levels < levels)
    return fail(RPE_ERR_STATE, "%s: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)", who, F.fgeo.levels, levels);
  HIP_TRY(hipSetDevice(c->device));
  if (F.sint_levels == F.fgeo.levels) return RPE_OK;
  F.sint_levels = 0;
  if (int rc = F.sint.reserve(c, (size_t)F.fgeo.off[F.fgeo.levels] * sizeof(float))) return rc;
  HIP_TRY(rpe::launch_frame_intensity(F.fcolor, F.fgeo, F.sint, c->stream));
  F.sint_levels = F.fgeo.levels;
  return RPE_OK;
}
bool weight_ok(double w) { return std::isfinite(w) && w > 0; }
// where a call reads the two volumes: the dense window (map = false), or the virtual volumes g of a box of the map through the grid of M
struct Field { bool map = false; rpe::VolumeGeometry g; rpe::MapRayView M{}; };
// the window's field, or with `box` the map's inside the box (lo = NULL: the map's bounds)
int field_of(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, Field& f) {
  f.g = c->vol.g;
  if (!box) return RPE_OK;
  const int rc = map_field(c, who, lo, hi, f.g, f.M);
  f.map = rc == RPE_OK;
  return rc;
}

// one round: launch, wait, the 32-double record of both terms in ne (cost and rows the geometric ones), the photometric cost / rows
int photo_round(rpe_context* c, const Field& f, const Level& lv, const float* fint, double dist_thr, double cos_thr, int use_normals, float lam,
                int geometric, const double* pose12, double* ne, double* pcost, double* prows) {
  if (f.map)
    HIP_TRY(rpe::launch_icp_map_sdf_photo(lv.f[0], lv.f[1], fint, lv.n, f.M, f.g, (float)dist_thr, (float)cos_thr, use_normals, lam, geometric,
                                          pose12, collect_target(c), c->stream));
  else
    HIP_TRY(rpe::launch_icp_sdf_photo(lv.f[0], lv.f[1], fint, lv.n, c->vol.d, c->vol.cd, f.g, (float)dist_thr, (float)cos_thr, use_normals, lam,
                                      geometric, pose12, collect_target(c), c->stream));
  int rc = wait_host(c, rpe::kNlLd);
  if (rc) return rc;
  for (int i = 0; i < 32; i++) ne[i] = i < 29 ? c->h_out[i] : 0.0;
  ne[29] = rpe::pivot_floor(false);   // the rows' products are fp32
  *pcost = c->h_out[29]; *prows = c->h_out[30];
  return RPE_OK;
}
// rpe_icp_sdf's host rounds on one level with the combined record
int photo_rounds(rpe_context* c, const Field& f, const rpe_icp_options* o, int l, int max_iter, double dist_thr, float lam, double* pose12, int* iters_out,
                 double* last_step, double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  const Level lv = level_of(c, l);   // the frame's side only
  const float* fint = c->fe.sint + c->fe.fgeo.off[l];
  GnRun run;   // run.weight: the geometric rows
  double pcost = 0, prows = 0;
  const int rc = gn_host_rounds([&](const double* pose, double* ne) {
    return photo_round(c, f, lv, fint, dist_thr, o->cos_thr, o->use_normals, lam, 1, pose, ne, &pcost, &prows); },
                                rpe::pivot_floor(false), 1.0, max_iter, o->tol, pose12, &run);
  if (rc == kGnRefused) {
    if (iters_out) *iters_out = run.it;
    return fail(RPE_ERR_DEGENERATE, "volume colour term: normal equations are not positive definite at iteration %d (%g + %g rows)", run.it,
                run.weight, prows);
  }
  if (rc) return rc;
  run.report(iters_out, last_step, final_cost, matched);
  if (photo_cost) *photo_cost = pcost;
  if (photo_matched) *photo_matched = (int64_t)prows;
  return RPE_OK;
}
int photo_options(const rpe_icp_options* o, double photo_weight, const double* pose12, const char* who) {
  if (!o || !pose12 || !(o->dist_thr >= 0)) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if (o->device_resident) return fail(RPE_ERR_ARG, "%s: host-driven only (device_resident must be 0)", who);
  if (!weight_ok(photo_weight)) return fail(RPE_ERR_ARG, "%s: photo_weight must be finite and > 0", who);
  return RPE_OK;
}

// ---- the four calls, on the window (box = false) or on a box of the map
int rows_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, int level, const double* pose12, double dist_thr,
              float* rows) {
  session_end(c);
  if (!c || !pose12 || !rows || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", who, RPE_MAX_LEVELS - 1);
  int rc = photo_ready(c, level + 1, who);
  if (rc) return rc;
  Field f;
  if ((rc = field_of(c, who, box, lo, hi, f))) return rc;
  const Level lv = level_of(c, level);
  const float* fint = c->fe.sint + c->fe.fgeo.off[level];
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, (size_t)lv.n * 7 * sizeof(float)))) return rc;
  hipError_t e = f.map ? rpe::launch_map_sdf_photo_rows(lv.f[0], fint, lv.n, f.M, f.g, (float)dist_thr, pose12, d_rows, c->stream)
                       : rpe::launch_sdf_photo_rows(lv.f[0], fint, lv.n, c->vol.d, c->vol.cd, f.g, (float)dist_thr, pose12, d_rows, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rows, d_rows, (size_t)lv.n * 7 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return RPE_OK;
}

int normal_eq_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, int level, const double* pose12,
                   double dist_thr, double weight, double* out32) {
  session_end(c);
  if (!c || !pose12 || !out32 || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !weight_ok(weight) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0, weight finite and > 0)", who, RPE_MAX_LEVELS - 1);
  int rc = photo_ready(c, level + 1, who);
  if (rc) return rc;
  Field f;
  if ((rc = field_of(c, who, box, lo, hi, f))) return rc;
  double ne[32], pcost = 0, prows = 0;
  if ((rc = photo_round(c, f, level_of(c, level), c->fe.sint + c->fe.fgeo.off[level], dist_thr, 0.0, 0, (float)weight, 0, pose12, ne, &pcost, &prows)))
    return rc;
  for (int i = 0; i < 32; i++) out32[i] = i < 27 ? ne[i] : 0.0;
  out32[27] = pcost; out32[28] = prows;
  out32[29] = rpe::pivot_floor(false);   // for rpe_gn_solve: the rows' products are fp32
  return RPE_OK;
}

int icp_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, double photo_weight,
             double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched, double* photo_cost,
             int64_t* photo_matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = photo_options(o, photo_weight, pose12, who);
  if (rc) return rc;
  if (o->max_iter < 1) return fail(RPE_ERR_ARG, "%s: max_iter >= 1", who);
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if ((rc = photo_ready(c, 1, who))) return rc;
  Field f;
  if ((rc = field_of(c, who, box, lo, hi, f))) return rc;
  return photo_rounds(c, f, o, 0, o->max_iter, o->dist_thr, (float)photo_weight, pose12, iters_out, last_step, final_cost, matched, photo_cost,
                      photo_matched);
}

int pyramid_call(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, double photo_weight,
                 int levels, const int* iters_per_level, const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step,
                 double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = photo_options(o, photo_weight, pose12, who);
  if (rc) return rc;
  if ((rc = pyramid_complaint(who, levels, iters_per_level, dist_thr_per_level))) return rc;
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if ((rc = photo_ready(c, levels, who))) return rc;
  Field f;
  if ((rc = field_of(c, who, box, lo, hi, f))) return rc;
  return coarse_to_fine(levels, iters_per_level, dist_thr_per_level, o->dist_thr, iters_out,
                        [&](int l, int rounds, double gate, bool fine, int* it) {
    return photo_rounds(c, f, o, l, rounds, gate, (float)photo_weight, pose12, it, fine ? last_step : nullptr, fine ? final_cost : nullptr,
                        fine ? matched : nullptr, fine ? photo_cost : nullptr, fine ? photo_matched : nullptr);
  });
}
}  // namespace

extern "C" {

int rpe_sdf_photo_rows(rpe_context* c, int level, const double* pose12, double dist_thr, float* rows) {
  return rows_call(c, "rpe_sdf_photo_rows", false, nullptr, nullptr, level, pose12, dist_thr, rows);
}
int rpe_sdf_photo_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double weight, double* out32) {
  return normal_eq_call(c, "rpe_sdf_photo_normal_eq", false, nullptr, nullptr, level, pose12, dist_thr, weight, out32);
}
int rpe_icp_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, double* pose12, int* iters_out, double* last_step,
                     double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return icp_call(c, "rpe_icp_sdf_rgbd", false, nullptr, nullptr, o, photo_weight, pose12, iters_out, last_step, final_cost, matched, photo_cost,
                  photo_matched);
}
int rpe_icp_pyramid_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, int levels, const int* iters_per_level,
                             const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                             int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return pyramid_call(c, "rpe_icp_pyramid_sdf_rgbd", false, nullptr, nullptr, o, photo_weight, levels, iters_per_level, dist_thr_per_level, pose12,
                      iters_out, last_step, final_cost, matched, photo_cost, photo_matched);
}

int rpe_map_sdf_photo_rows(rpe_context* c, int level, const double* pose12, double dist_thr, const int64_t lo[3], const int64_t hi[3],
                           float* rows) {
  return rows_call(c, "rpe_map_sdf_photo_rows", true, lo, hi, level, pose12, dist_thr, rows);
}
int rpe_map_sdf_photo_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double weight, const int64_t lo[3],
                                const int64_t hi[3], double* out32) {
  return normal_eq_call(c, "rpe_map_sdf_photo_normal_eq", true, lo, hi, level, pose12, dist_thr, weight, out32);
}
int rpe_icp_map_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, const int64_t lo[3], const int64_t hi[3],
                         double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched, double* photo_cost,
                         int64_t* photo_matched) {
  return icp_call(c, "rpe_icp_map_sdf_rgbd", true, lo, hi, o, photo_weight, pose12, iters_out, last_step, final_cost, matched, photo_cost,
                  photo_matched);
}
int rpe_icp_pyramid_map_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, int levels, const int* iters_per_level,
                                 const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                                 double* last_step, double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return pyramid_call(c, "rpe_icp_pyramid_map_sdf_rgbd", true, lo, hi, o, photo_weight, levels, iters_per_level, dist_thr_per_level, pose12,
                      iters_out, last_step, final_cost, matched, photo_cost, photo_matched);
}

}  // extern "C"
