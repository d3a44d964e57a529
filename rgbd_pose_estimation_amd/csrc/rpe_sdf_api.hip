// Part 3 of include/rgbd_pose_hip.h: the volume term and the volume colour term, on the window and on the whole map -- sixteen entry
// points, four calls (rows, normal equations, loop, coarse-to-fine loop) for each pairing of term and field, every call stated once.
//   THE VOLUME TERM (kernels in rpe_frontend.hip, rule in rpe_sdf_rule.hpp): a frame tracked against the TSDF volume itself.  Per-pixel
//     rows, the normal equations of one level, and the loops -- per round ONE launch, one host wait, the host solve and left update of
//     rpe_gn_host.hpp.  Reads the frame's maps and the volume.
//   THE VOLUME COLOUR TERM (`colour`; kernels in rpe_sdf_photo.hpp, compiled into rpe_frontend.hip): the photometric rows against the
//     colour volume beside the geometric ones, in the same launch.  Reads the frame's colour and the colour volume as well; the frame's
//     intensity pyramid is the calls' own (c->fe.sint), built with one launch of the photometric term's frame_intensity_kernel and kept
//     until the frame's depth or colour goes.
//   THE MAP form of each call (`box`; kernels in rpe_frontend.hip and rpe_map_sdf_photo.hpp) reads the virtual volume -- and virtual
//     colour volume -- of a box of the map, the window plus the archived bricks, through the brick grid of map_field
//     (rpe_frontend_host.hpp; rpe_mapmesh_api.hip builds it): built and uploaded once per call, into the volume's map list, for both
//     fetches and every round.
// The model, the model colour, the solver slots, the prepared photometric maps, the volumes and the archive are neither read nor replaced.
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

namespace {
// which of the sixteen a call is: its name for the messages, the term (colour: the photometric rows too) and the field (box: the map)
struct Kind { const char* who; bool colour, box; };

// what every call needs of the context; with colour also the intensity pyramid of all the frame's levels, built here if the current
// frame has none yet
int ready(rpe_context* c, bool colour, int levels, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (colour && !F.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (colour && !c->vol.have_color)
    return fail(RPE_ERR_STATE, "no colour volume: call rpe_volume_integrate_color or rpe_volume_color_upload first");
  if (F.fgeo.levels < levels)
    return fail(RPE_ERR_STATE, "%s: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)", who, F.fgeo.levels, levels);
  HIP_TRY(hipSetDevice(c->device));
  if (!colour || F.sint_levels == F.fgeo.levels) return RPE_OK;
  F.sint_levels = 0;
  if (int rc = F.sint.reserve(c, (size_t)F.fgeo.off[F.fgeo.levels] * sizeof(float))) return rc;
  HIP_TRY(rpe::launch_frame_intensity(F.fcolor, F.fgeo, F.sint, c->stream));
  F.sint_levels = F.fgeo.levels;
  return RPE_OK;
}
bool weight_ok(double w) { return std::isfinite(w) && w > 0; }
// where a call reads the volumes: the dense window (map = false), or the virtual volumes g of a box of the map through the grid of M
struct Field { bool map = false; rpe::VolumeGeometry g; rpe::MapRayView M{}; };
// the window's field, or with `box` the map's inside the box (lo = NULL: the map's bounds)
int field_of(rpe_context* c, const char* who, bool box, const int64_t* lo, const int64_t* hi, Field& f) {
  f.g = c->vol.g;
  if (!box) return RPE_OK;
  const int rc = map_field(c, who, lo, hi, f.g, f.M);
  f.map = rc == RPE_OK;
  return rc;
}
// the frame's intensity at level l for the colour term's kernels; nobody reads it without colour
const float* intensity_of(rpe_context* c, bool colour, int l) { return colour ? c->fe.sint + c->fe.fgeo.off[l] : nullptr; }

// one round: launch, wait, the 32-double record (H | g | geometric sum r^2 | geometric rows | pivot floor); with colour H and g are those
// of both terms (lam: the photometric weight; geometric = 0: of the photometric rows alone) and second = the photometric cost and rows
int sdf_round(rpe_context* c, const Field& f, const Level& lv, const float* fint, bool colour, double dist_thr, double cos_thr, int use_normals,
              float lam, int geometric, const double* pose12, double* ne, double* second) {
  // the robust weight is the context's (rpe_sdf_set_robust); kind NONE launches exactly what there was before there was one
  const auto& W = c->sdf_robust;
  const float gate = (float)dist_thr, cosine = (float)cos_thr, k = (float)W.k, photo_k = (float)W.photo_k;
  const rpe::ReduceTarget rt = collect_target(c);
  if (W.kind != RPE_ROBUST_NONE) {
    if (colour && f.map)
      HIP_TRY(rpe::launch_icp_map_sdf_photo_robust(lv.f[0], lv.f[1], fint, lv.n, f.M, f.g, gate, cosine, use_normals, lam, geometric, W.kind, k,
                                                   photo_k, pose12, rt, c->stream));
    else if (colour)
      HIP_TRY(rpe::launch_icp_sdf_photo_robust(lv.f[0], lv.f[1], fint, lv.n, c->vol.d, c->vol.cd, f.g, gate, cosine, use_normals, lam, geometric,
                                               W.kind, k, photo_k, pose12, rt, c->stream));
    else if (f.map)
      HIP_TRY(rpe::launch_icp_map_sdf_robust(lv.f[0], lv.f[1], lv.n, f.M, f.g, gate, cosine, use_normals, W.kind, k, pose12, rt, c->stream));
    else
      HIP_TRY(rpe::launch_icp_sdf_robust(lv.f[0], lv.f[1], lv.n, c->vol.d, f.g, gate, cosine, use_normals, W.kind, k, pose12, rt, c->stream));
  } else if (colour && f.map)
    HIP_TRY(rpe::launch_icp_map_sdf_photo(lv.f[0], lv.f[1], fint, lv.n, f.M, f.g, gate, cosine, use_normals, lam, geometric, pose12, rt, c->stream));
  else if (colour)
    HIP_TRY(rpe::launch_icp_sdf_photo(lv.f[0], lv.f[1], fint, lv.n, c->vol.d, c->vol.cd, f.g, gate, cosine, use_normals, lam, geometric, pose12, rt,
                                      c->stream));
  else if (f.map)
    HIP_TRY(rpe::launch_icp_map_sdf(lv.f[0], lv.f[1], lv.n, f.M, f.g, gate, cosine, use_normals, pose12, rt, c->stream));
  else
    HIP_TRY(rpe::launch_icp_sdf(lv.f[0], lv.f[1], lv.n, c->vol.d, f.g, gate, cosine, use_normals, pose12, rt, c->stream));
  int rc = wait_host(c, colour ? rpe::kNlLd : rpe::kNeLd);
  if (rc) return rc;
  round_record(c, ne);
  ne[29] = rpe::pivot_floor(false);   // the rows' products are fp32
  if (colour) { second[0] = c->h_out[29]; second[1] = c->h_out[30]; }
  return RPE_OK;
}
// the host rounds of one level (rpe_gn_host.hpp gn_host_level); out.matched: the geometric rows
int sdf_level(rpe_context* c, const Kind& K, const Field& f, const rpe_icp_options* o, int l, int max_iter, double dist_thr, float lam,
              double* pose12, const GnOut& out) {
  const Level lv = level_of(c, l);   // the frame's side only
  const float* fint = intensity_of(c, K.colour, l);
  return gn_host_level(
      [&](const double* pose, double* ne, double* second) {
        return sdf_round(c, f, lv, fint, K.colour, dist_thr, o->cos_thr, o->use_normals, lam, 1, pose, ne, second);
      },
      rpe::pivot_floor(false), max_iter, o->tol, pose12, out, [&](int it, double rows, double prows) {
        if (K.colour)
          return fail(RPE_ERR_DEGENERATE, "volume colour term: normal equations are not positive definite at iteration %d (%g + %g rows)", it,
                      rows, prows);
        return fail(RPE_ERR_DEGENERATE, "volume term: normal equations are not positive definite at iteration %d (%g rows)", it, rows);
      });
}
int loop_options(const Kind& K, const rpe_icp_options* o, double photo_weight, const double* pose12) {
  if (!o || !pose12 || !(o->dist_thr >= 0)) return fail(RPE_ERR_ARG, "%s: bad argument", K.who);
  if (o->device_resident) return fail(RPE_ERR_ARG, "%s: host-driven only (device_resident must be 0)", K.who);
  if (K.colour && !weight_ok(photo_weight)) return fail(RPE_ERR_ARG, "%s: photo_weight must be finite and > 0", K.who);
  return RPE_OK;
}

// ---- the four calls.  Without colour the photometric weight is not read; with it cos_thr and use_normals of the rows and of the
// normal equations are not (the photometric row asks for neither gate)
int rows_call(rpe_context* c, const Kind& K, const int64_t* lo, const int64_t* hi, int level, const double* pose12, double dist_thr,
              double cos_thr, int use_normals, float* rows) {
  session_end(c);
  if (!c || !pose12 || !rows || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", K.who, RPE_MAX_LEVELS - 1);
  int rc = ready(c, K.colour, level + 1, K.who);
  if (rc) return rc;
  Field f;
  if ((rc = field_of(c, K.who, K.box, lo, hi, f))) return rc;
  const Level lv = level_of(c, level);
  const float* fint = intensity_of(c, K.colour, level);
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, (size_t)lv.n * 7 * sizeof(float)))) return rc;
  hipError_t e;
  if (K.colour)
    e = f.map ? rpe::launch_map_sdf_photo_rows(lv.f[0], fint, lv.n, f.M, f.g, (float)dist_thr, pose12, d_rows, c->stream)
              : rpe::launch_sdf_photo_rows(lv.f[0], fint, lv.n, c->vol.d, c->vol.cd, f.g, (float)dist_thr, pose12, d_rows, c->stream);
  else
    e = f.map ? rpe::launch_map_sdf_rows(lv.f[0], lv.f[1], lv.n, f.M, f.g, (float)dist_thr, (float)cos_thr, use_normals != 0, pose12, d_rows,
                                         c->stream)
              : rpe::launch_sdf_rows(lv.f[0], lv.f[1], lv.n, c->vol.d, f.g, (float)dist_thr, (float)cos_thr, use_normals != 0, pose12, d_rows,
                                     c->stream);
  return rows_download(c, K.who, e, d_rows, lv.n, rows);
}

// the hook of the robust volume terms: the plane of weights of the level's rows under the context's setting (photo: the photometric
// rows', scale photo_k; else the geometric rows', scale k).  Checks and their order are rows_call's
int weights_call(rpe_context* c, const Kind& K, const int64_t* lo, const int64_t* hi, int level, const double* pose12, double dist_thr,
                 double cos_thr, int use_normals, float* weights) {
  session_end(c);
  if (!c || !pose12 || !weights || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || !lo != !hi)
    return fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", K.who, RPE_MAX_LEVELS - 1);
  int rc = ready(c, K.colour, level + 1, K.who);
  if (rc) return rc;
  Field f;
  if ((rc = field_of(c, K.who, K.box, lo, hi, f))) return rc;
  const Level lv = level_of(c, level);
  DevBuf<float> d_w;
  if ((rc = d_w.once(c, (size_t)lv.n * sizeof(float)))) return rc;
  const auto& W = c->sdf_robust;
  const hipError_t e = rpe::launch_sdf_robust_weights(lv.f[0], lv.f[1], intensity_of(c, K.colour, level), lv.n, c->vol.d,
                                                      K.colour ? (const unsigned short*)c->vol.cd : nullptr, f.map ? &f.M : nullptr, f.g,
                                                      (float)dist_thr, (float)cos_thr, use_normals != 0, K.colour, W.kind,
                                                      (float)(K.colour ? W.photo_k : W.k), pose12, d_w, c->stream);
  return rows_download(c, K.who, e, d_w, lv.n, weights, 1);
}

int normal_eq_call(rpe_context* c, const Kind& K, const int64_t* lo, const int64_t* hi, int level, const double* pose12, double dist_thr,
                   double cos_thr, int use_normals, double weight, double* out32) {
  session_end(c);
  if (!c || !pose12 || !out32 || level < 0 || level >= RPE_MAX_LEVELS || !(dist_thr >= 0) || (K.colour && !weight_ok(weight)) || !lo != !hi)
    return K.colour ? fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0, weight finite and > 0)", K.who, RPE_MAX_LEVELS - 1)
                    : fail(RPE_ERR_ARG, "%s: bad argument (level 0 .. %d, dist_thr >= 0)", K.who, RPE_MAX_LEVELS - 1);
  int rc = ready(c, K.colour, level + 1, K.who);
  if (rc) return rc;
  Field f;
  if ((rc = field_of(c, K.who, K.box, lo, hi, f))) return rc;
  // with colour: the photometric rows alone, no gate on the normals
  double ne[32], second[2] = {0, 0};
  if ((rc = sdf_round(c, f, level_of(c, level), intensity_of(c, K.colour, level), K.colour, dist_thr, K.colour ? 0.0 : cos_thr,
                      K.colour ? 0 : use_normals != 0, (float)weight, 0, pose12, ne, second)))
    return rc;
  if (K.colour) photo_only_record(ne, second[0], second[1], out32);
  else std::memcpy(out32, ne, sizeof ne);
  return RPE_OK;
}

int icp_call(rpe_context* c, const Kind& K, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, double photo_weight, double* pose12,
             const GnOut& out) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = loop_options(K, o, photo_weight, pose12);
  if (rc) return rc;
  if (o->max_iter < 1) return fail(RPE_ERR_ARG, "%s: max_iter >= 1", K.who);
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", K.who);
  if ((rc = ready(c, K.colour, 1, K.who))) return rc;
  Field f;
  if ((rc = field_of(c, K.who, K.box, lo, hi, f))) return rc;
  return sdf_level(c, K, f, o, 0, o->max_iter, o->dist_thr, (float)photo_weight, pose12, out);
}

int pyramid_call(rpe_context* c, const Kind& K, const int64_t* lo, const int64_t* hi, const rpe_icp_options* o, double photo_weight, int levels,
                 const int* iters_per_level, const double* dist_thr_per_level, double* pose12, const GnOut& out) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = loop_options(K, o, photo_weight, pose12);
  if (rc) return rc;
  if ((rc = pyramid_complaint(K.who, levels, iters_per_level, dist_thr_per_level))) return rc;
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: bad argument", K.who);
  if ((rc = ready(c, K.colour, levels, K.who))) return rc;
  Field f;
  if ((rc = field_of(c, K.who, K.box, lo, hi, f))) return rc;
  return coarse_to_fine(levels, iters_per_level, dist_thr_per_level, o->dist_thr, out.iters,
                        [&](int l, int rounds, double gate, bool fine, int* it) {
    return sdf_level(c, K, f, o, l, rounds, gate, (float)photo_weight, pose12, out.at_level(fine, it));
  });
}
}  // namespace

extern "C" {

// ---- the robust weight of all sixteen: the context's setting, and the hook that shows a level's weights
static_assert(RPE_ROBUST_NONE == rpe::kRobustNone && RPE_ROBUST_HUBER == rpe::kRobustHuber && RPE_ROBUST_TUKEY == rpe::kRobustTukey,
              "the kernels' kinds are the C ABI's");
int rpe_sdf_set_robust(rpe_context* c, int kind, double k, double photo_k) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (kind == RPE_ROBUST_CAUCHY) return fail(RPE_ERR_ARG, "rpe_sdf_set_robust: RPE_ROBUST_CAUCHY is not a kind of the volume terms (NONE, HUBER, TUKEY)");
  if (kind != RPE_ROBUST_NONE && kind != RPE_ROBUST_HUBER && kind != RPE_ROBUST_TUKEY)
    return fail(RPE_ERR_ARG, "rpe_sdf_set_robust: kind %d is none of RPE_ROBUST_NONE, RPE_ROBUST_HUBER, RPE_ROBUST_TUKEY", kind);
  if (kind == RPE_ROBUST_NONE) { c->sdf_robust = {}; return RPE_OK; }
  if (!(std::isfinite(k) && k >= 1e-6)) return fail(RPE_ERR_ARG, "rpe_sdf_set_robust: k must be finite and >= 1e-6");
  if (!(photo_k == 0 || (std::isfinite(photo_k) && photo_k >= 1e-6)))
    return fail(RPE_ERR_ARG, "rpe_sdf_set_robust: photo_k must be 0 (photometric rows at weight 1) or finite and >= 1e-6");
  c->sdf_robust.kind = kind; c->sdf_robust.k = k; c->sdf_robust.photo_k = photo_k;
  return RPE_OK;
}
int rpe_sdf_robust(rpe_context* c, int* kind, double* k, double* photo_k) {
  if (!c || !kind || !k || !photo_k) return fail(RPE_ERR_ARG, "rpe_sdf_robust: bad argument");
  *kind = c->sdf_robust.kind; *k = c->sdf_robust.k; *photo_k = c->sdf_robust.photo_k;
  return RPE_OK;
}
int rpe_sdf_robust_weights(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, int photo,
                           float* weights) {
  return weights_call(c, {"rpe_sdf_robust_weights", photo != 0, false}, nullptr, nullptr, level, pose12, dist_thr, cos_thr, use_normals, weights);
}
int rpe_map_sdf_robust_weights(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, int photo,
                               const int64_t lo[3], const int64_t hi[3], float* weights) {
  return weights_call(c, {"rpe_map_sdf_robust_weights", photo != 0, true}, lo, hi, level, pose12, dist_thr, cos_thr, use_normals, weights);
}

// ---- the volume term on the window ...
int rpe_sdf_rows(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, float* rows) {
  return rows_call(c, {"rpe_sdf_rows", false, false}, nullptr, nullptr, level, pose12, dist_thr, cos_thr, use_normals, rows);
}
int rpe_sdf_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, double* out32) {
  return normal_eq_call(c, {"rpe_sdf_normal_eq", false, false}, nullptr, nullptr, level, pose12, dist_thr, cos_thr, use_normals, 0.0, out32);
}
int rpe_icp_sdf(rpe_context* c, const rpe_icp_options* o, double* pose12, int* iters_out, double* last_step, double* final_cost,
                int64_t* matched) {
  return icp_call(c, {"rpe_icp_sdf", false, false}, nullptr, nullptr, o, 0.0, pose12, {iters_out, last_step, final_cost, matched});
}
int rpe_icp_pyramid_sdf(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level, const double* dist_thr_per_level,
                        double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched) {
  return pyramid_call(c, {"rpe_icp_pyramid_sdf", false, false}, nullptr, nullptr, o, 0.0, levels, iters_per_level, dist_thr_per_level, pose12,
                      {iters_out, last_step, final_cost, matched});
}

// ---- ... and on a box of the map
int rpe_map_sdf_rows(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, const int64_t lo[3],
                     const int64_t hi[3], float* rows) {
  return rows_call(c, {"rpe_map_sdf_rows", false, true}, lo, hi, level, pose12, dist_thr, cos_thr, use_normals, rows);
}
int rpe_map_sdf_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals,
                          const int64_t lo[3], const int64_t hi[3], double* out32) {
  return normal_eq_call(c, {"rpe_map_sdf_normal_eq", false, true}, lo, hi, level, pose12, dist_thr, cos_thr, use_normals, 0.0, out32);
}
int rpe_icp_map_sdf(rpe_context* c, const rpe_icp_options* o, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                    double* last_step, double* final_cost, int64_t* matched) {
  return icp_call(c, {"rpe_icp_map_sdf", false, true}, lo, hi, o, 0.0, pose12, {iters_out, last_step, final_cost, matched});
}
int rpe_icp_pyramid_map_sdf(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level,
                            const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                            double* last_step, double* final_cost, int64_t* matched) {
  return pyramid_call(c, {"rpe_icp_pyramid_map_sdf", false, true}, lo, hi, o, 0.0, levels, iters_per_level, dist_thr_per_level, pose12,
                      {iters_out, last_step, final_cost, matched});
}

// ---- the volume colour term on the window ...
int rpe_sdf_photo_rows(rpe_context* c, int level, const double* pose12, double dist_thr, float* rows) {
  return rows_call(c, {"rpe_sdf_photo_rows", true, false}, nullptr, nullptr, level, pose12, dist_thr, 0.0, 0, rows);
}
int rpe_sdf_photo_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double weight, double* out32) {
  return normal_eq_call(c, {"rpe_sdf_photo_normal_eq", true, false}, nullptr, nullptr, level, pose12, dist_thr, 0.0, 0, weight, out32);
}
int rpe_icp_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, double* pose12, int* iters_out, double* last_step,
                     double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return icp_call(c, {"rpe_icp_sdf_rgbd", true, false}, nullptr, nullptr, o, photo_weight, pose12,
                  {iters_out, last_step, final_cost, matched, photo_cost, photo_matched});
}
int rpe_icp_pyramid_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, int levels, const int* iters_per_level,
                             const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                             int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return pyramid_call(c, {"rpe_icp_pyramid_sdf_rgbd", true, false}, nullptr, nullptr, o, photo_weight, levels, iters_per_level,
                      dist_thr_per_level, pose12, {iters_out, last_step, final_cost, matched, photo_cost, photo_matched});
}

// ---- ... and on a box of the map
int rpe_map_sdf_photo_rows(rpe_context* c, int level, const double* pose12, double dist_thr, const int64_t lo[3], const int64_t hi[3],
                           float* rows) {
  return rows_call(c, {"rpe_map_sdf_photo_rows", true, true}, lo, hi, level, pose12, dist_thr, 0.0, 0, rows);
}
int rpe_map_sdf_photo_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double weight, const int64_t lo[3],
                                const int64_t hi[3], double* out32) {
  return normal_eq_call(c, {"rpe_map_sdf_photo_normal_eq", true, true}, lo, hi, level, pose12, dist_thr, 0.0, 0, weight, out32);
}
int rpe_icp_map_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, const int64_t lo[3], const int64_t hi[3],
                         double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched, double* photo_cost,
                         int64_t* photo_matched) {
  return icp_call(c, {"rpe_icp_map_sdf_rgbd", true, true}, lo, hi, o, photo_weight, pose12,
                  {iters_out, last_step, final_cost, matched, photo_cost, photo_matched});
}
int rpe_icp_pyramid_map_sdf_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, int levels, const int* iters_per_level,
                                 const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                                 double* last_step, double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  return pyramid_call(c, {"rpe_icp_pyramid_map_sdf_rgbd", true, true}, lo, hi, o, photo_weight, levels, iters_per_level, dist_thr_per_level,
                      pose12, {iters_out, last_step, final_cost, matched, photo_cost, photo_matched});
}

}  // extern "C"
