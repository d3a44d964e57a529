// Part 3 of include/rgbd_pose_hip.h: the photometric term beside ICP (kernels in rpe_photo.hip).  A model colour without a volume, the
// photometric maps of frame and model, the photometric normal equations and per-pixel rows, and the RGB-D ICP loops: per round ONE
// launch whose record carries the geometric and the photometric rows, one host wait, the host solve and left update of rpe_icp.
#include "rpe_frontend_host.hpp"
using namespace rpeh;

namespace {
// one level of what a round reads: the front end's level (frame vertex / normal, model vertex / normal, pixels, model camera) and
// the photometric maps beside it: the frame's intensity, the model's {I, gx, gy, zm}
struct PhotoLevel : Level { const float *fi, *pm; };
PhotoLevel photo_level(rpe_context* c, int l) {
  auto& F = c->fe;
  return {level_of(c, l), F.pint + F.fgeo.off[l], F.pmap + 4 * F.mgeo.off[l]};
}
int photo_ready(rpe_context* c, int levels, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_from_frame, rpe_model_upload or rpe_volume_raycast first");
  if (F.photo_levels < levels)
    return fail(RPE_ERR_STATE, "%s: the photometric maps are prepared for %d level(s), %d asked (rpe_photo_prepare; a new depth, colour, "
                "model or model colour drops them)", who, F.photo_levels, levels);
  return RPE_OK;
}
// one round: launch, wait, the 32-double record of both terms in ne (cost and pairs the geometric ones), second = the photometric
// cost and pairs
int rgbd_round(rpe_context* c, const PhotoLevel& lv, const rpe_icp_options* o, double dist_thr, float lam, int geometric,
               const double* pose12, double* ne, double* second) {
  HIP_TRY(rpe::launch_icp_photo(lv.f[0], lv.f[1], lv.fi, lv.n, lv.m[0], lv.m[1], lv.pm, lv.mcam, pose_f(c->fe.mpose), (float)dist_thr,
                                o ? (float)o->cos_thr : 0.f, lam, geometric, pose12, collect_target(c), c->stream));
  int rc = wait_host(c, rpe::kNlLd);
  if (rc) return rc;
  round_record(c, ne);
  second[0] = c->h_out[29]; second[1] = c->h_out[30];
  return RPE_OK;
}
// the host rounds of one level with the combined record (rpe_gn_host.hpp gn_host_level); out.matched: the geometric pairs
int rgbd_level(rpe_context* c, const rpe_icp_options* o, int l, int max_iter, double dist_thr, float lam, double* pose12, const GnOut& out) {
  const PhotoLevel lv = photo_level(c, l);
  return gn_host_level([&](const double* pose, double* ne, double* second) { return rgbd_round(c, lv, o, dist_thr, lam, 1, pose, ne, second); },
                       rpe::pivot_floor(false), max_iter, o->tol, pose12, out, [](int it, double pairs, double ppairs) {
    return fail(RPE_ERR_DEGENERATE, "RGB-D ICP: normal equations are not positive definite at iteration %d (%g + %g pairs)", it, pairs, ppairs);
  });
}
int rgbd_options(const rpe_icp_options* o, double photo_weight, const double* pose12, const char* who) {
  if (!o || !pose12 || !(o->dist_thr >= 0)) return fail(RPE_ERR_ARG, "%s: bad argument", who);
  if (o->kind != RPE_RES_P2PLANE || !o->use_normals)
    return fail(RPE_ERR_ARG, "%s: the geometric term is point-to-plane with use_normals = 1 (kind %d given)", who, o->kind);
  if (o->device_resident) return fail(RPE_ERR_ARG, "%s: host-driven only (device_resident must be 0)", who);
  if (!std::isfinite(photo_weight) || !(photo_weight > 0)) return fail(RPE_ERR_ARG, "%s: photo_weight must be finite and > 0", who);
  return RPE_OK;
}
}  // namespace

extern "C" {

int rpe_model_color_upload(rpe_context* c, const uint8_t* rgba) {
  session_end(c);
  if (!c || !rgba) return fail(RPE_ERR_ARG, "rpe_model_color_upload: bad argument");
  auto& F = c->fe;
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_upload, rpe_model_from_frame or rpe_volume_raycast first");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)F.mcam.width * F.mcam.height * 4;
  int rc = F.mcolor.reserve(c, bytes);
  if (rc) return rc;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.mcolor, rgba, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's buffer is free again on return
  F.have_mcolor = true;
  return RPE_OK;
}

int rpe_model_color_from_frame(rpe_context* c) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_from_frame first");
  if (!F.have_frame || !F.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  if (F.mcam.width != F.cam.width || F.mcam.height != F.cam.height)
    return fail(RPE_ERR_STATE, "rpe_model_color_from_frame: the model is %d x %d, the frame %d x %d", F.mcam.width, F.mcam.height,
                F.cam.width, F.cam.height);
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)F.mcam.width * F.mcam.height * 4;
  int rc = F.mcolor.reserve(c, bytes);
  if (rc) return rc;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.mcolor, F.fcolor, bytes, hipMemcpyDeviceToDevice, c->stream));
  F.have_mcolor = true;
  return RPE_OK;
}

int rpe_photo_prepare(rpe_context* c, int levels) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (levels < 1 || levels > RPE_MAX_LEVELS) return fail(RPE_ERR_ARG, "rpe_photo_prepare: levels must be 1 .. %d (got %d)", RPE_MAX_LEVELS, levels);
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!F.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_from_frame, rpe_model_upload or rpe_volume_raycast first");
  if (!F.have_mcolor)
    return fail(RPE_ERR_STATE, "no model colour: call rpe_model_sample_color, rpe_model_color_upload or rpe_model_color_from_frame");
  if (F.fgeo.levels < levels) return fail(RPE_ERR_STATE, "rpe_photo_prepare: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)",
      F.fgeo.levels, levels);
  if (F.mgeo.levels < levels) return fail(RPE_ERR_STATE, "rpe_photo_prepare: the model has %d level(s), %d asked (rpe_model_build_pyramid)",
      F.mgeo.levels, levels);
  HIP_TRY(hipSetDevice(c->device));
  rpe::PyramidGeometry fg = F.fgeo, mg = F.mgeo;
  fg.levels = levels; mg.levels = levels;
  int rc;
  if ((rc = F.pint.reserve(c, (size_t)fg.off[levels] * sizeof(float)))) return rc;
  if ((rc = F.pmap.reserve(c, (size_t)mg.off[levels] * 4 * sizeof(float)))) return rc;
  F.photo_levels = 0;
  HIP_TRY(rpe::launch_frame_intensity(F.fcolor, fg, F.pint, c->stream));
  HIP_TRY(rpe::launch_model_photo(F.mcolor, mg, F.mmap[0], F.mmap[1], pose_f(F.mpose), F.pmap, c->stream));
  F.photo_levels = levels;
  return RPE_OK;
}

int rpe_photo_download(rpe_context* c, int which, int level, float* out) {
  session_end(c);
  if (!c || !out || (which != RPE_PHOTO_FRAME && which != RPE_PHOTO_MODEL) || level < 0)
    return fail(RPE_ERR_ARG, "rpe_photo_download: bad argument");
  int rc = photo_ready(c, level + 1, "rpe_photo_download");
  if (rc) return rc;
  auto& F = c->fe;
  const bool model = which == RPE_PHOTO_MODEL;
  const rpe::PyramidGeometry& g = model ? F.mgeo : F.fgeo;
  const size_t n = (size_t)g.cam[level].width * g.cam[level].height;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, model ? F.pmap + 4 * g.off[level] : F.pint + g.off[level], n * (model ? 4 : 1) * sizeof(float),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_photo_normal_eq(rpe_context* c, int level, const double* pose12, double dist_thr, double weight, double* out32) {
  session_end(c);
  if (!c || !pose12 || !out32 || level < 0 || !(dist_thr >= 0) || !std::isfinite(weight) || !(weight > 0))
    return fail(RPE_ERR_ARG, "rpe_photo_normal_eq: bad argument (level >= 0, dist_thr >= 0, weight finite and > 0)");
  int rc = photo_ready(c, level + 1, "rpe_photo_normal_eq");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  double ne[32], second[2] = {0, 0};
  if ((rc = rgbd_round(c, photo_level(c, level), nullptr, dist_thr, (float)weight, 0, pose12, ne, second))) return rc;
  photo_only_record(ne, second[0], second[1], out32);
  return RPE_OK;
}

int rpe_photo_rows(rpe_context* c, int level, const double* pose12, double dist_thr, float* rows) {
  session_end(c);
  if (!c || !pose12 || !rows || level < 0 || !(dist_thr >= 0)) return fail(RPE_ERR_ARG, "rpe_photo_rows: bad argument");
  int rc = photo_ready(c, level + 1, "rpe_photo_rows");
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const PhotoLevel lv = photo_level(c, level);
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, (size_t)lv.n * 7 * sizeof(float)))) return rc;
  return rows_download(c, "rpe_photo_rows", rpe::launch_photo_rows(lv.f[0], lv.fi, lv.n, lv.pm, lv.mcam, pose_f(c->fe.mpose), (float)dist_thr,
                                                                   pose12, d_rows, c->stream), d_rows, lv.n, rows);
}

int rpe_icp_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, double* pose12, int* iters_out, double* last_step,
                 double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = rgbd_options(o, photo_weight, pose12, "rpe_icp_rgbd");
  if (rc) return rc;
  if (o->max_iter < 1) return fail(RPE_ERR_ARG, "rpe_icp_rgbd: max_iter >= 1");
  if ((rc = photo_ready(c, 1, "rpe_icp_rgbd"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = rgbd_level(c, o, 0, o->max_iter, o->dist_thr, (float)photo_weight, pose12,
                       {iters_out, last_step, final_cost, matched, photo_cost, photo_matched}))) return rc;
  // leave the pairs in the solver slots, under the returned pose (as a fused rpe_icp does)
  return rpe_associate(c, pose12, o->dist_thr, o->cos_thr, o->use_normals, nullptr);
}

int rpe_icp_pyramid_rgbd(rpe_context* c, const rpe_icp_options* o, double photo_weight, int levels, const int* iters_per_level,
                         const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                         int64_t* matched, double* photo_cost, int64_t* photo_matched) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  int rc = rgbd_options(o, photo_weight, pose12, "rpe_icp_pyramid_rgbd");
  if (rc) return rc;
  if ((rc = pyramid_complaint("rpe_icp_pyramid_rgbd", levels, iters_per_level, dist_thr_per_level))) return rc;
  if ((rc = photo_ready(c, levels, "rpe_icp_pyramid_rgbd"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const GnOut out{iters_out, last_step, final_cost, matched, photo_cost, photo_matched};
  rc = coarse_to_fine(levels, iters_per_level, dist_thr_per_level, o->dist_thr, iters_out,
                      [&](int l, int rounds, double gate, bool fine, int* it) {
    return rgbd_level(c, o, l, rounds, gate, (float)photo_weight, pose12, out.at_level(fine, it));
  });
  if (rc) return rc;
  return rpe_associate(c, pose12, dist_thr_per_level ? dist_thr_per_level[0] : o->dist_thr, o->cos_thr, o->use_normals, nullptr);
}

}  // extern "C"
