// Part 3 of include/rgbd_pose_hip.h: the depth-frame front end (back-projection, normals, projective association: kernels in
// rpe_frontend.hip) and ICP over it (fused rounds / resident grids: rpe_icp.hip).  No reference counterpart.
#include "rpe_frontend_host.hpp"
#include <memory>
using namespace rpeh;

namespace rpeh {
// the solver slots the association writes: the context's own storage, n = pixels, fp32
int claim_slots(rpe_context* c, int64_t n) {
  const size_t bytes = (size_t)n * 3 * sizeof(float);
  for (auto& slot : c->store) if (int rc = slot.reserve(c, bytes)) return rc;
  if (c->n != n || c->dtype != RPE_F32) {  // a different problem was loaded before: its masks / weights do not apply
    for (int i = 0; i < 3; i++) { c->mask[i] = nullptr; c->weight[i] = nullptr; }
  }
  c->n = n; c->dtype = RPE_F32;
  // (the association kernel rewrites them every round, NaN-marking the pixels without a partner: never promoted to "verified")
  for (int s = 0; s < RPE_NUM_ARRAYS; s++) { c->arr[s] = c->store[s]; arrays_changed(c, s, true); }
  return RPE_OK;
}
int model_room(rpe_context* c, int64_t n) {
  for (auto& m : c->fe.mmap) if (int rc = m.reserve(c, (size_t)n * 3 * sizeof(float))) return rc;
  return RPE_OK;
}
}  // namespace rpeh

extern "C" {
// ---------------------------------------------------------------------------------------------- Part 3: front end
namespace {
int associate_launch(rpe_context* c, const Level& lv, const double* pose12, double dist_thr, double cos_thr, int use_normals,
    bool pose_on_device, bool count) {
  auto& F = c->fe;
  const int64_t n = lv.n;
  const float d = (float)dist_thr;
  if (count) HIP_TRY(hipMemsetAsync(F.d_count, 0, sizeof(int), c->stream));
  HIP_TRY(rpe::launch_associate(lv.f[0], lv.f[1], lv.f[2], n, lv.m[0], lv.m[1], lv.mcam, pose_f(pose12), pose_f(F.mpose),
      d * d,
                                (float)cos_thr, use_normals, pose_on_device ? c->d_gn_pose : nullptr,
                                pose_on_device ? &c->d_gn_state->done : nullptr, (float*)c->arr[RPE_XW], (float*)c->arr[RPE_XC],
                                (float*)c->arr[RPE_BV], (float*)c->arr[RPE_NW], (float*)c->arr[RPE_NC], count ? F.d_count : nullptr, c->stream));
  return RPE_OK;
}
int associate_ready(rpe_context* c) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!c->fe.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!c->fe.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_from_frame or rpe_model_upload first");
  return RPE_OK;
}
static_assert(rpe::kMaxLevels == RPE_MAX_LEVELS, "one pyramid depth for kernels and ABI");
// fp64 level cameras, fp32 casts and level offsets of a `levels`-level pyramid over camera k0 (validated by camera_of).  Levels
// are concatenated; every level but the last is padded to a multiple of 4 pixels so that the next one starts 16-byte aligned.
int plan_levels(const rpe_camera& k0, int levels, rpe_camera* kc, rpe::PyramidGeometry* g) {
  if (levels < 1 || levels > RPE_MAX_LEVELS) return fail(RPE_ERR_ARG, "levels must be 1 .. %d (got %d)", RPE_MAX_LEVELS, levels);
  *g = rpe::PyramidGeometry{};
  g->levels = levels;
  for (int l = 0; l < levels; l++) {
    rpe_camera k = k0;
    if (l > 0) {
      const double s = (double)(1 << l);
      k.fx = k0.fx / s; k.fy = k0.fy / s; k.cx = (k0.cx + 0.5) / s - 0.5; k.cy = (k0.cy + 0.5) / s - 0.5;
      k.width = k0.width >> l; k.height = k0.height >> l;
      if (k.width < 1 || k.height < 1)
        return fail(RPE_ERR_ARG, "pyramid level %d of a %d x %d camera has no pixel", l, k0.width, k0.height);
    }
    int rc = camera_of(&k, &g->cam[l]);
    if (rc) return rc;
    kc[l] = k;
    const int64_t n = (int64_t)k.width * k.height;
    g->off[l + 1] = g->off[l] + (l + 1 < levels ? (n + 3) / 4 * 4 : n);
  }
  for (int l = levels + 1; l <= RPE_MAX_LEVELS; l++) g->off[l] = g->off[levels];
  return RPE_OK;
}
// room for the raw depth of n pixels (and the pair counter; filter on: the filtered depth, on first use or for a larger frame) and
// for `maps` pixels in each of the frame's three maps
int stage_depth(rpe_context* c, int depth_type, int64_t n, int64_t maps) {
  auto& F = c->fe;
  int rc;
  if ((rc = F.d_depth.reserve(c, (size_t)n * (depth_type == RPE_DEPTH_U16 ? 2 : 4))) || (rc = F.d_count.once(c, 64))) return rc;
  if (F.filter.radius > 0 && (rc = F.d_filt.reserve(c, (size_t)n * sizeof(float)))) return rc;
  for (auto& m : F.fmap) if ((rc = m.reserve(c, (size_t)maps * 3 * sizeof(float)))) return rc;
  return RPE_OK;
}
// what F1 / F1p read behind the upload: the raw depth as it came, or -- filter on -- F0's metric depth of it (float32, scale 1)
struct DepthSource { const void* d; int type; float scale; };
int depth_source(rpe_context* c, int depth_type, const rpe::Camera& k, float scale, float dmin, float dmax, DepthSource* src) {
  auto& F = c->fe;
  *src = DepthSource{F.d_depth, depth_type, scale};
  if (F.filter.radius == 0) return RPE_OK;
  HIP_TRY(rpe::launch_depth_filter(F.d_depth, depth_type, k.width, k.height, scale, dmin, dmax, F.fparams, F.d_filt, c->stream));
  *src = DepthSource{F.d_filt, RPE_DEPTH_F32, 1.0f};
  return RPE_OK;
}
}  // namespace

int rpe_frame_set_filter(rpe_context* c, const rpe_depth_filter* f) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!f || f->radius == 0) { F.filter = rpe_depth_filter{0, 0.0, 0.0, 0.0}; return RPE_OK; }
  if (f->radius < 0 || f->radius > RPE_FILTER_MAX_RADIUS)
    return fail(RPE_ERR_ARG, "rpe_frame_set_filter: radius must be 0 .. %d (got %d)", RPE_FILTER_MAX_RADIUS, f->radius);
  if (!std::isfinite(f->sigma_space) || !(f->sigma_space > 0) || !std::isfinite(f->depth_cut) || !(f->depth_cut > 0) ||
      !std::isfinite(f->depth_cut_z2) || f->depth_cut_z2 < 0)
    return fail(RPE_ERR_ARG, "rpe_frame_set_filter: need sigma_space > 0, depth_cut > 0 and depth_cut_z2 >= 0, all finite");
  rpe::FilterParams P{};
  P.radius = f->radius; P.a = (float)f->depth_cut; P.b = (float)f->depth_cut_z2;
  int i = 0;
  for (int dy = -f->radius; dy <= f->radius; dy++)
    for (int dx = -f->radius; dx <= f->radius; dx++)
      P.ws[i++] = (float)std::exp(-(double)(dx * dx + dy * dy) / (2 * f->sigma_space * f->sigma_space));
  F.filter = *f; F.fparams = P;
  return RPE_OK;
}

int rpe_frame_get_filter(rpe_context* c, rpe_depth_filter* out) {
  if (!c || !out) return fail(RPE_ERR_ARG, "rpe_frame_get_filter: bad argument");
  *out = c->fe.filter;
  return RPE_OK;
}

int rpe_frame_set_depth(rpe_context* c, const void* depth, int depth_type, const rpe_camera* cam, double depth_scale, double dmin,
                        double dmax, double max_jump) {
  session_end(c);
  if (!c || !depth || (depth_type != RPE_DEPTH_U16 && depth_type != RPE_DEPTH_F32)) return fail(RPE_ERR_ARG,
      "rpe_frame_set_depth: bad argument");
  rpe::Camera k;
  int rc = camera_of(cam, &k);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  const int64_t n = (int64_t)k.width * k.height;
  if ((rc = stage_depth(c, depth_type, n, n))) return rc;
  F.have_frame = false; F.have_fcolor = false; F.feat[0].have = false; F.photo_levels = 0; F.sint_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.d_depth, depth, (size_t)n * (depth_type == RPE_DEPTH_U16 ? 2 : 4), hipMemcpyHostToDevice, c->stream));
  DepthSource src;
  if ((rc = depth_source(c, depth_type, k, (float)depth_scale, (float)dmin, (float)dmax, &src))) return rc;
  HIP_TRY(rpe::launch_frame_maps(src.d, src.type, k, src.scale, (float)dmin, (float)dmax, (float)max_jump, F.fmap[0],
      F.fmap[1],
                                 F.fmap[2], c->stream));
  F.cam = k; F.have_frame = true;
  one_level(*cam, k, F.kcam, &F.fgeo);
  F.have_depth = false;
  return RPE_OK;
}

int rpe_frame_set_depth_pyramid(rpe_context* c, const void* depth, int depth_type, const rpe_camera* cam, double depth_scale,
                                double dmin, double dmax, double max_jump, int levels) {
  session_end(c);
  if (!c || !depth || !cam || (depth_type != RPE_DEPTH_U16 && depth_type != RPE_DEPTH_F32)) return fail(RPE_ERR_ARG,
      "rpe_frame_set_depth_pyramid: bad argument");
  rpe_camera kc[RPE_MAX_LEVELS];
  rpe::PyramidGeometry g;
  int rc = plan_levels(*cam, levels, kc, &g);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  const int64_t n = (int64_t)g.cam[0].width * g.cam[0].height, total = g.off[levels];
  if ((rc = stage_depth(c, depth_type, n, total)) || (rc = F.fdepth.reserve(c, (size_t)total * sizeof(float)))) return rc;
  F.have_frame = false; F.have_depth = false; F.have_fcolor = false; F.feat[0].have = false; F.photo_levels = 0; F.sint_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.d_depth, depth, (size_t)n * (depth_type == RPE_DEPTH_U16 ? 2 : 4), hipMemcpyHostToDevice, c->stream));
  DepthSource src;
  if ((rc = depth_source(c, depth_type, g.cam[0], (float)depth_scale, (float)dmin, (float)dmax, &src))) return rc;
  HIP_TRY(rpe::launch_frame_pyramid(src.d, src.type, g, src.scale, (float)dmin, (float)dmax, (float)max_jump, F.fdepth,
                                    F.fmap[0], F.fmap[1], F.fmap[2], c->stream));
  F.cam = g.cam[0]; F.fgeo = g;
  for (int l = 0; l < levels; l++) F.kcam[l] = kc[l];
  F.have_frame = true; F.have_depth = true;
  return RPE_OK;
}

int rpe_frame_download_level(rpe_context* c, int which, int level, float* out) {
  session_end(c);
  if (!c || !out || which < 0 || which > RPE_MAP_DEPTH) return fail(RPE_ERR_ARG, "rpe_frame_download_level: bad argument");
  auto& F = c->fe;
  const bool model = which == RPE_MAP_MODEL_VERTEX || which == RPE_MAP_MODEL_NORMAL;
  if (model ? !F.have_model : !F.have_frame) return fail(RPE_ERR_STATE, model ? "no model" : "no frame");
  const rpe::PyramidGeometry& g = model ? F.mgeo : F.fgeo;
  if (level < 0 || level >= g.levels)
    return fail(RPE_ERR_ARG, "rpe_frame_download_level: level %d of a %d-level %s", level, g.levels, model ? "model" : "frame");
  if (which == RPE_MAP_DEPTH && !F.have_depth)
    return fail(RPE_ERR_STATE, "no metric depth: the frame was set by rpe_frame_set_depth, not rpe_frame_set_depth_pyramid");
  const size_t n = (size_t)g.cam[level].width * g.cam[level].height;
  const float* src = which == RPE_MAP_DEPTH ? F.fdepth + g.off[level]
                     : (model ? F.mmap[which - RPE_MAP_MODEL_VERTEX] : F.fmap[which]) + 3 * g.off[level];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, src, n * (which == RPE_MAP_DEPTH ? 1 : 3) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_frame_level_camera(rpe_context* c, int level, int model, rpe_camera* out) {
  if (!c || !out) return fail(RPE_ERR_ARG, "rpe_frame_level_camera: bad argument");
  auto& F = c->fe;
  if (model ? !F.have_model : !F.have_frame) return fail(RPE_ERR_STATE, model ? "no model" : "no frame");
  const int levels = model ? F.mgeo.levels : F.fgeo.levels;
  if (level < 0 || level >= levels)
    return fail(RPE_ERR_ARG, "rpe_frame_level_camera: level %d of a %d-level %s", level, levels, model ? "model" : "frame");
  *out = model ? F.mkcam[level] : F.kcam[level];
  return RPE_OK;
}

int rpe_frame_download(rpe_context* c, int which, float* out) {
  session_end(c);
  if (!c || !out || which < 0 || which > RPE_MAP_MODEL_NORMAL) return fail(RPE_ERR_ARG, "rpe_frame_download: bad argument");
  auto& F = c->fe;
  const bool model = which >= RPE_MAP_MODEL_VERTEX;
  if (model ? !F.have_model : !F.have_frame) return fail(RPE_ERR_STATE, model ? "no model" : "no frame");
  const rpe::Camera& k = model ? F.mcam : F.cam;
  const float* src = model ? F.mmap[which - RPE_MAP_MODEL_VERTEX] : F.fmap[which];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, src, (size_t)k.width * k.height * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_model_from_frame(rpe_context* c, const double* pose12) {
  session_end(c);
  if (!c || !pose12) return fail(RPE_ERR_ARG, "rpe_model_from_frame: bad argument");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = F.fgeo.off[F.fgeo.levels];   // every level (one level: width * height)
  int rc = model_room(c, n);
  if (rc) return rc;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(rpe::launch_to_world(F.fmap[0], F.fmap[1], n, pose_f(pose12), F.mmap[0], F.mmap[1], c->stream));
  F.mcam = F.cam;
  F.mgeo = F.fgeo;
  for (int l = 0; l < RPE_MAX_LEVELS; l++) F.mkcam[l] = F.kcam[l];
  std::memcpy(F.mpose, pose12, sizeof(F.mpose));
  F.have_model = true;
  return RPE_OK;
}

int rpe_model_upload(rpe_context* c, const float* vertex_w, const float* normal_w, const rpe_camera* cam, const double* pose12) {
  session_end(c);
  if (!c || !vertex_w || !normal_w || !pose12) return fail(RPE_ERR_ARG, "rpe_model_upload: bad argument");
  rpe::Camera k;
  int rc = camera_of(cam, &k);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  const int64_t n = (int64_t)k.width * k.height;
  if ((rc = model_room(c, n))) return rc;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.mmap[0], vertex_w, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(F.mmap[1], normal_w, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the caller may free its buffers on return
  F.mcam = k;
  one_level(*cam, k, F.mkcam, &F.mgeo);
  std::memcpy(F.mpose, pose12, sizeof(F.mpose));
  F.have_model = true;
  return RPE_OK;
}

int rpe_model_build_pyramid(rpe_context* c, int levels) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_from_frame or rpe_model_upload first");
  rpe_camera kc[RPE_MAX_LEVELS];
  rpe::PyramidGeometry g;
  int rc = plan_levels(F.mkcam[0], levels, kc, &g);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)g.off[levels] * 3 * sizeof(float);
  if (F.mmap[0].bytes() < bytes) {   // grow, keeping level 0
    const size_t keep = (size_t)g.cam[0].width * g.cam[0].height * 3 * sizeof(float);
    const DevMem::Grow grow[] = {{&F.mmap[0], keep, bytes}, {&F.mmap[1], keep, bytes}};
    if ((rc = DevMem::regrow(c, "model pyramid", grow))) return rc;
  }
  F.photo_levels = 0;   // the model's levels move: the photometric map is laid out by them
  HIP_TRY(rpe::launch_model_pyramid(g, F.mmap[0], F.mmap[1], c->stream));
  F.mgeo = g;
  for (int l = 0; l < levels; l++) F.mkcam[l] = kc[l];
  return RPE_OK;
}

int rpe_associate(rpe_context* c, const double* pose12, double dist_thr, double cos_thr, int use_normals, int64_t* matched) {
  session_end(c);
  int rc = associate_ready(c);
  if (rc) return rc;
  if (!pose12 || !(dist_thr >= 0)) return fail(RPE_ERR_ARG, "rpe_associate: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = claim_slots(c, (int64_t)c->fe.cam.width * c->fe.cam.height))) return rc;
  if ((rc = associate_launch(c, level_of(c, 0), pose12, dist_thr, cos_thr, use_normals, false, matched != nullptr))) return rc;
  // read-out without a D2H copy or a stream synchronisation: a tiny kernel stores the counter into pinned host memory and raises a
  // sequence word
  if (matched) {
    const unsigned long long seq = ++c->vote_seq;
    HIP_TRY(rpe::launch_publish_i32(c->fe.d_count, 1, c->h_votes, c->h_flag2, seq, c->stream));
    if ((rc = wait_flag(c, c->h_flag2, seq))) return rc;
    *matched = c->h_votes[0];
  }
  return RPE_OK;
}

namespace {
// the loop of rpe_icp on one pyramid level (o->max_iter rounds, gate o->dist_thr) after claim_slots(c, lv.n); leave_pairs: a fused
// loop re-pairs under the returned pose at the end, so that the slots hold those pairs
int icp_level(rpe_context* c, const rpe_icp_options* o, const Level& lv, bool leave_pairs, double* pose12, int* iters_out,
              double* last_step, double* final_cost, int64_t* matched) {
  int rc = RPE_OK;
  GnRun run;   // run.weight: the pairs of the last round (the record's weight sum)
  bool host_rounds = false;
  const int64_t n = lv.n;
  const float dgate = (float)o->dist_thr;
  // one round's kernels, enqueued on the context's stream
  auto round = [&](const double* pose, const rpe::ReduceTarget& rt, bool pose_on_device) -> int {
    if (o->fused) {
      HIP_TRY(rpe::launch_icp_fused(lv.f[0], lv.f[1], n, lv.m[0], lv.m[1], lv.mcam, pose_f(c->fe.mpose), dgate * dgate,
          (float)o->cos_thr,
                                    o->use_normals, o->kind, pose, rt, c->stream));
      return RPE_OK;
    }
    int r = associate_launch(c, lv, pose, o->dist_thr, o->cos_thr, o->use_normals, pose_on_device, false);
    if (r) return r;
    HIP_TRY(rpe::launch_normal_eq(c->arrays(), o->kind, 0, pose, rt, c->stream));
    return RPE_OK;
  };
  if (o->device_resident) {
    rpe::GnState st;
    st.tol = o->tol; st.step = 0; st.cost = 0; st.max_iters = o->max_iter; st.iters = 0; st.done = 0; st.status = 0;
    HIP_TRY(hipMemcpyAsync(c->d_gn_pose, pose12, 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_gn_state, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
    rpe::ReduceTarget rt = host_target(c);
    rt.gn_pose = c->d_gn_pose; rt.gn = c->d_gn_state;
    static const bool auto_on = !(getenv("RPE_DEVICE_LOOP_RESIDENT") && atoi(getenv("RPE_DEVICE_LOOP_RESIDENT")) == 0);
    const bool want_auto = auto_on && c->resident && o->fused && o->max_iter >= 2 && !c->hostex && !c->comm && c->p2p_world < 1;
    // the device's resident slot until the result has arrived (end of this block's scope); a session in the slot: one launch per round
    std::unique_ptr<SlotHold> one_resident_grid(want_auto ? new SlotHold(resident_mutex(c->device)) : nullptr);
    bool one_launch = false;
    if (want_auto && *one_resident_grid) {
      // ONE launch: the resident grid pairs, sums, solves and updates by itself (icp_resident_kernel with resident_auto_stage)
      one_launch = true;
      int grid = 0, nacc = 0, max_rows = 1, rows_auto = 1;
      rpe::icp_resident_geometry(n, o->kind, c->max_blocks, &grid, &nacc, &max_rows, &rows_auto);
      const unsigned long long base = c->seq;
      (void)resident_run_shape(grid, nacc, max_rows, rows_auto, &rt);
      c->seq = base + (unsigned long long)o->max_iter + 1;
      rt.seq = c->seq;
      HIP_TRY(rpe::launch_icp_resident(lv.f[0], lv.f[1], n, lv.m[0], lv.m[1], lv.mcam, pose_f(c->fe.mpose), dgate * dgate,
          (float)o->cos_thr, o->use_normals,
                                       o->kind, nullptr, base, o->max_iter, rt, c->stream));
    } else {
      for (int k = 0; k < o->max_iter; k++) if ((rc = round(pose12, rt, true))) return rc;
    }
    if ((rc = wait_host(c, rpe::kNeLd))) return rc;
    if (one_launch && c->h_out[15] == 2.0) {
      // a workgroup's sums never arrived (the grid was not all resident at once): once more from the start pose, one launch per round
      note_lost_grid(c);
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipMemcpyAsync(c->d_gn_pose, pose12, 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(c->d_gn_state, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
      rt = host_target(c);
      rt.gn_pose = c->d_gn_pose; rt.gn = c->d_gn_state;
      for (int k = 0; k < o->max_iter; k++) if ((rc = round(pose12, rt, true))) return rc;
      if ((rc = wait_host(c, rpe::kNeLd))) return rc;
    }
    for (int i = 0; i < 12; i++) pose12[i] = c->h_out[i];
    run.step = c->h_out[12]; run.cost = c->h_out[13]; run.it = (int)c->h_out[14]; run.weight = c->h_out[16];
    if (c->h_out[15] == 2.0) { if (iters_out) *iters_out = run.it; return fail(RPE_ERR_HIP,
        "ICP device loop: a workgroup's sums never arrived at iteration %d", run.it); }
    if (c->h_out[15] != 0.0) { if (iters_out) *iters_out = run.it; return fail(RPE_ERR_DEGENERATE,
        "ICP: normal equations are not positive definite at iteration %d", run.it - 1); }
  } else if (o->fused && c->resident && c->host_resident && o->max_iter >= 2 && !c->hostex && !c->comm && c->p2p_world_saved < 1) {
    // host-driven ICP in ONE launch: the frame's pixels stay in registers, every iteration the host hands the pose over, the grid pairs
    // its pixels with the model under that pose and sends the run records back (rpe_icp.hip icp_resident_kernel)
    int grid = 0, nacc = 0, max_rows = 1, rows_auto = 1;
    rpe::icp_resident_geometry(n, o->kind, c->max_blocks, &grid, &nacc, &max_rows, &rows_auto);
    auto launch = [&](const rpe::ReduceTarget& rt, unsigned long long base) -> hipError_t {
      return rpe::launch_icp_resident(lv.f[0], lv.f[1], n, lv.m[0], lv.m[1], lv.mcam, pose_f(c->fe.mpose), dgate * dgate,
          (float)o->cos_thr, o->use_normals,
                                      o->kind, (const unsigned long long*)c->ctl, base, o->max_iter, rt, c->stream);
    };
    { SlotHold one_resident_grid(resident_mutex(c->device));
      if (!one_resident_grid) rc = kResidentBusy;   // (a session holds the slot: every round a launch)
      else rc = resident_host_loop(c, launch, grid, nacc, max_rows, rows_auto, 1.0, pose12, o->max_iter, o->tol, &run.it, &run.step, &run.cost,
          &run.weight, "ICP: normal equations"); }
    if (rc != RPE_OK && rc != kResidentLost && rc != kResidentBusy) { if (iters_out) *iters_out = run.it; return rc; }
    host_rounds = rc == kResidentLost || rc == kResidentBusy;   // the grid was lost after `it` whole rounds (or never launched): the rest one launch per round
  } else host_rounds = true;
  if (host_rounds) {
    rc = gn_host_rounds([&](const double* pose, double* ne) -> int {
      int r = round(pose, collect_target(c), false);
      if (r || (r = wait_host(c, rpe::kNeLd))) return r;
      for (int i = 0; i < 32; i++) ne[i] = c->h_out[i];
      return RPE_OK;
    }, rpe::pivot_floor(c->dtype == RPE_F64), 1.0, o->max_iter, o->tol, pose12, &run);
    if (rc == kGnRefused) {
      if (iters_out) *iters_out = run.it;
      return fail(RPE_ERR_DEGENERATE, "ICP: normal equations are not positive definite at iteration %d (%g pairs)", run.it, run.weight);
    }
    if (rc) return rc;
  }
  // leave the pairs in the slots
  if (leave_pairs && o->fused && (rc = associate_launch(c, lv, pose12, o->dist_thr, o->cos_thr, o->use_normals, false, false))) return rc;
  run.report(iters_out, last_step, final_cost, matched);
  return RPE_OK;
}

}  // namespace

int rpe_icp(rpe_context* c, const rpe_icp_options* o, double* pose12, int* iters_out, double* last_step, double* final_cost,
    int64_t* matched) {
  session_end(c);
  int rc = associate_ready(c);
  if (rc) return rc;
  if (!o || !pose12 || o->max_iter < 1 || (o->kind != RPE_RES_P2P && o->kind != RPE_RES_P2PLANE) || !(o->dist_thr >= 0))
    return fail(RPE_ERR_ARG, "rpe_icp: bad options (kind must be RPE_RES_P2P or RPE_RES_P2PLANE, max_iter >= 1)");
  if (o->kind == RPE_RES_P2PLANE && !o->use_normals)
    return fail(RPE_ERR_ARG, "rpe_icp: point-to-plane needs use_normals = 1 (pairs without a frame normal would poison the sums)");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = claim_slots(c, (int64_t)c->fe.cam.width * c->fe.cam.height))) return rc;
  return icp_level(c, o, level_of(c, 0), true, pose12, iters_out, last_step, final_cost, matched);
}

int rpe_icp_pyramid(rpe_context* c, const rpe_icp_options* o, int levels, const int* iters_per_level, const double* dist_thr_per_level,
                    double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched) {
  session_end(c);
  int rc = associate_ready(c);
  if (rc) return rc;
  if (!o || !pose12 || !iters_per_level || (o->kind != RPE_RES_P2P && o->kind != RPE_RES_P2PLANE) || !(o->dist_thr >= 0))
    return fail(RPE_ERR_ARG, "rpe_icp_pyramid: bad options (kind must be RPE_RES_P2P or RPE_RES_P2PLANE)");
  if (o->kind == RPE_RES_P2PLANE && !o->use_normals)
    return fail(RPE_ERR_ARG, "rpe_icp_pyramid: point-to-plane needs use_normals = 1");
  if ((rc = pyramid_complaint("rpe_icp_pyramid", levels, iters_per_level, dist_thr_per_level))) return rc;
  auto& F = c->fe;
  if (F.fgeo.levels < levels) return fail(RPE_ERR_STATE, "rpe_icp_pyramid: the frame has %d level(s), %d asked (rpe_frame_set_depth_pyramid)",
      F.fgeo.levels, levels);
  if (F.mgeo.levels < levels) return fail(RPE_ERR_STATE, "rpe_icp_pyramid: the model has %d level(s), %d asked (rpe_model_from_frame of a "
      "pyramid frame, or rpe_model_build_pyramid)", F.mgeo.levels, levels);
  HIP_TRY(hipSetDevice(c->device));
  return coarse_to_fine(levels, iters_per_level, dist_thr_per_level, o->dist_thr, iters_out,
                        [&](int l, int rounds, double gate, bool fine, int* it) -> int {
    rpe_icp_options lo = *o;
    lo.max_iter = rounds; lo.dist_thr = gate;
    const Level lv = level_of(c, l);
    if (int r = claim_slots(c, lv.n)) return r;
    return icp_level(c, &lo, lv, fine, pose12, it, fine ? last_step : nullptr, fine ? final_cost : nullptr, fine ? matched : nullptr);
  });
}

}  // extern "C"
