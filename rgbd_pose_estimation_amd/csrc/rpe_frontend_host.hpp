// What the Part 3 units of the C ABI share on the host (rpe_host.hpp lists the units): camera and pose casts, the solver slots a
// device-side producer writes, and the single copies of what the feature, keyframe, colour and rebuild units have in common, each
// defined in the unit that owns it.  Everything is internal to the library (namespace rpeh, hidden visibility).
#pragma once
#include "rpe_host.hpp"

namespace rpeh __attribute__((visibility("hidden"))) {

// an rpe_camera validated and cast to the kernels' fp32 camera
inline int camera_of(const rpe_camera* cam, rpe::Camera* out) {
  if (!cam || cam->width < 1 || cam->height < 1 || !(cam->fx > 0) || !(cam->fy > 0)
      || (int64_t)cam->width * cam->height > (int64_t)1 << 28)
    return fail(RPE_ERR_ARG, "bad camera (need width, height >= 1 and fx, fy > 0)");
  out->fx = (float)cam->fx; out->fy = (float)cam->fy; out->cx = (float)cam->cx; out->cy = (float)cam->cy;
  out->width = cam->width; out->height = cam->height;
  return RPE_OK;
}
using rpe::pose_f;   // (rpe_kernels.h: the one pose cast, the launchers' too)
// the solver slots a device-side producer writes (association, feature matches): the context's own storage, n columns, fp32
// (rpe_frontend_api.hip)
int claim_slots(rpe_context* c, int64_t n);
// room for n pixels in each of the model's two maps, content not kept (rpe_frontend_api.hip)
int model_room(rpe_context* c, int64_t n);
// the one-level pyramid of a single image (rpe_frame_set_depth, rpe_model_upload, rpe_volume_raycast)
inline void one_level(const rpe_camera& k, const rpe::Camera& f, rpe_camera* kc, rpe::PyramidGeometry* g) {
  *g = rpe::PyramidGeometry{};
  g->levels = 1; g->cam[0] = f; kc[0] = k;
  for (int l = 1; l <= RPE_MAX_LEVELS; l++) g->off[l] = (int64_t)f.width * f.height;
}
// one pyramid level of frame and model: maps (frame vertex, normal, bearing; model vertex, normal), pixels, model camera (level 0 = the
// single-level front end).  A side that is not there yields pointers nobody reads
struct Level { const float* f[3]; const float* m[2]; int64_t n; rpe::Camera mcam; };
inline Level level_of(rpe_context* c, int l) {
  auto& F = c->fe;
  Level L;
  for (int k = 0; k < 3; k++) L.f[k] = F.fmap[k] + 3 * F.fgeo.off[l];
  for (int k = 0; k < 2; k++) L.m[k] = F.mmap[k] + 3 * F.mgeo.off[l];
  L.n = (int64_t)F.fgeo.cam[l].width * F.fgeo.cam[l].height;
  L.mcam = F.mgeo.cam[l];
  return L;
}
// pyramid_args (rpe_gn_host.hpp) worded for the coarse-to-fine entry point `who`: RPE_ERR_ARG, or RPE_OK
inline int pyramid_complaint(const char* who, int levels, const int* iters_per_level, const double* dist_thr_per_level) {
  int l = 0;
  switch (pyramid_args(levels, iters_per_level, dist_thr_per_level, &l)) {
    case kPyramidLevels: return fail(RPE_ERR_ARG, "%s: levels must be 1 .. %d (got %d)", who, RPE_MAX_LEVELS, levels);
    case kPyramidRounds: return fail(RPE_ERR_ARG, "%s: level %d needs %s rounds (got %d)", who, l, l == 0 ? ">= 1" : ">= 0", iters_per_level[l]);
    case kPyramidGate: return fail(RPE_ERR_ARG, "%s: bad distance gate at level %d", who, l);
    case kPyramidOk: break;
  }
  return RPE_OK;
}

// ---- what the one-launch rounds and the rows calls of rpe_photo_api.hip and rpe_sdf_api.hip share
// the round's record as wait_host left it in c->h_out: H | g | cost | weight into ne[0 .. 28], zeros behind
inline void round_record(const rpe_context* c, double* ne) {
  for (int i = 0; i < 32; i++) ne[i] = i < 29 ? c->h_out[i] : 0.0;
}
// the record of a photometric-only round as the ..._normal_eq calls return it: H | g of ne, the photometric cost and rows in the places
// of the geometric ones, and the pivot floor for rpe_gn_solve (the rows' products are fp32)
inline void photo_only_record(const double* ne, double pcost, double prows, double* out32) {
  for (int i = 0; i < 32; i++) out32[i] = i < 27 ? ne[i] : 0.0;
  out32[27] = pcost; out32[28] = prows;
  out32[29] = rpe::pivot_floor(false);
}
// the tail of a rows call behind its launch (`launched`: what the launcher returned): the (7, n) rows down to the caller, one host wait
// (planes = 1: the plane of weights of the robust volume terms' hook)
inline int rows_download(rpe_context* c, const char* who, hipError_t launched, const float* d_rows, int64_t n, float* rows, int planes = 7) {
  hipError_t e = launched;
  if (e == hipSuccess) e = hipMemcpyAsync(rows, d_rows, (size_t)n * planes * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  return RPE_OK;
}

// ---- the keyframe list of a fuse (rpe_volume_fuse_keyframes, rpe_volume_map_fuse_keyframes; `who` names the caller in the messages):
// ids = NULL lists every keyframe that carries depth, by id.  An id outside the store or a count outside 1 .. RPE_MAX_KEYFRAMES is
// RPE_ERR_ARG; a listed keyframe without depth -- or, with `color`, without colour -- and an empty store are RPE_ERR_STATE.  On success
// table holds one entry per list entry: the attachment, its camera and the pose it is fused at (poses12, or the store's)
inline int fuse_list(rpe_context* c, const char* who, const int32_t* ids, int count, const double* poses12, bool color,
                     std::vector<rpe::FuseEntry>& table) {
  auto& K = c->kf;
  const int stored = (int)K.meta.size();
  auto has_depth = [&](int id) { return id < (int)K.att.size() && K.att[id].have_depth; };
  int32_t all[RPE_MAX_KEYFRAMES];
  if (!ids) {
    count = 0;
    for (int id = 0; id < stored; id++) if (has_depth(id)) all[count++] = id;
    if (count == 0) return fail(RPE_ERR_STATE, "%s: no keyframe has depth attached (rpe_keyframe_attach_frame)", who);
    ids = all;
  } else {
    if (count < 1 || count > RPE_MAX_KEYFRAMES) return fail(RPE_ERR_ARG, "%s: count 1 .. %d (got %d)", who, RPE_MAX_KEYFRAMES, count);
    for (int e = 0; e < count; e++)
      if (ids[e] < 0 || ids[e] >= stored) return fail(RPE_ERR_ARG, "%s: no keyframe %d (%d in the store)", who, ids[e], stored);
  }
  for (int e = 0; e < count; e++) {
    if (!has_depth(ids[e])) return fail(RPE_ERR_STATE, "%s: keyframe %d has no depth attached (rpe_keyframe_attach_frame)", who, ids[e]);
    if (color && !K.att[ids[e]].have_color) return fail(RPE_ERR_STATE, "%s: keyframe %d has no colour attached", who, ids[e]);
  }
  table.resize((size_t)count);
  for (int e = 0; e < count; e++) {
    const auto& A = K.att[ids[e]];
    table[e].z = A.z; table[e].rgba = color ? A.rgba.get() : nullptr; table[e].cam = A.cam;
    table[e].T = pose_f(poses12 ? poses12 + 12 * (size_t)e : K.meta[ids[e]].pose);
  }
  return RPE_OK;
}

// ---- rpe_color_api.hip
// the colour volume of the current volume: allocated on first use after rpe_volume_init, cleared to 0 unless `clear` is false (the
// caller overwrites every voxel)
int ensure_color_volume(rpe_context* c, bool clear);

// ---- rpe_feature_api.hip
extern const rpe_feature_options kFeatureDefaults;
extern const rpe_match_options kMatchDefaults;
int feature_options(const rpe_feature_options* o);   // the range check of either option struct (RPE_ERR_ARG)
int match_options(const rpe_match_options* o);
int ensure_lists(rpe_context* c);                    // c->fe.mlist, allocated on first use
// n ints a kernel left in device memory, through the pinned words every count of the front end takes: one host wait
int read_ints(rpe_context* c, const int* d_words, int n, int* out);
// rpe_features_detect on one side, unless that side was already detected with these options and the context's descriptor kind
int detect_if_stale(rpe_context* c, int which, const rpe_feature_options& fo);
// the m matches in the solver slots through rpe_run's own path, on the host-pointer form of the problem: five arrays of 3 x m floats
// down, the match quality as weight of every modality (m <= 4096: 240 KB at most).  pose12 is written on success only
int run_on_slots(rpe_context* c, int m, int method, double thre_3d, double thre_2d, double thre_nl, int* iter_io, double confidence,
                 uint64_t seed, int ls, double* pose12, int* max_votes, short* mask_out);

// ---- rpe_mapmesh_api.hip: the map -- the window plus the archived bricks -- for the calls that read a box of it
// what every such call asks of the context (`who` names the caller in the messages): a volume whose dims and total shift are multiples
// of 8 (RPE_ERR_STATE)
int map_state(const char* who, const rpe_context::Volume& V);
// the box's rules (RPE_ERR_ARG).  lo = NULL: the map's bounds.  On success G is the virtual volume's geometry and b0 / nb the box in bricks
int map_box(const char* who, const rpe_context::Volume& V, const int64_t* lo, const int64_t* hi, rpe::VolumeGeometry& G, int64_t b0[3],
            int64_t nb[3]);
// the brick grid (rpe_kernels.h MapRayView) of the box into h, one int32 per brick, and M's description of window and box; the caller
// refuses a box of more than kMaxGrid bricks first
constexpr int64_t kMaxGrid = (int64_t)1 << 24;
void build_grid(const rpe_context::Volume& V, const int64_t b0[3], const int64_t nb[3], std::vector<unsigned char>& h, rpe::MapRayView& M);
// the map's field inside the box (lo = NULL: the map's bounds), for the calls that track a frame against it (rpe_sdf_api.hip):
// the state and box rules of rpe_volume_map_raycast, then the brick grid built and uploaded ONCE, for every fetch
// and round of the call.  On success G is the virtual volume's geometry and M the view, both volumes and both planes of the pool
// included (null where there is none).  Nothing but the volume's map list is written
int map_field(rpe_context* c, const char* who, const int64_t* lo, const int64_t* hi, rpe::VolumeGeometry& G, rpe::MapRayView& M);

}  // namespace rpeh
