// Part 3 of include/rgbd_pose_hip.h: keyframes (kernels in rpe_keyframe.hip).  The model side's features -- descriptors, and the world
// vertex and normal at every keypoint -- kept in a packed store that belongs to the context; one frame matched against all of them in
// one pass (rpe_keyframes_query: the host waits once, for the counts and the ranking); one keyframe's matches in the solver slots
// (rpe_keyframe_match); and rpe_relocalize_keyframes: the best-ranked candidates through rpe_run, the one with the most votes kept.
#include "rpe_graph.h"
using namespace rpeh;

namespace {
constexpr int64_t kStoreStep = 8 * (int64_t)rpe::kMaxKeypoints;                        // the store's first allocation, keypoints
constexpr int64_t kStoreMax = (int64_t)rpe::kMaxKeyframes * rpe::kMaxKeypoints;

// room for `more` keypoints behind the store's last: the store doubles (from kStoreStep keypoints, up to its bound)
int ensure_store(rpe_context* c, int more) {
  auto& K = c->kf;
  int rc;
  if ((rc = K.off.once(c, (rpe::kMaxKeyframes + 1) * sizeof(int))) || (rc = K.rank.once(c, 2 * rpe::kMaxKeyframes * sizeof(int)))) return rc;
  const int64_t need = K.used + more;
  if (need <= K.cap()) return RPE_OK;
  int64_t cap = std::max(K.cap(), kStoreStep);
  while (cap < need) cap *= 2;
  cap = std::min(cap, kStoreMax);
  const size_t u = (size_t)K.used, n = (size_t)cap;
  const DevMem::Grow g[] = {{&K.desc, 8 * u * sizeof(unsigned int), 8 * n * sizeof(unsigned int)},
                            {&K.xw, 3 * u * sizeof(float), 3 * n * sizeof(float)},
                            {&K.nw, 3 * u * sizeof(float), 3 * n * sizeof(float)},
                            {&K.xy, 2 * u * sizeof(int), 2 * n * sizeof(int)},
                            {&K.back, 0, n * sizeof(int)}};
  return DevMem::regrow(c, "keyframe storage", g);
}
// `rows` rows of RPE_MAX_KEYPOINTS ints in each of d1 / idx / d2 (nothing in them outlives a call that asks for more)
int ensure_rows(rpe_context* c, int rows) {
  auto& K = c->kf;
  if (rows <= K.rows_cap()) return RPE_OK;
  int cap = std::max(K.rows_cap(), 8);
  while (cap < rows) cap *= 2;
  cap = std::min(cap, rpe::kMaxKeyframes);
  const size_t bytes = (size_t)cap * rpe::kMaxKeypoints * sizeof(int);
  const DevMem::Grow g[] = {{&K.d1, 0, bytes}, {&K.idx, 0, bytes}, {&K.d2, 0, bytes}};
  return DevMem::regrow(c, "keyframe storage", g);
}
int new_keyframe(rpe_context* c, int kind, int count, const double* pose12, int width, int height, int* id) {
  auto& K = c->kf;
  if (K.meta.empty()) K.kind = kind;
  rpe_context::Keyframes::Meta m;
  m.off = (int)K.used; m.count = count; m.width = width; m.height = height;
  std::memcpy(m.pose, pose12, sizeof(m.pose));
  K.meta.push_back(m);
  K.used += count;
  const int k = (int)K.meta.size(), end = (int)K.used;
  if (k == 1) { const int zero = 0; HIP_TRY(hipMemcpyAsync(K.off, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream)); }
  HIP_TRY(hipMemcpyAsync(K.off + k, &end, sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));      // `end` and the caller's arrays are the host's again
  if (id) *id = k - 1;
  return RPE_OK;
}
int store_ready(rpe_context* c, const char* who) {
  if (c->kf.meta.empty()) return fail(RPE_ERR_STATE, "%s: the keyframe store is empty (rpe_keyframe_add)", who);
  if (!c->fe.feat[RPE_FEAT_FRAME].have) return fail(RPE_ERR_STATE, "%s: no features of the frame (rpe_features_detect)", who);
  if (c->fe.feat[RPE_FEAT_FRAME].kind != c->kf.kind)
    return fail(RPE_ERR_STATE, "%s: the frame's descriptors are of kind %d, the store's of kind %d (rpe_features_set_descriptor)", who,
                c->fe.feat[RPE_FEAT_FRAME].kind, c->kf.kind);
  return RPE_OK;
}
// a store has one kind of descriptor, its first keyframe's
int kind_fits(rpe_context* c, int kind, const char* who) {
  if (!c->kf.meta.empty() && c->kf.kind != kind)
    return fail(RPE_ERR_STATE, "%s: descriptors of kind %d, the store's are of kind %d (rpe_keyframes_clear starts another store)", who, kind,
                c->kf.kind);
  return RPE_OK;
}
// list A (na descriptors) against the store's keyframes 0 .. segs - 1: behind a cross-check the pass of the store's first `before`
// keypoints against A first (K.back), then K2 with the acceptance test `acc` -- rows of d1 / idx / d2, the pairs that pass counted
// per keyframe in K.rank
int best_with_counts(rpe_context* c, const unsigned int* desc_a, int na, int before, int segs, const rpe_match_options& o,
                     rpe::KeyframeAccept* acc) {
  auto& K = c->kf;
  int rc;
  if ((rc = ensure_rows(c, segs))) return rc;
  HIP_TRY(hipMemsetAsync(K.rank, 0, (size_t)segs * sizeof(int), c->stream));
  if (o.cross_check)
    HIP_TRY(rpe::launch_keyframe_best(K.desc, before, desc_a, nullptr, 0, 1, 0, na, rpe::KeyframeAccept{0, 1, 1, nullptr}, nullptr, K.back,
                                      nullptr, nullptr, c->stream));
  *acc = rpe::KeyframeAccept{o.max_dist, o.ratio_num, o.ratio_den, o.cross_check ? K.back.get() : nullptr};
  HIP_TRY(rpe::launch_keyframe_best(desc_a, na, K.desc, K.off, 0, segs, 0, 0, *acc, K.d1, K.idx, K.d2, K.rank, c->stream));
  return RPE_OK;
}
// the frame's keypoints against every keyframe: row k of d1 / idx / d2 = keyframe k's, counts | order in K.rank and on the host
int query(rpe_context* c, const rpe_match_options& o, int* counts, int* order) {
  auto& K = c->kf;
  const auto& A = c->fe.feat[RPE_FEAT_FRAME];
  const int n = (int)K.meta.size();
  int rc;
  rpe::KeyframeAccept acc;
  if ((rc = best_with_counts(c, A.desc, A.count, (int)K.used, n, o, &acc))) return rc;   // (the cross-check: the whole store against the frame)
  HIP_TRY(rpe::launch_keyframe_rank(K.rank, n, K.rank + n, c->stream));            // the order directly behind the n counts
  int host[2 * rpe::kMaxKeyframes];
  if ((rc = read_ints(c, K.rank, 2 * n, host))) return rc;
  std::memcpy(counts, host, (size_t)n * sizeof(int));
  std::memcpy(order, host + n, (size_t)n * sizeof(int));
  return RPE_OK;
}
// keyframe `id` in the model's place, from row `row` of d1 / idx / d2 (and K.back behind a cross-check): the accepted list in
// frame-keypoint order, the problem declared, the five slots filled
int match_from_row(rpe_context* c, int id, int row, const rpe_match_options& o, int* matches) {
  auto& F = c->fe;
  auto& K = c->kf;
  const auto& A = F.feat[RPE_FEAT_FRAME];
  const auto& M = K.meta[id];
  int rc;
  if ((rc = ensure_lists(c))) return rc;
  rpe::MatchLists L = F.mlist.view();
  const size_t r = (size_t)row * A.count;
  L.d1 = K.d1 + r; L.idx = K.idx + r; L.d2 = K.d2 + r; L.back = K.back + M.off;
  F.matches = -1;
  HIP_TRY(rpe::launch_feature_accept(L, A.count, o.max_dist, o.ratio_num, o.ratio_den, o.cross_check, F.fwork.ctl, c->stream));
  int m = 0;
  if ((rc = read_ints(c, F.fwork.ctl + rpe::kFeatCtlMatches, 1, &m))) return rc;
  if (m > 0) {
    if ((rc = claim_slots(c, m))) return rc;
    HIP_TRY(rpe::launch_keyframe_gather(L.mf, L.mm, m, A.pix, F.fmap[0], F.fmap[1], F.fmap[2], K.store(), M.off, (float*)c->arr[RPE_XW],
                                        (float*)c->arr[RPE_XC], (float*)c->arr[RPE_BV], (float*)c->arr[RPE_NW], (float*)c->arr[RPE_NC], c->stream));
  } else if ((rc = rpe_set_problem(c, 0, RPE_F32))) return rc;
  F.matches = m; F.match_gen[0] = A.gen; F.match_kf = id;
  if (matches) *matches = m;
  return RPE_OK;
}
// keyframe id's attachment slot with room for n pixels of depth (and of colour); what was attached is dropped
int attachment_room(rpe_context* c, int id, size_t n, bool color) {
  auto& K = c->kf;
  if (K.att.size() < K.meta.size()) K.att.resize(K.meta.size());
  auto& A = K.att[id];
  A.have_depth = A.have_color = false;
  int rc;   // (a fuse in flight may still read the old planes: reserve waits for the stream before one goes)
  if ((rc = A.z.reserve(c, n * sizeof(float))) || (color && (rc = A.rgba.reserve(c, n * 4)))) return rc;
  return RPE_OK;
}
}  // namespace

extern "C" {

int rpe_keyframe_add(rpe_context* c, int* id) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  const auto& S = F.feat[RPE_FEAT_MODEL];
  if (!F.have_model || !S.have) return fail(RPE_ERR_STATE, "rpe_keyframe_add: no features of the model (rpe_features_detect with RPE_FEAT_MODEL)");
  if ((int)c->kf.meta.size() >= RPE_MAX_KEYFRAMES) return fail(RPE_ERR_STATE, "rpe_keyframe_add: the store is full (%d keyframes)", RPE_MAX_KEYFRAMES);
  int rc;
  if ((rc = kind_fits(c, S.kind, "rpe_keyframe_add"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_store(c, S.count))) return rc;
  HIP_TRY(rpe::launch_keyframe_snapshot(S.count, S.pix, S.xy, S.desc, F.mmap[0], F.mmap[1], c->kf.store(), (int)c->kf.used, c->stream));
  return new_keyframe(c, S.kind, S.count, F.mpose, F.mcam.width, F.mcam.height, id);
}

int rpe_keyframe_add_host(rpe_context* c, int count, const int32_t* xy, const uint32_t* desc, const float* xw, const float* nw,
                          const double* pose12, int width, int height, int* id) {
  session_end(c);
  if (!c || !pose12 || count < 0 || count > RPE_MAX_KEYPOINTS || width < 1 || height < 1 || (count > 0 && (!xy || !desc || !xw || !nw)))
    return fail(RPE_ERR_ARG, "rpe_keyframe_add_host: bad argument (count 0 .. %d, width, height >= 1, pose12 and the four arrays not NULL)",
                RPE_MAX_KEYPOINTS);
  for (int k = 0; k < count; k++)
    if (xy[2 * k] < 0 || xy[2 * k] >= width || xy[2 * k + 1] < 0 || xy[2 * k + 1] >= height)
      return fail(RPE_ERR_ARG, "rpe_keyframe_add_host: keypoint %d at (%d, %d) is outside the %d x %d image", k, xy[2 * k], xy[2 * k + 1], width, height);
  if ((int)c->kf.meta.size() >= RPE_MAX_KEYFRAMES) return fail(RPE_ERR_STATE, "rpe_keyframe_add_host: the store is full (%d keyframes)", RPE_MAX_KEYFRAMES);
  int rc;
  if ((rc = kind_fits(c, c->fe.desc_kind, "rpe_keyframe_add_host"))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_store(c, count))) return rc;
  auto& K = c->kf;
  const size_t o = (size_t)K.used, n = (size_t)count;
  if (n) {
    HIP_TRY(hipMemcpyAsync(K.desc + 8 * o, desc, 8 * n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(K.xw + 3 * o, xw, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(K.nw + 3 * o, nw, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(K.xy + 2 * o, xy, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  return new_keyframe(c, c->fe.desc_kind, count, pose12, width, height, id);
}

int rpe_keyframe_info(rpe_context* c, int id, int* count, double* pose12, int* width, int* height) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (id < 0 || id >= (int)c->kf.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_info: no keyframe %d (%d in the store)", id, (int)c->kf.meta.size());
  const auto& M = c->kf.meta[id];
  if (count) *count = M.count;
  if (pose12) std::memcpy(pose12, M.pose, sizeof(M.pose));
  if (width) *width = M.width;
  if (height) *height = M.height;
  return RPE_OK;
}

int rpe_keyframe_download(rpe_context* c, int id, int32_t* xy, uint32_t* desc, float* xw, float* nw) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (id < 0 || id >= (int)c->kf.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_download: no keyframe %d (%d in the store)", id, (int)c->kf.meta.size());
  HIP_TRY(hipSetDevice(c->device));
  const auto& K = c->kf;
  const size_t o = (size_t)K.meta[id].off, n = (size_t)K.meta[id].count;
  int rc;
  if (n && xy && (rc = copy_to_host(c, xy, K.xy + 2 * o, 2 * n * sizeof(int)))) return rc;
  if (n && desc && (rc = copy_to_host(c, desc, K.desc + 8 * o, 8 * n * sizeof(unsigned int)))) return rc;
  if (n && xw && (rc = copy_to_host(c, xw, K.xw + 3 * o, 3 * n * sizeof(float)))) return rc;
  if (n && nw && (rc = copy_to_host(c, nw, K.nw + 3 * o, 3 * n * sizeof(float)))) return rc;
  return RPE_OK;
}

int rpe_keyframes_count(rpe_context* c, int* count) {
  if (!c || !count) return fail(RPE_ERR_ARG, "rpe_keyframes_count: bad argument");
  *count = (int)c->kf.meta.size();
  return RPE_OK;
}

int rpe_keyframes_descriptor(rpe_context* c, int* kind) {
  if (!c || !kind) return fail(RPE_ERR_ARG, "rpe_keyframes_descriptor: bad argument");
  *kind = c->kf.meta.empty() ? -1 : c->kf.kind;
  return RPE_OK;
}

// ---- attachments: a keyframe's level-0 depth (and colour) kept beside it, for rpe_volume_fuse_keyframes (rpe_rebuild_api.hip)
int rpe_keyframe_attach_frame(rpe_context* c, int id) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& K = c->kf;
  const auto& F = c->fe;
  if (id < 0 || id >= (int)K.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_attach_frame: no keyframe %d (%d in the store)", id, (int)K.meta.size());
  if (!F.have_frame) return fail(RPE_ERR_STATE, "rpe_keyframe_attach_frame: no frame (rpe_frame_set_depth)");
  if (F.cam.width != K.meta[id].width || F.cam.height != K.meta[id].height)
    return fail(RPE_ERR_ARG, "rpe_keyframe_attach_frame: the frame is %d x %d, keyframe %d is %d x %d", F.cam.width, F.cam.height, id,
                K.meta[id].width, K.meta[id].height);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)F.cam.width * F.cam.height;
  int rc = attachment_room(c, id, n, F.have_fcolor);
  if (rc) return rc;
  auto& A = K.att[id];
  HIP_TRY(rpe::launch_attach_pack(F.fmap[0], F.have_fcolor ? F.fcolor.get() : nullptr, (int64_t)n, A.z, A.rgba, c->stream));
  A.cam = F.cam; A.kcam = F.kcam[0];
  A.have_depth = true; A.have_color = F.have_fcolor;
  return RPE_OK;
}

int rpe_keyframe_attach_host(rpe_context* c, int id, const float* z, const uint8_t* rgba, const rpe_camera* cam) {
  session_end(c);
  if (!c || !z) return fail(RPE_ERR_ARG, "rpe_keyframe_attach_host: bad argument");
  auto& K = c->kf;
  if (id < 0 || id >= (int)K.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_attach_host: no keyframe %d (%d in the store)", id, (int)K.meta.size());
  rpe::Camera k;
  int rc = camera_of(cam, &k);
  if (rc) return rc;
  if (k.width != K.meta[id].width || k.height != K.meta[id].height)
    return fail(RPE_ERR_ARG, "rpe_keyframe_attach_host: the camera is %d x %d, keyframe %d is %d x %d", k.width, k.height, id, K.meta[id].width,
                K.meta[id].height);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)k.width * k.height;
  if ((rc = attachment_room(c, id, n, rgba != nullptr))) return rc;
  auto& A = K.att[id];
  HIP_TRY(hipMemcpyAsync(A.z, z, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (rgba) HIP_TRY(hipMemcpyAsync(A.rgba, rgba, n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));      // the caller's arrays are free again on return
  A.cam = k; A.kcam = *cam;
  A.have_depth = true; A.have_color = rgba != nullptr;
  return RPE_OK;
}

int rpe_keyframe_attachment_info(rpe_context* c, int id, int* have_depth, int* have_color, rpe_camera* cam) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const auto& K = c->kf;
  if (id < 0 || id >= (int)K.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_attachment_info: no keyframe %d (%d in the store)", id, (int)K.meta.size());
  const bool have = id < (int)K.att.size() && K.att[id].have_depth;
  if (have_depth) *have_depth = have ? 1 : 0;
  if (have_color) *have_color = have && K.att[id].have_color ? 1 : 0;
  if (cam) *cam = have ? K.att[id].kcam : rpe_camera{0, 0, 0, 0, 0, 0};
  return RPE_OK;
}

int rpe_keyframe_attachment_download(rpe_context* c, int id, float* z, uint8_t* rgba) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const auto& K = c->kf;
  if (id < 0 || id >= (int)K.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_attachment_download: no keyframe %d (%d in the store)", id, (int)K.meta.size());
  const bool have = id < (int)K.att.size() && K.att[id].have_depth;
  if (z && !have) return fail(RPE_ERR_STATE, "rpe_keyframe_attachment_download: keyframe %d has no depth attached (rpe_keyframe_attach_frame)", id);
  if (rgba && !(have && K.att[id].have_color)) return fail(RPE_ERR_STATE, "rpe_keyframe_attachment_download: keyframe %d has no colour attached", id);
  if (!z && !rgba) return RPE_OK;
  HIP_TRY(hipSetDevice(c->device));
  const auto& A = K.att[id];
  const size_t n = (size_t)A.cam.width * A.cam.height;
  int rc;
  if (z && (rc = copy_to_host(c, z, A.z, n * sizeof(float)))) return rc;
  if (rgba && (rc = copy_to_host(c, rgba, A.rgba, n * 4))) return rc;
  return RPE_OK;
}

int rpe_keyframes_clear(rpe_context* c) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& A : c->kf.att) A.have_depth = A.have_color = false;   // the planes stay, for the next keyframe of that id
  c->kf.meta.clear();
  c->kf.used = 0;                                  // the storage stays, for the next map
  c->kf.kind = -1;
  if (c->fe.match_kf >= 0) { c->fe.matches = -1; c->fe.match_kf = -1; }
  graph_drop_from(c, 0);                           // the graph's edges named these keyframes
  return RPE_OK;
}

// The graph's edges from the store's own matcher (the graph itself: rpe_graph_api.hip).  Per newer keyframe j: the cross-check (every
// keypoint of the keyframes before j against j's list), K2 with A = j's rows of the store and the segments 0 .. j - 1 -- j rows of
// d1 / idx / d2, never the whole K x K --, ONE host wait for the j counts, room for the kept pairs, and G1 that writes them at the offsets the host hands it.
int rpe_keyframes_link(rpe_context* c, int first, const rpe_match_options* mopt, int min_matches, int* edges, int64_t* pairs) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const rpe_match_options o = mopt ? *mopt : kMatchDefaults;
  int rc = match_options(&o);
  if (rc) return rc;
  auto& K = c->kf;
  const int n = (int)K.meta.size();
  if (n == 0) return fail(RPE_ERR_STATE, "rpe_keyframes_link: the keyframe store is empty (rpe_keyframe_add)");
  if (first < 0 || first > n || min_matches < 3 || min_matches > RPE_MAX_KEYPOINTS)
    return fail(RPE_ERR_ARG, "rpe_keyframes_link: first 0 .. %d (got %d), min_matches 3 .. %d (got %d)", n, first, RPE_MAX_KEYPOINTS, min_matches);
  HIP_TRY(hipSetDevice(c->device));
  rpe_graph* G = graph_of(c);
  graph_drop_from(c, first);
  for (int j = std::max(first, 1); j < n; j++) {
    const auto& M = K.meta[j];
    if (M.count == 0 || M.off == 0) continue;      // no keypoint of its own, or none before it
    rpe::KeyframeAccept acc;
    if ((rc = best_with_counts(c, K.desc + 8 * (size_t)M.off, M.count, M.off, j, o, &acc))) return rc;
    int counts[rpe::kMaxKeyframes];
    if ((rc = read_ints(c, K.rank, j, counts))) return rc;
    int64_t total = 0;
    for (int i = 0; i < j; i++) if (counts[i] >= min_matches) total += counts[i];
    if (total == 0) continue;
    if (G->used + total > kGraphMaxPairs) return fail(RPE_ERR_STATE, "rpe_keyframes_link: more than 2^30 pairs");
    if ((rc = graph_reserve(c, total))) return rc;
    // where each kept edge's pairs go (-1: the edge is dropped): handed to G1 by value, so nothing is uploaded or waited for
    rpe::GraphBases base;
    for (int i = 0; i < j; i++) {
      base.v[i] = -1;
      if (counts[i] >= min_matches) { base.v[i] = (int)G->used; G->edges.push_back(rpe_graph::Edge{j, i, (int)G->used, counts[i]}); G->used += counts[i]; }
    }
    HIP_TRY(rpe::launch_graph_pack(K.d1, K.idx, K.d2, M.count, j, K.off, acc, K.rank, base, G->a, G->b, c->stream));
  }
  G->dirty = true;
  if (edges) *edges = (int)G->edges.size();
  if (pairs) *pairs = G->pairs();
  return RPE_OK;
}

int rpe_keyframes_query(rpe_context* c, const rpe_match_options* mopt, int* counts, int* order) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const rpe_match_options o = mopt ? *mopt : kMatchDefaults;
  int rc = match_options(&o);
  if (rc || (rc = store_ready(c, "rpe_keyframes_query"))) return rc;   // an empty store has no K ints to ask room for: the state first
  if (!counts || !order) return fail(RPE_ERR_ARG, "rpe_keyframes_query: counts and order must not be NULL");
  HIP_TRY(hipSetDevice(c->device));
  return query(c, o, counts, order);
}

int rpe_keyframe_match(rpe_context* c, int id, const rpe_match_options* mopt, int* matches) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const rpe_match_options o = mopt ? *mopt : kMatchDefaults;
  int rc = match_options(&o);
  if (rc || (rc = store_ready(c, "rpe_keyframe_match"))) return rc;
  auto& K = c->kf;
  if (id < 0 || id >= (int)K.meta.size()) return fail(RPE_ERR_ARG, "rpe_keyframe_match: no keyframe %d (%d in the store)", id, (int)K.meta.size());
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_rows(c, 1))) return rc;
  const auto& A = c->fe.feat[RPE_FEAT_FRAME];
  const auto& M = K.meta[id];
  c->fe.matches = -1;
  HIP_TRY(rpe::launch_keyframe_best(A.desc, A.count, K.desc, K.off, id, 1, 0, 0, rpe::KeyframeAccept{0, 1, 1, nullptr}, K.d1, K.idx, K.d2,
                                    nullptr, c->stream));
  if (o.cross_check)
    HIP_TRY(rpe::launch_keyframe_best(K.desc + 8 * (size_t)M.off, M.count, A.desc, nullptr, 0, 1, 0, A.count, rpe::KeyframeAccept{0, 1, 1, nullptr},
                                      nullptr, K.back + M.off, nullptr, nullptr, c->stream));
  return match_from_row(c, id, 0, o, matches);
}

int rpe_relocalize_keyframes(rpe_context* c, const rpe_feature_options* fopt, const rpe_match_options* mopt, int candidates, int method,
                             double thre_3d, double thre_2d, double thre_nl, int* iter_io, double confidence, uint64_t seed, int ls,
                             int min_matches, double* pose12, int* keyframe, int* matches, int* max_votes, short* mask_out) {
  session_end(c);
  if (!c || !pose12 || !iter_io || method < 0 || method > 9 || candidates < 1)
    return fail(RPE_ERR_ARG, "rpe_relocalize_keyframes: bad argument (method 0 .. 9, candidates >= 1, pose12 and iter_io not NULL)");
  if (min_matches < 4 || min_matches > RPE_MAX_KEYPOINTS) return fail(RPE_ERR_ARG, "rpe_relocalize_keyframes: min_matches 4 .. %d (got %d)",
                                                                     RPE_MAX_KEYPOINTS, min_matches);
  const rpe_feature_options fo = fopt ? *fopt : kFeatureDefaults;
  const rpe_match_options mo = mopt ? *mopt : kMatchDefaults;
  int rc;
  if ((rc = match_options(&mo)) || (rc = feature_options(&fo))) return rc;
  auto& K = c->kf;
  if (K.meta.empty()) return fail(RPE_ERR_STATE, "rpe_relocalize_keyframes: the keyframe store is empty (rpe_keyframe_add)");
  if (c->fe.desc_kind != K.kind)
    return fail(RPE_ERR_STATE, "rpe_relocalize_keyframes: the context describes with kind %d, the store's descriptors are of kind %d "
                "(rpe_features_set_descriptor)", c->fe.desc_kind, K.kind);
  if ((rc = detect_if_stale(c, RPE_FEAT_FRAME, fo))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const int n = (int)K.meta.size();
  std::vector<int> counts(n), order(n);
  c->fe.matches = -1;
  if ((rc = query(c, mo, counts.data(), order.data()))) return rc;
  if (keyframe) *keyframe = order[0];
  if (matches) *matches = counts[order[0]];
  if (counts[order[0]] < min_matches)
    return fail(RPE_ERR_DEGENERATE, "rpe_relocalize_keyframes: the best keyframe (%d) has %d matches, %d needed (%d keyframes)", order[0],
                counts[order[0]], min_matches, n);
  const int iter_in = *iter_io;
  int win = -1, win_votes = -1, win_iter = iter_in, win_m = 0, last = -1;
  double win_pose[12];
  std::vector<short> win_mask, mask;
  for (int r = 0; r < n && r < candidates && counts[order[r]] >= min_matches; r++) {
    const int id = order[r];
    int m = 0;
    if ((rc = match_from_row(c, id, id, mo, &m))) return rc;
    last = id;
    // rpe_relocalize's own run: the downloaded arrays through rpe_run, the match quality as weight of every modality
    double pose[12];
    int it = iter_in, votes = 0;
    mask.assign((size_t)m * 3, 0);
    rc = run_on_slots(c, m, method, thre_3d, thre_2d, thre_nl, &it, confidence, seed, ls, pose, &votes, mask.data());
    if (rc == RPE_ERR_DEGENERATE) continue;        // refused as rank-deficient: the next candidate
    if (rc) return rc;
    if (votes > win_votes) {                       // a tie stays with the better rank
      win = id; win_votes = votes; win_iter = it; win_m = m;
      std::memcpy(win_pose, pose, sizeof(win_pose));
      win_mask.swap(mask);
    }
  }
  if (win < 0) return fail(RPE_ERR_DEGENERATE, "rpe_relocalize_keyframes: every candidate's matches were refused as rank-deficient");
  if (last != win && (rc = match_from_row(c, win, win, mo, nullptr))) return rc;   // slots and match list are the winner's
  std::memcpy(pose12, win_pose, sizeof(win_pose));
  *iter_io = win_iter;
  if (keyframe) *keyframe = win;
  if (matches) *matches = win_m;
  if (max_votes) *max_votes = win_votes;
  if (mask_out) std::memcpy(mask_out, win_mask.data(), win_mask.size() * sizeof(short));
  return RPE_OK;
}

}  // extern "C"
