// Part 3 of include/rgbd_pose_hip.h: features and relocalisation (kernels in rpe_feature.hip).  Keypoints and descriptors of the frame
// and of the model view, their matches in the five solver slots, and rpe_relocalize: the matches through rpe_run -- a pose without a
// pose guess, for ICP to refine.  The host waits for one count per detection and one per match list.
#include "rpe_frontend_host.hpp"
using namespace rpeh;

namespace rpeh {
const rpe_feature_options kFeatureDefaults = {12, RPE_MAX_KEYPOINTS};
const rpe_match_options kMatchDefaults = {64, 8, 10, 0};
int feature_options(const rpe_feature_options* o) {
  if (o->threshold < 1 || o->threshold > 255 || o->max_keypoints < 1 || o->max_keypoints > RPE_MAX_KEYPOINTS)
    return fail(RPE_ERR_ARG, "feature options: threshold 1 .. 255 (got %d), max_keypoints 1 .. %d (got %d)", o->threshold, RPE_MAX_KEYPOINTS,
                o->max_keypoints);
  return RPE_OK;
}
int match_options(const rpe_match_options* o) {
  if (o->max_dist < 0 || o->max_dist > 256 || o->ratio_num < 1 || o->ratio_den < 1 || o->ratio_num > 65536 || o->ratio_den > 65536 ||
      (o->cross_check != 0 && o->cross_check != 1))
    return fail(RPE_ERR_ARG, "match options: max_dist 0 .. 256 (got %d), ratio_num / ratio_den 1 .. 65536 (got %d / %d), cross_check 0 or 1 (got %d)",
                o->max_dist, o->ratio_num, o->ratio_den, o->cross_check);
  return RPE_OK;
}
int ensure_lists(rpe_context* c) {
  auto& L = c->fe.mlist;
  int rc;
  for (DevBuf<int>* p : {&L.d1, &L.idx, &L.d2, &L.back, &L.mf, &L.mm, &L.md1, &L.md2})
    if ((rc = p->once(c, rpe::kMaxKeypoints * sizeof(int)))) return rc;
  return L.mw.once(c, rpe::kMaxKeypoints * sizeof(float));
}
int read_ints(rpe_context* c, const int* d_words, int n, int* out) {
  const unsigned long long seq = ++c->vote_seq;
  HIP_TRY(rpe::launch_publish_i32(d_words, n, c->h_votes, c->h_flag2, seq, c->stream));
  int rc = wait_flag(c, c->h_flag2, seq);
  if (rc) return rc;
  std::memcpy(out, c->h_votes, (size_t)n * sizeof(int));
  return RPE_OK;
}
int detect_if_stale(rpe_context* c, int which, const rpe_feature_options& fo) {
  const auto& S = c->fe.feat[which];
  if (S.have && S.threshold == fo.threshold && S.max_keypoints == fo.max_keypoints && S.kind == c->fe.desc_kind && S.levels == c->fe.levels)
    return RPE_OK;
  return rpe_features_detect(c, which, &fo, nullptr);
}
int run_on_slots(rpe_context* c, int m, int method, double thre_3d, double thre_2d, double thre_nl, int* iter_io, double confidence,
                 uint64_t seed, int ls, double* pose12, int* max_votes, short* mask_out) {
  const size_t n3 = (size_t)m * 3;
  std::vector<float> host(5 * n3 + 3 * (size_t)m);
  float* a[RPE_NUM_ARRAYS];
  int rc;
  for (int s = 0; s < RPE_NUM_ARRAYS; s++) {
    a[s] = host.data() + s * n3;
    if ((rc = copy_to_host(c, a[s], c->arr[s], n3 * sizeof(float)))) return rc;
  }
  float* wq = host.data() + 5 * n3;
  if ((rc = copy_to_host(c, wq, c->fe.mlist.mw, (size_t)m * sizeof(float)))) return rc;
  for (int k = 1; k < 3; k++) std::memcpy(wq + (size_t)k * m, wq, (size_t)m * sizeof(float));
  rpe_problem p{};
  p.n = m; p.dtype = RPE_F32;
  p.xw = a[RPE_XW]; p.xc = a[RPE_XC]; p.bv = a[RPE_BV]; p.nw = a[RPE_NW]; p.nc = a[RPE_NC];
  p.weights = wq; p.wcols = 3;
  p.fx = c->fe.kcam[0].fx; p.fy = c->fe.kcam[0].fy;
  double R9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t3[3] = {0, 0, 0};
  if ((rc = rpe_run(method, &p, thre_3d, thre_2d, thre_nl, iter_io, confidence, seed, ls, RPE_SCORE_EXACT, nullptr, R9, t3, max_votes, mask_out)))
    return rc;
  for (int i = 0; i < 9; i++) pose12[i] = R9[i];
  for (int i = 0; i < 3; i++) pose12[9 + i] = t3[i];
  return RPE_OK;
}
}  // namespace rpeh

namespace {
// the detector's workspace for the levels L of an image (one level: the image itself), and one side's keypoint arrays
// (RPE_MAX_KEYPOINTS slots, allocated on first use)
int ensure_work(rpe_context* c, const rpe::FeatLevels& L) {
  auto& W = c->fe.fwork;
  const size_t n = (size_t)L.base[rpe::kFeatMaxLevels];
  // no two 8-neighbours both survive the suppression, and nothing is suppressed across levels: at most ceil(w / 2) * ceil(h / 2)
  // survivors per level
  size_t survivors = 0;
  for (int l = 0; l < L.n; l++) survivors += ((size_t)L.w[l] * L.h[l] + L.w[l] + L.h[l] + 1) / 4 + 1;
  int rc;
  if ((rc = W.score.reserve(c, n * sizeof(int))) || (rc = W.box.reserve(c, n * sizeof(unsigned short))) ||
      (rc = W.chunk.reserve(c, (n / 256 + 2) * sizeof(int))) || (rc = W.spix.reserve(c, survivors * sizeof(int)))) return rc;
  if (L.n > 1 && ((rc = W.lum.reserve(c, n * sizeof(unsigned short))) || (rc = W.kidx.once(c, rpe::kMaxKeypoints * sizeof(int))))) return rc;
  if ((rc = W.hist.once(c, rpe::kFeatScoreBins * sizeof(unsigned int)))) return rc;
  return W.ctl.once(c, rpe::kFeatCtlWords * sizeof(int));
}
int ensure_side(rpe_context* c, int which, int levels) {
  auto& S = c->fe.feat[which];
  const size_t k = rpe::kMaxKeypoints;
  int rc;
  if ((rc = S.pix.once(c, k * sizeof(int))) || (rc = S.score.once(c, k * sizeof(int))) || (rc = S.xy.once(c, 2 * k * sizeof(int))) ||
      (rc = S.desc.once(c, 8 * k * sizeof(unsigned int)))) return rc;
  if (levels > 1 && ((rc = S.level.once(c, k * sizeof(int))) || (rc = S.lxy.once(c, 2 * k * sizeof(int))))) return rc;
  return S.bin.once(c, k * sizeof(int));
}
int no_features(int which) {
  return fail(RPE_ERR_STATE, "no features of the %s: call rpe_features_detect (a new depth, colour or model drops them)",
              which == RPE_FEAT_MODEL ? "model" : "frame");
}
int side_ready(rpe_context* c, int which) {
  auto& F = c->fe;
  if (which == RPE_FEAT_FRAME) {
    if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
    if (!F.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  } else {
    if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_model_upload, rpe_model_from_frame or rpe_volume_raycast first");
    if (!F.have_mcolor)
      return fail(RPE_ERR_STATE, "no model colour: call rpe_model_sample_color, rpe_model_color_upload or rpe_model_color_from_frame");
  }
  return RPE_OK;
}
bool matches_current(const rpe_context* c) {
  auto& F = c->fe;
  if (F.match_kf >= 0) return F.matches >= 0 && F.feat[0].have && F.match_gen[0] == F.feat[0].gen;   // rpe_keyframe_match's list
  return F.matches >= 0 && F.feat[0].have && F.feat[1].have && F.match_gen[0] == F.feat[0].gen && F.match_gen[1] == F.feat[1].gen;
}
}  // namespace

extern "C" {

int rpe_features_detect(rpe_context* c, int which, const rpe_feature_options* opt, int* count) {
  session_end(c);
  if (!c || (which != RPE_FEAT_FRAME && which != RPE_FEAT_MODEL)) return fail(RPE_ERR_ARG, "rpe_features_detect: bad argument");
  const rpe_feature_options o = opt ? *opt : kFeatureDefaults;
  int rc = feature_options(&o);
  if (rc) return rc;
  if ((rc = side_ready(c, which))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  auto& S = F.feat[which];
  const bool model = which == RPE_FEAT_MODEL;
  const rpe::Camera& k = model ? F.mcam : F.cam;
  const rpe::FeatLevels lv = rpe::feature_levels(k.width, k.height, F.levels);
  if ((rc = ensure_work(c, lv)) || (rc = ensure_side(c, which, F.levels))) return rc;
  S.have = false;
  const unsigned int* rgba = model ? F.mcolor : F.fcolor;
  const float *vmap = model ? F.mmap[0] : F.fmap[0], *nmap = model ? F.mmap[1] : F.fmap[1];
  if (F.levels == 1)      // one level is the stage as it was: the same six kernels on the image itself
    HIP_TRY(rpe::launch_feature_detect(rgba, vmap, nmap, k.width, k.height, o.threshold, o.max_keypoints, F.fwork.view(), F.desc_kind, S.pix,
                                       S.score, S.xy, S.desc, S.bin, c->stream));
  else
    HIP_TRY(rpe::launch_feature_detect_levels(rgba, vmap, nmap, lv, o.threshold, o.max_keypoints, F.fwork.view(), F.desc_kind, S.pix, S.score,
                                              S.xy, S.desc, S.bin, S.level, S.lxy, c->stream));
  if ((rc = read_ints(c, F.fwork.ctl + rpe::kFeatCtlCount, 1, &S.count))) return rc;
  S.have = true; S.gen++; S.threshold = o.threshold; S.max_keypoints = o.max_keypoints; S.kind = F.desc_kind; S.levels = F.levels;
  if (count) *count = S.count;
  return RPE_OK;
}

int rpe_features_download(rpe_context* c, int which, int32_t* xy, int32_t* score, uint32_t* desc) {
  session_end(c);
  if (!c || (which != RPE_FEAT_FRAME && which != RPE_FEAT_MODEL)) return fail(RPE_ERR_ARG, "rpe_features_download: bad argument");
  auto& S = c->fe.feat[which];
  if (!S.have) return no_features(which);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)S.count;
  int rc;
  if (n && xy && (rc = copy_to_host(c, xy, S.xy, n * 2 * sizeof(int)))) return rc;
  if (n && score && (rc = copy_to_host(c, score, S.score, n * sizeof(int)))) return rc;
  if (n && desc && (rc = copy_to_host(c, desc, S.desc, n * 8 * sizeof(unsigned int)))) return rc;
  return RPE_OK;
}

int rpe_features_set_descriptor(rpe_context* c, int kind) {
  session_end(c);
  if (!c || (kind != RPE_DESC_UPRIGHT && kind != RPE_DESC_ORIENTED))
    return fail(RPE_ERR_ARG, "rpe_features_set_descriptor: kind RPE_DESC_UPRIGHT or RPE_DESC_ORIENTED (got %d)", kind);
  auto& F = c->fe;
  if (kind == F.desc_kind) return RPE_OK;
  F.desc_kind = kind;                    // descriptors of two kinds never meet: both sides and the match list go
  F.feat[0].have = false; F.feat[1].have = false; F.matches = -1; F.match_kf = -1;
  return RPE_OK;
}

int rpe_features_get_descriptor(rpe_context* c, int* kind) {
  if (!c || !kind) return fail(RPE_ERR_ARG, "rpe_features_get_descriptor: bad argument");
  *kind = c->fe.desc_kind;
  return RPE_OK;
}

int rpe_features_set_levels(rpe_context* c, int levels) {
  session_end(c);
  if (!c || levels < 1 || levels > rpe::kFeatMaxLevels)
    return fail(RPE_ERR_ARG, "rpe_features_set_levels: levels 1 .. %d (got %d)", rpe::kFeatMaxLevels, levels);
  auto& F = c->fe;
  if (levels == F.levels) return RPE_OK;
  F.levels = levels;                     // ids and yields differ between ladders: both sides and the match list go
  F.feat[0].have = false; F.feat[1].have = false; F.matches = -1; F.match_kf = -1;
  return RPE_OK;
}

int rpe_features_get_levels(rpe_context* c, int* levels) {
  if (!c || !levels) return fail(RPE_ERR_ARG, "rpe_features_get_levels: bad argument");
  *levels = c->fe.levels;
  return RPE_OK;
}

int rpe_features_scale(rpe_context* c, int which, int32_t* level, int32_t* lxy) {
  session_end(c);
  if (!c || (which != RPE_FEAT_FRAME && which != RPE_FEAT_MODEL)) return fail(RPE_ERR_ARG, "rpe_features_scale: bad argument");
  auto& S = c->fe.feat[which];
  if (!S.have) return no_features(which);
  const size_t n = (size_t)S.count;
  if (!n) return RPE_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if (S.levels == 1) {                   // the image itself: level 0, and the level pixel is the keypoint's pixel
    if (level) std::memset(level, 0, n * sizeof(int32_t));
    return lxy ? copy_to_host(c, lxy, S.xy, n * 2 * sizeof(int)) : RPE_OK;
  }
  if (level && (rc = copy_to_host(c, level, S.level, n * sizeof(int)))) return rc;
  return lxy ? copy_to_host(c, lxy, S.lxy, n * 2 * sizeof(int)) : RPE_OK;
}

int rpe_features_angles(rpe_context* c, int which, int32_t* bins) {
  session_end(c);
  if (!c || (which != RPE_FEAT_FRAME && which != RPE_FEAT_MODEL)) return fail(RPE_ERR_ARG, "rpe_features_angles: bad argument");
  auto& S = c->fe.feat[which];
  if (!S.have) return no_features(which);
  const size_t n = (size_t)S.count;
  if (!n || !bins) return RPE_OK;
  if (S.kind != RPE_DESC_ORIENTED) { std::memset(bins, 0, n * sizeof(int32_t)); return RPE_OK; }   // an upright patch is not turned
  HIP_TRY(hipSetDevice(c->device));
  return copy_to_host(c, bins, S.bin, n * sizeof(int));
}

int rpe_features_match(rpe_context* c, const rpe_match_options* opt, int* matches) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const rpe_match_options o = opt ? *opt : kMatchDefaults;
  int rc = match_options(&o);
  if (rc) return rc;
  if ((rc = side_ready(c, RPE_FEAT_FRAME)) || (rc = side_ready(c, RPE_FEAT_MODEL))) return rc;
  auto& F = c->fe;
  auto &A = F.feat[RPE_FEAT_FRAME], &B = F.feat[RPE_FEAT_MODEL];
  if (!A.have || !B.have) return fail(RPE_ERR_STATE, "rpe_features_match: no features of the %s (rpe_features_detect)", A.have ? "model" : "frame");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensure_lists(c))) return rc;
  const rpe::MatchLists L = F.mlist.view();
  F.matches = -1; F.match_kf = -1;
  HIP_TRY(rpe::launch_feature_best(A.desc, A.count, B.desc, B.count, L.d1, L.idx, L.d2, c->stream));
  // the cross-check: the same pass with the roles swapped (its distances land in the match lists' slots, rewritten below)
  if (o.cross_check) HIP_TRY(rpe::launch_feature_best(B.desc, B.count, A.desc, A.count, L.md1, L.back, L.md2, c->stream));
  HIP_TRY(rpe::launch_feature_accept(L, A.count, o.max_dist, o.ratio_num, o.ratio_den, o.cross_check, F.fwork.ctl, c->stream));
  int m = 0;
  if ((rc = read_ints(c, F.fwork.ctl + rpe::kFeatCtlMatches, 1, &m))) return rc;
  if (m > 0) {
    if ((rc = claim_slots(c, m))) return rc;
    HIP_TRY(rpe::launch_feature_gather(L, m, A.pix, B.pix, F.fmap[0], F.fmap[1], F.fmap[2], F.mmap[0], F.mmap[1], (float*)c->arr[RPE_XW],
                                       (float*)c->arr[RPE_XC], (float*)c->arr[RPE_BV], (float*)c->arr[RPE_NW], (float*)c->arr[RPE_NC], c->stream));
  } else if ((rc = rpe_set_problem(c, 0, RPE_F32))) return rc;
  F.matches = m; F.match_gen[0] = A.gen; F.match_gen[1] = B.gen;
  if (matches) *matches = m;
  return RPE_OK;
}

int rpe_matches_download(rpe_context* c, int32_t* frame_idx, int32_t* model_idx, int32_t* d1, int32_t* d2, float* weight) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!matches_current(c)) return fail(RPE_ERR_STATE, "no matches: call rpe_features_match (a new detection on either side drops them)");
  HIP_TRY(hipSetDevice(c->device));
  const auto& L = c->fe.mlist;
  const size_t bytes = (size_t)c->fe.matches * sizeof(int);
  int rc;
  if (bytes && frame_idx && (rc = copy_to_host(c, frame_idx, L.mf, bytes))) return rc;
  if (bytes && model_idx && (rc = copy_to_host(c, model_idx, L.mm, bytes))) return rc;
  if (bytes && d1 && (rc = copy_to_host(c, d1, L.md1, bytes))) return rc;
  if (bytes && d2 && (rc = copy_to_host(c, d2, L.md2, bytes))) return rc;
  if (bytes && weight && (rc = copy_to_host(c, weight, L.mw, bytes))) return rc;
  return RPE_OK;
}

int rpe_relocalize(rpe_context* c, const rpe_feature_options* fopt, const rpe_match_options* mopt, int method, double thre_3d, double thre_2d,
                   double thre_nl, int* iter_io, double confidence, uint64_t seed, int ls, int min_matches, double* pose12, int* matches,
                   int* max_votes, short* mask_out) {
  session_end(c);
  if (!c || !pose12 || method < 0 || method > 9) return fail(RPE_ERR_ARG, "rpe_relocalize: bad argument (method 0 .. 9, pose12 not NULL)");
  if (min_matches < 4 || min_matches > RPE_MAX_KEYPOINTS) return fail(RPE_ERR_ARG, "rpe_relocalize: min_matches 4 .. %d (got %d)",
                                                                     RPE_MAX_KEYPOINTS, min_matches);
  const rpe_feature_options fo = fopt ? *fopt : kFeatureDefaults;
  const rpe_match_options mo = mopt ? *mopt : kMatchDefaults;
  int rc;
  if ((rc = feature_options(&fo)) || (rc = match_options(&mo))) return rc;
  for (int which : {RPE_FEAT_FRAME, RPE_FEAT_MODEL}) {
    if ((rc = side_ready(c, which)) || (rc = detect_if_stale(c, which, fo))) return rc;
  }
  int m = 0;
  if ((rc = rpe_features_match(c, &mo, &m))) return rc;
  if (matches) *matches = m;
  if (m < min_matches) return fail(RPE_ERR_DEGENERATE, "rpe_relocalize: %d matches, %d needed (%d / %d keypoints)", m, min_matches,
                                   c->fe.feat[0].count, c->fe.feat[1].count);
  return run_on_slots(c, m, method, thre_3d, thre_2d, thre_nl, iter_io, confidence, seed, ls, pose12, max_votes, mask_out);
}

}  // extern "C"
