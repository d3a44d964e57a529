// Part 3 of include/rgbd_pose_hip.h: the volume rebuilt from the keyframes (kernels in rpe_rebuild.hip).  The attachments themselves
// -- a keyframe's depth plane, colour and camera -- are the store's (rpe_keyframe_api.hip); here a list of them is fused into the
// context's volume in one launch, leaving what volume_init + one integrate per keyframe would leave, bit for bit.
#include "rpe_frontend_host.hpp"
using namespace rpeh;

extern "C" {

int rpe_volume_fuse_keyframes(rpe_context* c, const int32_t* ids, int count, const double* poses12, int flags) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (flags & ~(RPE_FUSE_CLEAR | RPE_FUSE_COLOR | RPE_FUSE_NO_CULL)) return fail(RPE_ERR_ARG, "rpe_volume_fuse_keyframes: unknown flags 0x%x", flags);
  const bool clear = flags & RPE_FUSE_CLEAR, color = flags & RPE_FUSE_COLOR, cull = !(flags & RPE_FUSE_NO_CULL);
  auto& V = c->vol;
  auto& K = c->kf;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  const int stored = (int)K.meta.size();
  auto has_depth = [&](int id) { return id < (int)K.att.size() && K.att[id].have_depth; };
  // the list
  int32_t all[RPE_MAX_KEYFRAMES];
  if (!ids) {
    count = 0;
    for (int id = 0; id < stored; id++) if (has_depth(id)) all[count++] = id;
    if (count == 0) return fail(RPE_ERR_STATE, "rpe_volume_fuse_keyframes: no keyframe has depth attached (rpe_keyframe_attach_frame)");
    ids = all;
  } else {
    if (count < 1 || count > RPE_MAX_KEYFRAMES) return fail(RPE_ERR_ARG, "rpe_volume_fuse_keyframes: count 1 .. %d (got %d)", RPE_MAX_KEYFRAMES, count);
    for (int e = 0; e < count; e++)
      if (ids[e] < 0 || ids[e] >= stored) return fail(RPE_ERR_ARG, "rpe_volume_fuse_keyframes: no keyframe %d (%d in the store)", ids[e], stored);
  }
  for (int e = 0; e < count; e++) {
    if (!has_depth(ids[e])) return fail(RPE_ERR_STATE, "rpe_volume_fuse_keyframes: keyframe %d has no depth attached (rpe_keyframe_attach_frame)", ids[e]);
    if (color && !K.att[ids[e]].have_color) return fail(RPE_ERR_STATE, "rpe_volume_fuse_keyframes: keyframe %d has no colour attached", ids[e]);
  }
  HIP_TRY(hipSetDevice(c->device));
  std::vector<rpe::FuseEntry> table((size_t)count);
  for (int e = 0; e < count; e++) {
    const auto& A = K.att[ids[e]];
    table[e].z = A.z; table[e].rgba = color ? A.rgba : nullptr; table[e].cam = A.cam;
    table[e].T = pose_f(poses12 ? poses12 + 12 * (size_t)e : K.meta[ids[e]].pose);
  }
  if (int rc = K.d_table.once(c, RPE_MAX_KEYFRAMES * sizeof(rpe::FuseEntry))) return rc;
  // the call's one host wait: the table is the host's again (and an earlier fuse has read the table it was given)
  HIP_TRY(hipMemcpyAsync(K.d_table, table.data(), table.size() * sizeof(rpe::FuseEntry), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the volume's state, as rpe_volume_init (clear) and rpe_volume_integrate_color (color) leave it
  if (clear) { V.have_mesh = false; V.have_color = false; }
  if (color) if (int rc = ensure_color_volume(c, !clear)) return rc;   // with clear the kernel writes every colour voxel itself
  HIP_TRY(rpe::launch_volume_fuse(V.d, color ? V.cd : nullptr, V.g, K.d_table, count, clear, color, cull, c->stream));
  return RPE_OK;
}

}  // extern "C"
