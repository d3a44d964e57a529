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
  std::vector<rpe::FuseEntry> table;
  if (int rc = fuse_list(c, "rpe_volume_fuse_keyframes", ids, count, poses12, color, table)) return rc;
  count = (int)table.size();
  HIP_TRY(hipSetDevice(c->device));
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
