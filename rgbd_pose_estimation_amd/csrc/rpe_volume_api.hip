// Part 3 of include/rgbd_pose_hip.h: the TSDF volume of the front end (kernels in rpe_volume.hip).  Frames are fused into the
// context's volume; a raycast of the volume becomes the model the next frame is registered against, through the same allocation and
// model state rpe_model_upload leaves (one level, the raycast's pose and camera).
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

extern "C" {

int rpe_volume_init(rpe_context* c, const rpe_volume_desc* d) {
  session_end(c);
  if (!c || !d) return fail(RPE_ERR_ARG, "rpe_volume_init: bad argument");
  for (int a = 0; a < 3; a++)
    if (d->dim[a] < 2 || d->dim[a] > 1024) return fail(RPE_ERR_ARG, "rpe_volume_init: dim[%d] = %d is outside 2 .. 1024", a, d->dim[a]);
  if (!(d->voxel_size > 0) || !std::isfinite(d->voxel_size) || !(d->trunc > 0) || !std::isfinite(d->trunc))
    return fail(RPE_ERR_ARG, "rpe_volume_init: voxel_size and trunc must be finite and > 0");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(d->origin[a])) return fail(RPE_ERR_ARG, "rpe_volume_init: origin must be finite");
  if (d->max_weight < 1) return fail(RPE_ERR_ARG, "rpe_volume_init: max_weight must be >= 1 (got %d)", d->max_weight);
  rpe::VolumeGeometry g;
  for (int a = 0; a < 3; a++) { g.dim[a] = d->dim[a]; g.o[a] = (float)d->origin[a]; }
  g.s = (float)d->voxel_size; g.tr = (float)d->trunc; g.W = (float)d->max_weight;
  if (!(g.s > 0) || !(g.tr > 0)) return fail(RPE_ERR_ARG, "rpe_volume_init: voxel_size and trunc must stay > 0 in fp32");
  HIP_TRY(hipSetDevice(c->device));
  auto& V = c->vol;
  const size_t bytes = (size_t)g.dim[0] * g.dim[1] * g.dim[2] * 2 * sizeof(float);
  if (V.arc.on) if (int rc = archive_drop(c)) return rc;   // the archive belongs to the volume it was switched on for
  V.have = false;
  V.have_mesh = false;
  V.have_color = false;
  if (V.d.bytes() < bytes) {   // the mesh workspace, the colour volume and the shift's spares follow the volume's size: they go before it grows
    if (V.d) HIP_TRY(hipStreamSynchronize(c->stream));
    V.ws = {}; V.cd = {}; V.d_spare = {}; V.cd_spare = {};
  }
  if (int rc = V.d.reserve(c, bytes)) return rc;
  HIP_TRY(hipMemsetAsync(V.d, 0, bytes, c->stream));
  V.g = g;
  V.desc = *d;
  V.total[0] = V.total[1] = V.total[2] = 0;
  V.have = true;
  return RPE_OK;
}

int rpe_volume_integrate(rpe_context* c, const double* pose12) {
  session_end(c);
  if (!c || !pose12) return fail(RPE_ERR_ARG, "rpe_volume_integrate: bad argument");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!c->fe.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(rpe::launch_volume_integrate(c->vol.d, c->vol.g, c->fe.fmap[0], c->fe.cam, pose_f(pose12), c->stream));
  return RPE_OK;
}

int rpe_volume_raycast(rpe_context* c, const double* pose12, const rpe_camera* cam, double dmin, double dmax) {
  session_end(c);
  if (!c || !pose12) return fail(RPE_ERR_ARG, "rpe_volume_raycast: bad argument");
  rpe::Camera k;
  int rc = camera_of(cam, &k);
  if (rc) return rc;
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!(dmin >= 0) || !(dmax > dmin) || !std::isfinite(dmax))
    return fail(RPE_ERR_ARG, "rpe_volume_raycast: need 0 <= dmin < dmax, both finite (got %g, %g)", dmin, dmax);
  const double samples = ((double)(float)dmax - (double)(float)dmin) / (double)c->vol.g.s;
  if (!(samples <= (double)(1 << 22)))
    return fail(RPE_ERR_ARG, "rpe_volume_raycast: %.0f samples per ray ((dmax - dmin) / voxel_size) exceed 2^22", samples);
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  const int64_t n = (int64_t)k.width * k.height;
  if ((rc = model_room(c, n))) return rc;
  F.have_model = false;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(rpe::launch_volume_raycast(c->vol.d, c->vol.g, k, pose_f(pose12), (float)dmin, (float)dmax, F.mmap[0], F.mmap[1], c->stream));
  F.mcam = k;
  one_level(*cam, k, F.mkcam, &F.mgeo);
  std::memcpy(F.mpose, pose12, sizeof(F.mpose));
  F.have_model = true;
  return RPE_OK;
}

int rpe_volume_download(rpe_context* c, float* out) {
  session_end(c);
  if (!c || !out) return fail(RPE_ERR_ARG, "rpe_volume_download: bad argument");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  const rpe::VolumeGeometry& g = c->vol.g;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, c->vol.d, (size_t)g.dim[0] * g.dim[1] * g.dim[2] * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_volume_upload(rpe_context* c, const float* in) {
  session_end(c);
  if (!c || !in) return fail(RPE_ERR_ARG, "rpe_volume_upload: bad argument");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  const rpe::VolumeGeometry& g = c->vol.g;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->vol.d, in, (size_t)g.dim[0] * g.dim[1] * g.dim[2] * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's buffer is free again on return
  return RPE_OK;
}

}  // extern "C"
