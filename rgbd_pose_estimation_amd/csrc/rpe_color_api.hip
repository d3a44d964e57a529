// Part 3 of include/rgbd_pose_hip.h: colour beside the TSDF volume (kernels in rpe_color.hip).  A registered RGB image becomes the
// frame's RGBA8 map; the colour integrate fuses it into a binary16 colour volume at the tsdf's voxel index; the colour field is sampled
// back at the model's level-0 vertices and at the last mesh's vertices.
#include "rpe_frontend_host.hpp"
using namespace rpeh;

namespace rpeh {
int ensure_color_volume(rpe_context* c, bool clear) {
  auto& V = c->vol;
  if (V.have_color) return RPE_OK;
  const size_t bytes = (size_t)V.g.dim[0] * V.g.dim[1] * V.g.dim[2] * 4 * sizeof(unsigned short);
  if (int rc = V.cd.reserve(c, bytes)) return rc;
  if (clear) HIP_TRY(hipMemsetAsync(V.cd, 0, bytes, c->stream));
  V.have_color = true;
  return RPE_OK;
}
}  // namespace rpeh

extern "C" {

int rpe_frame_set_color(rpe_context* c, const uint8_t* pixels, int format) {
  session_end(c);
  if (!c || !pixels || (format != RPE_COLOR_RGB8 && format != RPE_COLOR_BGR8)) return fail(RPE_ERR_ARG, "rpe_frame_set_color: bad argument");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first (the colour is registered to its depth)");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)F.cam.width * F.cam.height;
  int rc;
  if ((rc = F.d_rgb.reserve(c, (size_t)n * 3)) || (rc = F.fcolor.reserve(c, (size_t)n * 4))) return rc;
  F.have_fcolor = false; F.feat[0].have = false; F.photo_levels = 0; F.sint_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.d_rgb, pixels, (size_t)n * 3, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(rpe::launch_frame_color(F.d_rgb, n, format == RPE_COLOR_BGR8 ? 1 : 0, F.fcolor, c->stream));
  F.have_fcolor = true;
  return RPE_OK;
}

int rpe_volume_integrate_color(rpe_context* c, const double* pose12) {
  session_end(c);
  if (!c || !pose12) return fail(RPE_ERR_ARG, "rpe_volume_integrate_color: bad argument");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!c->fe.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first");
  if (!c->fe.have_fcolor) return fail(RPE_ERR_STATE, "no frame colour: call rpe_frame_set_color after the frame's depth");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_color_volume(c, true);
  if (rc) return rc;
  HIP_TRY(rpe::launch_volume_integrate_color(c->vol.d, c->vol.cd, c->vol.g, c->fe.fmap[0], c->fe.fcolor, c->fe.cam, pose_f(pose12),
                                             c->stream));
  return RPE_OK;
}

int rpe_model_sample_color(rpe_context* c) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  auto& F = c->fe;
  if (!F.have_model) return fail(RPE_ERR_STATE, "no model: call rpe_volume_raycast, rpe_model_upload or rpe_model_from_frame first");
  if (!c->vol.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!c->vol.have_color) return fail(RPE_ERR_STATE, "no colour volume: call rpe_volume_integrate_color or rpe_volume_color_upload first");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)F.mcam.width * F.mcam.height;
  int rc = F.mcolor.reserve(c, (size_t)n * 4);
  if (rc) return rc;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  HIP_TRY(rpe::launch_color_sample(c->vol.cd, c->vol.g, F.mmap[0], n, F.mcolor, c->stream));
  F.have_mcolor = true;
  return RPE_OK;
}

int rpe_color_download(rpe_context* c, int which, uint8_t* rgba) {
  session_end(c);
  if (!c || !rgba || (which != RPE_COLOR_FRAME && which != RPE_COLOR_MODEL)) return fail(RPE_ERR_ARG, "rpe_color_download: bad argument");
  const auto& F = c->fe;
  const bool model = which == RPE_COLOR_MODEL;
  if (model ? !F.have_mcolor : !F.have_fcolor)
    return fail(RPE_ERR_STATE, model ? "no model colour: call rpe_model_sample_color after the model is set"
                                     : "no frame colour: call rpe_frame_set_color after the frame's depth");
  const rpe::Camera& k = model ? F.mcam : F.cam;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(rgba, model ? F.mcolor : F.fcolor, (size_t)k.width * k.height * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_volume_mesh_colors(rpe_context* c, uint8_t* rgba) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_mesh_colors: bad argument");
  auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!V.have_mesh) return fail(RPE_ERR_STATE, "no mesh: call rpe_volume_mesh first (rpe_volume_init drops the mesh)");
  if (V.mesh_is_map ? !V.map_color : !V.have_color)
    return fail(RPE_ERR_STATE, V.mesh_is_map ? "no colour: the map had neither a colour volume nor a colour plane in the archive when rpe_volume_map_mesh ran"
                                             : "no colour volume: call rpe_volume_integrate_color or rpe_volume_color_upload first");
  if (V.nv > 0 && !rgba) return fail(RPE_ERR_ARG, "rpe_volume_mesh_colors: bad argument");
  if (V.nv == 0) return RPE_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (V.mesh_is_map) {   // sampled during the extraction (rpe_mapmesh.hip P3)
    HIP_TRY(hipMemcpyAsync(rgba, V.mc, (size_t)V.nv * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RPE_OK;
  }
  int rc = V.mc.reserve(c, (size_t)V.nv * 4);
  if (rc) return rc;
  HIP_TRY(rpe::launch_color_sample(V.cd, V.g, V.mv, V.nv, V.mc, c->stream));
  HIP_TRY(hipMemcpyAsync(rgba, V.mc, (size_t)V.nv * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_volume_color_download(rpe_context* c, uint16_t* rgbw) {
  session_end(c);
  if (!c || !rgbw) return fail(RPE_ERR_ARG, "rpe_volume_color_download: bad argument");
  const auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!V.have_color) return fail(RPE_ERR_STATE, "no colour volume: call rpe_volume_integrate_color or rpe_volume_color_upload first");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(rgbw, V.cd, (size_t)V.g.dim[0] * V.g.dim[1] * V.g.dim[2] * 4 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_volume_color_upload(rpe_context* c, const uint16_t* rgbw) {
  session_end(c);
  if (!c || !rgbw) return fail(RPE_ERR_ARG, "rpe_volume_color_upload: bad argument");
  auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_color_volume(c, false);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(V.cd, rgbw, (size_t)V.g.dim[0] * V.g.dim[1] * V.g.dim[2] * 4 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // the caller's buffer is free again on return
  return RPE_OK;
}

}  // extern "C"
