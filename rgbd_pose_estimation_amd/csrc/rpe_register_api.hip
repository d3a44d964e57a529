// Part 3 of include/rgbd_pose_hip.h: colour registration (kernels in rpe_register.hip).  The image of a separate colour camera is staged
// to RGBA8 at its own size (C1 of rpe_color.hip), the depth frame's level-0 vertices are splatted into a z-buffer over the colour image
// (R1, skipped with cell = 0) and every depth pixel gathers its colour, or none (R2), into the frame colour rpe_frame_set_color fills.
#include "rpe_frontend_host.hpp"
using namespace rpeh;

namespace {

// the rig validated and cast to the kernels' form (RPE_ERR_ARG)
int rig_of(const rpe_color_rig* r, rpe::RegisterRig* out) {
  const rpe_camera& k = r->cam;
  if (k.width < 2 || k.height < 2 || !std::isfinite(k.fx) || !std::isfinite(k.fy) || !(k.fx > 0) || !(k.fy > 0) || !std::isfinite(k.cx) ||
      !std::isfinite(k.cy))
    return fail(RPE_ERR_ARG, "rpe_frame_register_color: the colour camera needs at least 2 x 2 pixels, finite fx, fy > 0 and a finite "
                             "centre (got %d x %d, fx %g, fy %g, cx %g, cy %g)", k.width, k.height, k.fx, k.fy, k.cx, k.cy);
  if (int rc = camera_of(&k, &out->cam)) return rc;
  if (r->cell < 0 || r->cell > 16) return fail(RPE_ERR_ARG, "rpe_frame_register_color: cell must be 0 .. 16, got %d", r->cell);
  for (double d : r->dist) if (!std::isfinite(d)) return fail(RPE_ERR_ARG, "rpe_frame_register_color: non-finite distortion coefficient");
  for (double p : r->pose12) if (!std::isfinite(p)) return fail(RPE_ERR_ARG, "rpe_frame_register_color: non-finite pose");
  if (!std::isfinite(r->occl_tol) || !std::isfinite(r->occl_tol_z2) || !std::isfinite(r->r2_max) || r->occl_tol < 0 || r->occl_tol_z2 < 0 ||
      r->r2_max < 0)
    return fail(RPE_ERR_ARG, "rpe_frame_register_color: occl_tol, occl_tol_z2 and r2_max must be finite and >= 0");
  out->T = pose_f(r->pose12);
  out->k1 = (float)r->dist[0]; out->k2 = (float)r->dist[1]; out->p1 = (float)r->dist[2]; out->p2 = (float)r->dist[3];
  out->k3 = (float)r->dist[4];
  out->r2_max = (float)r->r2_max;
  out->cell = r->cell;
  out->gw = r->cell ? (k.width + r->cell - 1) / r->cell : 0;
  out->gh = r->cell ? (k.height + r->cell - 1) / r->cell : 0;
  out->a = (float)r->occl_tol; out->b = (float)r->occl_tol_z2;
  return RPE_OK;
}

}  // namespace

extern "C" {

int rpe_frame_register_color(rpe_context* c, const uint8_t* pixels, int format, const rpe_color_rig* rig, int64_t* known) {
  session_end(c);
  if (!c || !pixels || !rig || (format != RPE_COLOR_RGB8 && format != RPE_COLOR_BGR8))
    return fail(RPE_ERR_ARG, "rpe_frame_register_color: bad argument");
  auto& F = c->fe;
  if (!F.have_frame) return fail(RPE_ERR_STATE, "no frame: call rpe_frame_set_depth first (the colour is registered to its depth)");
  rpe::RegisterRig G;
  int rc = rig_of(rig, &G);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)F.cam.width * F.cam.height, nc = (int64_t)G.cam.width * G.cam.height;
  // the z-buffer in its factored form (base-cell minima, rpe_register.hip), and behind it the words that count the A = 255 pixels
  const size_t zwords = G.cell ? (size_t)(G.gw + 1) * (G.gh + 1) : 0;
  if ((rc = F.rg_rgb.reserve(c, (size_t)nc * 3)) || (rc = F.rg_rgba.reserve(c, (size_t)nc * 4)) ||
      (rc = F.rg_zbuf.reserve(c, (zwords + rpe::kRegCountWords) * 4)) || (rc = F.fcolor.reserve(c, (size_t)n * 4)))
    return rc;
  F.have_fcolor = false; F.feat[0].have = false; F.photo_levels = 0; F.sint_levels = 0;
  HIP_TRY(hipMemcpyAsync(F.rg_rgb, pixels, (size_t)nc * 3, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(rpe::launch_frame_color(F.rg_rgb, nc, format == RPE_COLOR_BGR8 ? 1 : 0, F.rg_rgba, c->stream));
  unsigned int* count = known ? F.rg_zbuf + zwords : nullptr;
  if (G.cell > 0) {
    HIP_TRY(hipMemsetAsync(F.rg_zbuf, 0xff, zwords * 4, c->stream));
    HIP_TRY(rpe::launch_register_splat(F.fmap[0], n, G, F.rg_zbuf, c->stream));
  }
  if (count) HIP_TRY(hipMemsetAsync(count, 0, rpe::kRegCountWords * 4, c->stream));
  HIP_TRY(rpe::launch_register_gather(F.fmap[0], n, G, F.rg_zbuf, F.rg_rgba, F.fcolor, count, c->stream));
  F.have_fcolor = true;
  if (known) {
    int k[rpe::kRegCountWords];
    if ((rc = read_ints(c, reinterpret_cast<const int*>(count), rpe::kRegCountWords, k))) return rc;
    int64_t sum = 0;
    for (int v : k) sum += v;
    *known = sum;
  }
  return RPE_OK;
}

}  // extern "C"
