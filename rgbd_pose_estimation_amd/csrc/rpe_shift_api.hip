// Part 3 of include/rgbd_pose_hip.h: the moving volume (kernel in rpe_shift.hip).  The window of the TSDF and colour volume moves by
// whole voxels: the voxels that stay are moved inside the arrays, the ones that come in are cleared, and the geometry every other
// kernel reads follows from the init-time origin and the total shift, rounded once.  rpe_volume_follow proposes the shift that brings
// a point in front of the camera back to the window's centre; rpe_volume_geometry says where the window is.
// Memory: the shift is OUT OF PLACE.  The context keeps a spare of the tsdf volume (8 B per voxel) and, when there is a colour volume,
// of that too (8 B per voxel), reserved on the first shift and swapped with the live arrays after each: 16 B per voxel more, 2 GB at
// 512^3 with colour, for a kernel whose every voxel is read once and written once with no ordering between workgroups to rely on.
// rpe_volume_init drops the spares when the volume grows.  With the volume archive on (rpe_archive_api.hip) a shift is bracketed by
// archive_leave and archive_enter; with it off the path below is what it was, call for call, and the host does not wait.
#include "rpe_frontend_host.hpp"
#include <cmath>
#include <utility>
using namespace rpeh;

#pragma clang fp contract(off)   // rpe_volume_follow and the origin are the header's expressions, operation by operation

namespace {

constexpr int64_t kMaxTotal = (int64_t)1 << 30;   // |total shift| per axis, and |v| of rpe_volume_follow

inline double origin_now(const rpe_context::Volume& V, int a, int64_t total) { return V.desc.origin[a] + (double)total * V.desc.voxel_size; }

}  // namespace

extern "C" {

int rpe_volume_shift(rpe_context* c, const int32_t shift[3]) {
  session_end(c);
  if (!c || !shift) return fail(RPE_ERR_ARG, "rpe_volume_shift: bad argument");
  auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (shift[0] == 0 && shift[1] == 0 && shift[2] == 0) return RPE_OK;   // nothing changes, the last mesh included
  int64_t total[3];
  float o[3];
  bool all_out = false;
  for (int a = 0; a < 3; a++) {
    total[a] = V.total[a] + (int64_t)shift[a];
    if (total[a] > kMaxTotal || total[a] < -kMaxTotal)
      return fail(RPE_ERR_ARG, "rpe_volume_shift: the total shift along axis %d would be %lld voxels; at most 2^30 either way", a, (long long)total[a]);
    o[a] = (float)origin_now(V, a, total[a]);
    if (!std::isfinite(o[a])) return fail(RPE_ERR_ARG, "rpe_volume_shift: the origin along axis %d would not be finite in fp32", a);
    all_out = all_out || shift[a] >= V.g.dim[a] || shift[a] <= -V.g.dim[a];
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t nvox = (size_t)V.g.dim[0] * V.g.dim[1] * V.g.dim[2];
  const size_t bytes = nvox * 2 * sizeof(float), cbytes = nvox * 4 * sizeof(unsigned short);
  // the archive (rpe_archive_api.hip), if it is on: the non-zero bricks that leave go into the pool before the window moves, the ones
  // that return are written over the zeros behind it.  Everything that can refuse the shift does so before the first brick is copied
  ArchivePlan plan;
  if (V.arc.on) {
    int rc;
    if (!all_out && (rc = V.d_spare.reserve(c, bytes))) return rc;
    if (!all_out && V.have_color && (rc = V.cd_spare.reserve(c, cbytes))) return rc;
    if ((rc = archive_leave(c, shift, total, &plan))) return rc;
  }
  if (all_out) {   // no voxel stays: the window is cleared where it is
    HIP_TRY(hipMemsetAsync(V.d, 0, bytes, c->stream));
    if (V.have_color) HIP_TRY(hipMemsetAsync(V.cd, 0, cbytes, c->stream));
  } else {
    int rc;
    if ((rc = V.d_spare.reserve(c, bytes))) return rc;
    if (V.have_color && (rc = V.cd_spare.reserve(c, cbytes))) return rc;
    const int d[3] = {shift[0], shift[1], shift[2]};
    HIP_TRY(rpe::launch_volume_shift(V.d, V.d_spare, V.have_color ? V.cd.get() : nullptr, V.have_color ? V.cd_spare.get() : nullptr, V.g.dim,
                                     d, c->stream));
    // the stream orders whatever comes next behind the kernel; the old arrays are the next shift's spares
    std::swap(V.d, V.d_spare);
    if (V.have_color) std::swap(V.cd, V.cd_spare);
  }
  for (int a = 0; a < 3; a++) { V.total[a] = total[a]; V.g.o[a] = o[a]; }
  V.have_mesh = false;
  if (V.arc.on) return archive_enter(c, plan);
  return RPE_OK;
}

int rpe_volume_geometry(rpe_context* c, rpe_volume_desc* desc, int64_t total_shift[3]) {
  session_end(c);
  if (!c || !desc) return fail(RPE_ERR_ARG, "rpe_volume_geometry: bad argument");
  const auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  *desc = V.desc;
  for (int a = 0; a < 3; a++) {
    desc->origin[a] = origin_now(V, a, V.total[a]);
    if (total_shift) total_shift[a] = V.total[a];
  }
  return RPE_OK;
}

int rpe_volume_follow(rpe_context* c, const double* pose12, double look_ahead, int granule, int32_t shift[3]) {
  session_end(c);
  if (!c || !pose12 || !shift) return fail(RPE_ERR_ARG, "rpe_volume_follow: bad argument");
  if (granule < 1) return fail(RPE_ERR_ARG, "rpe_volume_follow: granule must be >= 1 (got %d)", granule);
  if (!(look_ahead >= 0) || !std::isfinite(look_ahead))
    return fail(RPE_ERR_ARG, "rpe_volume_follow: look_ahead must be finite and >= 0 (got %g)", look_ahead);
  const auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  const double* R = pose12;
  const double* t = pose12 + 9;
  const double p[3] = {0.0 - t[0], 0.0 - t[1], look_ahead - t[2]};
  int32_t out[3];
  for (int a = 0; a < 3; a++) {
    const double w = R[a] * p[0] + R[3 + a] * p[1] + R[6 + a] * p[2];   // R^T p: the world point look_ahead metres ahead
    const double centre = origin_now(V, a, V.total[a]) + 0.5 * V.desc.dim[a] * V.desc.voxel_size;
    const double v = (w - centre) / V.desc.voxel_size;
    if (!(std::fabs(v) <= (double)kMaxTotal))
      return fail(RPE_ERR_ARG, "rpe_volume_follow: the target is %g voxels off the centre along axis %d; at most 2^30", v, a);
    out[a] = (int32_t)(granule * (int)std::trunc(v / granule));
  }
  for (int a = 0; a < 3; a++) shift[a] = out[a];
  return RPE_OK;
}

}  // extern "C"
