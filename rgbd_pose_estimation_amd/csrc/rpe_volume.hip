// gfx950 kernels of the TSDF VOLUME (the KinectFusion half of the front end): depth frames are fused into a truncated signed distance
// volume, and the volume is raycast from a pose into the model maps the next frame's ICP registers against.
//
//   V1  volume_integrate_kernel   one frame (level-0 vertex map) into the volume under a pose: a streaming read-modify-write over the
//                                 voxels the frame sees.  Voxels are float2 {tsdf, weight}; a lane owns 4 consecutive voxels (two
//                                 16-byte pairs) and projects all four before it touches the volume, so that a voxel outside the
//                                 frustum, behind the surface or on invalid depth costs no volume traffic.
//   V2  volume_raycast_kernel     one ray per pixel, marched at fixed steps of one voxel through trilinear gathers of the volume,
//                                 up to the first zero crossing; the hit and the volume's gradient there become the model's world
//                                 vertex and normal.  A workgroup owns a 16 x 16 pixel tile (four 8 x 8 waves), so that neighbouring
//                                 rays gather the same L2 lines.
//
// The conventions (include/rgbd_pose_hip.h Part 3, "TSDF volume") are followed BIT-EXACTLY: fp32, the written order, no FMA contraction;
// tests/volume_oracle.py is their numpy statement.
#include "rpe_assoc.h"
#include "rpe_volume_field.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kVolBlock = 256;    // integrate: 4 voxels per lane
constexpr int kRayTile = 16;      // raycast: 16 x 16 pixels per workgroup, 8 x 8 per wave

// ---------------------------------------------------------------------------------------------- V1
// The voxel's projection (voxel_sdf), its update (fuse) and the lane's pairs: rpe_volume_field.hpp (shared with the colour integrate
// of rpe_color.hip).

// nvox <= 2^30 (dims <= 1024): the flat voxel index fits 32 bits, byte offsets do not
__global__ __launch_bounds__(kVolBlock) void volume_integrate_kernel(float* __restrict__ vol, VolumeGeometry G, int64_t nvox,
                                                                     const float* __restrict__ vmap, Camera cam, PoseF T) {
  const int64_t first = ((int64_t)blockIdx.x * kVolBlock + threadIdx.x) * 4;
  if (first >= nvox) return;
  const unsigned flat = (unsigned)first, d0 = (unsigned)G.dim[0], d1 = (unsigned)G.dim[1];
  int i = (int)(flat % d0), j = (int)((flat / d0) % d1), k = (int)(flat / d0 / d1);
  float f[4];
  bool up[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    f[q] = 0.0f;
    up[q] = first + q < nvox && voxel_sdf(G, vmap, cam, T, i, j, k, f[q]);
    if (++i == G.dim[0]) { i = 0; if (++j == G.dim[1]) { j = 0; ++k; } }
  }
  // the two 16-byte pairs of the lane (load_pair / store_pair): all loads before the first store
  float4 v[2];
#pragma unroll
  for (int p = 0; p < 2; p++) v[p] = load_pair(vol, first + 2 * p, nvox, up[2 * p] || up[2 * p + 1]);
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const bool lo = up[2 * p], hi = up[2 * p + 1];
    if (lo) fuse(v[p].x, v[p].y, f[2 * p], G.W);
    if (hi) fuse(v[p].z, v[p].w, f[2 * p + 1], G.W);
    store_pair(vol, first + 2 * p, v[p], lo, hi);
  }
}

// ---------------------------------------------------------------------------------------------- V2
// F(p) and the model normal: rpe_volume_field.hpp (shared with the mesh normals of rpe_mesh.hip).

// The ray rule -- sample positions, hit test, z*, the six-sample normal, NaN without a hit -- is ray_march / ray_normal of
// rpe_volume_field.hpp over the dense field (shared with the map raycast of rpe_frontend.hip).
__global__ __launch_bounds__(kRayTile * kRayTile) void volume_raycast_kernel(const float* __restrict__ vol, VolumeGeometry G, Camera cam,
                                                                             PoseF T, float dmin, float dmax, float* __restrict__ mv,
                                                                             float* __restrict__ mn) {
  const int tiles_x = (cam.width + kRayTile - 1) / kRayTile;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int u = (blockIdx.x % tiles_x) * kRayTile + (wave % 2) * 8 + lane % 8;
  const int v = (blockIdx.x / tiles_x) * kRayTile + (wave / 2) * 8 + lane / 8;
  if (u >= cam.width || v >= cam.height) return;
  const float xn = ((float)u - cam.cx) / cam.fx, yn = ((float)v - cam.cy) / cam.fy;
  const float zh = ray_march([&](float x, float y, float z, float& F) { return field(vol, G, x, y, z, F); }, T, xn, yn, G.s, dmin, dmax);
  float ox = qnan(), oy = qnan(), oz = qnan(), nx = qnan(), ny = qnan(), nz = qnan();
  if (zh == zh) {
    to_world(T, xn * zh, yn * zh, zh, ox, oy, oz);
    (void)field_normal(vol, G, ox, oy, oz, nx, ny, nz);   // leaves the NaN normal where a sample is unknown
  }
  const int64_t o = 3 * ((int64_t)v * cam.width + u);
  mv[o] = ox; mv[o + 1] = oy; mv[o + 2] = oz;
  mn[o] = nx; mn[o + 1] = ny; mn[o + 2] = nz;
}

}  // namespace

hipError_t launch_volume_integrate(float* vol, const VolumeGeometry& G, const float* vmap, const Camera& cam, const PoseF& T,
                                   hipStream_t s) {
  const int64_t nvox = (int64_t)G.dim[0] * G.dim[1] * G.dim[2];
  const int64_t blocks = (nvox + 4 * kVolBlock - 1) / (4 * kVolBlock);
  hipLaunchKernelGGL(volume_integrate_kernel, dim3((unsigned)blocks), dim3(kVolBlock), 0, s, vol, G, nvox, vmap, cam, T);
  return hipGetLastError();
}

hipError_t launch_volume_raycast(const float* vol, const VolumeGeometry& G, const Camera& cam, const PoseF& T, float dmin, float dmax,
                                 float* mv, float* mn, hipStream_t s) {
  const int tiles = ((cam.width + kRayTile - 1) / kRayTile) * ((cam.height + kRayTile - 1) / kRayTile);
  hipLaunchKernelGGL(volume_raycast_kernel, dim3(tiles), dim3(kRayTile * kRayTile), 0, s, vol, G, cam, T, dmin, dmax, mv, mn);
  return hipGetLastError();
}

RPE_PRELOAD(volume_integrate_kernel);

}  // namespace rpe
