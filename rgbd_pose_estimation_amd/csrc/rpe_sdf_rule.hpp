// THE VOLUME TERM, per frame pixel (include/rgbd_pose_hip.h Part 3, "Volume term"; tests/sdf_oracle.py is its numpy statement): a frame
// vertex is moved to the world under the pose guess, the trilinear TSDF there is the residual and the gradient of the same eight
// corners is the row.  No model view, no projective association.  Followed BIT-EXACTLY: fp32, the written order, no FMA contraction
// (rpe_volume_field.hpp switches it off to the end of the including unit, so a unit includes this header AFTER its other kernels).
// The rule is a template over the corner fetch, as ray_march is over the field: dense_corners reads the window; a fetch over the brick
// grid of the map raycast can follow without the rule being written again.
#pragma once
#include "rpe_volume_field.hpp"

namespace rpe {
namespace {

struct SdfParams {
  float gate;        // |r| <= gate [m]
  float c;           // normal gate
  float k;           // tr / s: tsdf per voxel -> metres per metre
  int use_normals;
};

// the eight corner voxels {tsdf, weight} of the cell i0 of the dense window, v[di + 2 dj + 4 dk], as field() loads them
struct dense_corners {
  const float* __restrict__ vol;
  int64_t sy, sz;
  __device__ __forceinline__ dense_corners(const float* __restrict__ v, const VolumeGeometry& G)
      : vol(v), sy(2 * (int64_t)G.dim[0]), sz(2 * (int64_t)G.dim[0] * G.dim[1]) {}
  __device__ __forceinline__ bool operator()(const int (&i0)[3], float2 (&v)[8]) const {
    const float* b = vol + (int64_t)i0[2] * sz + (int64_t)i0[1] * sy + 2 * (int64_t)i0[0];
    v[0] = *reinterpret_cast<const float2*>(b); v[1] = *reinterpret_cast<const float2*>(b + 2);
    v[2] = *reinterpret_cast<const float2*>(b + sy); v[3] = *reinterpret_cast<const float2*>(b + sy + 2);
    v[4] = *reinterpret_cast<const float2*>(b + sz); v[5] = *reinterpret_cast<const float2*>(b + sz + 2);
    v[6] = *reinterpret_cast<const float2*>(b + sz + sy); v[7] = *reinterpret_cast<const float2*>(b + sz + sy + 2);
    return true;
  }
};

// Steps 1-2: the cell of the frame vertex (x, y, z) under the pose guess T (Xc = R Xw + t).  Without one -- a vertex that is not finite,
// a world point outside the cell range -- false, and cell 0 with a = 0, so that a caller may fetch corners before it looks at the answer.
__device__ __forceinline__ bool sdf_cell(const VolumeGeometry& G, const PoseF& T, float x, float y, float z, int (&i0)[3], float (&a)[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) { i0[k] = 0; a[k] = 0.f; }
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return false;
  float wx, wy, wz;
  to_world(T, x, y, z, wx, wy, wz);
  return cell(G, wx, wy, wz, i0, a);
}

// Steps 3-6 and 8 on the cell's corner voxels v[di + 2 dj + 4 dk] and a: r [m] and J = [a | Xc x a], 0 when the pixel has no row so far;
// len is step 5's, for the normal gate.
__device__ __forceinline__ bool sdf_row(const float2 (&v)[8], const float (&a)[3], const VolumeGeometry& G, const PoseF& T, const SdfParams& Q,
                                        float x, float y, float z, float& r, float (&J)[6], float& len) {
  r = 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) J[k] = 0.f;
  bool ok = true;
#pragma unroll
  for (int m = 0; m < 8; m++) ok = ok && v[m].y > 0.0f && fabsf(v[m].x) < 1.0f;   // known, and no corner saturated (false for a NaN tsdf)
  const float D = trilerp(v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, a[0], a[1], a[2]);
  const float res = D * G.tr;
  ok = ok && fabsf(res) <= Q.gate;
  const float gx = bilerp(v[1].x - v[0].x, v[3].x - v[2].x, v[5].x - v[4].x, v[7].x - v[6].x, a[1], a[2]);
  const float gy = lerp(lerp(v[2].x - v[0].x, v[3].x - v[1].x, a[0]), lerp(v[6].x - v[4].x, v[7].x - v[5].x, a[0]), a[2]);
  const float gz = lerp(lerp(v[4].x - v[0].x, v[5].x - v[1].x, a[0]), lerp(v[6].x - v[2].x, v[7].x - v[3].x, a[0]), a[1]);
  len = sqrtf((gx * gx + gy * gy) + gz * gz);
  ok = ok && len > 0.0f;
  if (!ok) return false;
  const float mx = gx * Q.k, my = gy * Q.k, mz = gz * Q.k;
  const float a0 = -((T.R[0] * mx + T.R[1] * my) + T.R[2] * mz);
  const float a1 = -((T.R[3] * mx + T.R[4] * my) + T.R[5] * mz);
  const float a2 = -((T.R[6] * mx + T.R[7] * my) + T.R[8] * mz);
  r = res;
  J[0] = a0; J[1] = a1; J[2] = a2;
  J[3] = y * a2 - z * a1; J[4] = z * a0 - x * a2; J[5] = x * a1 - y * a0;
  return true;
}

// Step 7 on a row that stands so far (J[0..2] = a, len): the frame normal agrees with the field's gradient.  A row that fails is cleared.
__device__ __forceinline__ bool sdf_normal_gate(const SdfParams& Q, float nx, float ny, float nz, float len, float& r, float (&J)[6]) {
  const bool ok = __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz) &&
                  (-((J[0] * nx + J[1] * ny) + J[2] * nz)) / (len * Q.k) >= Q.c;
  if (!ok) {
    r = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = 0.f;
  }
  return ok;
}

// Steps 1-6 and 8 for one pixel.  Corners: (i0, v[8]) -> false when the cell has no voxels.
template <class Corners>
__device__ __forceinline__ bool sdf_pixel_row(Corners corners, const VolumeGeometry& G, const PoseF& T, const SdfParams& Q, float x, float y,
                                              float z, float& r, float (&J)[6], float& len) {
  int i0[3];
  float a[3];
  float2 v[8];
  const bool in = sdf_cell(G, T, x, y, z, i0, a);   // (without a cell: cell 0, whose corners are fetched and not looked at)
  const bool have = corners(i0, v);
  const bool ok = sdf_row(v, a, G, T, Q, x, y, z, r, J, len);
  if (in && have && ok) return true;
  r = 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) J[k] = 0.f;
  return false;
}

// The whole rule for one pixel.
template <class Corners>
__device__ __forceinline__ bool sdf_pixel(Corners corners, const VolumeGeometry& G, const PoseF& T, const SdfParams& Q, float x, float y,
                                          float z, float nx, float ny, float nz, float& r, float (&J)[6]) {
  float len;
  bool ok = sdf_pixel_row(corners, G, T, Q, x, y, z, r, J, len);
  if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nx, ny, nz, len, r, J);
  return ok;
}

}  // namespace
}  // namespace rpe
