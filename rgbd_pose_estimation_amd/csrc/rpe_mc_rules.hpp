// The marching-cubes RULES of include/rgbd_pose_hip.h Part 3 ("Mesh") beside their tables (rpe_mc_tables.h), each stated once for
// rpe_mesh.hip (a dense volume) and rpe_mapmesh.hip (the map's listed bricks); a caller hands in where a corner, case byte or id comes
// from.  BIT-EXACT: rpe_volume_field.hpp, which both need for the field anyway, switches FMA contraction off for the including unit.
#pragma once
#include "rpe_volume_field.hpp"

namespace rpe {
namespace mc {

// The case of a cube from its corners, corner(n) = {tsdf, weight} of corner n = di + 2 dj + 4 dk: known iff weight >= wmin and the tsdf
// is finite; bit n iff tsdf <= 0; 0 unless all 8 corners are known.
template <class Corner>
__device__ __forceinline__ unsigned cube_case(Corner corner, float wmin) {
  unsigned m = 0;
  bool active = true;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    const float2 v = corner(n);
    active = active && v.y >= wmin && __builtin_isfinite(v.x);
    m |= (v.x <= 0.0f ? 1u : 0u) << n;
  }
  return active ? m : 0u;
}

__device__ __forceinline__ unsigned crossed(unsigned c, int a, int b) { return ((c >> a) ^ (c >> b)) & 1u; }
// used-edge bit a of a voxel: its edge along axis a is crossed in a cube containing it; cDDD = the case at (i - di, j - dj, k - dk)
__device__ __forceinline__ unsigned used_edges(unsigned c000, unsigned c100, unsigned c010, unsigned c110, unsigned c001, unsigned c101,
                                               unsigned c011) {
  const unsigned x = crossed(c000, 0, 1) | crossed(c010, 2, 3) | crossed(c001, 4, 5) | crossed(c011, 6, 7);
  const unsigned y = crossed(c000, 0, 2) | crossed(c100, 1, 3) | crossed(c001, 4, 6) | crossed(c101, 5, 7);
  const unsigned z = crossed(c000, 0, 4) | crossed(c100, 1, 5) | crossed(c010, 2, 6) | crossed(c110, 3, 7);
  return x | (y << 1) | (z << 2);
}

// The vertex on voxel ijk's edge along `axis`, Fa, Fb its two tsdf values: o + (((float)i + 0.5f) + t) * s along it, the centre's across
__device__ __forceinline__ void edge_vertex(const VolumeGeometry& G, const int ijk[3], int axis, float Fa, float Fb, float p[3]) {
  const float t = Fa / (Fa - Fb);
#pragma unroll
  for (int q = 0; q < 3; q++) p[q] = q == axis ? G.o[q] + (((float)ijk[q] + 0.5f) + t) * G.s : G.o[q] + ((float)ijk[q] + 0.5f) * G.s;
}

// The id of a triangle corner on its owner voxel's edge along `axis`: the owner's first id plus its used edges of lower axis.
__device__ __forceinline__ int corner_id(int first, unsigned used, unsigned axis) { return first + (int)__popc(used & ((1u << axis) - 1u)); }

}  // namespace mc
}  // namespace rpe
