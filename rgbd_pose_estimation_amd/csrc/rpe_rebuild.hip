// gfx950 kernels that REBUILD the TSDF / colour volume from the keyframes' attachments (include/rgbd_pose_hip.h Part 3, "Keyframe depth
// and rebuilding the volume"): after a loop closure every keyframe's depth is fused again at its corrected pose.
//
//   R1  attach_pack_kernel   the current frame's level-0 depth -- z of the stride-3 vertex map -- into a keyframe's packed plane (one fp32
//                            per pixel, NaN = invalid), and its RGBA8 map copied beside it.
//   R2  volume_fuse_kernel   ONE pass over the volume for a LIST of keyframes.  A workgroup owns a brick of 32 x 8 x 4 voxels, a lane four
//                            voxels consecutive in x; their {tsdf, w} and {r, g, b, wc} stay in registers while the lane walks the list
//                            in order -- voxel_project / fuse / blend of rpe_volume_field.hpp, V1's and C2's own code, so that the chain
//                            of updates per voxel is the one the frame-by-frame route runs, bit for bit -- and are written once.  An
//                            entry's descriptor (depth and colour pointers, camera, pose) is the same for the whole workgroup and comes
//                            from a device table.  Before the loop the workgroup tests every entry against the bounding box of its voxel
//                            centres (one entry per thread) and skips the entries that cannot update any of them.
//                            CLEAR: nothing is loaded, every voxel is stored (the memset of rpe_volume_init folded in); otherwise the
//                            brick is loaded once and only updated voxels are stored, a 16-byte pair at a time where both are.
//
// fp32, the written order, no FMA contraction; tests/rebuild_oracle.py is the numpy statement (a loop over the integrate oracles).
#include "rpe_assoc.h"
#include "rpe_volume_field.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kPackBlock = 256;
constexpr int kFuseBlock = 256;                          // 8 x 8 x 4 lanes, 4 voxels in x each
constexpr int kBrickX = 32, kBrickY = 8, kBrickZ = 4;
static_assert(kFuseBlock >= kMaxKeyframes, "one thread per list entry in the cull");

// ---------------------------------------------------------------------------------------------- R1
__global__ __launch_bounds__(kPackBlock) void attach_pack_kernel(const float* __restrict__ vmap, const unsigned int* __restrict__ fcolor,
                                                                 int64_t n, float* __restrict__ z, unsigned int* __restrict__ rgba) {
  const int64_t i = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
  if (i >= n) return;
  z[i] = vmap[3 * i + 2];
  if (fcolor) rgba[i] = fcolor[i];
}

// ---------------------------------------------------------------------------------------------- R2
// (the cull -- box_can_update -- is rpe_volume_field.hpp's, shared with the map fuse of rpe_mapfuse.hpp)
// grid: one workgroup per brick, bricks in x fastest; at most 32 x 128 x 256 = 2^20 of them (dims <= 1024)
template <bool CLEAR, bool COLOR>
__global__ __launch_bounds__(kFuseBlock) void volume_fuse_kernel(float* __restrict__ vol, unsigned short* __restrict__ cvol, VolumeGeometry G,
                                                                 const FuseEntry* __restrict__ table, int count, int cull) {
  __shared__ int keep[kMaxKeyframes];
  const int t = threadIdx.x;
  const unsigned bx = (unsigned)(G.dim[0] + kBrickX - 1) / kBrickX, by = (unsigned)(G.dim[1] + kBrickY - 1) / kBrickY;
  const unsigned b = blockIdx.x;
  const int i0 = (int)(b % bx) * kBrickX, j0 = (int)((b / bx) % by) * kBrickY, k0 = (int)(b / bx / by) * kBrickZ;

  // ---- the cull: entry t against the box of this brick's voxel centres
  int mine = 0;
  if (t < count) {
    mine = 1;
    if (cull) {
      const int i1 = min(i0 + kBrickX, G.dim[0]) - 1, j1 = min(j0 + kBrickY, G.dim[1]) - 1, k1 = min(k0 + kBrickZ, G.dim[2]) - 1;
      const float lo[3] = {G.o[0] + ((float)i0 + 0.5f) * G.s, G.o[1] + ((float)j0 + 0.5f) * G.s, G.o[2] + ((float)k0 + 0.5f) * G.s};
      const float hi[3] = {G.o[0] + ((float)i1 + 0.5f) * G.s, G.o[1] + ((float)j1 + 0.5f) * G.s, G.o[2] + ((float)k1 + 0.5f) * G.s};
      mine = box_can_update(lo, hi, table[t].cam, table[t].T) ? 1 : 0;
    }
  }
  if (t < kMaxKeyframes) keep[t] = mine;
  const int any = __syncthreads_or(mine);
  if (!CLEAR && !any) return;                      // nothing to update and nothing to clear: the brick keeps its bits

  // ---- the lane's four voxels (i .. i + 3, j, k)
  const int i = i0 + (t & 7) * 4, j = j0 + ((t >> 3) & 7), k = k0 + (t >> 6);
  const bool row = j < G.dim[1] && k < G.dim[2];
  bool valid[4];
#pragma unroll
  for (int q = 0; q < 4; q++) valid[q] = row && i + q < G.dim[0];
  if (!valid[0]) return;                           // (no barrier below)
  const int64_t first = ((int64_t)k * G.dim[1] + j) * G.dim[0] + i;
  // an even dim0 puts every row, and with it every lane's first voxel, on a 16-byte boundary, and a pair is then valid as a whole;
  // with an odd dim0 the lane moves its voxels one by one
  const bool pair16 = (G.dim[0] & 1) == 0;
  float ts[4], w[4];
  unsigned rg[4], bw[4];
  bool up[4], cu[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { ts[q] = 0.0f; w[q] = 0.0f; rg[q] = 0u; bw[q] = 0u; up[q] = false; cu[q] = false; }
  if (!CLEAR) {
    if (pair16) {
#pragma unroll
      for (int p = 0; p < 2; p++) {
        if (!valid[2 * p]) continue;
        const float4 v = *reinterpret_cast<const float4*>(vol + 2 * (first + 2 * p));
        ts[2 * p] = v.x; w[2 * p] = v.y; ts[2 * p + 1] = v.z; w[2 * p + 1] = v.w;
        if (COLOR) {
          const uint4 c = *reinterpret_cast<const uint4*>(cvol + 4 * (first + 2 * p));
          rg[2 * p] = c.x; bw[2 * p] = c.y; rg[2 * p + 1] = c.z; bw[2 * p + 1] = c.w;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (!valid[q]) continue;
        const float2 v = *reinterpret_cast<const float2*>(vol + 2 * (first + q));
        ts[q] = v.x; w[q] = v.y;
        if (COLOR) { const uint2 c = *reinterpret_cast<const uint2*>(cvol + 4 * (first + q)); rg[q] = c.x; bw[q] = c.y; }
      }
    }
  }

  // ---- the list, in order: every voxel takes its observations as the frame-by-frame route hands them out
  for (int e = 0; e < count; e++) {
    if (!__builtin_amdgcn_readfirstlane(keep[e])) continue;
    const FuseEntry& E = table[e];
    float f[4], sdf[4];
    int64_t pix[4];
    bool hit[4], band[4];
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      f[q] = 0.0f; sdf[q] = 0.0f; pix[q] = 0;
      hit[q] = valid[q] && voxel_project<1, 0>(G, E.z, E.cam, E.T, i + q, j, k, f[q], sdf[q], pix[q]);
      band[q] = COLOR && hit[q] && sdf[q] <= G.tr;
    }
    if (COLOR) {
#pragma unroll
      for (int q = 0; q < 4; q++) o[q] = band[q] ? E.rgba[pix[q]] : 0u;
      // A = 0: the pixel has no colour (as C2)
#pragma unroll
      for (int q = 0; q < 4; q++) band[q] = band[q] && (o[q] >> 24) != 0u;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (hit[q]) { fuse(ts[q], w[q], f[q], G.W); up[q] = true; }
      if (COLOR && band[q]) { blend(rg[q], bw[q], o[q], G.W); cu[q] = true; }
    }
  }

  // ---- written once
  if (pair16) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      if (!valid[2 * p]) continue;
      const int a = 2 * p, c = 2 * p + 1;
      float* q = vol + 2 * (first + a);
      const bool lo = CLEAR || up[a], hi = CLEAR || up[c];
      if (lo && hi) *reinterpret_cast<float4*>(q) = make_float4(ts[a], w[a], ts[c], w[c]);
      else if (lo) *reinterpret_cast<float2*>(q) = make_float2(ts[a], w[a]);
      else if (hi) *reinterpret_cast<float2*>(q + 2) = make_float2(ts[c], w[c]);
      if (COLOR) {
        unsigned short* qc = cvol + 4 * (first + a);
        const bool clo = CLEAR || cu[a], chi = CLEAR || cu[c];
        if (clo && chi) *reinterpret_cast<uint4*>(qc) = make_uint4(rg[a], bw[a], rg[c], bw[c]);
        else if (clo) *reinterpret_cast<uint2*>(qc) = make_uint2(rg[a], bw[a]);
        else if (chi) *reinterpret_cast<uint2*>(qc + 4) = make_uint2(rg[c], bw[c]);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (!valid[q]) continue;
      if (CLEAR || up[q]) *reinterpret_cast<float2*>(vol + 2 * (first + q)) = make_float2(ts[q], w[q]);
      if (COLOR && (CLEAR || cu[q])) *reinterpret_cast<uint2*>(cvol + 4 * (first + q)) = make_uint2(rg[q], bw[q]);
    }
  }
}

}  // namespace

hipError_t launch_attach_pack(const float* vmap, const unsigned int* fcolor, int64_t n, float* z, unsigned int* rgba, hipStream_t s) {
  const int64_t blocks = (n + kPackBlock - 1) / kPackBlock;
  hipLaunchKernelGGL(attach_pack_kernel, dim3((unsigned)blocks), dim3(kPackBlock), 0, s, vmap, fcolor, n, z, rgba);
  return hipGetLastError();
}

hipError_t launch_volume_fuse(float* vol, unsigned short* cvol, const VolumeGeometry& G, const FuseEntry* table, int count, bool clear,
                              bool color, bool cull, hipStream_t s) {
  const unsigned bricks = (unsigned)((G.dim[0] + kBrickX - 1) / kBrickX) * (unsigned)((G.dim[1] + kBrickY - 1) / kBrickY) *
                          (unsigned)((G.dim[2] + kBrickZ - 1) / kBrickZ);
  const dim3 grid(bricks), block(kFuseBlock);
  const int c = cull ? 1 : 0;
  if (clear && color) hipLaunchKernelGGL((volume_fuse_kernel<true, true>), grid, block, 0, s, vol, cvol, G, table, count, c);
  else if (clear) hipLaunchKernelGGL((volume_fuse_kernel<true, false>), grid, block, 0, s, vol, cvol, G, table, count, c);
  else if (color) hipLaunchKernelGGL((volume_fuse_kernel<false, true>), grid, block, 0, s, vol, cvol, G, table, count, c);
  else hipLaunchKernelGGL((volume_fuse_kernel<false, false>), grid, block, 0, s, vol, cvol, G, table, count, c);
  return hipGetLastError();
}

RPE_PRELOAD(attach_pack_kernel);

}  // namespace rpe
