// THE MAP FUSE (include/rgbd_pose_hip.h Part 3, "Map fuse"; included by rpe_frontend.hip, beside the map raycast and the map volume term):
// a LIST of keyframes fused into the bricks of a box of the map, in the window or in the archive's pool.  R2 of rpe_rebuild.hip on the
// VIRTUAL volume G of the box: voxel (8 bx + x, 8 by + y, 8 bz + z) of brick (bx, by, bz) of the box projects with voxel_project, takes
// fuse / blend in list order and is culled with box_can_update -- rpe_volume_field.hpp's text, no arithmetic of its own here.  What this
// kernel adds is where a brick's 4 KB lie (brick_word: the window's arrays or a pool slot, one path) and the two passes:
//
//   map_fuse_kernel<CLEAR, COLOR, MARK>   one workgroup of 128 threads (two waves) per brick, a lane four voxels consecutive in x (half a
//                       row: 32 bytes of either volume, two 16-byte accesses); their {tsdf, w} and {rg, bw} stay in registers while the lane
//                       walks the list in order.  LDS: the cull's keep[] flags only; no atomics.
//     MARK (pass 1)     over EVERY brick of the box, from zeros, no volume access: flags[brick] = 1 if any result word is non-zero (what an
//                       absent brick, or any brick under CLEAR, would hold) | 2 if any voxel was updated (whether a present brick changes).
//     pass 2            over the host's list of {box brick, source, fresh}: fresh (always under CLEAR) = start from zeros and store every
//                       voxel, the colour brick too where a colour plane exists (zeros without COLOR: a slot's last tenant, or the box's
//                       colour under CLEAR); else the brick is loaded once and the 16-byte pairs that hold an updated voxel are stored.
#pragma once
#include "rpe_volume_field.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kMapFuseBlock = 128;                       // 2 x 8 x 8 lanes, 4 voxels in x each
static_assert(2 * kMapFuseBlock >= kMaxKeyframes, "two list entries per thread in the cull");

template <bool CLEAR, bool COLOR, bool MARK>
__global__ __launch_bounds__(kMapFuseBlock) void map_fuse_kernel(MapFuseView M, VolumeGeometry G) {
  __shared__ int keep[kMaxKeyframes];
  const int t = threadIdx.x;
  int b, src = kMapAbsent;
  bool fresh = true;
  if (MARK) b = (int)blockIdx.x;
  else {
    const int* e = M.list + 3 * (int64_t)blockIdx.x;
    b = e[0]; src = e[1]; fresh = CLEAR || e[2] != 0;
  }
  const unsigned nbx = (unsigned)M.nb[0], nby = (unsigned)M.nb[1];
  if ((unsigned)b >= nbx * nby * (unsigned)M.nb[2]) return;          // (the whole workgroup; the box holds <= 2^24 bricks)
  const int i0 = (int)((unsigned)b % nbx) * 8, j0 = (int)(((unsigned)b / nbx) % nby) * 8, k0 = (int)((unsigned)b / nbx / nby) * 8;

  // ---- the cull: entries t and t + 128 against the box of this brick's voxel centres
  int mine = 0;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int e = t + r * kMapFuseBlock;
    int k = 0;
    if (e < M.count) {
      k = 1;
      if (M.cull) {
        const float lo[3] = {G.o[0] + ((float)i0 + 0.5f) * G.s, G.o[1] + ((float)j0 + 0.5f) * G.s, G.o[2] + ((float)k0 + 0.5f) * G.s};
        const float hi[3] = {G.o[0] + ((float)(i0 + 7) + 0.5f) * G.s, G.o[1] + ((float)(j0 + 7) + 0.5f) * G.s,
                             G.o[2] + ((float)(k0 + 7) + 0.5f) * G.s};
        k = box_can_update(lo, hi, M.table[e].cam, M.table[e].T) ? 1 : 0;
      }
    }
    if (e < kMaxKeyframes) keep[e] = k;
    mine |= k;
  }
  const int any = __syncthreads_or(mine);
  if (!any) {
    if (MARK) { if (t == 0) M.flags[b] = 0u; return; }
    if (!fresh) return;                                              // nothing to update: the brick keeps its bits
  }

  // ---- the lane's four voxels (i .. i + 3, j, k) of the virtual volume, and where they lie
  const int x = (t & 1) * 4, y = (t >> 1) & 7, z = t >> 4;
  const int i = i0 + x, j = j0 + y, k = k0 + z;
  unsigned int *dst = nullptr, *cdst = nullptr;
  if (!MARK) {
    int64_t w;
    bool pooled;
    if (!brick_word(M, src, x, y, z, w, pooled)) return;             // not a window brick, not a slot below the capacity: no address
    dst = pooled ? M.pool : M.vol;
    cdst = pooled ? M.cpool : M.cvol;
    if (!dst || (COLOR && !cdst)) return;
    dst += w;
    if (cdst) cdst += w;
  }
  float ts[4], wt[4];
  unsigned rg[4], bw[4];
  bool up[4], cu[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { ts[q] = 0.0f; wt[q] = 0.0f; rg[q] = 0u; bw[q] = 0u; up[q] = false; cu[q] = false; }
  if (!MARK && !fresh) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const uint4 v = *reinterpret_cast<const uint4*>(dst + 4 * p);
      ts[2 * p] = __uint_as_float(v.x); wt[2 * p] = __uint_as_float(v.y); ts[2 * p + 1] = __uint_as_float(v.z); wt[2 * p + 1] = __uint_as_float(v.w);
      if (COLOR) {
        const uint4 c = *reinterpret_cast<const uint4*>(cdst + 4 * p);
        rg[2 * p] = c.x; bw[2 * p] = c.y; rg[2 * p + 1] = c.z; bw[2 * p + 1] = c.w;
      }
    }
  }

  // ---- the list, in order (R2's loop)
  for (int e = 0; e < M.count; e++) {
    if (!__builtin_amdgcn_readfirstlane(keep[e])) continue;
    const FuseEntry& E = M.table[e];
    float f[4], sdf[4];
    int64_t pix[4];
    bool hit[4], band[4];
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      f[q] = 0.0f; sdf[q] = 0.0f; pix[q] = 0;
      hit[q] = voxel_project<1, 0>(G, E.z, E.cam, E.T, i + q, j, k, f[q], sdf[q], pix[q]);
      band[q] = COLOR && hit[q] && sdf[q] <= G.tr;
    }
    if (COLOR) {
#pragma unroll
      for (int q = 0; q < 4; q++) o[q] = band[q] ? E.rgba[pix[q]] : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) band[q] = band[q] && (o[q] >> 24) != 0u;   // A = 0: the pixel has no colour
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (hit[q]) { fuse(ts[q], wt[q], f[q], G.W); up[q] = true; }
      if (COLOR && band[q]) { blend(rg[q], bw[q], o[q], G.W); cu[q] = true; }
    }
  }

  if (MARK) {
    unsigned words = 0u;
    bool touched = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      words |= __float_as_uint(ts[q]) | __float_as_uint(wt[q]) | rg[q] | bw[q];
      touched = touched || up[q] || cu[q];
    }
    const int nonzero = __syncthreads_or(words != 0u), updated = __syncthreads_or(touched);
    if (t == 0) M.flags[b] = (nonzero ? 1u : 0u) | (updated ? 2u : 0u);
    return;
  }

  // ---- written once, 16 bytes at a time
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int a = 2 * p, c = 2 * p + 1;
    if (fresh || up[a] || up[c])
      *reinterpret_cast<uint4*>(dst + 4 * p) = make_uint4(__float_as_uint(ts[a]), __float_as_uint(wt[a]), __float_as_uint(ts[c]), __float_as_uint(wt[c]));
    if (COLOR) {
      if (fresh || cu[a] || cu[c]) *reinterpret_cast<uint4*>(cdst + 4 * p) = make_uint4(rg[a], bw[a], rg[c], bw[c]);
    } else if (fresh && cdst) {
      *reinterpret_cast<uint4*>(cdst + 4 * p) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

}  // namespace

hipError_t launch_map_fuse_mark(const MapFuseView& M, const VolumeGeometry& G, bool color, hipStream_t s) {
  if (M.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)M.n), block(kMapFuseBlock);
  if (color) hipLaunchKernelGGL((map_fuse_kernel<true, true, true>), grid, block, 0, s, M, G);
  else hipLaunchKernelGGL((map_fuse_kernel<true, false, true>), grid, block, 0, s, M, G);
  return hipGetLastError();
}

hipError_t launch_map_fuse(const MapFuseView& M, const VolumeGeometry& G, bool clear, bool color, hipStream_t s) {
  if (M.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)M.n), block(kMapFuseBlock);
  if (clear && color) hipLaunchKernelGGL((map_fuse_kernel<true, true, false>), grid, block, 0, s, M, G);
  else if (clear) hipLaunchKernelGGL((map_fuse_kernel<true, false, false>), grid, block, 0, s, M, G);
  else if (color) hipLaunchKernelGGL((map_fuse_kernel<false, true, false>), grid, block, 0, s, M, G);
  else hipLaunchKernelGGL((map_fuse_kernel<false, false, false>), grid, block, 0, s, M, G);
  return hipGetLastError();
}

}  // namespace rpe
