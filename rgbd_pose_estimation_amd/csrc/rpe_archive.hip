// gfx950 kernels of the volume archive (include/rgbd_pose_hip.h Part 3, "Volume archive"; host side in rpe_archive_api.hip): the bricks
// -- 8 x 8 x 8 voxels, aligned in world voxel coordinates -- that a shift of the moving volume pushes out of the window are kept in a
// pool of 4-KB slots and written back when the window returns over them.  A brick of the window is 64 rows of 8 voxels = 64 bytes each,
// dim0 voxels apart; a slot holds the same 64 rows back to back, in (z, y, x) order.
//
//   A1  brick_occupancy_kernel   Visits only the bricks that leave: at most three disjoint boxes of bricks, enumerated box after box with
//                                x fastest.  One wave per brick; a lane ORs its four 16-byte loads of the tsdf brick and, with a colour
//                                volume, its four of the colour brick (all eight issued before the first use), one ballot says whether
//                                any of the brick's 32-bit words is non-zero, lane 0 writes the brick's flag.  No atomics, no LDS.
//   A2  brick_copy_kernel        Takes a list of (window brick, slot) pairs; one wave per pair.  TO_POOL gathers the window's 64-byte rows
//                                into the slot's contiguous 4 KB, !TO_POOL scatters them back.  16-byte loads and stores only, all of a
//                                lane's loads before its first store, both volumes in one launch.  COLOR = 0: tsdf only; 1: the colour
//                                brick too; 2 (TO_POOL only): there is a colour pool but no colour volume, the slot's colour is zeroed.
//
// Chunk c = 64 u + lane (u = 0 .. 3) of a brick is the 16 bytes at byte 16 c of its slot: row c / 4 (z = row / 8, y = row % 8), voxels
// 2 (c % 4) and the next of that row.  So one wave instruction touches 1 KB of the slot in one piece and sixteen 64-byte rows of the window.
// Indices as in rpe_shift.hip: the voxel index fits 32 bits (dims <= 1024), the word index is formed in 64 bits.  An address is formed
// only for a brick inside the window (its index below the number of bricks) and a slot below the pool's capacity; a pair that fails
// either test is skipped.  The words move as integers.  tests/archive_oracle.py is the numpy statement.
#include "rpe_kernels.h"
#include <cstdint>

namespace rpe {

namespace {

constexpr int kArchiveBlock = 256;                     // 4 waves = 4 bricks per workgroup
constexpr int kBrickChunks = 4;                        // 16-byte chunks per lane and volume: 64 lanes x 4 x 16 B = 4 KB
constexpr int64_t kSlotWords = kArchiveSlotBytes / 4;

struct BrickGrid { int dim0, dim1; int nb[3]; unsigned nbricks; };

// the voxel index of chunk c of the brick (bx, by, bz): even, so the chunk is 16-byte aligned in the window
__device__ __forceinline__ unsigned chunk_voxel(const BrickGrid& G, unsigned v0, int c) {
  const unsigned row = (unsigned)c >> 2, z = row >> 3, y = row & 7u;
  return v0 + (z * (unsigned)G.dim1 + y) * (unsigned)G.dim0 + 2u * ((unsigned)c & 3u);
}
__device__ __forceinline__ unsigned brick_voxel0(const BrickGrid& G, unsigned bx, unsigned by, unsigned bz) {
  return ((bz * 8u) * (unsigned)G.dim1 + by * 8u) * (unsigned)G.dim0 + bx * 8u;
}
__device__ __forceinline__ uint4 load16(const uint32_t* __restrict__ p, int64_t word) { return *reinterpret_cast<const uint4*>(p + word); }
__device__ __forceinline__ void store16(uint32_t* __restrict__ p, int64_t word, const uint4& a) { *reinterpret_cast<uint4*>(p + word) = a; }

template <bool COLOR>
__global__ __launch_bounds__(kArchiveBlock) void brick_occupancy_kernel(const uint32_t* __restrict__ vol, const uint32_t* __restrict__ cvol,
                                                                        BrickGrid G, ArchiveBoxes B, uint32_t* __restrict__ flags) {
  const int lane = (int)(threadIdx.x & 63u);
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kArchiveBlock / 64) + (threadIdx.x >> 6)));
  if (g >= B.first[3]) return;                         // the whole wave
  const int b = g >= B.first[2] ? 2 : g >= B.first[1] ? 1 : 0;
  int r = g - B.first[b];
  const int x = B.lo[b][0] + r % B.n[b][0]; r /= B.n[b][0];
  const int y = B.lo[b][1] + r % B.n[b][1];
  const int z = B.lo[b][2] + r / B.n[b][1];
  if (x < 0 || x >= G.nb[0] || y < 0 || y >= G.nb[1] || z < 0 || z >= G.nb[2]) return;   // not a brick of the window: no address
  const unsigned v0 = brick_voxel0(G, (unsigned)x, (unsigned)y, (unsigned)z);
  uint4 a[kBrickChunks], c[kBrickChunks];
#pragma unroll
  for (int u = 0; u < kBrickChunks; u++) {
    const int64_t w = 2 * (int64_t)chunk_voxel(G, v0, 64 * u + lane);
    a[u] = load16(vol, w);
    c[u] = COLOR ? load16(cvol, w) : make_uint4(0u, 0u, 0u, 0u);
  }
  uint32_t any = 0;
#pragma unroll
  for (int u = 0; u < kBrickChunks; u++) any |= a[u].x | a[u].y | a[u].z | a[u].w | c[u].x | c[u].y | c[u].z | c[u].w;
  const unsigned long long m = __ballot(any != 0u);
  if (lane == 0) flags[g] = m ? 1u : 0u;
}

template <bool TO_POOL, int COLOR>
__global__ __launch_bounds__(kArchiveBlock) void brick_copy_kernel(uint32_t* __restrict__ vol, uint32_t* __restrict__ cvol,
                                                                   uint32_t* __restrict__ pool, uint32_t* __restrict__ cpool, BrickGrid G,
                                                                   const int2* __restrict__ pairs, int n, int capacity) {
  const int lane = (int)(threadIdx.x & 63u);
  const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kArchiveBlock / 64) + (threadIdx.x >> 6)));
  if (g >= n) return;
  const int2 p = pairs[g];
  if (p.x < 0 || (unsigned)p.x >= G.nbricks || p.y < 0 || p.y >= capacity) return;   // no address outside the window or the pool
  const unsigned bx = (unsigned)p.x % (unsigned)G.nb[0], t = (unsigned)p.x / (unsigned)G.nb[0];
  const unsigned by = t % (unsigned)G.nb[1], bz = t / (unsigned)G.nb[1];
  const unsigned v0 = brick_voxel0(G, bx, by, bz);
  const int64_t s0 = (int64_t)p.y * kSlotWords;
  uint4 a[kBrickChunks], c[kBrickChunks];
  int64_t w[kBrickChunks];
#pragma unroll
  for (int u = 0; u < kBrickChunks; u++) {
    const int ch = 64 * u + lane;
    w[u] = 2 * (int64_t)chunk_voxel(G, v0, ch);
    const int64_t s = s0 + 4 * ch;
    a[u] = TO_POOL ? load16(vol, w[u]) : load16(pool, s);
    c[u] = make_uint4(0u, 0u, 0u, 0u);
    if (COLOR == 1) c[u] = TO_POOL ? load16(cvol, w[u]) : load16(cpool, s);
  }
#pragma unroll
  for (int u = 0; u < kBrickChunks; u++) {
    const int64_t s = s0 + 4 * (64 * u + lane);
    if (TO_POOL) { store16(pool, s, a[u]); if (COLOR != 0) store16(cpool, s, c[u]); }
    else { store16(vol, w[u], a[u]); if (COLOR == 1) store16(cvol, w[u], c[u]); }
  }
}

BrickGrid grid_of(const int dim[3]) {
  BrickGrid G;
  G.dim0 = dim[0]; G.dim1 = dim[1];
  for (int a = 0; a < 3; a++) G.nb[a] = dim[a] / 8;
  G.nbricks = (unsigned)G.nb[0] * (unsigned)G.nb[1] * (unsigned)G.nb[2];
  return G;
}

}  // namespace

hipError_t launch_brick_occupancy(const float* vol, const unsigned short* cvol, const int dim[3], const ArchiveBoxes& B, unsigned int* flags,
                                  hipStream_t s) {
  if (B.first[3] <= 0) return hipSuccess;
  const dim3 grid((unsigned)((B.first[3] + kArchiveBlock / 64 - 1) / (kArchiveBlock / 64))), block(kArchiveBlock);
  const uint32_t* v = reinterpret_cast<const uint32_t*>(vol);
  const uint32_t* cv = reinterpret_cast<const uint32_t*>(cvol);
  if (cvol) hipLaunchKernelGGL((brick_occupancy_kernel<true>), grid, block, 0, s, v, cv, grid_of(dim), B, flags);
  else hipLaunchKernelGGL((brick_occupancy_kernel<false>), grid, block, 0, s, v, cv, grid_of(dim), B, flags);
  return hipGetLastError();
}

hipError_t launch_brick_copy(bool to_pool, float* vol, unsigned short* cvol, unsigned int* pool, unsigned int* cpool, const int dim[3],
                             const int* pairs, int n, int capacity, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + kArchiveBlock / 64 - 1) / (kArchiveBlock / 64))), block(kArchiveBlock);
  uint32_t* v = reinterpret_cast<uint32_t*>(vol);
  uint32_t* cv = reinterpret_cast<uint32_t*>(cvol);
  const int2* pr = reinterpret_cast<const int2*>(pairs);
  const BrickGrid G = grid_of(dim);
  // the colour brick moves when the window and the pool both have colour; a brick that leaves a window WITHOUT colour zeroes its slot's
  // colour (the slot may have held another brick's); a brick that returns to a window whose colour the pool never saw finds the zeros
  // the shift left
  const int color = cvol && cpool ? 1 : to_pool && cpool ? 2 : 0;
  if (to_pool) {
    if (color == 1) hipLaunchKernelGGL((brick_copy_kernel<true, 1>), grid, block, 0, s, v, cv, pool, cpool, G, pr, n, capacity);
    else if (color == 2) hipLaunchKernelGGL((brick_copy_kernel<true, 2>), grid, block, 0, s, v, cv, pool, cpool, G, pr, n, capacity);
    else hipLaunchKernelGGL((brick_copy_kernel<true, 0>), grid, block, 0, s, v, cv, pool, cpool, G, pr, n, capacity);
  } else {
    if (color == 1) hipLaunchKernelGGL((brick_copy_kernel<false, 1>), grid, block, 0, s, v, cv, pool, cpool, G, pr, n, capacity);
    else hipLaunchKernelGGL((brick_copy_kernel<false, 0>), grid, block, 0, s, v, cv, pool, cpool, G, pr, n, capacity);
  }
  return hipGetLastError();
}

RPE_PRELOAD(brick_occupancy_kernel<false>);

}  // namespace rpe
