// gfx950 kernel that MOVES the TSDF / colour volume by whole voxels (include/rgbd_pose_hip.h Part 3, "Moving volume";
// rpe_volume_shift): new voxel (i, j, k) := old voxel (i + di, j + dj, k + dk) where that lies inside the old window, all-zero bits
// elsewhere.  Out of place: the kernel reads the volume and writes a spare of the same size, the host swaps the two.
//
//   S1  volume_shift_kernel   A pure streaming kernel.  Both volumes hold 8 bytes per voxel at the same voxel index -- {tsdf, weight} as
//                             two floats, {r, g, b, wc} as four binary16 -- so both move as pairs of 32-bit words through the same code,
//                             in one launch.  A lane owns kShiftUnroll PAIRS of voxels that are consecutive in the linear voxel index
//                             (2p, 2p + 1): the destination of a pair is 16-byte aligned whatever the dims (an odd dim0 only lets a
//                             pair straddle a row end; each voxel carries its own (i, j, k)), and every store is one 16-byte store (the
//                             last voxel of an odd volume: 8 bytes).  The source of voxel v is v + delta with
//                             delta = di + dim0 * (dj + dim1 * dk), the same for every voxel whose source is inside.  Both sources inside
//                             and delta even: one aligned 16-byte load.  delta odd (an odd di in a volume of even dim0, say): the source
//                             pair is only 8-byte aligned and is read with two 8-byte loads -- no lane exchange, no load of a voxel
//                             the lane does not own (DESIGN.md section 5 has the reasoning).  A voxel whose source is outside is
//                             written as zeros without a load.  All loads of a lane are issued before its first store.
//
// The words are moved as integers: NaN payloads, -0 and denormals keep their bits.  The voxel index fits 32 bits (dims <= 1024: at most
// 2^30 voxels); the WORD index reaches 2^31 and is formed in 64 bits.  A source index is formed only for a voxel whose source (i + di,
// j + dj, k + dk) passed the range test, so it is the index of a voxel of the old volume: no access leaves the two arrays.
// tests/shift_oracle.py is the numpy statement.
#include "rpe_kernels.h"
#include <cstdint>

namespace rpe {

namespace {

constexpr int kShiftBlock = 256;
constexpr int kShiftUnroll = 4;   // pairs per lane: 4 x (16 + 16) bytes of loads in flight with a colour volume

struct ShiftArgs { int dim[3]; int d[3]; unsigned nvox; long long delta; };

// the pair (v0, v0 + 1) of one volume: load phase
__device__ __forceinline__ uint4 load_pair(const uint32_t* __restrict__ src, int64_t s0, bool in0, bool in1, bool even) {
  uint4 a = make_uint4(0u, 0u, 0u, 0u);
  if (in0 && in1 && even) return *reinterpret_cast<const uint4*>(src + 2 * s0);
  if (in0) { const uint2 t = *reinterpret_cast<const uint2*>(src + 2 * s0); a.x = t.x; a.y = t.y; }
  if (in1) { const uint2 t = *reinterpret_cast<const uint2*>(src + 2 * (s0 + 1)); a.z = t.x; a.w = t.y; }
  return a;
}

__device__ __forceinline__ void store_pair(uint32_t* __restrict__ dst, unsigned v0, bool has1, const uint4& a) {
  uint32_t* q = dst + 2 * (int64_t)v0;
  if (has1) *reinterpret_cast<uint4*>(q) = a;
  else *reinterpret_cast<uint2*>(q) = make_uint2(a.x, a.y);
}

template <bool COLOR>
__global__ __launch_bounds__(kShiftBlock) void volume_shift_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                   const uint32_t* __restrict__ csrc, uint32_t* __restrict__ cdst,
                                                                   ShiftArgs S) {
  const unsigned d0 = (unsigned)S.dim[0], d1 = (unsigned)S.dim[1];
  const bool even = (S.delta & 1) == 0;
  uint4 a[kShiftUnroll], c[kShiftUnroll];
  unsigned v[kShiftUnroll];
  bool live[kShiftUnroll], has1[kShiftUnroll];
#pragma unroll
  for (int u = 0; u < kShiftUnroll; u++) {
    // (blocks x kShiftUnroll x kShiftBlock pairs cover nvox with less than one block's worth to spare: 2p stays below 2^31)
    const unsigned v0 = 2u * ((blockIdx.x * kShiftUnroll + u) * kShiftBlock + threadIdx.x);
    v[u] = v0;
    live[u] = v0 < S.nvox;
    has1[u] = live[u] && v0 + 1u < S.nvox;
    a[u] = make_uint4(0u, 0u, 0u, 0u); c[u] = a[u];
    if (!live[u]) continue;
    const unsigned row = v0 / d0;
    int i = (int)(v0 - row * d0), k = (int)(row / d1), j = (int)(row - (unsigned)k * d1);
    auto inside = [&](int ii, int jj, int kk) {
      const int x = ii + S.d[0], y = jj + S.d[1], z = kk + S.d[2];
      return x >= 0 && x < S.dim[0] && y >= 0 && y < S.dim[1] && z >= 0 && z < S.dim[2];
    };
    const bool in0 = inside(i, j, k);
    if (++i == S.dim[0]) { i = 0; if (++j == S.dim[1]) { j = 0; k++; } }
    const bool in1 = has1[u] && inside(i, j, k);
    const int64_t s0 = (int64_t)v0 + S.delta;   // used only where in0 (s0) or in1 (s0 + 1) vouches for it
    a[u] = load_pair(src, s0, in0, in1, even);
    if (COLOR) c[u] = load_pair(csrc, s0, in0, in1, even);
  }
#pragma unroll
  for (int u = 0; u < kShiftUnroll; u++) {
    if (!live[u]) continue;
    store_pair(dst, v[u], has1[u], a[u]);
    if (COLOR) store_pair(cdst, v[u], has1[u], c[u]);
  }
}

}  // namespace

hipError_t launch_volume_shift(const float* vol, float* vol_out, const unsigned short* cvol, unsigned short* cvol_out, const int dim[3],
                               const int shift[3], hipStream_t s) {
  ShiftArgs S;
  for (int a = 0; a < 3; a++) { S.dim[a] = dim[a]; S.d[a] = shift[a]; }
  S.nvox = (unsigned)((int64_t)dim[0] * dim[1] * dim[2]);
  S.delta = (long long)shift[0] + (long long)dim[0] * ((long long)shift[1] + (long long)dim[1] * (long long)shift[2]);
  const unsigned per_block = 2u * kShiftUnroll * kShiftBlock;
  const dim3 grid((S.nvox + per_block - 1) / per_block), block(kShiftBlock);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(vol);
  uint32_t* dst = reinterpret_cast<uint32_t*>(vol_out);
  const uint32_t* csrc = reinterpret_cast<const uint32_t*>(cvol);
  uint32_t* cdst = reinterpret_cast<uint32_t*>(cvol_out);
  if (cvol) hipLaunchKernelGGL((volume_shift_kernel<true>), grid, block, 0, s, src, dst, csrc, cdst, S);
  else hipLaunchKernelGGL((volume_shift_kernel<false>), grid, block, 0, s, src, dst, csrc, cdst, S);
  return hipGetLastError();
}

RPE_PRELOAD(volume_shift_kernel<false>);

}  // namespace rpe
