// The workgroup scan the two mesh extractions place their ids with (rpe_mesh.hip M3-M5, rpe_mapmesh.hip P2-P4).
#pragma once
#include <hip/hip_runtime.h>

namespace rpe {
namespace {

// exclusive scan of x over the workgroup (NT threads): wave prefix by shuffles, the wave totals through LDS; `total` = the sum
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T x, T* lds, T& total) {
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  T inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    T run = 0;
    for (int w = 0; w < NT / 64; w++) { const T t = lds[w]; lds[w] = run; run += t; }
    lds[NT / 64] = run;
  }
  __syncthreads();
  const T r = lds[wave] + inc - x;
  total = lds[NT / 64];
  __syncthreads();   // lds is reused by the next call
  return r;
}

}  // namespace
}  // namespace rpe
