// gfx950 kernels that REGISTER a separate colour camera to the depth frame (include/rgbd_pose_hip.h Part 3, "Colour registration"): every
// depth pixel's level-0 vertex is moved into the colour camera, projected through its five-coefficient Brown-Conrady model and given the
// bilinear colour there -- unless something nearer projects into the same z-buffer cell, in which case the colour camera does not see
// the point and the pixel gets no colour (0x00000000) rather than the occluder's.
//
//   R1  register_splat_kernel    one depth pixel per lane: the projection, then the bits of Xk.z (a positive float: ordered as unsigned)
//                                by ONE no-return atomic minimum into the word of its base cell (i0, j0).  An integer minimum does not
//                                depend on arrival order: the buffer, and with it the output, is repeatable bit for bit.
//   R2  register_gather_kernel   one depth pixel per lane: the SAME projection (rig_project, one __device__ function, so that both kernels
//                                see the same bits), the visibility test against the pixel's own cell, four 4-byte gathers from the colour
//                                camera's RGBA8 image, the bilinear blend per channel and the RGBA8 store; optionally counts the A = 255
//                                pixels (one add per workgroup, over kRegCountWords words).
//
// The z-buffer of the header -- every pixel's z into the up to four cells (i0 + di, j0 + dj) inside the grid -- is kept in FACTORED form:
// the buffer holds the minimum per BASE cell, B(i0, j0), over (gw + 1) x (gh + 1) words (i0 = -1 .. gw - 1, stored at i0 + 1), and a
// cell's value is Z(ci, cj) = min of B(ci - di, cj - dj), di, dj = 0, 1, taken by R2 when it reads.  A minimum of minima is the same
// minimum, so Z is bit for bit the header's; a base cell outside the grid in one direction still feeds the cells inside (the border
// column and row of B), and cells outside the grid are never read.  One atomic per pixel instead of four: at 640 x 480 into a 640 x 480
// camera with cell 3 the four-atomic form spent 37 us in R1 on 34 240 words.
//
// The 3-byte colour image is staged to RGBA8 by C1 (rpe_color.hip) and the z-buffer is cleared by a memset; cell = 0 runs R2 alone.
// fp32, the written order, no FMA contraction; tests/register_oracle.py is the numpy statement.
#include "rpe_kernels.h"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kRegBlock = 256;   // one depth pixel per lane

struct RigPoint { float px, py, z; int x0, y0; };

// depth pixel i through the rig: false = no colour and no shadow
__device__ __forceinline__ bool rig_project(const RegisterRig& G, const float* __restrict__ vmap, int64_t i, RigPoint& P) {
  const float inf = __int_as_float(0x7f800000);
  const float X = vmap[3 * i], Y = vmap[3 * i + 1], Z = vmap[3 * i + 2];
  if (!(fabsf(X) < inf && fabsf(Y) < inf && fabsf(Z) < inf)) return false;
  const float kx = G.T.R[0] * X + G.T.R[1] * Y + G.T.R[2] * Z + G.T.t[0];
  const float ky = G.T.R[3] * X + G.T.R[4] * Y + G.T.R[5] * Z + G.T.t[1];
  const float kz = G.T.R[6] * X + G.T.R[7] * Y + G.T.R[8] * Z + G.T.t[2];
  if (!(kz > 0.0f)) return false;
  const float x = kx / kz, y = ky / kz;
  const float r2 = x * x + y * y;
  if (G.r2_max > 0.0f && !(r2 <= G.r2_max)) return false;
  const float rad = 1.0f + r2 * (G.k1 + r2 * (G.k2 + r2 * G.k3));
  const float xd = x * rad + ((2.0f * G.p1) * (x * y) + G.p2 * (r2 + 2.0f * (x * x)));
  const float yd = y * rad + (G.p1 * (r2 + 2.0f * (y * y)) + (2.0f * G.p2) * (x * y));
  const float px = G.cam.fx * xd + G.cam.cx, py = G.cam.fy * yd + G.cam.cy;
  if (!(fabsf(px) < inf && fabsf(py) < inf)) return false;
  const float x0 = floorf(px), y0 = floorf(py);
  if (!(x0 >= 0.0f && x0 <= (float)(G.cam.width - 2) && y0 >= 0.0f && y0 <= (float)(G.cam.height - 2))) return false;
  P.px = px; P.py = py; P.z = kz; P.x0 = (int)x0; P.y0 = (int)y0;
  return true;
}

// ---------------------------------------------------------------------------------------------- R1
__global__ __launch_bounds__(kRegBlock) void register_splat_kernel(const float* __restrict__ vmap, int64_t n, RegisterRig G,
                                                                   unsigned int* __restrict__ zbuf) {
  const int64_t i = (int64_t)blockIdx.x * kRegBlock + threadIdx.x;
  if (i >= n) return;
  RigPoint P;
  if (!rig_project(G, vmap, i, P)) return;
  const float fc = (float)G.cell;
  // base cell, stored at +1: i0 = -1 .. gw - 1 and j0 = -1 .. gh - 1 for a pixel that passed the range test (checked all the same)
  const int bi = (int)floorf((P.px + 0.5f) / fc - 0.5f) + 1, bj = (int)floorf((P.py + 0.5f) / fc - 0.5f) + 1;
  if (bi >= 0 && bi <= G.gw && bj >= 0 && bj <= G.gh) atomicMin(zbuf + bj * (G.gw + 1) + bi, (unsigned)__float_as_int(P.z));
}

// ---------------------------------------------------------------------------------------------- R2
// q(x) of the colour block
__device__ __forceinline__ unsigned quantise(float x) { return (unsigned)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f); }
__device__ __forceinline__ float lerp(float p, float q, float s) { return p + (q - p) * s; }

__global__ __launch_bounds__(kRegBlock) void register_gather_kernel(const float* __restrict__ vmap, int64_t n, RegisterRig G,
                                                                    const unsigned int* __restrict__ zbuf,
                                                                    const unsigned int* __restrict__ crgba, unsigned int* __restrict__ out,
                                                                    unsigned int* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * kRegBlock + threadIdx.x;
  const bool mine = i < n;                         // (no early return: the count below meets at a barrier)
  RigPoint P;
  bool ok = mine && rig_project(G, vmap, i, P);
  if (ok && G.cell > 0) {
    const float fc = (float)G.cell;
    const int ci = (int)floorf(((P.px + 0.5f) / fc - 0.5f) + 0.5f), cj = (int)floorf(((P.py + 0.5f) / fc - 0.5f) + 0.5f);
    ok = ci >= 0 && ci < G.gw && cj >= 0 && cj < G.gh;   // (always, for a pixel that passed the range test)
    if (ok) {
      // Z(ci, cj) = min of the base cells (ci - di, cj - dj), stored at +1: rows cj, cj + 1 and columns ci, ci + 1 of the buffer
      const unsigned int* b = zbuf + cj * (G.gw + 1) + ci;
      const unsigned zb = min(min(b[0], b[1]), min(b[G.gw + 1], b[G.gw + 2]));
      const float zmin = __int_as_float((int)zb);
      ok = (P.z - zmin) <= G.a + G.b * (zmin * zmin);
    }
  }
  unsigned rgba = 0u;
  if (ok) {
    const unsigned int* p = crgba + (int64_t)P.y0 * G.cam.width + P.x0;
    const unsigned c00 = p[0], c10 = p[1], c01 = p[G.cam.width], c11 = p[G.cam.width + 1];
    const float s = P.px - (float)P.x0, u = P.py - (float)P.y0;
    rgba = 0xff000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int sh = 8 * ch;
      const float top = lerp((float)((c00 >> sh) & 0xffu), (float)((c10 >> sh) & 0xffu), s);
      const float bot = lerp((float)((c01 >> sh) & 0xffu), (float)((c11 >> sh) & 0xffu), s);
      rgba |= quantise(lerp(top, bot, u)) << sh;
    }
  }
  if (mine) out[i] = rgba;
  // the count: summed over the workgroup first, then ONE add per workgroup, spread over kRegCountWords words that the host adds up.
  // (One add per wave on one word was measured at 45 - 57 us for R2 against 4.5 us without a count: 4 800 adds on one address.)
  if (count) {
    const int k = __syncthreads_count(ok ? 1 : 0);
    if (threadIdx.x == 0 && k) atomicAdd(count + (blockIdx.x % kRegCountWords), (unsigned)k);
  }
}

}  // namespace

hipError_t launch_register_splat(const float* vmap, int64_t n, const RegisterRig& G, unsigned int* zbuf, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kRegBlock - 1) / kRegBlock;
  hipLaunchKernelGGL(register_splat_kernel, dim3((unsigned)blocks), dim3(kRegBlock), 0, s, vmap, n, G, zbuf);
  return hipGetLastError();
}

hipError_t launch_register_gather(const float* vmap, int64_t n, const RegisterRig& G, const unsigned int* zbuf, const unsigned int* crgba,
                                  unsigned int* out, unsigned int* count, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kRegBlock - 1) / kRegBlock;
  hipLaunchKernelGGL(register_gather_kernel, dim3((unsigned)blocks), dim3(kRegBlock), 0, s, vmap, n, G, zbuf, crgba, out, count);
  return hipGetLastError();
}

RPE_PRELOAD(register_gather_kernel);

}  // namespace rpe
