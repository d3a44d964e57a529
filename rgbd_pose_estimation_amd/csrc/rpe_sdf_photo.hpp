// THE VOLUME COLOUR TERM (include/rgbd_pose_hip.h Part 3, "Volume colour term"; tests/sdf_photo_oracle.py is its numpy statement; included
// by rpe_frontend.hip, behind the volume term whose cell, corner fetch and row it shares): a photometric term beside the volume term.  A
// frame vertex is moved to the world under the pose guess; in the cell it lands in, the trilinear LUMA of the eight colour-volume corners
// against the frame's intensity is the residual, the gradient of the same eight lumas the row.  No raycast, no model, no model colour.
// Followed BIT-EXACTLY: fp32, the written order, no FMA contraction (rpe_volume_field.hpp has switched it off).  The rule is a template
// over the colour-corner fetch, as the volume term's is over the TSDF's: dense_colour_corners reads the window's colour volume; a fetch
// over the brick grid's colour planes can follow without the rule being written again.
//
//   sdf_photo_rows_kernel       {r, J[0..5]} of the photometric row of every frame pixel, unscaled (NaN where there is no row): the
//                               residual image and the tests' hook.
//   icp_sdf_photo_kernel<GEO, BLK>  one Gauss-Newton round in ONE launch over the level's pixels.  ONE pixel per loop trip, as
//                               icp_map_sdf_kernel: per pixel 16 B streamed (vertex, intensity; 28 B with the normal gate) and sixteen
//                               8-byte gathers -- the cell's eight {tsdf, weight} and eight {r, g, b, wc} corners, whose addresses depend
//                               on the cell alone and are all issued before the first is looked at.  GEO: the volume term's row (weight 1,
//                               normal gate included) AND the photometric row (weight lam), both widened to fp64 and their 56 products
//                               added with fp64 fused multiply-adds (a product of two floats is exact in fp64); else the photometric
//                               row alone.  One reduction, one record of 31 sums laid out as icp_photo_kernel's: H (21) | g (6) of both
//                               terms | geometric cost | geometric rows | photometric cost | photometric rows.
#pragma once
#include "rpe_sdf_rule.hpp"

namespace rpe {
namespace {

// the eight corner voxels {r | g << 16, b | wc << 16} (binary16, as blend's) of the cell i0 of the dense window's colour volume,
// c[di + 2 dj + 4 dk]: the colour volume holds a voxel at the TSDF's index
struct dense_colour_corners {
  const uint2* __restrict__ cvol;
  int64_t sy, sz;
  __device__ __forceinline__ dense_colour_corners(const uint2* __restrict__ c, const VolumeGeometry& G)
      : cvol(c), sy((int64_t)G.dim[0]), sz((int64_t)G.dim[0] * G.dim[1]) {}
  __device__ __forceinline__ bool operator()(const int (&i0)[3], uint2 (&c)[8]) const {
    const uint2* b = cvol + (int64_t)i0[2] * sz + (int64_t)i0[1] * sy + (int64_t)i0[0];
    c[0] = b[0]; c[1] = b[1];
    c[2] = b[sy]; c[3] = b[sy + 1];
    c[4] = b[sz]; c[5] = b[sz + 1];
    c[6] = b[sz + sy]; c[7] = b[sz + sy + 1];
    return true;
  }
};

// step 3: a corner's luma on the 0 .. 255 scale, from its binary16 channels widened exactly
__device__ __forceinline__ float corner_luma(const uint2& c) {
  return (0.299f * h2f(c.x & 0xffffu) + 0.587f * h2f(c.x >> 16)) + 0.114f * h2f(c.y & 0xffffu);
}

// step 3 on the cell's colour corners c[di + 2 dj + 4 dk]: the eight lumas; false unless all eight colour weights are > 0
__device__ __forceinline__ bool colour_lumas(const uint2 (&c)[8], float (&l)[8]) {
  bool known = true;
#pragma unroll
  for (int m = 0; m < 8; m++) { known = known && h2f(c[m].y >> 16) > 0.0f; l[m] = corner_luma(c[m]); }
  return known;
}

// Steps 2, 4 and 5 on the cell's TSDF corners v, the colour corners' lumas l (both [di + 2 dj + 4 dk]; known: colour_lumas' answer) and
// a: the UNSCALED r [levels] and J = [a | Xc x a], 0 when the pixel has no row.  The slope and normal gates of the volume term are not
// asked: a photometric row stands wherever the point lies on the fused surface within the gate and the cell has colour.  A colour channel
// that is NaN or Inf under a weight > 0 is not gated either: it goes into r and J as any value does
//
// In two parts, so that a caller whose colour fetch is dear may ask the TSDF corners first and fetch colour only past them.  Step 2,
// what the TSDF corners alone decide, on top of the earlier answers `ok`:
__device__ __forceinline__ bool sdf_photo_gate(const float2 (&v)[8], const float (&a)[3], const VolumeGeometry& G, float gate, bool ok) {
#pragma unroll
  for (int m = 0; m < 8; m++) ok = ok && v[m].y > 0.0f && fabsf(v[m].x) < 1.0f;
  const float D = trilerp(v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, a[0], a[1], a[2]);
  return ok && fabsf(D * G.tr) <= gate;
}
// ... and steps 4 and 5 for a pixel that every gate has let through (ok)
__device__ __forceinline__ bool sdf_photo_value(bool ok, const float (&l)[8], const float (&a)[3], const VolumeGeometry& G, const PoseF& T, float x,
                                                float y, float z, float If, float& r, float (&J)[6]) {
  r = 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) J[k] = 0.f;
  if (!ok) return false;
  const float Iv = trilerp(l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], a[0], a[1], a[2]);
  const float gx = bilerp(l[1] - l[0], l[3] - l[2], l[5] - l[4], l[7] - l[6], a[1], a[2]);
  const float gy = lerp(lerp(l[2] - l[0], l[3] - l[1], a[0]), lerp(l[6] - l[4], l[7] - l[5], a[0]), a[2]);
  const float gz = lerp(lerp(l[4] - l[0], l[5] - l[1], a[0]), lerp(l[6] - l[2], l[7] - l[3], a[0]), a[1]);
  const float mx = gx / G.s, my = gy / G.s, mz = gz / G.s;
  const float a0 = -((T.R[0] * mx + T.R[1] * my) + T.R[2] * mz);
  const float a1 = -((T.R[3] * mx + T.R[4] * my) + T.R[5] * mz);
  const float a2 = -((T.R[6] * mx + T.R[7] * my) + T.R[8] * mz);
  r = Iv - If;
  J[0] = a0; J[1] = a1; J[2] = a2;
  J[3] = y * a2 - z * a1; J[4] = z * a0 - x * a2; J[5] = x * a1 - y * a0;
  return true;
}
__device__ __forceinline__ bool sdf_photo_row(const float2 (&v)[8], const float (&l)[8], bool known, const float (&a)[3], const VolumeGeometry& G,
                                              const PoseF& T, float gate, float x, float y, float z, float If, float& r, float (&J)[6]) {
  return sdf_photo_value(sdf_photo_gate(v, a, G, gate, known && __builtin_isfinite(If)), l, a, G, T, x, y, z, If, r, J);
}

// The whole rule for one pixel.  Corners / Colours: (i0, corner[8]) -> false when the cell has no voxels.
template <class Corners, class Colours>
__device__ __forceinline__ bool sdf_photo_pixel(Corners corners, Colours colours, const VolumeGeometry& G, const PoseF& T, float gate, float x,
                                                float y, float z, float If, float& r, float (&J)[6]) {
  int i0[3];
  float a[3];
  float2 v[8];
  uint2 c[8];
  const bool in = sdf_cell(G, T, x, y, z, i0, a);   // (without a cell: cell 0, whose corners are fetched and not looked at)
  const bool have = corners(i0, v);
  const bool col = colours(i0, c);
  float l[8];
  const bool known = colour_lumas(c, l);
  const bool ok = sdf_photo_row(v, l, known, a, G, T, gate, x, y, z, If, r, J);
  if (in && have && col && ok) return true;
  r = 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) J[k] = 0.f;
  return false;
}

constexpr int kSdfPhotoAcc = 31;

// The round kernel's arguments as the kernarg segment lays them out, for late_finish_at
struct SdfPhotoRoundArgs {
  const float* vmap; const float* nmap; const float* fint; int64_t n; const float* vol; const uint2* cvol;
  VolumeGeometry G; SdfParams Q; float lam; PoseF T; Finish fin;
};
// (tests/test_sdf_photo_oracle.py reads the same offset and size from the code object's metadata)
static_assert(offsetof(SdfPhotoRoundArgs, fin) == 152 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(SdfPhotoRoundArgs, T) == 104 && sizeof(PoseF) == 48, "photo_late_pose: where the kernarg segment holds the pose");

// late_pose_at (rpe_frontend.hip) for this kernel, as icp_map_sdf_kernel's late_pose and for its reason: beside geometry, gates and six
// pointers the pose as a plain argument costs 2 scalar spills, and the vector register that holds them is the 129th
__device__ __forceinline__ PoseF photo_late_pose() { return late_pose_at((unsigned)offsetof(SdfPhotoRoundArgs, T)); }

// a row into the fp64 sums: H and g into the shared entries, the cost into its own.  A pixel without a row has r = 0 and J = 0
__device__ __forceinline__ void add_row_f64(const float r, const float (&J)[6], double (&acc)[29], int cost) {
  double Jd[6];
#pragma unroll
  for (int a = 0; a < 6; a++) Jd[a] = (double)J[a];
  const double rd = (double)r;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int b = a; b < 6; b++) { acc[k] = __builtin_fma(Jd[a], Jd[b], acc[k]); k++; }
    acc[21 + a] = __builtin_fma(Jd[a], rd, acc[21 + a]);
  }
  acc[cost] = __builtin_fma(rd, rd, acc[cost]);
}

// four waves per SIMD's worth of registers: 128
template <bool GEO, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_sdf_photo_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, const float* __restrict__ fint, int64_t n, const float* __restrict__ vol,
    const uint2* __restrict__ cvol, VolumeGeometry G, SdfParams Q, float lam, PoseF /* read by photo_late_pose */,
    Finish /* read by late_finish_at */) {
  double acc[29];   // 0 .. 26 H | g of both terms, 27 the geometric cost, 28 the photometric cost
#pragma unroll
  for (int k = 0; k < 29; k++) acc[k] = 0.0;
  float grows = 0.f, prows = 0.f;
  const dense_corners corners(vol, G);
  const dense_colour_corners colours(cvol, G);
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2], If = fint[i];
    int i0[3];
    float a[3];
    float2 v[8];
    uint2 c[8];
    const bool in = sdf_cell(G, photo_late_pose(), x, y, z, i0, a);
    corners(i0, v);   // sixteen gathers whose addresses the cell alone decides: all in flight before the first is looked at
    colours(i0, c);
    float l[8], r, J[6];
    const bool known = colour_lumas(c, l);   // (the colour corners are done with before either row is formed: 9 registers for 16)
    const bool okp = sdf_photo_row(v, l, known, a, G, photo_late_pose(), Q.gate, x, y, z, If, r, J) && in;
    // step 6: r' = lam r, J' = lam J in fp32 (0 for a pixel without a row)
    r = okp ? lam * r : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = okp ? lam * J[k] : 0.f;
    add_row_f64(r, J, acc, 28);
    prows += okp ? 1.f : 0.f;   // (a thread sees fewer than 2^24 pixels: exact)
    if (GEO) {
      // the geometric row is formed behind the photometric one, when the lumas are dead: left to itself the compiler pairs the two
      // gradients' arithmetic (both run down the same lerp chain) into packed operations on register pairs, and the copies into those
      // pairs are the 129th register
#pragma unroll
      for (int m = 0; m < 8; m++) asm volatile("" : "+v"(v[m].x) : "v"(r));
      float len;
      bool ok = sdf_row(v, a, G, photo_late_pose(), Q, x, y, z, r, J, len) && in;
      if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
      if (!ok) {
        r = 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) J[k] = 0.f;
      }
      add_row_f64(r, J, acc, 27);
      grows += ok ? 1.f : 0.f;
    }
  }
  double sums[kSdfPhotoAcc];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)grows; sums[29] = acc[28]; sums[30] = (double)prows;
  reduce_and_finish<kSdfPhotoAcc, kNlLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(SdfPhotoRoundArgs, fin)));   // host-driven only
}

__global__ __launch_bounds__(kSdfRowsBlock) void sdf_photo_rows_kernel(const float* __restrict__ vmap, const float* __restrict__ fint, int64_t n,
                                                                       const float* __restrict__ vol, const uint2* __restrict__ cvol,
                                                                       VolumeGeometry G, float gate, PoseF T, float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kSdfRowsBlock + threadIdx.x;
  if (i >= n) return;
  float r, J[6];
  const bool ok = sdf_photo_pixel(dense_corners(vol, G), dense_colour_corners(cvol, G), G, T, gate, vmap[3 * i], vmap[3 * i + 1],
                                  vmap[3 * i + 2], fint[i], r, J);
  store_row(rows, n, i, ok, r, J);
}

// a node per new kernel, beside the unit's own (one code object: whichever is touched first loads all of it)
namespace photo_rows_node { RPE_PRELOAD(sdf_photo_rows_kernel); }
namespace photo_round_node { RPE_PRELOAD(icp_sdf_photo_kernel<true, 256>); }

}  // namespace

hipError_t launch_icp_sdf_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol, const unsigned short* cvol,
                                const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const uint2* cv = reinterpret_cast<const uint2*>(cvol);
  const int blk = pick_block(rt);   // one pixel per thread while the grid allows it
  const int grid = round_grid(rt, n, blk);
#define RPE_SDF_PHOTO_LAUNCH(GEO, B) \
  hipLaunchKernelGGL((icp_sdf_photo_kernel<GEO, B>), dim3(grid), dim3(B), 0, s, vmap, nmap, fint, n, vol, cv, G, Q, lam, T, fin)
  if (blk == 512) { if (geometric) RPE_SDF_PHOTO_LAUNCH(true, 512); else RPE_SDF_PHOTO_LAUNCH(false, 512); }
  else { if (geometric) RPE_SDF_PHOTO_LAUNCH(true, 256); else RPE_SDF_PHOTO_LAUNCH(false, 256); }
#undef RPE_SDF_PHOTO_LAUNCH
  return hipGetLastError();
}

hipError_t launch_sdf_photo_rows(const float* vmap, const float* fint, int64_t n, const float* vol, const unsigned short* cvol,
                                 const VolumeGeometry& G, float dist_thr, const double* pose12, float* rows, hipStream_t s) {
  const int64_t blocks = (n + kSdfRowsBlock - 1) / kSdfRowsBlock;
  hipLaunchKernelGGL(sdf_photo_rows_kernel, dim3((unsigned)blocks), dim3(kSdfRowsBlock), 0, s, vmap, fint, n, vol,
                     reinterpret_cast<const uint2*>(cvol), G, dist_thr, pose_f(pose12), rows);
  return hipGetLastError();
}

}  // namespace rpe

// the same term on the whole map -- the window plus the archived bricks: the fetch over the brick grid's colour planes and its two kernels
#include "rpe_map_sdf_photo.hpp"
