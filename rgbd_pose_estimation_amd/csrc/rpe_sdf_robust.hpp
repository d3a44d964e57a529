// THE ROBUST VOLUME TERMS (include/rgbd_pose_hip.h Part 3, "Robust volume terms"; tests/sdf_robust_oracle.py is their numpy statement;
// included by rpe_map_sdf_photo.hpp at its end, so compiled into rpe_frontend.hip behind the four volume terms): the round kernels of the volume term and of the volume colour
// term, on the window and on the map, with the robust weight of rpe_sdf_robust_rule.hpp on every row.  No new per-pixel arithmetic but
// the weight: cell, corner fetches, rows and gates are the siblings' device functions (rpe_sdf_rule.hpp, rpe_sdf_photo.hpp, the map
// fetches of rpe_frontend.hip and rpe_map_sdf_photo.hpp), composed as the siblings compose them, and the records are laid out as theirs.
// The siblings themselves are untouched: with the robust kind NONE the host launches them, so the unweighted calls give the bits they
// gave.  The kind is a template argument (no scalar register); the scales are arguments of their own, behind the gates.
//
//   icp_sdf_robust_kernel<KIND, BLK>                  icp_sdf_kernel's record, formed as icp_map_sdf_kernel forms its own: ONE pixel per loop trip,
//                                                     the row and its weight widened to fp64 (w J is exact there).  sdf_group's four pixels
//                                                     in flight fill icp_sdf_kernel's 128 registers: with the weights it spills.
//   icp_map_sdf_robust_kernel<KIND, BLK>              icp_map_sdf_kernel with the weight.
//   icp_sdf_photo_robust_kernel<KIND, GEO, BLK>       icp_sdf_photo_kernel: the geometric row weighted with k, the photometric row with
//   icp_map_sdf_photo_robust_kernel<KIND, GEO, BLK>   photo_k on its UNSCALED residual, then scaled by lam as it was; photo_k = 0: weight 1.
//   sdf_robust_weights_kernel<MAP, PHOTO>             the tests' hook: the rows kernels' rule, then the weight; NaN where there is no row.
#pragma once
#include "rpe_sdf_robust_rule.hpp"

namespace rpe {
namespace {

// the scales of the colour kernels: the geometric row's [m] and the photometric row's [levels, before lam; 0 = weight 1]
struct RobustScales { float k, photo_k; };

// add_row_f64 with a weight: w J J^T into H, w J r into g, w r^2 into the cost.  w J and w r are exact in fp64 (two floats), so a sum
// carries fp64 accumulation error only, as the siblings'.  A pixel without a row has r = 0 and J = 0
__device__ __forceinline__ void add_weighted_row_f64(const float w, const float r, const float (&J)[6], double (&acc)[29], int cost) {
  double Jd[6];
#pragma unroll
  for (int a = 0; a < 6; a++) Jd[a] = (double)J[a];
  const double rd = (double)r;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    // the weight is widened where it is used (the empty asm keeps the six conversions apart): held as a double through the rows it is
    // the 129th register of icp_map_sdf_photo_robust_kernel<.., false, ..>
    float wa = w;
    asm volatile("" : "+v"(wa));
    const double x = (double)wa * Jd[a];
#pragma unroll
    for (int b = a; b < 6; b++) { acc[k] = __builtin_fma(x, Jd[b], acc[k]); k++; }
    acc[21 + a] = __builtin_fma(x, rd, acc[21 + a]);
  }
  acc[cost] = __builtin_fma((double)w * rd, rd, acc[cost]);
}

// ---------------------------------------------------------------------------------------------- the volume term on the window
struct SdfRobustRoundArgs { const float* vmap; const float* nmap; int64_t n; const float* vol; VolumeGeometry G; SdfParams Q; float k; PoseF T; Finish fin; };
// (tests/test_sdf_robust_oracle.py reads the same offset and size from the code object's metadata)
static_assert(offsetof(SdfRobustRoundArgs, fin) == 136 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");

template <int KIND, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_sdf_robust_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n, const float* __restrict__ vol, VolumeGeometry G, SdfParams Q,
    float k, PoseF T, Finish /* read by late_finish_at */) {
  double acc[29];   // 0 .. 27 as icp_sdf_kernel's sums; 28 is not used
#pragma unroll
  for (int i = 0; i < 29; i++) acc[i] = 0.0;
  float rows = 0.f;
  const dense_corners corners(vol, G);
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    // sdf_pixel in its parts, as icp_map_sdf_kernel's trip: the normal is fetched behind the corners
    float r, J[6], len;
    bool ok = sdf_pixel_row(corners, G, T, Q, vmap[q], vmap[q + 1], vmap[q + 2], r, J, len);
    if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
    add_weighted_row_f64(ok ? robust_weight<KIND>(r, k) : 0.f, r, J, acc, 27);   // (a pixel without a row has r = 0 and J = 0)
    rows += ok ? 1.f : 0.f;   // every row that passed the gates (a thread sees fewer than 2^24 pixels: exact)
  }
  double sums[29];
#pragma unroll
  for (int i = 0; i < 28; i++) sums[i] = acc[i];
  sums[28] = (double)rows;
  reduce_and_finish<29, kNeLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(SdfRobustRoundArgs, fin)));   // host-driven only
}

// ---------------------------------------------------------------------------------------------- ... and on the map
struct MapSdfRobustRoundArgs { const float* vmap; const float* nmap; int64_t n; MapSdfView S; VolumeGeometry G; SdfParams Q; float k; PoseF T; Finish fin; };
static_assert(offsetof(MapSdfRobustRoundArgs, fin) == 192 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(MapSdfRobustRoundArgs, T) == 144 && sizeof(PoseF) == 48, "map_robust_late_pose: where the kernarg segment holds the pose");
__device__ __forceinline__ PoseF map_robust_late_pose() { return late_pose_at((unsigned)offsetof(MapSdfRobustRoundArgs, T)); }

template <int KIND, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_map_sdf_robust_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n, MapSdfView S, VolumeGeometry G, SdfParams Q, float k,
    PoseF /* read by map_robust_late_pose */, Finish /* read by late_finish_at */) {
  const MapRayView M = ray_view(S);
  double acc[29];   // 0 .. 27 as icp_map_sdf_kernel's; 28 is not used
#pragma unroll
  for (int i = 0; i < 29; i++) acc[i] = 0.0;
  float rows = 0.f;
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2];   // icp_map_sdf_kernel's trip
    int i0[3];
    float a[3], r, J[6], len;
    float2 v[8];
    const bool in = sdf_cell(G, map_robust_late_pose(), x, y, z, i0, a);
    const bool have = map_sdf_corners{M}(i0, v);
    bool ok = sdf_row(v, a, G, map_robust_late_pose(), Q, x, y, z, r, J, len) && in && have;
    if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
    if (!ok) {
      r = 0.f;
#pragma unroll
      for (int m = 0; m < 6; m++) J[m] = 0.f;
    }
    add_weighted_row_f64(ok ? robust_weight<KIND>(r, k) : 0.f, r, J, acc, 27);
    rows += ok ? 1.f : 0.f;   // every row that passed the gates (a thread sees fewer than 2^24 pixels: exact)
  }
  double sums[29];
#pragma unroll
  for (int i = 0; i < 28; i++) sums[i] = acc[i];
  sums[28] = (double)rows;
  reduce_and_finish<29, kNeLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(MapSdfRobustRoundArgs, fin)));   // host-driven only
}

// ---------------------------------------------------------------------------------------------- the volume colour term on the window
struct SdfPhotoRobustRoundArgs {
  const float* vmap; const float* nmap; const float* fint; int64_t n; const float* vol; const uint2* cvol;
  VolumeGeometry G; SdfParams Q; float lam; RobustScales W; PoseF T; Finish fin;
};
static_assert(offsetof(SdfPhotoRobustRoundArgs, fin) == 160 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(SdfPhotoRobustRoundArgs, T) == 112 && sizeof(PoseF) == 48, "photo_robust_late_pose: where the kernarg segment holds the pose");
__device__ __forceinline__ PoseF photo_robust_late_pose() { return late_pose_at((unsigned)offsetof(SdfPhotoRobustRoundArgs, T)); }

template <int KIND, bool GEO, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_sdf_photo_robust_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, const float* __restrict__ fint, int64_t n, const float* __restrict__ vol,
    const uint2* __restrict__ cvol, VolumeGeometry G, SdfParams Q, float lam, RobustScales W, PoseF /* read by photo_robust_late_pose */,
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
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2], If = fint[i];   // icp_sdf_photo_kernel's trip
    int i0[3];
    float a[3];
    float2 v[8];
    uint2 c[8];
    const bool in = sdf_cell(G, photo_robust_late_pose(), x, y, z, i0, a);
    corners(i0, v);
    colours(i0, c);
    float l[8], r, J[6];
    const bool known = colour_lumas(c, l);
    const bool okp = sdf_photo_row(v, l, known, a, G, photo_robust_late_pose(), Q.gate, x, y, z, If, r, J) && in;
    const float wp = okp ? robust_photo_weight<KIND>(r, W.photo_k) : 0.f;   // of the unscaled residual
    r = okp ? lam * r : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = okp ? lam * J[k] : 0.f;
    add_weighted_row_f64(wp, r, J, acc, 28);
    prows += okp ? 1.f : 0.f;
    if (GEO) {
#pragma unroll
      for (int m = 0; m < 8; m++) asm volatile("" : "+v"(v[m].x) : "v"(r));   // the geometric row behind the photometric one, as the sibling's
      float len;
      bool ok = sdf_row(v, a, G, photo_robust_late_pose(), Q, x, y, z, r, J, len) && in;
      if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
      if (!ok) {
        r = 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) J[k] = 0.f;
      }
      add_weighted_row_f64(ok ? robust_weight<KIND>(r, W.k) : 0.f, r, J, acc, 27);
      grows += ok ? 1.f : 0.f;
    }
  }
  double sums[kSdfPhotoAcc];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)grows; sums[29] = acc[28]; sums[30] = (double)prows;
  reduce_and_finish<kSdfPhotoAcc, kNlLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(SdfPhotoRobustRoundArgs, fin)));   // host-driven only
}

// ---------------------------------------------------------------------------------------------- ... and on the map
struct MapSdfPhotoRobustRoundArgs {
  const float* vmap; const float* nmap; const float* fint; int64_t n; MapSdfPhotoView P; VolumeGeometry G; SdfParams Q; float lam;
  RobustScales W; PoseF T; Finish fin;
};
static_assert(offsetof(MapSdfPhotoRobustRoundArgs, fin) == 224 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(MapSdfPhotoRobustRoundArgs, T) == 176 && sizeof(PoseF) == 48, "map_photo_robust_late_pose: where the kernarg segment holds the pose");
static_assert(offsetof(MapSdfPhotoRobustRoundArgs, P) == 32 && sizeof(MapSdfPhotoView) == 80, "map_photo_late_view: where the kernarg segment holds the view");
static_assert(offsetof(MapSdfPhotoRobustRoundArgs, P) == offsetof(MapSdfPhotoRoundArgs, P), "map_photo_late_view reads the sibling's offset");
__device__ __forceinline__ PoseF map_photo_robust_late_pose() { return late_pose_at((unsigned)offsetof(MapSdfPhotoRobustRoundArgs, T)); }

template <int KIND, bool GEO, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(GEO ? 2 : 4))) void icp_map_sdf_photo_robust_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, const float* __restrict__ fint, int64_t n,
    MapSdfPhotoView /* read by map_photo_late_view */, VolumeGeometry G, SdfParams Q, float lam, RobustScales W,
    PoseF /* read by map_photo_robust_late_pose */, Finish /* read by late_finish_at */) {
  double acc[29];   // 0 .. 26 H | g of both terms, 27 the geometric cost, 28 the photometric cost
#pragma unroll
  for (int k = 0; k < 29; k++) acc[k] = 0.0;
  float grows = 0.f, prows = 0.f;
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2];   // icp_map_sdf_photo_kernel's trip
    int i0[3];
    float a[3], r, J[6];
    bool past;
    {
      float2 v[8];
      const bool in = sdf_cell(G, map_photo_robust_late_pose(), x, y, z, i0, a);
      const MapRayView M = map_photo_late_view();
      const bool have = map_sdf_corners{M}(i0, v) && in;
      if (GEO) {
        float len;
        bool ok = sdf_row(v, a, G, map_photo_robust_late_pose(), Q, x, y, z, r, J, len) && have;
        if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
        if (!ok) {
          r = 0.f;
#pragma unroll
          for (int k = 0; k < 6; k++) J[k] = 0.f;
        }
        add_weighted_row_f64(ok ? robust_weight<KIND>(r, W.k) : 0.f, r, J, acc, 27);
        grows += ok ? 1.f : 0.f;
      }
      past = sdf_photo_gate(v, a, G, Q.gate, have);
    }
    uint2 c[8];
#pragma unroll
    for (int m = 0; m < 8; m++) c[m] = make_uint2(0u, 0u);
    if (past) { const MapRayView M = map_photo_late_view(); map_colour_corners{M}(i0, c); }
    float l[8];
    const bool known = colour_lumas(c, l);
    const float If = fint[i];
    const bool okp = sdf_photo_value(past && known && __builtin_isfinite(If), l, a, G, map_photo_robust_late_pose(), x, y, z, If, r, J);
    const float wp = okp ? robust_photo_weight<KIND>(r, W.photo_k) : 0.f;   // of the unscaled residual
    r = okp ? lam * r : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = okp ? lam * J[k] : 0.f;
    add_weighted_row_f64(wp, r, J, acc, 28);
    prows += okp ? 1.f : 0.f;
  }
  double sums[kSdfPhotoAcc];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)grows; sums[29] = acc[28]; sums[30] = (double)prows;
  reduce_and_finish<kSdfPhotoAcc, kNlLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(MapSdfPhotoRobustRoundArgs, fin)));   // host-driven only
}

// ---------------------------------------------------------------------------------------------- the hook
// The plane of weights of a level: the rows kernels' rule for one pixel (sdf_pixel / sdf_photo_pixel, with the window's or the map's
// fetches), then the weight of its residual; NaN where the pixel has no row.  scale = 0 (a photometric plane with photo_k = 0) and kind
// NONE: 1 for every row.  vol / cvol are read without MAP, P with it
template <bool MAP, bool PHOTO>
__global__ __launch_bounds__(kSdfRowsBlock) void sdf_robust_weights_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                                           const float* __restrict__ fint, int64_t n,
                                                                           const float* __restrict__ vol, const uint2* __restrict__ cvol,
                                                                           MapSdfPhotoView P, VolumeGeometry G, SdfParams Q, int kind, float scale,
                                                                           PoseF T, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kSdfRowsBlock + threadIdx.x;
  if (i >= n) return;
  const MapRayView M = ray_view(P);
  const float x = vmap[3 * i], y = vmap[3 * i + 1], z = vmap[3 * i + 2];
  float r, J[6];
  bool ok;
  if (PHOTO) {
    ok = MAP ? sdf_photo_pixel(map_sdf_corners{M}, map_colour_corners{M}, G, T, Q.gate, x, y, z, fint[i], r, J)
             : sdf_photo_pixel(dense_corners(vol, G), dense_colour_corners(cvol, G), G, T, Q.gate, x, y, z, fint[i], r, J);
  } else {
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (Q.use_normals) { nx = nmap[3 * i]; ny = nmap[3 * i + 1]; nz = nmap[3 * i + 2]; }
    ok = MAP ? sdf_pixel(map_sdf_corners{M}, G, T, Q, x, y, z, nx, ny, nz, r, J) : sdf_pixel(dense_corners(vol, G), G, T, Q, x, y, z, nx, ny, nz, r, J);
  }
  out[i] = !ok ? qnan() : scale > 0.0f ? robust_weight(kind, r, scale) : 1.0f;
}

// a node per new kernel, beside the unit's own (one code object: whichever is touched first loads all of it)
namespace robust_round_node { RPE_PRELOAD(icp_sdf_robust_kernel<kRobustHuber, 256>); }
namespace map_robust_round_node { RPE_PRELOAD(icp_map_sdf_robust_kernel<kRobustHuber, 256>); }
namespace photo_robust_round_node { RPE_PRELOAD(icp_sdf_photo_robust_kernel<kRobustHuber, true, 256>); }
namespace map_photo_robust_round_node { RPE_PRELOAD(icp_map_sdf_photo_robust_kernel<kRobustHuber, true, 256>); }
namespace robust_weights_node { RPE_PRELOAD(sdf_robust_weights_kernel<false, false>); }

}  // namespace

// kind: kRobustHuber or kRobustTukey (the host has checked it)
#define RPE_ROBUST_BY_KIND(LAUNCH) \
  do { if (kind == kRobustHuber) { LAUNCH(kRobustHuber); } else { LAUNCH(kRobustTukey); } } while (0)

hipError_t launch_icp_sdf_robust(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                                 float cos_thr, int use_normals, int kind, float k, const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const int blk = pick_block(rt);
  const int grid = round_grid(rt, n, blk);   // one pixel per thread while the grid allows it
#define RPE_LAUNCH(K) \
  if (blk == 512) hipLaunchKernelGGL((icp_sdf_robust_kernel<K, 512>), dim3(grid), dim3(512), 0, s, vmap, nmap, n, vol, G, Q, k, T, fin); \
  else hipLaunchKernelGGL((icp_sdf_robust_kernel<K, 256>), dim3(grid), dim3(256), 0, s, vmap, nmap, n, vol, G, Q, k, T, fin)
  RPE_ROBUST_BY_KIND(RPE_LAUNCH);
#undef RPE_LAUNCH
  return hipGetLastError();
}

hipError_t launch_icp_map_sdf_robust(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G,
                                     float dist_thr, float cos_thr, int use_normals, int kind, float k, const double* pose12,
                                     const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const MapSdfView S = sdf_view(M);
  const int blk = pick_block(rt);
  const int grid = round_grid(rt, n, blk);
#define RPE_LAUNCH(K) \
  if (blk == 512) hipLaunchKernelGGL((icp_map_sdf_robust_kernel<K, 512>), dim3(grid), dim3(512), 0, s, vmap, nmap, n, S, G, Q, k, T, fin); \
  else hipLaunchKernelGGL((icp_map_sdf_robust_kernel<K, 256>), dim3(grid), dim3(256), 0, s, vmap, nmap, n, S, G, Q, k, T, fin)
  RPE_ROBUST_BY_KIND(RPE_LAUNCH);
#undef RPE_LAUNCH
  return hipGetLastError();
}

hipError_t launch_icp_sdf_photo_robust(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol,
                                       const unsigned short* cvol, const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals,
                                       float lam, int geometric, int kind, float k, float photo_k, const double* pose12, const ReduceTarget& rt,
                                       hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const RobustScales W{k, photo_k};
  const uint2* cv = reinterpret_cast<const uint2*>(cvol);
  const int blk = pick_block(rt);
  const int grid = round_grid(rt, n, blk);
#define RPE_LAUNCH_ONE(K, GEO, B) \
  hipLaunchKernelGGL((icp_sdf_photo_robust_kernel<K, GEO, B>), dim3(grid), dim3(B), 0, s, vmap, nmap, fint, n, vol, cv, G, Q, lam, W, T, fin)
#define RPE_LAUNCH(K) \
  if (blk == 512) { if (geometric) RPE_LAUNCH_ONE(K, true, 512); else RPE_LAUNCH_ONE(K, false, 512); } \
  else { if (geometric) RPE_LAUNCH_ONE(K, true, 256); else RPE_LAUNCH_ONE(K, false, 256); }
  RPE_ROBUST_BY_KIND(RPE_LAUNCH);
#undef RPE_LAUNCH
#undef RPE_LAUNCH_ONE
  return hipGetLastError();
}

hipError_t launch_icp_map_sdf_photo_robust(const float* vmap, const float* nmap, const float* fint, int64_t n, const MapRayView& M,
                                           const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                           int kind, float k, float photo_k, const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const RobustScales W{k, photo_k};
  const MapSdfPhotoView P = photo_view(M);
  const int blk = pick_block(rt);
  const int grid = round_grid(rt, n, blk);
#define RPE_LAUNCH_ONE(K, GEO, B) \
  hipLaunchKernelGGL((icp_map_sdf_photo_robust_kernel<K, GEO, B>), dim3(grid), dim3(B), 0, s, vmap, nmap, fint, n, P, G, Q, lam, W, T, fin)
#define RPE_LAUNCH(K) \
  if (blk == 512) { if (geometric) RPE_LAUNCH_ONE(K, true, 512); else RPE_LAUNCH_ONE(K, false, 512); } \
  else { if (geometric) RPE_LAUNCH_ONE(K, true, 256); else RPE_LAUNCH_ONE(K, false, 256); }
  RPE_ROBUST_BY_KIND(RPE_LAUNCH);
#undef RPE_LAUNCH
#undef RPE_LAUNCH_ONE
  return hipGetLastError();
}
#undef RPE_ROBUST_BY_KIND

hipError_t launch_sdf_robust_weights(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol,
                                     const unsigned short* cvol, const MapRayView* M, const VolumeGeometry& G, float dist_thr, float cos_thr,
                                     int use_normals, int photo, int kind, float scale, const double* pose12, float* out, hipStream_t s) {
  const int64_t blocks = (n + kSdfRowsBlock - 1) / kSdfRowsBlock;
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const MapSdfPhotoView P = M ? photo_view(*M) : MapSdfPhotoView{};
  const uint2* cv = reinterpret_cast<const uint2*>(cvol);
#define RPE_LAUNCH(MAP, PHOTO) \
  hipLaunchKernelGGL((sdf_robust_weights_kernel<MAP, PHOTO>), dim3((unsigned)blocks), dim3(kSdfRowsBlock), 0, s, vmap, nmap, fint, n, vol, cv, P, \
                     G, Q, kind, scale, T, out)
  if (M) { if (photo) RPE_LAUNCH(true, true); else RPE_LAUNCH(true, false); }
  else { if (photo) RPE_LAUNCH(false, true); else RPE_LAUNCH(false, false); }
#undef RPE_LAUNCH
  return hipGetLastError();
}

}  // namespace rpe
