// gfx950 kernels of the PHOTOMETRIC term beside ICP (include/rgbd_pose_hip.h Part 3, "Photometric term"): tracking against the model's
// colour as well as its geometry, so that a wall, a floor or a corridor -- where point-to-plane ICP holds three of the six degrees of
// freedom with nothing -- still has a unique pose.
//
//   P1  frame_intensity_kernel   the frame's intensity pyramid: one float per pixel per level, every level in ONE launch (a level-l
//                                pixel folds its 4^l colours in the nested 2 x 2 order, so no level waits for the one below it).
//   P2  model_photo_kernel       the model's photometric map, one float4 {I, gx, gy, zm} per model pixel per level, every level in one
//                                launch: intensity, its central differences, and the model vertex's depth in the model camera,
//                                NaN wherever the model normal is (the normals are NaN across depth jumps: that one poison keeps
//                                every bilinear and gradient stencil off the occlusion edges).
//   P3  icp_photo_kernel<KIND>   one Gauss-Newton round in one pass over the level's frame pixels.  KIND = point-to-plane: the geometric
//                                row exactly as icp_fused_kernel forms it (associate_pixel + pair_group) AND the photometric row, one
//                                reduction, one record of 31 sums.  KIND = none: the photometric row alone.  Per pixel it streams 28 B
//                                (vertex, normal, intensity), gathers 24 B for the geometric pair and four 16-byte map entries for the
//                                photometric one (the two of a row are neighbours); the gathers land in L2 like the ICP kernels'.
//   P4  photo_rows_kernel        {r, J[0..5]} of every frame pixel (NaN where there is no pair) through the same device function: the
//                                residual image and the per-pixel hook of the tests.
//
// Steps 1-5 of the term (photo_pixel) are followed BIT-EXACTLY: fp32, the written order, no FMA contraction; tests/photo_oracle.py is
// their numpy statement.  The sums are add_row2's fused multiply-adds into partial sums of one group of 4 pixels, widened to fp64 per
// group.  Record: 31 sums -- H upper triangle (21) | g (6) of BOTH terms | geometric cost | geometric pairs | photometric cost |
// photometric pairs -- through the 64-double record form of rpe_reduce.hpp (LD = kNlLd, the form the 44-sum kernels use): entries
// 29 and 30 are sums in their own right, not guests in the padding of the 32-double record.
#include "rpe_residuals.hpp"
#include "rpe_assoc.h"

namespace rpe {

namespace {

constexpr int KIND_NONE = -1;     // icp_photo_kernel: no geometric term
constexpr int kPhotoAcc = 31;
constexpr int kPrepBlock = 256;   // P1, P2, P4: one pixel per lane

struct PhotoParams {
  float A[9];   // -(R_m R^T), row-major
  float gate;   // occlusion gate on |zm - Xm.z| [m]
  float lam;    // weight of the term [m per intensity level]
};

__device__ __forceinline__ float lerp1(float p, float q, float s) {
#pragma clang fp contract(off)
  return p + (q - p) * s;
}
__device__ __forceinline__ bool fin4(const float4& m) {
  return __builtin_isfinite(m.x) && __builtin_isfinite(m.y) && __builtin_isfinite(m.z) && __builtin_isfinite(m.w);
}

// intensity of level L at (u, v) from the level-0 RGBA8 map of width w0: level 0 = ((0.299 r + 0.587 g) + 0.114 b), NaN when A = 0;
// level L = (((a + b) + c) + d) * 0.25 over the 2 x 2 block of level L - 1 (a NaN member makes it NaN)
template <int L> __device__ __forceinline__ float intensity_at(const unsigned int* __restrict__ rgba, int w0, int u, int v) {
#pragma clang fp contract(off)
  if constexpr (L == 0) {
    const unsigned c = rgba[(int64_t)v * w0 + u];
    const float i = (0.299f * (float)(c & 0xffu) + 0.587f * (float)((c >> 8) & 0xffu)) + 0.114f * (float)((c >> 16) & 0xffu);
    return (c >> 24) != 0u ? i : __int_as_float(0x7fc00000);
  } else {
    const float a = intensity_at<L - 1>(rgba, w0, 2 * u, 2 * v), b = intensity_at<L - 1>(rgba, w0, 2 * u + 1, 2 * v);
    const float c = intensity_at<L - 1>(rgba, w0, 2 * u, 2 * v + 1), d = intensity_at<L - 1>(rgba, w0, 2 * u + 1, 2 * v + 1);
    return (((a + b) + c) + d) * 0.25f;
  }
}
__device__ __forceinline__ float intensity_level(int l, const unsigned int* __restrict__ rgba, int w0, int u, int v) {
  switch (l) {
    case 0: return intensity_at<0>(rgba, w0, u, v);
    case 1: return intensity_at<1>(rgba, w0, u, v);
    case 2: return intensity_at<2>(rgba, w0, u, v);
    default: return intensity_at<3>(rgba, w0, u, v);
  }
}
static_assert(kMaxLevels == 4, "intensity_level serves levels 0 .. 3");

// which level the concatenated pixel index e belongs to, and its index there (-1: padding between two levels)
__device__ __forceinline__ int level_of_pixel(const PyramidGeometry& G, int64_t e, int64_t& i) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kMaxLevels; k++) if (k < G.levels && e >= G.off[k]) l = k;
  i = e - G.off[l];
  return i < (int64_t)G.cam[l].width * G.cam[l].height ? l : -1;
}

// ---------------------------------------------------------------------------------------------- P1
__global__ __launch_bounds__(kPrepBlock) void frame_intensity_kernel(const unsigned int* __restrict__ rgba, PyramidGeometry G,
                                                                     float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (e >= G.off[G.levels]) return;
  int64_t i;
  const int l = level_of_pixel(G, e, i);
  if (l < 0) return;
  const int w = G.cam[l].width;
  out[e] = intensity_level(l, rgba, G.cam[0].width, (int)(i % w), (int)(i / w));
}

// ---------------------------------------------------------------------------------------------- P2
__global__ __launch_bounds__(kPrepBlock) void model_photo_kernel(const unsigned int* __restrict__ rgba, PyramidGeometry G,
                                                                 const float* __restrict__ mv, const float* __restrict__ mn, PoseF M,
                                                                 float4* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (e >= G.off[G.levels]) return;
  int64_t i;
  const int l = level_of_pixel(G, e, i);
  if (l < 0) return;
  const int w = G.cam[l].width, h = G.cam[l].height, w0 = G.cam[0].width;
  const int u = (int)(i % w), v = (int)(i / w);
  const float nan = __int_as_float(0x7fc00000);
  float4 o;
  o.x = intensity_level(l, rgba, w0, u, v);
  o.y = (u >= 1 && u <= w - 2) ? 0.5f * (intensity_level(l, rgba, w0, u + 1, v) - intensity_level(l, rgba, w0, u - 1, v)) : nan;
  o.z = (v >= 1 && v <= h - 2) ? 0.5f * (intensity_level(l, rgba, w0, u, v + 1) - intensity_level(l, rgba, w0, u, v - 1)) : nan;
  const float x = mv[3 * e], y = mv[3 * e + 1], z = mv[3 * e + 2];
  const float nx = mn[3 * e], ny = mn[3 * e + 1], nz = mn[3 * e + 2];
  const float zm = ((M.R[6] * x + M.R[7] * y) + M.R[8] * z) + M.t[2];
  o.w = (nx != nx || ny != ny || nz != nz) ? nan : zm;
  out[e] = o;
}

// ---------------------------------------------------------------------------------------------- the term, per frame pixel
// Frame vertex (x, y, z) with intensity If under the pose guess T (Xc = R Xw + t): steps 1-5 of the header.  r and J are the
// UNSCALED residual and row, 0 when there is no pair.
__device__ __forceinline__ bool photo_pixel(const PoseF& T, const AssocParams& P, const PhotoParams& Q, const float4* __restrict__ pmap,
                                            float x, float y, float z, float If, float& r, float (&J)[6]) {
#pragma clang fp contract(off)
  bool ok = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && __builtin_isfinite(If);
  float wx, wy, wz;
  to_world(T, x, y, z, wx, wy, wz);
  const float px = P.M.R[0] * wx + P.M.R[1] * wy + P.M.R[2] * wz + P.M.t[0];
  const float py = P.M.R[3] * wx + P.M.R[4] * wy + P.M.R[5] * wz + P.M.t[1];
  const float pz = P.M.R[6] * wx + P.M.R[7] * wy + P.M.R[8] * wz + P.M.t[2];
  ok = ok && pz > 0.0f;
  const float xs = P.mcam.fx * (px / pz) + P.mcam.cx, ys = P.mcam.fy * (py / pz) + P.mcam.cy;
  const float x0 = floorf(xs), y0 = floorf(ys);
  ok = ok && x0 >= 0.0f && x0 <= (float)(P.mcam.width - 2) && y0 >= 0.0f && y0 <= (float)(P.mcam.height - 2);
  r = 0.f;
#pragma unroll
  for (int k = 0; k < 6; k++) J[k] = 0.f;
  if (ok) {
    const int64_t j = (int64_t)(int)y0 * P.mcam.width + (int)x0;
    const float4 m00 = pmap[j], m10 = pmap[j + 1], m01 = pmap[j + P.mcam.width], m11 = pmap[j + P.mcam.width + 1];
    ok = fin4(m00) && fin4(m10) && fin4(m01) && fin4(m11) && fabsf(m00.w - pz) <= Q.gate && fabsf(m10.w - pz) <= Q.gate &&
         fabsf(m01.w - pz) <= Q.gate && fabsf(m11.w - pz) <= Q.gate;
    const float a = xs - x0, b = ys - y0;
    const float Is = lerp1(lerp1(m00.x, m10.x, a), lerp1(m01.x, m11.x, a), b);
    const float Gx = lerp1(lerp1(m00.y, m10.y, a), lerp1(m01.y, m11.y, a), b);
    const float Gy = lerp1(lerp1(m00.z, m10.z, a), lerp1(m01.z, m11.z, a), b);
    const float gfx = Gx * P.mcam.fx, gfy = Gy * P.mcam.fy;
    const float qx = gfx / pz, qy = gfy / pz, qz = -((gfx * px + gfy * py) / (pz * pz));
    const float ax = (qx * Q.A[0] + qy * Q.A[3]) + qz * Q.A[6];
    const float ay = (qx * Q.A[1] + qy * Q.A[4]) + qz * Q.A[7];
    const float az = (qx * Q.A[2] + qy * Q.A[5]) + qz * Q.A[8];
    r = ok ? Is - If : 0.f;
    J[0] = ok ? ax : 0.f; J[1] = ok ? ay : 0.f; J[2] = ok ? az : 0.f;
    J[3] = ok ? y * az - z * ay : 0.f; J[4] = ok ? z * ax - x * az : 0.f; J[5] = ok ? x * ay - y * ax : 0.f;
  }
  return ok;
}

// one group of 4 pixels of the photometric term into the accumulators: rows scaled by lam, add_row2 on pairs of pixels, the group's
// partial sums widened to fp64 once (H, g into the shared entries 0 .. 26, cost and pairs into 29 and 30)
__device__ __forceinline__ void photo_group(const PoseF& T, const AssocParams& P, const PhotoParams& Q, const float4* __restrict__ pmap,
                                            const float (&V)[12], const float (&I)[4], double (&acc)[kPhotoAcc]) {
#pragma clang fp contract(off)
  typedef float V2 __attribute__((ext_vector_type(2)));
  V2 s2[29];
#pragma unroll
  for (int k = 0; k < 29; k++) s2[k] = V2{0.f, 0.f};
  float cnt = 0.f;
#pragma unroll
  for (int p = 0; p < 2; p++) {
    float r[2], J[2][6];
    bool ok[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int i = 2 * p + e;
      ok[e] = photo_pixel(T, P, Q, pmap, V[3 * i], V[3 * i + 1], V[3 * i + 2], I[i], r[e], J[e]);
      cnt += ok[e] ? 1.f : 0.f;
    }
    V2 Jv[6];
#pragma unroll
    for (int a = 0; a < 6; a++) Jv[a] = V2{Q.lam * J[0][a], Q.lam * J[1][a]};
    add_row2<V2>(Jv, V2{Q.lam * r[0], Q.lam * r[1]}, V2{ok[0] ? 1.f : 0.f, ok[1] ? 1.f : 0.f}, s2);
  }
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] += (double)(s2[k].x + s2[k].y);
  acc[29] += (double)(s2[27].x + s2[27].y);
  acc[30] += (double)cnt;
}

// the geometric term of one group, exactly icp_fused_kernel's: associate_pixel, NaN-marked columns for the pixels without a partner,
// pair_group, one widening per group
__device__ __forceinline__ void geometric_group(const PoseK<double>& pose, const PoseF& T, const AssocParams& P, const float* __restrict__ mv,
                                                const float* __restrict__ mn, const float (&V)[12], const float (&N)[12], int npresent,
                                                double (&acc)[kPhotoAcc]) {
  typedef float V2 __attribute__((ext_vector_type(2)));
  const short m_none[4] = {1, 1, 1, 1};
  const float w_none[4] = {1.f, 1.f, 1.f, 1.f};
  const float nan = __int_as_float(0x7fc00000);
  float vw[12], vb[12], vc[12];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float gx, gy, gz;
    const bool ok = associate_pixel(T, P, mv, mn, V[3 * i], V[3 * i + 1], V[3 * i + 2], N[3 * i], N[3 * i + 1], N[3 * i + 2], vw[3 * i],
                                    vw[3 * i + 1], vw[3 * i + 2], gx, gy, gz);
#pragma unroll
    for (int k = 0; k < 3; k++) { vb[3 * i + k] = ok ? V[3 * i + k] : nan; vc[3 * i + k] = ok ? N[3 * i + k] : nan; }
  }
  V2 s2[29];
#pragma unroll
  for (int k = 0; k < 29; k++) s2[k] = V2{0.f, 0.f};
  pair_group<float, KIND_P2PLANE, false, false, false, 29>(pose, vw, vb, vc, m_none, w_none, npresent, s2);
#pragma unroll
  for (int k = 0; k < 29; k++) acc[k] += (double)(s2[k].x + s2[k].y);
}

// ---------------------------------------------------------------------------------------------- P3
template <int KIND, int BLK>
__global__ __launch_bounds__(BLK) void icp_photo_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                        const float* __restrict__ fint, int64_t n, const float* __restrict__ mv,
                                                        const float* __restrict__ mn, const float4* __restrict__ pmap, AssocParams P,
                                                        PhotoParams Q, PoseK<double> pose, Finish fin) {
  static_assert(KIND == KIND_P2PLANE || KIND == KIND_NONE, "geometric terms beside the photometric one");
  PoseF T;
#pragma unroll
  for (int k = 0; k < 9; k++) T.R[k] = (float)pose.R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) T.t[k] = (float)pose.t[k];
  double acc[kPhotoAcc];
#pragma unroll
  for (int k = 0; k < kPhotoAcc; k++) acc[k] = 0.0;
  const int64_t full = n / 4;
  const int64_t stride = (int64_t)gridDim.x * BLK;
  const float4* __restrict__ v4 = reinterpret_cast<const float4*>(vmap);
  const float4* __restrict__ n4 = reinterpret_cast<const float4*>(nmap);
  const float4* __restrict__ i4 = reinterpret_cast<const float4*>(fint);
  for (int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x; g < full; g += stride) {
    float V[12];
    unpack3(v4[3 * g], v4[3 * g + 1], v4[3 * g + 2], V);
    const float4 iv = i4[g];
    const float I[4] = {iv.x, iv.y, iv.z, iv.w};
    if constexpr (KIND == KIND_P2PLANE) {
      float N[12];
      unpack3(n4[3 * g], n4[3 * g + 1], n4[3 * g + 2], N);
      geometric_group(pose, T, P, mv, mn, V, N, 4, acc);
    }
    photo_group(T, P, Q, pmap, V, I, acc);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && full * 4 < n) {  // leftover pixels
    const float nan = __int_as_float(0x7fc00000);
    const int left = (int)(n - full * 4);
    float V[12], N[12], I[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool in = i < left;
      const int64_t q = full * 4 + i;
#pragma unroll
      for (int k = 0; k < 3; k++) { V[3 * i + k] = in ? vmap[3 * q + k] : nan; N[3 * i + k] = in ? nmap[3 * q + k] : nan; }
      I[i] = in ? fint[q] : nan;
    }
    if constexpr (KIND == KIND_P2PLANE) geometric_group(pose, T, P, mv, mn, V, N, left, acc);
    photo_group(T, P, Q, pmap, V, I, acc);
  }
  reduce_and_finish<kPhotoAcc, kNlLd, 0, BLK>(acc, fin);
}

// ---------------------------------------------------------------------------------------------- P4
__global__ __launch_bounds__(kPrepBlock) void photo_rows_kernel(const float* __restrict__ vmap, const float* __restrict__ fint, int64_t n,
                                                                const float4* __restrict__ pmap, AssocParams P, PhotoParams Q, PoseF T,
                                                                float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (i >= n) return;
  float r, J[6];
  const bool ok = photo_pixel(T, P, Q, pmap, vmap[3 * i], vmap[3 * i + 1], vmap[3 * i + 2], fint[i], r, J);
  const float nan = __int_as_float(0x7fc00000);
  rows[i] = ok ? r : nan;
#pragma unroll
  for (int k = 0; k < 6; k++) rows[(int64_t)(k + 1) * n + i] = ok ? J[k] : nan;
}

// A = -(R_m R^T) in fp32, each entry summed left to right
PhotoParams photo_params(const PoseF& M, const PoseF& T, float gate, float lam) {
#pragma clang fp contract(off)
  PhotoParams Q;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      float s = M.R[3 * i] * T.R[3 * j];
      s = s + M.R[3 * i + 1] * T.R[3 * j + 1];
      s = s + M.R[3 * i + 2] * T.R[3 * j + 2];
      Q.A[3 * i + j] = -s;
    }
  Q.gate = gate; Q.lam = lam;
  return Q;
}
PoseF pose_f32(const double* p12) {
  PoseF T;
  for (int i = 0; i < 9; i++) T.R[i] = (float)p12[i];
  for (int i = 0; i < 3; i++) T.t[i] = (float)p12[9 + i];
  return T;
}

}  // namespace

hipError_t launch_frame_intensity(const unsigned int* rgba, const PyramidGeometry& G, float* out, hipStream_t s) {
  const int64_t blocks = (G.off[G.levels] + kPrepBlock - 1) / kPrepBlock;
  hipLaunchKernelGGL(frame_intensity_kernel, dim3((unsigned)blocks), dim3(kPrepBlock), 0, s, rgba, G, out);
  return hipGetLastError();
}

hipError_t launch_model_photo(const unsigned int* rgba, const PyramidGeometry& G, const float* mv, const float* mn, const PoseF& M,
                              float* out4, hipStream_t s) {
  const int64_t blocks = (G.off[G.levels] + kPrepBlock - 1) / kPrepBlock;
  hipLaunchKernelGGL(model_photo_kernel, dim3((unsigned)blocks), dim3(kPrepBlock), 0, s, rgba, G, mv, mn, M, reinterpret_cast<float4*>(out4));
  return hipGetLastError();
}

hipError_t launch_icp_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* mv, const float* mn,
                            const float* pmap4, const Camera& mcam, const PoseF& M, float dist_thr, float cos_thr, float lam, int geometric,
                            const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  AssocParams P;
  P.mcam = mcam; P.M = M; P.dist_sq = dist_thr * dist_thr; P.cos_thr = cos_thr; P.use_normals = 1;
  const PhotoParams Q = photo_params(M, pose_f32(pose12), dist_thr, lam);
  const PoseK<double> pose = make_pose<double>(pose12);
  const Finish fin = make_finish(rt);
  const float4* pm = reinterpret_cast<const float4*>(pmap4);
  // geometry as the fused ICP round's: one pixel group per thread while the grid allows it
  const int blk = pick_block(rt);
  const int64_t groups = (n + 3) / 4;
  int G = rt.max_blocks;
  if ((int64_t)G > (groups + blk - 1) / blk) G = (int)((groups + blk - 1) / blk);
  if (G < 1) G = 1;
#define RPE_PHOTO_LAUNCH(K, B) hipLaunchKernelGGL((icp_photo_kernel<K, B>), dim3(G), dim3(B), 0, s, vmap, nmap, fint, n, mv, mn, pm, P, Q, pose, fin)
  if (blk == 512) { if (geometric) RPE_PHOTO_LAUNCH(KIND_P2PLANE, 512); else RPE_PHOTO_LAUNCH(KIND_NONE, 512); }
  else { if (geometric) RPE_PHOTO_LAUNCH(KIND_P2PLANE, 256); else RPE_PHOTO_LAUNCH(KIND_NONE, 256); }
#undef RPE_PHOTO_LAUNCH
  return hipGetLastError();
}

hipError_t launch_photo_rows(const float* vmap, const float* fint, int64_t n, const float* pmap4, const Camera& mcam, const PoseF& M,
                             float dist_thr, const double* pose12, float* rows, hipStream_t s) {
  AssocParams P;
  P.mcam = mcam; P.M = M; P.dist_sq = dist_thr * dist_thr; P.cos_thr = 0.f; P.use_normals = 0;
  const PoseF T = pose_f32(pose12);
  const PhotoParams Q = photo_params(M, T, dist_thr, 1.0f);
  const int64_t blocks = (n + kPrepBlock - 1) / kPrepBlock;
  hipLaunchKernelGGL(photo_rows_kernel, dim3((unsigned)blocks), dim3(kPrepBlock), 0, s, vmap, fint, n, reinterpret_cast<const float4*>(pmap4),
                     P, Q, T, rows);
  return hipGetLastError();
}

RPE_PRELOAD(icp_photo_kernel<KIND_P2PLANE, 256>);

}  // namespace rpe
