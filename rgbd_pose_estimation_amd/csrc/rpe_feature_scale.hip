// gfx950 kernels of the FEATURE stage's SCALE LEVELS (rpe_features_set_levels(n), n > 1): the detector and the descriptors of
// rpe_feature.hip / rpe_feature_oriented.hip on a fixed ladder of up to four levels of scale p / q = 1, 2/3, 1/2, 1/3, so that a camera
// that has moved closer to what it mapped finds the corners it mapped.  The levels' pixels lie end to end in ONE index space (FeatLevels:
// index = base[l] + v * w[l] + u), and every stage runs once over all of it:
//
//   D0  feat_resample_kernel          a thread per level pixel: the rounded mean of the q x q block of the level-0 luma repeated p times
//                                     per axis, and whether every source pixel is known; two bytes per pixel (Y | K << 8), level 0 too.
//                                     The sources are read straight from the RGBA image: a level pixel has at most 3 x 3 of them, its
//                                     row neighbours share them, and the image of a side stays in the L2 (1.2 MB at 640 x 480).
//   D1s feat_score_levels_kernel      D1 on the bytes of D0: a workgroup owns a 32 x 8 tile OF ONE LEVEL (the grid is the levels' tiles
//                                     end to end); the finite test reads the view's vertex and normal at the level-0 pixel the level
//                                     pixel stands at.
//   D2s feat_nms_levels_kernel        D2 with the row width of the pixel's level: chunks of 256 consecutive indices, which may
//   D4s feat_compact_levels_kernel    straddle two levels; the survivors' indices come out in (level, level pixel) order.
//   D3, D5                            rpe_feature.hip's own (launch_feature_scan, launch_feature_select): they see a linear index only.
//   D6s feat_describe_levels_kernel   D6 on the keypoint's level, and what a keypoint reports: the level-0 pixel it stands at (pix, xy),
//   D6os feat_describe_oriented_levels_kernel   its level and its level pixel.  D6os: D6o likewise, moments over D0's luma of the level.
//
// The rule (include/rgbd_pose_hip.h Part 3, "Scale levels") is integer arithmetic and comparisons throughout; tests/scale_oracle.py is
// its numpy statement and the results are its bits.  Nothing is placed by an atomic: ids come from scans.
#include "rpe_assoc.h"
#include "rpe_feature_rules.hpp"   // luma, the segment test, survives: shared with rpe_feature.hip / rpe_feature_oriented.hip
#include "rpe_scan.hpp"

namespace rpe {

namespace {

constexpr int kChunk = 256;

// a[l] by comparisons (l is a register value: an indexed read of a kernel argument could go through scratch)
__device__ __forceinline__ int at(const int* a, int l) { return l == 0 ? a[0] : l == 1 ? a[1] : l == 2 ? a[2] : a[3]; }
// the level of index i < first[4]; the entries of empty levels equal first[4], so no index reaches them
__device__ __forceinline__ int level_of(const int* first, int i) { return (i >= first[1]) + (i >= first[2]) + (i >= first[3]); }
__device__ __forceinline__ int level_p(int l) { return l == 1 ? 2 : 1; }
__device__ __forceinline__ int level_q(int l) { return l == 0 ? 1 : l == 2 ? 2 : 3; }
// the level-0 pixel that level pixel u stands at: floor(((2 u + 1) q - p) / (2 p)) < w[l] q / p <= w[0]
__device__ __forceinline__ int centre(int u, int p, int q) { return ((2 * u + 1) * q - p) / (2 * p); }

// ---------------------------------------------------------------------------------------------- D0
__global__ __launch_bounds__(256) void feat_resample_kernel(const unsigned int* __restrict__ rgba, FeatLevels L,
                                                           unsigned short* __restrict__ lum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L.base[kFeatMaxLevels]) return;
  const int l = level_of(L.base, i), wl = at(L.w, l), local = i - at(L.base, l);
  const int v = local / wl, u = local - v * wl, p = level_p(l), q = level_q(l), w0 = L.w[0];
  unsigned sum = 0, known = 1;
  // the sources lie in the image: (q u + q - 1) / p <= (q w[l] - 1) / p < w[0], since q w[l] <= p w[0]; the rows likewise
  for (int j = 0; j < q; j++) {
    const int sy = (q * v + j) / p;
    for (int k = 0; k < q; k++) {
      const int sx = (q * u + k) / p;
      const unsigned px = rgba[sy * w0 + sx];
      const unsigned a = (px >> 24) != 0;
      const unsigned y = luma(px);
      sum += a ? y : 0u;
      known &= a;
    }
  }
  const unsigned q2 = (unsigned)(q * q);
  lum[i] = (unsigned short)((sum + q2 / 2) / q2 | known << 8);
}

// ---------------------------------------------------------------------------------------------- D1s
__global__ __launch_bounds__(kTileX * kTileY) void feat_score_levels_kernel(const unsigned short* __restrict__ lum,
                                                                           const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                                           FeatLevels L, int thr, int* __restrict__ score,
                                                                           unsigned short* __restrict__ box) {
  __shared__ FeatTile t;
  const int b = blockIdx.x, l = level_of(L.tile, b), tb = b - at(L.tile, l), tiles_x = at(L.tiles_x, l);
  const int w = at(L.w, l), h = at(L.h, l), base = at(L.base, l);
  const int by = tb / tiles_x, bx = tb - by * tiles_x;
  const int u0 = bx * kTileX, v0 = by * kTileY;
  for (int i = threadIdx.x; i < kLdsX * kLdsY; i += kTileX * kTileY) {
    const int ly = i / kLdsX, lx = i - ly * kLdsX;
    const int gu = u0 + lx - kHalo, gv = v0 + ly - kHalo;
    t[ly][lx] = gu >= 0 && gu < w && gv >= 0 && gv < h ? lum[base + gv * w + gu] : (unsigned short)0;   // outside: Y = 0, unknown
  }
  __syncthreads();
  const int tx = threadIdx.x & (kTileX - 1), ty = threadIdx.x / kTileX;
  const int u = u0 + tx, v = v0 + ty;
  if (u >= w || v >= h) return;
  const int cx = tx + kHalo, cy = ty + kHalo, idx = base + v * w + u;
  int S = 0;   // the 5 x 5 box sum, what the descriptor compares (stated in D1 and D1s: rpe_feature_rules.hpp, header)
#pragma unroll
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) S += t[cy + dy][cx + dx] & 0xff;
  box[idx] = (unsigned short)S;
  const int w0 = L.w[0];
  score[idx] = segment_score(t, cx, cy, u, v, w, h, thr, [=] {
    // the geometry of a level keypoint is that of the level-0 pixel it stands at (inside the image: see centre())
    const int p = level_p(l), q = level_q(l);
    const int64_t g = (int64_t)centre(v, p, q) * w0 + centre(u, p, q);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && __builtin_isfinite(vmap[3 * g + k]) && __builtin_isfinite(nmap[3 * g + k]);
    return fin;
  });
}

// ---------------------------------------------------------------------------------------------- D2s, D4s
// survives (rpe_feature_rules.hpp) with w = the row width of the pixel's level: its eight neighbours lie in the same level
__global__ __launch_bounds__(kChunk) void feat_nms_levels_kernel(const int* __restrict__ score, FeatLevels L, int* __restrict__ chunk,
                                                                unsigned int* __restrict__ hist) {
  const int i = blockIdx.x * kChunk + threadIdx.x;
  const bool keep = i < L.base[kFeatMaxLevels] && survives(score, i, at(L.w, level_of(L.base, i)));
  if (keep) atomicAdd(&hist[min(score[i], kFeatScoreBins - 1)], 1u);   // a count: its value does not depend on the adds' order
  const int cnt = __syncthreads_count(keep);
  if (threadIdx.x == 0) chunk[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(kChunk) void feat_compact_levels_kernel(const int* __restrict__ score, FeatLevels L,
                                                                    const int* __restrict__ chunk, int* __restrict__ spix) {
  __shared__ int lds[kChunk / 64 + 1];
  const int i = blockIdx.x * kChunk + threadIdx.x;
  const bool keep = i < L.base[kFeatMaxLevels] && survives(score, i, at(L.w, level_of(L.base, i)));
  int total;
  const int rank = block_exclusive_scan<kChunk>(keep ? 1 : 0, lds, total);
  if (keep) spix[chunk[blockIdx.x] + rank] = i;
}

// ---------------------------------------------------------------------------------------------- D6s, D6os
// where keypoint k of the levels' index space lies, and what it reports (one lane stores it)
struct LevelKeypoint { int l, u, v, w, h, base; };
__device__ __forceinline__ LevelKeypoint level_keypoint(const FeatLevels& L, int g) {
  LevelKeypoint K;
  K.l = level_of(L.base, g); K.w = at(L.w, K.l); K.h = at(L.h, K.l); K.base = at(L.base, K.l);
  const int local = g - K.base;
  K.v = local / K.w; K.u = local - K.v * K.w;
  return K;
}
__device__ __forceinline__ void report(const FeatLevels& L, const LevelKeypoint& K, int k, int* __restrict__ kp_pix, int* __restrict__ kp_xy,
                                       int* __restrict__ kp_level, int* __restrict__ kp_lxy) {
  const int p = level_p(K.l), q = level_q(K.l), x = centre(K.u, p, q), y = centre(K.v, p, q);
  kp_pix[k] = y * L.w[0] + x;
  kp_xy[2 * k] = x; kp_xy[2 * k + 1] = y;
  kp_level[k] = K.l;
  kp_lxy[2 * k] = K.u; kp_lxy[2 * k + 1] = K.v;
}
// the word store of D6s and D6os; D6 (rpe_feature.hip) and D6o (rpe_feature_oriented.hip) state it too (see rpe_feature_rules.hpp)
__device__ __forceinline__ void store_words(const unsigned long long (&m)[4], int lane, int k, unsigned int* __restrict__ kp_desc) {
  if (lane < 8) {
    const int j = lane >> 1;
    const unsigned long long mj = j == 0 ? m[0] : j == 1 ? m[1] : j == 2 ? m[2] : m[3];
    kp_desc[8 * k + lane] = (unsigned int)(mj >> (32 * (lane & 1)));
  }
}

__global__ __launch_bounds__(256) void feat_describe_levels_kernel(const unsigned short* __restrict__ box, FeatLevels L,
                                                                  const int* __restrict__ ctl, const int* __restrict__ kidx,
                                                                  int* __restrict__ kp_pix, int* __restrict__ kp_xy,
                                                                  unsigned int* __restrict__ kp_desc, int* __restrict__ kp_level,
                                                                  int* __restrict__ kp_lxy) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= ctl[kFeatCtlCount]) return;
  const int g = kidx[k];
  const LevelKeypoint K = level_keypoint(L, g);
  unsigned long long m[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    // D6's tests, stated here and in rpe_feature.hip (see rpe_feature_rules.hpp); both samples are pixels of the level (16 px inside)
    const signed char* q = kBriefPairs[j * 64 + lane];
    const int a = box[g + q[1] * K.w + q[0]], b = box[g + q[3] * K.w + q[2]];
    m[j] = __ballot(a < b);
  }
  store_words(m, lane, k, kp_desc);
  if (lane == 8) report(L, K, k, kp_pix, kp_xy, kp_level, kp_lxy);
}

__global__ __launch_bounds__(256) void feat_describe_oriented_levels_kernel(const unsigned short* __restrict__ lum,
                                                                           const unsigned short* __restrict__ box, FeatLevels L,
                                                                           const int* __restrict__ ctl, const int* __restrict__ kidx,
                                                                           int* __restrict__ kp_pix, int* __restrict__ kp_xy,
                                                                           unsigned int* __restrict__ kp_desc, int* __restrict__ kp_bin,
                                                                           int* __restrict__ kp_level, int* __restrict__ kp_lxy) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= ctl[kFeatCtlCount]) return;
  const int g = kidx[k];
  const LevelKeypoint K = level_keypoint(L, g);
  // moments, angle bin and steered tests: stated here and in D6o of rpe_feature_oriented.hip (see rpe_feature_rules.hpp)
  // the moments: a keypoint lies 16 px inside its level, the whole disc with it
  int m10 = 0, m01 = 0;
  for (int i = lane; i < kDiscPixels; i += 64) {
    const int dx = kDisc.d[i][0], dy = kDisc.d[i][1];
    const int y = lum[g + dy * K.w + dx] & 0xff;
    m10 += dx * y; m01 += dy * y;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { m10 += __shfl_xor(m10, o); m01 += __shfl_xor(m01, o); }
  // lane l scores bin l % 32 (both halves of the wave hold the same 32 candidates); the larger score wins, the lower bin on a tie
  int bin = lane & (kAngleBins - 1);
  long long best = (long long)m10 * kAngleCos[bin] + (long long)m01 * kAngleCos[(bin + 24) & (kAngleBins - 1)];
#pragma unroll
  for (int o = kAngleBins / 2; o >= 1; o >>= 1) {
    const long long os = __shfl_xor(best, o);
    const int ob = __shfl_xor(bin, o);
    if (os > best || (os == best && ob < bin)) { best = os; bin = ob; }
  }
  bin = __builtin_amdgcn_readfirstlane(bin);
  const int c = kAngleCos[bin], s = kAngleCos[(bin + 24) & (kAngleBins - 1)];
  const unsigned short* lbox = box + K.base;
  unsigned long long m[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const signed char* q = kBriefPairs[j * 64 + lane];
    // >> on a negative int is the arithmetic shift: floor.  A sample outside THE LEVEL's image reads 0
    const int ax = K.u + ((q[0] * c - q[1] * s + 512) >> 10), ay = K.v + ((q[0] * s + q[1] * c + 512) >> 10);
    const int bx = K.u + ((q[2] * c - q[3] * s + 512) >> 10), by = K.v + ((q[2] * s + q[3] * c + 512) >> 10);
    const bool aok = ax >= 0 && ax < K.w && ay >= 0 && ay < K.h, bok = bx >= 0 && bx < K.w && by >= 0 && by < K.h;
    const int a = aok ? lbox[ay * K.w + ax] : 0, b = bok ? lbox[by * K.w + bx] : 0;
    m[j] = __ballot(a < b);
  }
  store_words(m, lane, k, kp_desc);
  if (lane == 8) report(L, K, k, kp_pix, kp_xy, kp_level, kp_lxy);
  if (lane == 9) kp_bin[k] = bin;
}

}  // namespace

hipError_t launch_feature_detect_levels(const unsigned int* rgba, const float* vmap, const float* nmap, const FeatLevels& L, int threshold,
                                        int max_keypoints, const FeatureWork& W, int kind, int* kp_pix, int* kp_score, int* kp_xy,
                                        unsigned int* kp_desc, int* kp_bin, int* kp_level, int* kp_lxy, hipStream_t s) {
  const int n = L.base[kFeatMaxLevels], nchunks = (n + kChunk - 1) / kChunk;
  hipError_t e = hipMemsetAsync(W.hist, 0, kFeatScoreBins * sizeof(unsigned int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(feat_resample_kernel, dim3(nchunks), dim3(256), 0, s, rgba, L, W.lum);
  hipLaunchKernelGGL(feat_score_levels_kernel, dim3(L.tile[kFeatMaxLevels]), dim3(kTileX * kTileY), 0, s, W.lum, vmap, nmap, L, threshold,
                     W.score, W.box);
  hipLaunchKernelGGL(feat_nms_levels_kernel, dim3(nchunks), dim3(kChunk), 0, s, W.score, L, W.chunk, W.hist);
  if ((e = launch_feature_scan(W, nchunks, max_keypoints, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(feat_compact_levels_kernel, dim3(nchunks), dim3(kChunk), 0, s, W.score, L, W.chunk, W.spix);
  if ((e = launch_feature_select(W, max_keypoints, W.kidx, kp_score, s)) != hipSuccess) return e;
  if (kind == kDescOriented)
    hipLaunchKernelGGL(feat_describe_oriented_levels_kernel, dim3((max_keypoints + 3) / 4), dim3(256), 0, s, W.lum, W.box, L, W.ctl, W.kidx,
                       kp_pix, kp_xy, kp_desc, kp_bin, kp_level, kp_lxy);
  else
    hipLaunchKernelGGL(feat_describe_levels_kernel, dim3((max_keypoints + 3) / 4), dim3(256), 0, s, W.box, L, W.ctl, W.kidx, kp_pix, kp_xy,
                       kp_desc, kp_level, kp_lxy);
  return hipGetLastError();
}

RPE_PRELOAD(feat_score_levels_kernel);

}  // namespace rpe
