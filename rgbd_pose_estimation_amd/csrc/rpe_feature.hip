// gfx950 kernels of the FEATURE stage: keypoints and binary descriptors of a view's colour, and their matches between the frame and the
// model view -- the correspondences of a relocalisation, made without a pose guess.
//
//   D1  feat_score_kernel      a workgroup owns a 32 x 8 tile and keeps its u8 luma (+ the A != 0 bit) with a halo of 3 in LDS: the 5 x 5
//                              box sum of every pixel (u16 image, what the descriptor compares) and the segment-test score of the ring of
//                              radius 3 (int image, 0 = no corner).
//   D2  feat_nms_kernel        3 x 3 non-maximum suppression on the scores; per chunk of 256 consecutive pixels the number of
//                              survivors, and the histogram of their scores (a count: its value does not depend on the adds' order).
//   D3  feat_scan_kernel       one workgroup: chunk counts -> chunk offsets, the survivors' total, and from the histogram the score cut
//                              T and the number of score-T survivors to keep when there are more survivors than max_keypoints.
//   D4  feat_compact_kernel    the survivors' pixel indices, in pixel order (offset of the chunk + rank in the chunk).
//   D5  feat_select_kernel     one workgroup walks the survivors: kept iff score > T, or score == T and among the first `ties` of
//                              those in pixel order; the kept ones' slot = their rank (two scans per 1024 survivors).
//   D6  feat_describe_kernel   one wave per keypoint: lane l makes tests l, l + 64, l + 128, l + 192 on the box-sum image, four ballots
//                              are the eight words, lanes 0-7 store them (one 32-byte row).  (RPE_DESC_ORIENTED: its sibling D6o in
//                              rpe_feature_oriented.hip takes this kernel's place in the detection.)
//   M1  feat_best_kernel       16 lanes per keypoint of list A, its descriptor in 8 registers; list B streams through LDS in tiles of
//                              256 descriptors laid out word-major (lanes of a group read consecutive banks, the wave's four groups the
//                              same addresses); (d1, index, d2) per lane, merged across the 16 lanes under the tie rule.
//   M2  feat_accept_kernel     one workgroup: distance, ratio and cross-check tests, the accepted matches in frame-keypoint order.
//   M3  feat_gather_kernel     the matched pixels' vertices, normals and bearings into the five solver slots.
//
// The conventions (include/rgbd_pose_hip.h Part 3, "Features and relocalisation") are integer arithmetic and comparisons throughout;
// tests/feature_oracle.py is their numpy statement and the results are its bits.  Nothing is placed by an atomic: ids come from scans.
#include "rpe_assoc.h"
#include "rpe_feature_rules.hpp"   // the rules the scale levels share: luma, the segment test, survives

namespace rpe {

namespace {

constexpr int kChunk = 256;      // D2, D4: pixels per workgroup
constexpr int kWide = 1024;      // D3, D5, M2: the single workgroup
constexpr int kGroup = 16;       // M1: lanes per keypoint
constexpr int kTileB = 256;      // M1: descriptors of list B per LDS tile

// exclusive scan of v over the workgroup's B threads (B a multiple of 64) and the sum of all; lds: B / 64 ints, free again on return
template <int B> __device__ __forceinline__ int block_scan(int v, int* lds, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < B / 64; k++) { const int t = lds[k]; base += k < wave ? t : 0; tot += t; }
  __syncthreads();
  total = tot;
  return base + x - v;
}

// ---------------------------------------------------------------------------------------------- D1
__global__ __launch_bounds__(kTileX * kTileY) void feat_score_kernel(const unsigned int* __restrict__ rgba, const float* __restrict__ vmap,
                                                                    const float* __restrict__ nmap, int w, int h, int thr,
                                                                    int* __restrict__ score, unsigned short* __restrict__ box) {
  __shared__ FeatTile t;
  const int u0 = blockIdx.x * kTileX, v0 = blockIdx.y * kTileY;
  for (int i = threadIdx.x; i < kLdsX * kLdsY; i += kTileX * kTileY) {
    const int ly = i / kLdsX, lx = i - ly * kLdsX;
    const int gu = u0 + lx - kHalo, gv = v0 + ly - kHalo;
    unsigned px = 0;
    if (gu >= 0 && gu < w && gv >= 0 && gv < h) px = rgba[gv * w + gu];
    const unsigned known = (px >> 24) != 0;
    const unsigned y = luma(px);
    t[ly][lx] = (unsigned short)(known ? (y | 0x100u) : 0u);
  }
  __syncthreads();
  const int tx = threadIdx.x & (kTileX - 1), ty = threadIdx.x / kTileX;
  const int u = u0 + tx, v = v0 + ty;
  if (u >= w || v >= h) return;
  const int cx = tx + kHalo, cy = ty + kHalo, idx = v * w + u;
  int S = 0;   // the 5 x 5 box sum, what the descriptor compares (stated in D1 and D1s: rpe_feature_rules.hpp, header)
#pragma unroll
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) S += t[cy + dy][cx + dx] & 0xff;
  box[idx] = (unsigned short)S;
  score[idx] = segment_score(t, cx, cy, u, v, w, h, thr, [=] {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && __builtin_isfinite(vmap[3 * (int64_t)idx + k]) && __builtin_isfinite(nmap[3 * (int64_t)idx + k]);
    return fin;
  });
}

// ---------------------------------------------------------------------------------------------- D2, D4
// survives(score, i, w): rpe_feature_rules.hpp
__global__ __launch_bounds__(kChunk) void feat_nms_kernel(const int* __restrict__ score, int n, int w, int* __restrict__ chunk,
                                                         unsigned int* __restrict__ hist) {
  const int i = blockIdx.x * kChunk + threadIdx.x;
  const bool keep = i < n && survives(score, i, w);
  if (keep) atomicAdd(&hist[min(score[i], kFeatScoreBins - 1)], 1u);
  const int cnt = __syncthreads_count(keep);
  if (threadIdx.x == 0) chunk[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(kChunk) void feat_compact_kernel(const int* __restrict__ score, int n, int w, const int* __restrict__ chunk,
                                                             int* __restrict__ spix) {
  __shared__ int lds[kChunk / 64];
  const int i = blockIdx.x * kChunk + threadIdx.x;
  const bool keep = i < n && survives(score, i, w);
  int total;
  const int rank = block_scan<kChunk>(keep ? 1 : 0, lds, total);
  if (keep) spix[chunk[blockIdx.x] + rank] = i;
}

// ---------------------------------------------------------------------------------------------- D3
__global__ __launch_bounds__(kWide) void feat_scan_kernel(int* __restrict__ chunk, int nchunks, const unsigned int* __restrict__ hist,
                                                         int max_keypoints, int* __restrict__ ctl) {
  __shared__ int lds[kWide / 64];
  int run = 0;
  for (int base = 0; base < nchunks; base += kWide) {
    const int i = base + threadIdx.x;
    const int v = i < nchunks ? chunk[i] : 0;
    int total;
    const int ex = block_scan<kWide>(v, lds, total);
    if (i < nchunks) chunk[i] = run + ex;
    run += total;
  }
  // the cut: the largest T with #(score >= T) >= max_keypoints; this thread owns four bins, scores descending with the thread index
  constexpr int per = kFeatScoreBins / kWide;
  const int top = kFeatScoreBins - 1 - per * threadIdx.x;
  int mine[per], own = 0;
#pragma unroll
  for (int k = 0; k < per; k++) { mine[k] = (int)hist[top - k]; own += mine[k]; }
  int total;
  int above = block_scan<kWide>(own, lds, total);
  if (threadIdx.x == 0) { ctl[kFeatCtlSurvivors] = run; if (run <= max_keypoints) { ctl[kFeatCtlCut] = 0; ctl[kFeatCtlTies] = 0; } }
  if (run > max_keypoints) {
#pragma unroll
    for (int k = 0; k < per; k++) {
      if (above < max_keypoints && above + mine[k] >= max_keypoints) { ctl[kFeatCtlCut] = top - k; ctl[kFeatCtlTies] = max_keypoints - above; }
      above += mine[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------- D5
__global__ __launch_bounds__(kWide) void feat_select_kernel(const int* __restrict__ score, const int* __restrict__ spix, int max_keypoints,
                                                           int* __restrict__ ctl, int* __restrict__ kp_pix, int* __restrict__ kp_score) {
  __shared__ int lds[kWide / 64];
  const int n = ctl[kFeatCtlSurvivors], T = ctl[kFeatCtlCut], ties = ctl[kFeatCtlTies];
  int run_eq = 0, run_keep = 0;
  for (int base = 0; base < n; base += kWide) {
    const int i = base + threadIdx.x;
    const int p = i < n ? spix[i] : 0;
    const int s = i < n ? score[p] : 0;
    const bool eq = i < n && s == T;
    int total;
    const int eq_rank = run_eq + block_scan<kWide>(eq ? 1 : 0, lds, total);
    run_eq += total;
    const bool keep = i < n && (s > T || (eq && eq_rank < ties));
    const int slot = run_keep + block_scan<kWide>(keep ? 1 : 0, lds, total);
    run_keep += total;
    if (keep && slot < max_keypoints) { kp_pix[slot] = p; kp_score[slot] = s; }
  }
  if (threadIdx.x == 0) ctl[kFeatCtlCount] = min(run_keep, max_keypoints);
}

// ---------------------------------------------------------------------------------------------- D6
__global__ __launch_bounds__(256) void feat_describe_kernel(const unsigned short* __restrict__ box, int w, const int* __restrict__ ctl,
                                                           const int* __restrict__ kp_pix, int* __restrict__ kp_xy,
                                                           unsigned int* __restrict__ kp_desc) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= ctl[kFeatCtlCount]) return;
  const int p = kp_pix[k];
  unsigned long long m[4];
  // the tests and the word store: stated here and in rpe_feature_scale.hip (see rpe_feature_rules.hpp)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const signed char* q = kBriefPairs[j * 64 + lane];
    const int a = box[p + q[1] * w + q[0]], b = box[p + q[3] * w + q[2]];
    m[j] = __ballot(a < b);
  }
  if (lane < 8) {
    const int j = lane >> 1;
    const unsigned long long mj = j == 0 ? m[0] : j == 1 ? m[1] : j == 2 ? m[2] : m[3];
    kp_desc[8 * k + lane] = (unsigned int)(mj >> (32 * (lane & 1)));
  }
  if (lane == 8) { kp_xy[2 * k] = p % w; kp_xy[2 * k + 1] = p / w; }
}

// ---------------------------------------------------------------------------------------------- M1
struct Best { int d1, idx, d2; };
// the best two of two disjoint sets: the smaller (d1, idx) wins, the loser's d1 competes for d2
__device__ __forceinline__ Best merge(const Best& a, const Best& b) {
  const bool af = a.d1 < b.d1 || (a.d1 == b.d1 && (unsigned)a.idx < (unsigned)b.idx);   // idx -1 (nothing seen) loses every tie
  Best r;
  r.d1 = af ? a.d1 : b.d1; r.idx = af ? a.idx : b.idx;
  r.d2 = af ? min(a.d2, b.d1) : min(b.d2, a.d1);
  return r;
}

__global__ __launch_bounds__(256) void feat_best_kernel(const unsigned int* __restrict__ desc_a, int na, const unsigned int* __restrict__ desc_b,
                                                       int nb, int* __restrict__ od1, int* __restrict__ oidx, int* __restrict__ od2) {
  __shared__ unsigned int tile[8][kTileB];
  const int q = blockIdx.x * (256 / kGroup) + threadIdx.x / kGroup, sub = threadIdx.x & (kGroup - 1);
  uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
  if (q < na) { qa = ((const uint4*)desc_a)[2 * q]; qb = ((const uint4*)desc_a)[2 * q + 1]; }
  Best best{257, -1, 257};
  for (int base = 0; base < nb; base += kTileB) {
    __syncthreads();
    const int mine = base + threadIdx.x;
    uint4 ta = make_uint4(0, 0, 0, 0), tb = ta;
    if (mine < nb) { ta = ((const uint4*)desc_b)[2 * mine]; tb = ((const uint4*)desc_b)[2 * mine + 1]; }
    tile[0][threadIdx.x] = ta.x; tile[1][threadIdx.x] = ta.y; tile[2][threadIdx.x] = ta.z; tile[3][threadIdx.x] = ta.w;
    tile[4][threadIdx.x] = tb.x; tile[5][threadIdx.x] = tb.y; tile[6][threadIdx.x] = tb.z; tile[7][threadIdx.x] = tb.w;
    __syncthreads();
    const int cnt = min(kTileB, nb - base);
#pragma unroll 4
    for (int j = sub; j < cnt; j += kGroup) {     // ascending index per lane: strict < keeps the lowest on a tie
      const int d = (__popc(qa.x ^ tile[0][j]) + __popc(qa.y ^ tile[1][j])) + (__popc(qa.z ^ tile[2][j]) + __popc(qa.w ^ tile[3][j]))
                  + (__popc(qb.x ^ tile[4][j]) + __popc(qb.y ^ tile[5][j])) + (__popc(qb.z ^ tile[6][j]) + __popc(qb.w ^ tile[7][j]));
      if (d < best.d1) { best.d2 = best.d1; best.d1 = d; best.idx = base + j; }
      else if (d < best.d2) best.d2 = d;
    }
  }
#pragma unroll
  for (int o = kGroup / 2; o >= 1; o >>= 1) {
    Best other;
    other.d1 = __shfl_xor(best.d1, o); other.idx = __shfl_xor(best.idx, o); other.d2 = __shfl_xor(best.d2, o);
    best = merge(best, other);
  }
  if (sub == 0 && q < na) { od1[q] = best.d1; oidx[q] = best.idx; od2[q] = best.d2; }
}

// ---------------------------------------------------------------------------------------------- M2, M3
__global__ __launch_bounds__(kWide) void feat_accept_kernel(MatchLists L, int nf, int max_dist, int ratio_num, int ratio_den, int cross_check,
                                                           int* __restrict__ ctl) {
  __shared__ int lds[kWide / 64];
  int run = 0;
  for (int base = 0; base < nf; base += kWide) {
    const int q = base + threadIdx.x;
    bool ok = false;
    int d1 = 0, d2 = 0, idx = -1;
    if (q < nf) {
      d1 = L.d1[q]; d2 = L.d2[q]; idx = L.idx[q];
      ok = idx >= 0 && d1 <= max_dist && d1 * ratio_den < d2 * ratio_num;
      if (ok && cross_check) ok = L.back[idx] == q;
    }
    int total;
    const int slot = run + block_scan<kWide>(ok ? 1 : 0, lds, total);
    run += total;
    if (ok) { L.mf[slot] = q; L.mm[slot] = idx; L.md1[slot] = d1; L.md2[slot] = d2; L.mw[slot] = (float)(256 - d1); }
  }
  if (threadIdx.x == 0) ctl[kFeatCtlMatches] = run;
}

__global__ __launch_bounds__(256) void feat_gather_kernel(MatchLists L, int matches, const int* __restrict__ fpix, const int* __restrict__ mpix,
                                                         const float* __restrict__ fv, const float* __restrict__ fn, const float* __restrict__ fb,
                                                         const float* __restrict__ mv, const float* __restrict__ mn, float* __restrict__ xw,
                                                         float* __restrict__ xc, float* __restrict__ bv, float* __restrict__ nw,
                                                         float* __restrict__ nc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= matches) return;
  const int64_t f = fpix[L.mf[k]], m = mpix[L.mm[k]];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    xw[3 * k + c] = mv[3 * m + c]; nw[3 * k + c] = mn[3 * m + c];
    xc[3 * k + c] = fv[3 * f + c]; nc[3 * k + c] = fn[3 * f + c]; bv[3 * k + c] = fb[3 * f + c];
  }
}

}  // namespace

hipError_t launch_feature_detect(const unsigned int* rgba, const float* vmap, const float* nmap, int w, int h, int threshold, int max_keypoints,
                                 const FeatureWork& W, int kind, int* kp_pix, int* kp_score, int* kp_xy, unsigned int* kp_desc, int* kp_bin,
                                 hipStream_t s) {
  const int n = w * h, nchunks = (n + kChunk - 1) / kChunk;
  hipError_t e = hipMemsetAsync(W.hist, 0, kFeatScoreBins * sizeof(unsigned int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(feat_score_kernel, dim3((w + kTileX - 1) / kTileX, (h + kTileY - 1) / kTileY), dim3(kTileX * kTileY), 0, s, rgba, vmap,
                     nmap, w, h, threshold, W.score, W.box);
  hipLaunchKernelGGL(feat_nms_kernel, dim3(nchunks), dim3(kChunk), 0, s, W.score, n, w, W.chunk, W.hist);
  hipLaunchKernelGGL(feat_scan_kernel, dim3(1), dim3(kWide), 0, s, W.chunk, nchunks, W.hist, max_keypoints, W.ctl);
  hipLaunchKernelGGL(feat_compact_kernel, dim3(nchunks), dim3(kChunk), 0, s, W.score, n, w, W.chunk, W.spix);
  hipLaunchKernelGGL(feat_select_kernel, dim3(1), dim3(kWide), 0, s, W.score, W.spix, max_keypoints, W.ctl, kp_pix, kp_score);
  if (kind == kDescOriented) return launch_feature_describe_oriented(rgba, W.box, w, h, max_keypoints, W.ctl, kp_pix, kp_xy, kp_desc, kp_bin, s);
  hipLaunchKernelGGL(feat_describe_kernel, dim3((max_keypoints + 3) / 4), dim3(256), 0, s, W.box, w, W.ctl, kp_pix, kp_xy, kp_desc);
  return hipGetLastError();
}

hipError_t launch_feature_scan(const FeatureWork& W, int nchunks, int max_keypoints, hipStream_t s) {
  hipLaunchKernelGGL(feat_scan_kernel, dim3(1), dim3(kWide), 0, s, W.chunk, nchunks, W.hist, max_keypoints, W.ctl);
  return hipGetLastError();
}

hipError_t launch_feature_select(const FeatureWork& W, int max_keypoints, int* kp_idx, int* kp_score, hipStream_t s) {
  hipLaunchKernelGGL(feat_select_kernel, dim3(1), dim3(kWide), 0, s, W.score, W.spix, max_keypoints, W.ctl, kp_idx, kp_score);
  return hipGetLastError();
}

hipError_t launch_feature_best(const unsigned int* desc_a, int na, const unsigned int* desc_b, int nb, int* d1, int* idx, int* d2, hipStream_t s) {
  if (na <= 0) return hipSuccess;
  hipLaunchKernelGGL(feat_best_kernel, dim3((na + 256 / kGroup - 1) / (256 / kGroup)), dim3(256), 0, s, desc_a, na, desc_b, nb, d1, idx, d2);
  return hipGetLastError();
}

hipError_t launch_feature_accept(const MatchLists& L, int nf, int max_dist, int ratio_num, int ratio_den, int cross_check, int* ctl, hipStream_t s) {
  hipLaunchKernelGGL(feat_accept_kernel, dim3(1), dim3(kWide), 0, s, L, nf, max_dist, ratio_num, ratio_den, cross_check, ctl);
  return hipGetLastError();
}

hipError_t launch_feature_gather(const MatchLists& L, int matches, const int* fpix, const int* mpix, const float* fv, const float* fn,
                                 const float* fb, const float* mv, const float* mn, float* xw, float* xc, float* bv, float* nw, float* nc,
                                 hipStream_t s) {
  if (matches <= 0) return hipSuccess;
  hipLaunchKernelGGL(feat_gather_kernel, dim3((matches + 255) / 256), dim3(256), 0, s, L, matches, fpix, mpix, fv, fn, fb, mv, mn, xw, xc, bv,
                     nw, nc);
  return hipGetLastError();
}

RPE_PRELOAD(feat_best_kernel);

}  // namespace rpe
