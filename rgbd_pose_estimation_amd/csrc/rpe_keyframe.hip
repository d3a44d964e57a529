// gfx950 kernels of the KEYFRAME store: the features of many model views kept on the device, and one frame matched against all of them
// at once -- which keyframe a lost tracker should relocalise against, without re-detecting anything.
//
//   K1  kf_snapshot_kernel   per model keypoint: its descriptor row, xy, and the model's level-0 world vertex and normal at its pixel,
//                            into the packed store at the keyframe's offset.
//   K2  kf_best_kernel       (d1, index, d2) of every keypoint of list A over every SEGMENT of list B.  One lane per keypoint of A, its
//                            descriptor in 8 registers; the descriptors of B are the same for the whole wave and come through the
//                            scalar cache, so a pair costs 16 vector instructions (xor + counting add per word) and its compares --
//                            no LDS traffic, no cross-lane merge.  The four waves of a workgroup take contiguous quarters of the
//                            segment and wave 0 merges them in index order under the tie rule.  Grid: groups of 64 keypoints of A x
//                            segments.  The query is A = the frame, segments = the keyframes; the cross-check is A = the whole store,
//                            one segment = the frame.  A workgroup's work is its own segment's length: an empty keyframe costs its
//                            workgroups one offset read and one store.  With `counts` the acceptance test of rpe_features_match is
//                            applied to the merged result and the accepted pairs are counted per segment (one atomicAdd per
//                            workgroup: an integer count, its value does not depend on the adds' order).
//   K3  kf_rank_kernel       one workgroup: the keyframes ordered by (count descending, id ascending); rank = the number of keyframes
//                            that come before.
//   K4  kf_gather_kernel     the five solver slots of one keyframe's accepted matches: XW / NW from the store, XC / NC / BV from the
//                            frame's maps.  (The accepted list itself is M2 of rpe_feature.hip, on the keyframe's row of K2's output:
//                            ids from scans, frame-keypoint order.)
//
// The rules are those of include/rgbd_pose_hip.h Part 3 ("Features and relocalisation", "Keyframes"): integer arithmetic and comparisons
// only; tests/keyframe_oracle.py is their numpy statement and the results are its bits.
#include "rpe_assoc.h"

namespace rpe {

namespace {

constexpr int kLanes = 64;     // K2: keypoints of list A per workgroup, one per lane
constexpr int kWaves = 4;      // K2: waves per workgroup, a contiguous quarter of the segment each

// ---------------------------------------------------------------------------------------------- K1
__global__ __launch_bounds__(256) void kf_snapshot_kernel(int count, const int* __restrict__ pix, const int* __restrict__ xy,
                                                         const unsigned int* __restrict__ desc, const float* __restrict__ mv,
                                                         const float* __restrict__ mn, KeyframeStore S, int base) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const int64_t o = (int64_t)base + k, p = pix[k];
  ((uint4*)S.desc)[2 * o] = ((const uint4*)desc)[2 * k];
  ((uint4*)S.desc)[2 * o + 1] = ((const uint4*)desc)[2 * k + 1];
  ((int2*)S.xy)[o] = ((const int2*)xy)[k];
#pragma unroll
  for (int c = 0; c < 3; c++) { S.xw[3 * o + c] = mv[3 * p + c]; S.nw[3 * o + c] = mn[3 * p + c]; }
}

// ---------------------------------------------------------------------------------------------- K2
struct Best { int d1, idx, d2; };
// the best two of two disjoint sets: the smaller (d1, idx) wins, the loser's d1 competes for d2
__device__ __forceinline__ Best merge(const Best& a, const Best& b) {
  const bool af = a.d1 < b.d1 || (a.d1 == b.d1 && (unsigned)a.idx < (unsigned)b.idx);   // idx -1 (nothing seen) loses every tie
  Best r;
  r.d1 = af ? a.d1 : b.d1; r.idx = af ? a.idx : b.idx;
  r.d2 = af ? min(a.d2, b.d1) : min(b.d2, a.d1);
  return r;
}

__global__ __launch_bounds__(kLanes * kWaves) void kf_best_kernel(const unsigned int* __restrict__ desc_a, int na,
                                                                 const unsigned int* __restrict__ desc_b, const int* __restrict__ off,
                                                                 int seg0, int one_lo, int one_n, KeyframeAccept acc,
                                                                 int* __restrict__ od1, int* __restrict__ oidx, int* __restrict__ od2,
                                                                 int* __restrict__ counts) {
  __shared__ int part[kWaves - 1][3][kLanes];
  const int lane = threadIdx.x & (kLanes - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int seg = seg0 + blockIdx.y;
  const int q = blockIdx.x * kLanes + lane;
  // the segment of list B: keyframe `seg` of the store, or (off == nullptr) the one list [one_lo, one_lo + one_n)
  const int b0 = off ? off[seg] : one_lo, nb = off ? off[seg + 1] - b0 : one_n;
  const int64_t o = (int64_t)blockIdx.y * na + q;
  if (nb <= 0) {                                  // the same for the whole workgroup
    if (wave == 0 && q < na) { if (od1) od1[o] = 257; oidx[o] = -1; if (od2) od2[o] = 257; }
    return;
  }
  uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
  if (q < na) { qa = ((const uint4*)desc_a)[2 * (int64_t)q]; qb = ((const uint4*)desc_a)[2 * (int64_t)q + 1]; }
  const int per = (nb + kWaves - 1) / kWaves, lo = wave * per, hi = min(nb, lo + per);
  const uint4* __restrict__ B = (const uint4*)desc_b + 2 * (int64_t)b0;
  Best best{257, -1, 257};
#pragma unroll 4
  for (int j = lo; j < hi; j++) {                 // j is the wave's: one descriptor of B for all 64 lanes.  Ascending index per lane:
    const uint4 ta = B[2 * j], tb = B[2 * j + 1]; // strict < keeps the lowest on a tie
    const int d = (__popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y)) + (__popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w))
                + (__popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y)) + (__popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w));
    if (d < best.d1) { best.d2 = best.d1; best.d1 = d; best.idx = j; }
    else if (d < best.d2) best.d2 = d;
  }
  if (wave > 0) { part[wave - 1][0][lane] = best.d1; part[wave - 1][1][lane] = best.idx; part[wave - 1][2][lane] = best.d2; }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < kWaves - 1; w++) best = merge(best, Best{part[w][0][lane], part[w][1][lane], part[w][2][lane]});
  if (q < na) { if (od1) od1[o] = best.d1; oidx[o] = best.idx; if (od2) od2[o] = best.d2; }
  if (counts) {
    bool ok = q < na && best.idx >= 0 && best.d1 <= acc.max_dist && best.d1 * acc.ratio_den < best.d2 * acc.ratio_num;
    if (ok && acc.back) ok = acc.back[b0 + best.idx] == q;
    const int n = __popcll(__ballot(ok));
    if (lane == 0 && n > 0) atomicAdd(&counts[seg], n);
  }
}

// ---------------------------------------------------------------------------------------------- K3
__global__ __launch_bounds__(256) void kf_rank_kernel(const int* __restrict__ counts, int K, int* __restrict__ order) {
  __shared__ int c[256];
  const int i = threadIdx.x;
  c[i] = i < K ? counts[i] : -1;
  __syncthreads();
  if (i >= K) return;
  const int mine = c[i];
  int before = 0;
  for (int j = 0; j < K; j++) before += (c[j] > mine || (c[j] == mine && j < i)) ? 1 : 0;
  order[before] = i;
}

// ---------------------------------------------------------------------------------------------- K4
__global__ __launch_bounds__(256) void kf_gather_kernel(const int* __restrict__ mf, const int* __restrict__ mm, int matches,
                                                       const int* __restrict__ fpix, const float* __restrict__ fv,
                                                       const float* __restrict__ fn, const float* __restrict__ fb, KeyframeStore S, int base,
                                                       float* __restrict__ xw, float* __restrict__ xc, float* __restrict__ bv,
                                                       float* __restrict__ nw, float* __restrict__ nc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= matches) return;
  const int64_t f = fpix[mf[k]], m = (int64_t)base + mm[k];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    xw[3 * k + c] = S.xw[3 * m + c]; nw[3 * k + c] = S.nw[3 * m + c];
    xc[3 * k + c] = fv[3 * f + c]; nc[3 * k + c] = fn[3 * f + c]; bv[3 * k + c] = fb[3 * f + c];
  }
}

}  // namespace

hipError_t launch_keyframe_snapshot(int count, const int* pix, const int* xy, const unsigned int* desc, const float* mv, const float* mn,
                                    const KeyframeStore& S, int base, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(kf_snapshot_kernel, dim3((count + 255) / 256), dim3(256), 0, s, count, pix, xy, desc, mv, mn, S, base);
  return hipGetLastError();
}

hipError_t launch_keyframe_best(const unsigned int* desc_a, int na, const unsigned int* desc_b, const int* off, int seg0, int segments,
                                int one_lo, int one_n, const KeyframeAccept& acc, int* d1, int* idx, int* d2, int* counts, hipStream_t s) {
  if (na <= 0 || segments <= 0) return hipSuccess;
  hipLaunchKernelGGL(kf_best_kernel, dim3((na + kLanes - 1) / kLanes, segments), dim3(kLanes * kWaves), 0, s, desc_a, na, desc_b, off, seg0,
                     one_lo, one_n, acc, d1, idx, d2, counts);
  return hipGetLastError();
}

hipError_t launch_keyframe_rank(const int* counts, int K, int* order, hipStream_t s) {
  if (K < 1 || K > 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kf_rank_kernel, dim3(1), dim3(256), 0, s, counts, K, order);
  return hipGetLastError();
}

hipError_t launch_keyframe_gather(const int* mf, const int* mm, int matches, const int* fpix, const float* fv, const float* fn,
                                  const float* fb, const KeyframeStore& S, int base, float* xw, float* xc, float* bv, float* nw, float* nc,
                                  hipStream_t s) {
  if (matches <= 0) return hipSuccess;
  hipLaunchKernelGGL(kf_gather_kernel, dim3((matches + 255) / 256), dim3(256), 0, s, mf, mm, matches, fpix, fv, fn, fb, S, base, xw, xc, bv,
                     nw, nc);
  return hipGetLastError();
}

RPE_PRELOAD(kf_best_kernel);

}  // namespace rpe
