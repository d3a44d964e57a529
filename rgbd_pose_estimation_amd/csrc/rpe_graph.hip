// gfx950 kernels of the KEYFRAME GRAPH: the keyframes of the store linked by their matches, and all of their poses refined jointly.
//
//   G1  graph_pack_kernel    per (keyframe j, older keyframe i): the accepted matches of j's keypoints against i's, compacted in the
//                            order of j's keypoints into the pair arrays at the offset the host gives for i.  One workgroup per i; 16 consecutive
//                            keypoints per thread, the positions from a scan over the threads' counts (shuffles within a wave, the four
//                            waves' totals through LDS) -- no atomics, the order is the list order.  The acceptance
//                            test is K2's (rpe_keyframe.hip), on K2's own rows.
//   G2  graph_round_kernel   ONE launch for every edge of the graph, one workgroup per edge (3 .. 4096 pairs: at most 16 per thread).
//                            Per pair, in fp32 with the operation order below: X = C_j x_a + c_j, Y = C_i x_b + c_i, r = X - Y and the
//                            gate.  Everything behind the fp32 rows is fp64: the 38 sums of the record are sums of products of the
//                            fp32 values X, Y, r formed in fp64 (a product of two fp32 numbers is exact there), per thread in pair
//                            order, then over the wave by the fixed shuffle-down tree 32, 16, 8, 4, 2, 1, then the four waves in
//                            wave order.  No float atomics: the same call gives the same bits.
//   G3  graph_rows_kernel    r of every pair (NaN where it does not count): the inspection form of G2's rows.
//   G4  graph_apply_kernel   the store rewritten at the corrected poses: xw <- C_k xw + c_k, nw <- C_k nw.
//
// The fp32 operation order, everywhere (tests/graph_oracle.py states it in numpy): with C row-major and c,
//   X[r] = (((C[3r] * x[0]) + (C[3r + 1] * x[1])) + (C[3r + 2] * x[2])) + c[r]      -- every product and sum rounded on its own, no FMA
//   N[r] =  ((C[3r] * n[0]) + (C[3r + 1] * n[1])) + (C[3r + 2] * n[2])
//   r = X - Y,  s = ((r0 * r0) + (r1 * r1)) + (r2 * r2);  the pair counts iff the six coordinates of x_a, x_b are finite and s < gate2.
//
// The raw record (kGraphRaw doubles per edge; the sums run over the counted pairs, X of keyframe j, Y of keyframe i):
//   [0] pairs  [1] sum |r|^2  [2..4] sum r  [5..7] sum r x X  [8..10] sum Y x r  [11..13] sum X  [14..16] sum Y
//   [17..22] sum X X^T (xx xy xz yy yz zz)  [23..28] sum Y Y^T  [29..37] sum X Y^T (row-major: [29 + 3a + b] = sum X_a Y_b)
// These are the Gauss-Newton blocks with the Jacobians taken in the WORLD frame, A(X) = [-I, [X]x]: the residual's derivative by
// keyframe k's update is A(X_k) M_k with the 6 x 6 matrix M_k of the pose alone, so the host turns the record into the blocks of
// include/rgbd_pose_hip.h (RPE_GRAPH_RECORD) with three small fp64 products per edge (rpe_graph_api.hip graph_record) and the device
// needs no pose, only the corrections.
#include "rpe_assoc.h"

namespace rpe {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = kMaxKeypoints / kThreads;   // 16
constexpr int kSums = 38;

// ---------------------------------------------------------------------------------------------- G1
__global__ __launch_bounds__(kThreads) void graph_pack_kernel(const int* __restrict__ d1, const int* __restrict__ idx,
                                                             const int* __restrict__ d2, int na, const int* __restrict__ off,
                                                             KeyframeAccept acc, const int* __restrict__ counts,
                                                             GraphBases base, int* __restrict__ a, int* __restrict__ b) {
  __shared__ int wave_total[kThreads / 64];
  const int seg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int out = base.v[seg], mine = counts[seg];
  if (out < 0) return;                             // the same for the whole workgroup
  const int b0 = off[seg];
  const int64_t row = (int64_t)seg * na;
  int keep[kPerThread];
  unsigned ok = 0;
#pragma unroll
  for (int u = 0; u < kPerThread; u++) {
    const int q = t * kPerThread + u;
    keep[u] = -1;
    if (q < na) {
      const int e1 = d1[row + q], ei = idx[row + q], e2 = d2[row + q];
      bool good = ei >= 0 && e1 <= acc.max_dist && e1 * acc.ratio_den < e2 * acc.ratio_num;
      if (good && acc.back) good = acc.back[b0 + ei] == q;
      if (good) { ok |= 1u << u; keep[u] = ei; }
    }
  }
  // exclusive scan of the threads' counts: inclusive over the wave by shuffles, the waves' totals through LDS
  const int n = __popc(ok);
  int incl = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int rank = incl - n;
  for (int w = 0; w < wave; w++) rank += wave_total[w];
#pragma unroll
  for (int u = 0; u < kPerThread; u++)
    if ((ok >> u) & 1u) {
      if (rank < mine) { a[out + rank] = t * kPerThread + u; b[out + rank] = keep[u]; }   // never past the count the host made room for
      rank++;
    }
}

// ---------------------------------------------------------------------------------------------- the fp32 rows
struct Corr { float C[9], c[3]; };
__device__ __forceinline__ Corr load_corr(const float* __restrict__ corr, int k) {
  Corr T;
#pragma unroll
  for (int m = 0; m < 9; m++) T.C[m] = corr[kGraphCorr * k + m];
#pragma unroll
  for (int m = 0; m < 3; m++) T.c[m] = corr[kGraphCorr * k + 9 + m];
  return T;
}
// (plain * and + under the pragma: the __fmul_rn / __fadd_rn of the HIP headers are inlined functions compiled with contraction on,
// and the compiler fuses across them whatever the caller says)
__device__ __forceinline__ float rot_row(const float* C, int r, const float* x) {
#pragma clang fp contract(off)
  return ((C[3 * r] * x[0]) + (C[3 * r + 1] * x[1])) + (C[3 * r + 2] * x[2]);
}
__device__ __forceinline__ bool finite3(const float* x) { return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]); }
// one pair: X, Y, r; true iff it counts
__device__ __forceinline__ bool graph_pair(const float* __restrict__ xw, int64_t pa, int64_t pb, const Corr& Tj, const Corr& Ti, float gate2,
                                           float* X, float* Y, float* r) {
#pragma clang fp contract(off)
  const float xa[3] = {xw[3 * pa], xw[3 * pa + 1], xw[3 * pa + 2]}, xb[3] = {xw[3 * pb], xw[3 * pb + 1], xw[3 * pb + 2]};
#pragma unroll
  for (int m = 0; m < 3; m++) {
    X[m] = rot_row(Tj.C, m, xa) + Tj.c[m];
    Y[m] = rot_row(Ti.C, m, xb) + Ti.c[m];
    r[m] = X[m] - Y[m];
  }
  const float s = ((r[0] * r[0]) + (r[1] * r[1])) + (r[2] * r[2]);
  return finite3(xa) && finite3(xb) && s < gate2;
}

// ---------------------------------------------------------------------------------------------- G2
__global__ __launch_bounds__(kThreads) void graph_round_kernel(const GraphEdgeDev* __restrict__ edges, const int* __restrict__ a,
                                                              const int* __restrict__ b, KeyframeStore S, const float* __restrict__ corr,
                                                              float gate2, double* __restrict__ raw) {
  __shared__ double part[kThreads / 64][kSums];
  const GraphEdgeDev E = edges[blockIdx.x];
  const Corr Tj = load_corr(corr, E.j), Ti = load_corr(corr, E.i);
  const int64_t oj = S.off[E.j], oi = S.off[E.i];
  double acc[kSums];
#pragma unroll
  for (int m = 0; m < kSums; m++) acc[m] = 0.0;
  for (int k = threadIdx.x; k < E.count; k += kThreads) {         // a thread's pairs in pair order
    float Xf[3], Yf[3], rf[3];
    if (!graph_pair(S.xw, oj + a[E.off + k], oi + b[E.off + k], Tj, Ti, gate2, Xf, Yf, rf)) continue;
    const double X[3] = {Xf[0], Xf[1], Xf[2]}, Y[3] = {Yf[0], Yf[1], Yf[2]}, r[3] = {rf[0], rf[1], rf[2]};
    double term[kSums];
    term[0] = 1.0;
    term[1] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const int u = (m + 1) % 3, v = (m + 2) % 3;
      term[2 + m] = r[m];
      term[5 + m] = r[u] * X[v] - r[v] * X[u];       // (r x X)[m]
      term[8 + m] = Y[u] * r[v] - Y[v] * r[u];       // (Y x r)[m]
      term[11 + m] = X[m];
      term[14 + m] = Y[m];
#pragma unroll
      for (int n = 0; n < 3; n++) term[29 + 3 * m + n] = X[m] * Y[n];
    }
    term[17] = X[0] * X[0]; term[18] = X[0] * X[1]; term[19] = X[0] * X[2]; term[20] = X[1] * X[1]; term[21] = X[1] * X[2]; term[22] = X[2] * X[2];
    term[23] = Y[0] * Y[0]; term[24] = Y[0] * Y[1]; term[25] = Y[0] * Y[2]; term[26] = Y[1] * Y[1]; term[27] = Y[1] * Y[2]; term[28] = Y[2] * Y[2];
#pragma unroll
    for (int m = 0; m < kSums; m++) acc[m] += term[m];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < kSums; m++) {
    double v = acc[m];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if (lane == 0) part[wave][m] = v;
  }
  __syncthreads();
  if (threadIdx.x < kGraphRaw) {
    double v = 0.0;
    if (threadIdx.x < kSums) v = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    raw[(int64_t)blockIdx.x * kGraphRaw + threadIdx.x] = v;
  }
}

// ---------------------------------------------------------------------------------------------- G3
__global__ __launch_bounds__(kThreads) void graph_rows_kernel(const GraphEdgeDev* __restrict__ edges, const int* __restrict__ a,
                                                             const int* __restrict__ b, KeyframeStore S, const float* __restrict__ corr,
                                                             float gate2, float* __restrict__ rows) {
  const GraphEdgeDev E = edges[blockIdx.x];
  const Corr Tj = load_corr(corr, E.j), Ti = load_corr(corr, E.i);
  const int64_t oj = S.off[E.j], oi = S.off[E.i];
  const float nan = __int_as_float(0x7fc00000);
  for (int k = threadIdx.x; k < E.count; k += kThreads) {
    float X[3], Y[3], r[3];
    const bool ok = graph_pair(S.xw, oj + a[E.off + k], oi + b[E.off + k], Tj, Ti, gate2, X, Y, r);
    const int64_t o = 3 * ((int64_t)E.out + k);
#pragma unroll
    for (int m = 0; m < 3; m++) rows[o + m] = ok ? r[m] : nan;
  }
}

// ---------------------------------------------------------------------------------------------- G4
__global__ __launch_bounds__(kThreads) void graph_apply_kernel(KeyframeStore S, int K, int used, const float* __restrict__ corr) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= used) return;
  int lo = 0, hi = K;                              // the keyframe that owns keypoint p: the last k with off[k] <= p (empty ones are skipped)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (S.off[mid] <= p) lo = mid; else hi = mid; }
  const Corr T = load_corr(corr, lo);
  const float x[3] = {S.xw[3 * (int64_t)p], S.xw[3 * (int64_t)p + 1], S.xw[3 * (int64_t)p + 2]};
  const float n[3] = {S.nw[3 * (int64_t)p], S.nw[3 * (int64_t)p + 1], S.nw[3 * (int64_t)p + 2]};
#pragma unroll
  for (int m = 0; m < 3; m++) {
    S.xw[3 * (int64_t)p + m] = rot_row(T.C, m, x) + T.c[m];
    S.nw[3 * (int64_t)p + m] = rot_row(T.C, m, n);
  }
}

}  // namespace

hipError_t launch_graph_pack(const int* d1, const int* idx, const int* d2, int na, int segs, const int* off, const KeyframeAccept& acc,
                             const int* counts, const GraphBases& base, int* a, int* b, hipStream_t s) {
  if (na <= 0 || segs <= 0) return hipSuccess;
  if (na > kMaxKeypoints) return hipErrorInvalidValue;
  hipLaunchKernelGGL(graph_pack_kernel, dim3(segs), dim3(kThreads), 0, s, d1, idx, d2, na, off, acc, counts, base, a, b);
  return hipGetLastError();
}

hipError_t launch_graph_round(const GraphEdgeDev* edges, int n_edges, const int* a, const int* b, const KeyframeStore& S, const float* corr,
                              float gate2, double* raw, hipStream_t s) {
  if (n_edges <= 0) return hipSuccess;
  hipLaunchKernelGGL(graph_round_kernel, dim3(n_edges), dim3(kThreads), 0, s, edges, a, b, S, corr, gate2, raw);
  return hipGetLastError();
}

hipError_t launch_graph_rows(const GraphEdgeDev* edges, int n_edges, const int* a, const int* b, const KeyframeStore& S, const float* corr,
                             float gate2, float* rows, hipStream_t s) {
  if (n_edges <= 0) return hipSuccess;
  hipLaunchKernelGGL(graph_rows_kernel, dim3(n_edges), dim3(kThreads), 0, s, edges, a, b, S, corr, gate2, rows);
  return hipGetLastError();
}

hipError_t launch_graph_apply(const KeyframeStore& S, int K, int used, const float* corr, hipStream_t s) {
  if (K <= 0 || used <= 0) return hipSuccess;
  hipLaunchKernelGGL(graph_apply_kernel, dim3((used + kThreads - 1) / kThreads), dim3(kThreads), 0, s, S, K, used, corr);
  return hipGetLastError();
}

RPE_PRELOAD(graph_round_kernel);

}  // namespace rpe
