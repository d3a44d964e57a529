// gfx950 kernel of the FEATURE stage's ORIENTED descriptor (RPE_DESC_ORIENTED), the sibling of D6 in rpe_feature.hip:
//
//   D6o feat_describe_oriented_kernel   one wave per keypoint.  The 64 lanes stride over the 529 pixels of the disc of radius 13 and sum
//                                       dx Y and dy Y of the luma (D1's expression on the RGBA image); the two moments are reduced
//                                       across the wave; lanes 0-31 each score one of the 32 angle bins, m10 C[k] + m01 S[k] in int64,
//                                       and a wave argmax picks the bin (the lowest k on a tie); then D6's four tests per lane on
//                                       offsets turned by the bin, a sample outside the image reading 0, four ballots, eight word
//                                       stores, and the bin.
//
// The conventions (include/rgbd_pose_hip.h Part 3, "Oriented descriptor") are integer arithmetic and comparisons throughout;
// tests/oriented_oracle.py is their numpy statement and the results are its bits.  No floating point, no atomics; the sums are integer
// sums, so the order of the reduction does not matter.  The unit is its own so that rpe_feature.hip, and the upright D6 in it, compile
// to what they were.
#include "rpe_assoc.h"
#include "rpe_feature_rules.hpp"   // luma; the tables (rpe_brief_table.h, rpe_feature_disc.h: the angle table and the disc, shared with D6os)

namespace rpe {

namespace {

__global__ __launch_bounds__(256) void feat_describe_oriented_kernel(const unsigned int* __restrict__ rgba,
                                                                    const unsigned short* __restrict__ box, int w, int h,
                                                                    const int* __restrict__ ctl, const int* __restrict__ kp_pix,
                                                                    int* __restrict__ kp_xy, unsigned int* __restrict__ kp_desc,
                                                                    int* __restrict__ kp_bin) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= ctl[kFeatCtlCount]) return;
  const int p = kp_pix[k];
  const int u = p % w, v = p / w;
  // moments, angle bin, steered tests and word store: stated here and in rpe_feature_scale.hip (see rpe_feature_rules.hpp)
  // the moments: a keypoint lies 16 px inside the image, the whole disc with it
  int m10 = 0, m01 = 0;
  for (int i = lane; i < kDiscPixels; i += 64) {
    const int dx = kDisc.d[i][0], dy = kDisc.d[i][1];
    const unsigned px = rgba[p + dy * w + dx];
    const int y = (px >> 24) != 0 ? (int)luma(px) : 0;
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
  unsigned long long m[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const signed char* q = kBriefPairs[j * 64 + lane];
    // >> on a negative int is the arithmetic shift: floor
    const int ax = u + ((q[0] * c - q[1] * s + 512) >> 10), ay = v + ((q[0] * s + q[1] * c + 512) >> 10);
    const int bx = u + ((q[2] * c - q[3] * s + 512) >> 10), by = v + ((q[2] * s + q[3] * c + 512) >> 10);
    const bool aok = ax >= 0 && ax < w && ay >= 0 && ay < h, bok = bx >= 0 && bx < w && by >= 0 && by < h;
    const int a = aok ? box[ay * w + ax] : 0, b = bok ? box[by * w + bx] : 0;
    m[j] = __ballot(a < b);
  }
  if (lane < 8) {
    const int j = lane >> 1;
    const unsigned long long mj = j == 0 ? m[0] : j == 1 ? m[1] : j == 2 ? m[2] : m[3];
    kp_desc[8 * k + lane] = (unsigned int)(mj >> (32 * (lane & 1)));
  }
  if (lane == 8) { kp_xy[2 * k] = u; kp_xy[2 * k + 1] = v; }
  if (lane == 9) kp_bin[k] = bin;
}

}  // namespace

hipError_t launch_feature_describe_oriented(const unsigned int* rgba, const unsigned short* box, int w, int h, int max_keypoints,
                                            const int* ctl, const int* kp_pix, int* kp_xy, unsigned int* kp_desc, int* kp_bin,
                                            hipStream_t s) {
  hipLaunchKernelGGL(feat_describe_oriented_kernel, dim3((max_keypoints + 3) / 4), dim3(256), 0, s, rgba, box, w, h, ctl, kp_pix, kp_xy,
                     kp_desc, kp_bin);
  return hipGetLastError();
}

RPE_PRELOAD(feat_describe_oriented_kernel);

}  // namespace rpe
