// The tables of the ORIENTED descriptor that its two kernels share (D6o in rpe_feature_oriented.hip, D6os in rpe_feature_scale.hip):
// the cosines of the 32 angle bins and the offsets of the moment disc, as include/rgbd_pose_hip.h Part 3 ("Oriented descriptor") states
// them.  Each unit that includes this holds its own copy (internal linkage).
#pragma once
#include <hip/hip_runtime.h>

namespace rpe {

namespace {

constexpr int kAngleBins = 32, kDiscRadius = 13, kDiscPixels = 529;

// round(1024 cos(2 pi k / 32)) as the header states them; the sine is the cosine a quarter turn back: S[k] = C[(k + 24) % 32]
__constant__ int kAngleCos[kAngleBins] = {1024, 1004, 946, 851, 724, 569, 392, 200, 0, -200, -392, -569, -724, -851, -946, -1004,
                                          -1024, -1004, -946, -851, -724, -569, -392, -200, 0, 200, 392, 569, 724, 851, 946, 1004};

// the offsets of the disc dx^2 + dy^2 <= 169 in row order, listed by the compiler
struct Disc {
  signed char d[kDiscPixels][2] = {};
  int count = 0;
  constexpr Disc() {
    for (int dy = -kDiscRadius; dy <= kDiscRadius; dy++)
      for (int dx = -kDiscRadius; dx <= kDiscRadius; dx++)
        if (dx * dx + dy * dy <= kDiscRadius * kDiscRadius) {
          if (count < kDiscPixels) { d[count][0] = (signed char)dx; d[count][1] = (signed char)dy; }
          count++;
        }
  }
};
constexpr Disc kDiscHost{};
static_assert(kDiscHost.count == kDiscPixels, "the disc of radius 13 has 529 pixels");
__device__ const Disc kDisc = kDiscHost;

}  // namespace

}  // namespace rpe
