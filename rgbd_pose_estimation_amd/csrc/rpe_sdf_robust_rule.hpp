// THE ROBUST WEIGHT OF A VOLUME-TERM ROW (include/rgbd_pose_hip.h Part 3, "Robust volume terms"; tests/sdf_robust_oracle.py is its numpy
// statement): the IRLS weight w of a row with residual r and scale k, stated once for the four round kernels of rpe_sdf_robust.hpp and
// their weight-plane hook.  r and k are in metres for the geometric row, in unscaled intensity levels (before lam) for the photometric
// one.  Followed BIT-EXACTLY like the rules it sits beside: fp32, the written order, no FMA contraction (rpe_volume_field.hpp switches it
// off to the end of the including unit).  A weighted row contributes w J J^T to H, w J r to g and w r^2 to the cost of its term; the row
// count counts every row that passed the gates, weight 0 included.
#pragma once
#include "rpe_volume_field.hpp"

namespace rpe {
namespace {

// (the kinds kRobustHuber / kRobustTukey: rpe_kernels.h)
// Huber: 1 inside the scale, k / |r| beyond it
__device__ __forceinline__ float huber_weight(float r, float k) {
  const float s = fabsf(r);
  return s <= k ? 1.0f : k / s;
}
// Tukey's biweight: (1 - (r / k)^2)^2 inside the scale, exactly 0 from |r| = k on
__device__ __forceinline__ float tukey_weight(float r, float k) {
  const float u = r / k;
  const float q = 1.0f - u * u;
  return fabsf(r) < k ? q * q : 0.0f;
}
// the kind as a template argument (the round kernels: it costs no scalar register) ...
template <int KIND>
__device__ __forceinline__ float robust_weight(float r, float k) {
  static_assert(KIND == kRobustHuber || KIND == kRobustTukey, "a robust kind of the volume terms");
  return KIND == kRobustHuber ? huber_weight(r, k) : tukey_weight(r, k);
}
// ... and as a value (the hook; kind NONE: every row has weight 1)
__device__ __forceinline__ float robust_weight(int kind, float r, float k) {
  return kind == kRobustHuber ? huber_weight(r, k) : kind == kRobustTukey ? tukey_weight(r, k) : 1.0f;
}
// the photometric row's: photo_k = 0 leaves it at weight 1
template <int KIND>
__device__ __forceinline__ float robust_photo_weight(float r, float photo_k) {
  return photo_k > 0.0f ? robust_weight<KIND>(r, photo_k) : 1.0f;
}

}  // namespace
}  // namespace rpe
