// gfx950 kernels of the COLOUR half of the TSDF volume: a registered RGB image is fused beside the depth, and the fused colour is
// sampled back at world points (the model's vertices, the mesh's vertices).
//
//   C1  frame_color_kernel              the 3-byte staging upload of one frame into its RGBA8 map (A = 255), RGB or BGR order.
//   C2  volume_integrate_color_kernel   V1 (rpe_volume.hip) plus the colour: the tsdf half is V1's code (voxel_project / fuse and
//                                       the {tsdf, w} pairs of rpe_volume_field.hpp) and touches the same voxels with the same bits; a voxel that V1 updates
//                                       and that lies inside the truncation band (sdf <= tr) also blends the frame colour of its pixel
//                                       into its four binary16 {r, g, b, wc}, unless that pixel has A = 0 (no colour).  A lane owns 4 voxels: two 16-byte {tsdf, w} pairs and two
//                                       16-byte colour pairs, each loaded and stored only where one of its voxels is updated, plus one
//                                       4-byte frame-colour gather per band voxel.
//   C3  color_sample_kernel             RGBA8 of the colour field C at N world points (stride 3 floats), one lane per point, eight 8-byte
//                                       corner gathers.  Serves the model colour map and the mesh colours.
//
// The conventions (include/rgbd_pose_hip.h Part 3, "Colour") are followed BIT-EXACTLY: fp32, the written order, no FMA contraction;
// tests/color_oracle.py is their numpy statement.
#include "rpe_assoc.h"
#include "rpe_volume_field.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kVolBlock = 256;    // C2: 4 voxels per lane, as V1
constexpr int kColorBlock = 256;  // C1, C3: one pixel / point per lane

// binary16 <-> fp32 (h2f, f2h) and the colour update of one voxel (blend): rpe_volume_field.hpp, shared with rpe_rebuild.hip.

// ---------------------------------------------------------------------------------------------- C1
__global__ __launch_bounds__(kColorBlock) void frame_color_kernel(const unsigned char* __restrict__ rgb, int64_t n, int bgr,
                                                                  unsigned int* __restrict__ rgba) {
  const int64_t i = (int64_t)blockIdx.x * kColorBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned a = rgb[3 * i], g = rgb[3 * i + 1], c = rgb[3 * i + 2];
  const unsigned r = bgr ? c : a, b = bgr ? a : c;
  rgba[i] = r | g << 8 | b << 16 | 0xff000000u;
}

// ---------------------------------------------------------------------------------------------- C2
// A voxel's colour update: blend (rpe_volume_field.hpp).
// nvox <= 2^30 (dims <= 1024): the flat voxel index fits 32 bits, byte offsets do not
__global__ __launch_bounds__(kVolBlock) void volume_integrate_color_kernel(float* __restrict__ vol, unsigned short* __restrict__ cvol,
                                                                           VolumeGeometry G, int64_t nvox, const float* __restrict__ vmap,
                                                                           const unsigned int* __restrict__ rgba, Camera cam, PoseF T) {
  const int64_t first = ((int64_t)blockIdx.x * kVolBlock + threadIdx.x) * 4;
  if (first >= nvox) return;
  const unsigned flat = (unsigned)first, d0 = (unsigned)G.dim[0], d1 = (unsigned)G.dim[1];
  int i = (int)(flat % d0), j = (int)((flat / d0) % d1), k = (int)(flat / d0 / d1);
  float f[4], sdf[4];
  int64_t pix[4];
  bool up[4], band[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    f[q] = 0.0f; sdf[q] = 0.0f; pix[q] = 0;
    up[q] = first + q < nvox && voxel_project(G, vmap, cam, T, i, j, k, f[q], sdf[q], pix[q]);
    band[q] = up[q] && sdf[q] <= G.tr;
    if (++i == G.dim[0]) { i = 0; if (++j == G.dim[1]) { j = 0; ++k; } }
  }
  // the lane's two {tsdf, w} pairs and two colour pairs: a pair is loaded if either of its voxels is updated (colour: in the band)
  float4 v[2];
  uint4 c[2];
  unsigned o[4];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int64_t a = first + 2 * p;
    v[p] = load_pair(vol, a, nvox, up[2 * p] || up[2 * p + 1]);
    c[p] = make_uint4(0u, 0u, 0u, 0u);
    if (band[2 * p] || band[2 * p + 1]) {
      if (a + 1 < nvox) c[p] = *reinterpret_cast<const uint4*>(cvol + 4 * a);
      else { const uint2 h = *reinterpret_cast<const uint2*>(cvol + 4 * a); c[p].x = h.x; c[p].y = h.y; }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) o[q] = band[q] ? rgba[pix[q]] : 0u;
  // A = 0: the pixel has no colour (rpe_frame_register_color), so the voxel gets no colour update and no colour store
#pragma unroll
  for (int q = 0; q < 4; q++) band[q] = band[q] && (o[q] >> 24) != 0u;
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const bool lo = up[2 * p], hi = up[2 * p + 1];
    if (lo) fuse(v[p].x, v[p].y, f[2 * p], G.W);
    if (hi) fuse(v[p].z, v[p].w, f[2 * p + 1], G.W);
    store_pair(vol, first + 2 * p, v[p], lo, hi);
  }
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const bool lo = band[2 * p], hi = band[2 * p + 1];
    if (!lo && !hi) continue;
    unsigned short* q = cvol + 4 * (first + 2 * p);
    if (lo) blend(c[p].x, c[p].y, o[2 * p], G.W);
    if (hi) blend(c[p].z, c[p].w, o[2 * p + 1], G.W);
    if (lo && hi) *reinterpret_cast<uint4*>(q) = c[p];
    else if (lo) *reinterpret_cast<uint2*>(q) = make_uint2(c[p].x, c[p].y);
    else *reinterpret_cast<uint2*>(q + 4) = make_uint2(c[p].z, c[p].w);
  }
}

// ---------------------------------------------------------------------------------------------- C3
// C(p): F's cell (g, i0, a and the in-range rule: cell); known iff in range and all eight corner colour weights are > 0; each channel
// with F's lerp chain (trilerp) on (float) of the binary16 values.  q(x) = (uint8)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f)
// (quantise).  All three, and the chain from the eight corners to the byte quadruple (colour_rgba): rpe_volume_field.hpp, shared with the
// map mesh of rpe_mapmesh.hip and the map raycast of rpe_frontend.hip.
__global__ __launch_bounds__(kColorBlock) void color_sample_kernel(const unsigned short* __restrict__ cvol, VolumeGeometry G,
                                                                   const float* __restrict__ pts, int64_t n,
                                                                   unsigned int* __restrict__ rgba) {
  const int64_t e = (int64_t)blockIdx.x * kColorBlock + threadIdx.x;
  if (e >= n) return;
  const float px = pts[3 * e], py = pts[3 * e + 1], pz = pts[3 * e + 2];
  unsigned out = 0u;
  int i0[3];
  float a[3];
  if (cell(G, px, py, pz, i0, a)) {
    const int64_t sy = 4 * (int64_t)G.dim[0], sz = sy * G.dim[1];
    const unsigned short* b = cvol + (int64_t)i0[2] * sz + (int64_t)i0[1] * sy + 4 * (int64_t)i0[0];
    uint2 v[8];   // corner n = di + 2 dj + 4 dk
#pragma unroll
    for (int m = 0; m < 8; m++) v[m] = *reinterpret_cast<const uint2*>(b + ((m & 4) ? sz : 0) + ((m & 2) ? sy : 0) + ((m & 1) ? 4 : 0));
    out = colour_rgba(v, a);
  }
  rgba[e] = out;
}

}  // namespace

hipError_t launch_frame_color(const unsigned char* rgb, int64_t n, int bgr, unsigned int* rgba, hipStream_t s) {
  const int64_t blocks = (n + kColorBlock - 1) / kColorBlock;
  hipLaunchKernelGGL(frame_color_kernel, dim3((unsigned)blocks), dim3(kColorBlock), 0, s, rgb, n, bgr, rgba);
  return hipGetLastError();
}

hipError_t launch_volume_integrate_color(float* vol, unsigned short* cvol, const VolumeGeometry& G, const float* vmap,
                                         const unsigned int* rgba, const Camera& cam, const PoseF& T, hipStream_t s) {
  const int64_t nvox = (int64_t)G.dim[0] * G.dim[1] * G.dim[2];
  const int64_t blocks = (nvox + 4 * kVolBlock - 1) / (4 * kVolBlock);
  hipLaunchKernelGGL(volume_integrate_color_kernel, dim3((unsigned)blocks), dim3(kVolBlock), 0, s, vol, cvol, G, nvox, vmap, rgba, cam, T);
  return hipGetLastError();
}

hipError_t launch_color_sample(const unsigned short* cvol, const VolumeGeometry& G, const float* pts, int64_t n, unsigned int* rgba,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kColorBlock - 1) / kColorBlock;
  hipLaunchKernelGGL(color_sample_kernel, dim3((unsigned)blocks), dim3(kColorBlock), 0, s, cvol, G, pts, n, rgba);
  return hipGetLastError();
}

RPE_PRELOAD(volume_integrate_color_kernel);

}  // namespace rpe
