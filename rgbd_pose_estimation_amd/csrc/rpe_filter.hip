// gfx950 kernel of the DEPTH FILTER, the optional first stage of the front end (include/rgbd_pose_hip.h Part 3, "Depth filter"):
//
//   F0  depth_filter_kernel   raw depth -> bilateral-filtered metric depth of level 0, which F1 / F1p (rpe_frontend.hip) then read as
//                             RPE_DEPTH_F32 with scale 1.  Spatial weights: a host-made Gaussian table; range weight: the biweight
//                             (1 - x)^2 of x = ((d - c) / cut)^2, cut = a + b c^2 growing with the square of the range as a depth
//                             sensor's noise does.  A polynomial on purpose: exact in fp32, no exp on the device.
//
// A workgroup owns a 32 x 32 tile of level 0 plus a halo of r pixels, converted and range-gated once on the way into LDS (metric fp32,
// NaN = invalid or outside the image), so that every tap is an LDS read and needs no bounds test.  Thread t owns 4 consecutive pixels
// of tile row t / 8 (16-byte stores where the row allows, as depth_pyramid_kernel); per window row it slides a 4-value register
// window over the LDS row: one ds_read_b32 per tap column for the 4 pixels.  LDS row stride 41 dwords: the 32 lanes of a ds_read_b32
// group are 4 tile rows of 8 lanes, 4 dwords apart within a row, and 41 = 1 (mod 4) puts the rows on the four residues: no bank
// conflict.  The window loops are rolled and their bounds wave-uniform: one kernel for every radius; the spatial table is a kernel
// argument, so its reads are scalar loads.  At 640 x 480 the grid is 300 workgroups of 6.4 KiB LDS: more than one per CU, launch bound.
//
// The arithmetic is the header's, fp32 in the written order with FMA contraction off; tests/filter_oracle.py states it in numpy and
// the results are its bits.  The unit is its own so that rpe_frontend.hip compiles to what it was.
#include "rpe_kernels.h"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kFilterBlock = 256;
constexpr int kFilterTile = 32;                                       // tile side; thread t: row t / 8, columns 4 (t % 8) .. +3
constexpr int kFilterSpan = kFilterTile + 2 * kFilterMaxRadius;       // tile plus halo at the largest radius
constexpr int kFilterStride = kFilterSpan + 1;                        // 41: see above
static_assert(kFilterStride % 4 == 1, "LDS row stride must be 1 (mod 4) for conflict-free ds_read_b32");
static_assert(kFilterBlock * 4 == kFilterTile * kFilterTile, "4 pixels per thread");

template <class D>
__global__ __launch_bounds__(kFilterBlock) void depth_filter_kernel(const D* __restrict__ raw, int w, int h, float scale, float dmin,
                                                                    float dmax, FilterParams P, float* __restrict__ out) {
  __shared__ float tile[kFilterSpan * kFilterStride];
  const int r = P.radius;
  const int tiles_x = (w + kFilterTile - 1) / kFilterTile;
  const int u0 = (blockIdx.x % tiles_x) * kFilterTile, v0 = (blockIdx.x / tiles_x) * kFilterTile;
  const float nan = qnan();
  // tile and halo, (32 + 2r)^2 pixels: metric depth, NaN outside (dmin, dmax) and outside the image
  const int span = kFilterTile + 2 * r;
  for (int i = threadIdx.x; i < span * span; i += kFilterBlock) {
    const int y = i / span, x = i - y * span;
    const int v = v0 - r + y, u = u0 - r + x;
    float z = nan;
    if (u >= 0 && u < w && v >= 0 && v < h) {
      const float d = (float)raw[(int64_t)v * w + u] * scale;
      z = d > dmin && d < dmax ? d : nan;
    }
    tile[y * kFilterStride + x] = z;
  }
  __syncthreads();
  const int row = threadIdx.x / 8, col = 4 * (threadIdx.x % 8);
  const int v = v0 + row, u = u0 + col;
  if (v >= h || u >= w) return;
  const float* centre = tile + (row + r) * kFilterStride + col + r;
  float c[4], inv[4], num[4], den[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    c[k] = centre[k];
    const float cut = P.a + P.b * (c[k] * c[k]);
    inv[k] = 1.0f / cut;
    num[k] = 0.0f; den[k] = 0.0f;
  }
  const int win = 2 * r + 1;
#pragma unroll 1
  for (int j = 0; j < win; j++) {                  // dy = j - r
    const float* line = tile + (row + j) * kFilterStride + col;
    float d[4];
    d[0] = line[0]; d[1] = line[1]; d[2] = line[2];
#pragma unroll 1
    for (int i = 0; i < win; i++) {                // dx = i - r: pixel k reads column col + k + i
      d[3] = line[i + 3];
      const float ws = P.ws[j * win + i];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float t = (d[k] - c[k]) * inv[k];
        const float x = t * t;
        const bool keep = x < 1.0f;                // false for a NaN neighbour and for a NaN centre
        const float wr = (1.0f - x) * (1.0f - x);
        const float wgt = ws * wr;
        const float n1 = num[k] + wgt * d[k], d1 = den[k] + wgt;
        num[k] = keep ? n1 : num[k];
        den[k] = keep ? d1 : den[k];
      }
      d[0] = d[1]; d[1] = d[2]; d[2] = d[3];
    }
  }
  float z[4];
#pragma unroll
  for (int k = 0; k < 4; k++) z[k] = c[k] == c[k] ? num[k] / den[k] : nan;
  float* o = out + (int64_t)v * w + u;
  if ((w & 3) == 0 && u + 3 < w) *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
  else for (int k = 0; k < 4; k++) if (u + k < w) o[k] = z[k];
}

}  // namespace

hipError_t launch_depth_filter(const void* d_depth, int depth_type, int width, int height, float scale, float dmin, float dmax,
                               const FilterParams& P, float* out, hipStream_t s) {
  if (width < 1 || height < 1) return hipSuccess;
  if (P.radius < 1 || P.radius > kFilterMaxRadius) return hipErrorInvalidValue;
  const int tiles = ((width + kFilterTile - 1) / kFilterTile) * ((height + kFilterTile - 1) / kFilterTile);
  if (depth_type == 0)
    hipLaunchKernelGGL(depth_filter_kernel<unsigned short>, dim3(tiles), dim3(kFilterBlock), 0, s, (const unsigned short*)d_depth, width,
                       height, scale, dmin, dmax, P, out);
  else
    hipLaunchKernelGGL(depth_filter_kernel<float>, dim3(tiles), dim3(kFilterBlock), 0, s, (const float*)d_depth, width, height, scale,
                       dmin, dmax, P, out);
  return hipGetLastError();
}

RPE_PRELOAD(depth_filter_kernel<float>);

}  // namespace rpe
