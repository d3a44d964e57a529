// gfx950 kernels of the FRONT END: the step before the hot path.  They turn a 640x480
// depth frame into the correspondence arrays the solvers consume -- points_c / normal_c / bearingVectors of the current
// frame, points_g / normal_g of the model -- so that those arrays are BORN in HBM (no 3 x N host matrices, no upload).
//
//   F1  frame_maps_kernel       depth image -> vertex map (pinhole back-projection, the camera of Simulator.hpp:150-162:
//                               u - cx = f X / Z), unit bearing vectors (the conversion of Simulator.hpp:215-222) and a
//                               normal map (central differences of the vertex map, oriented towards the camera)
//   F2  to_world_kernel         frame maps -> world maps under a pose (Xw = R^T (Xc - t)): the model of the next frame
//   F1p depth_pyramid_kernel + pyramid_maps_kernel: metric depth of every pyramid level (LDS tiles), then F1's arithmetic on
//                               every level (workgroups partitioned by level)
//   F2p model_pyramid_kernel    model maps of levels 1 .. L-1 from level 0 (KinectFusion resize); F2 on all levels at once = one
//                               to_world_kernel launch over the concatenated levels
//   F3  associate_kernel        projective data association of the frame against the model under a pose guess, with a
//                               distance and a normal-angle gate; writes XW XC BV NW NC aligned per pixel
//   R0  map_occupancy_kernel + R1 map_raycast_kernel: the model maps raycast from the MAP -- the window plus the archived bricks -- through
//                               a grid of bricks (include/rgbd_pose_hip.h Part 3, "Map raycast"; host side in rpe_mapmesh_api.hip).  They
//                               build model maps, as F2 / F2p do, contraction is off here as they need it, and every other volume unit
//                               pins its exact set of kernels in the gate table of tests/unit_gates.py: that is why they live in this
//                               unit.  A unit of their own comes with a gate entry of its own (0 spills, 0 scratch, no LDS; <= 128 and
//                               <= 64 registers, which tests/test_mapray_oracle.py holds them to meanwhile).
//
// The reference has no such stage (its arrays come from Simulator.hpp or from the caller), so there is no reference text
// to follow: parity is against the numpy statement of the same arithmetic that the tests hold, BIT-EXACT -- every expression below is
// evaluated in fp32 in the written order with FMA contraction off, and the numpy statement performs the same IEEE operations.
// All three kernels are image-parallel and HBM/L2 streaming: one thread owns 4 consecutive pixels so that every
// xyz-interleaved map is read and written as three 16-byte accesses per lane, like the solver kernels read them.
#include "rpe_assoc.h"
#include "rpe_volume_field.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kFeBlock = 256;

template <class D> __device__ __forceinline__ float depth_at(const D* __restrict__ d, int idx,
    float scale) { return (float)d[idx] * scale; }

struct Vtx { float x, y, z; bool ok; };

template <class D>
__device__ __forceinline__ Vtx vertex_at(const D* __restrict__ depth, const Camera& cam, int u, int v, float scale, float dmin,
    float dmax) {
  Vtx r;
  const float z = depth_at(depth, v * cam.width + u, scale);
  r.ok = z > dmin && z < dmax;  // false for NaN
  const float xn = ((float)u - cam.cx) / cam.fx, yn = ((float)v - cam.cy) / cam.fy;
  r.x = xn * z; r.y = yn * z; r.z = z;
  return r;
}

__device__ __forceinline__ void store4(float* __restrict__ out, int64_t g, int64_t n, const float (&v)[12]) {
  if ((g + 1) * 4 <= n) {
    float4* q = reinterpret_cast<float4*>(out) + 3 * g;
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
    q[2] = make_float4(v[8], v[9], v[10], v[11]);
  } else {
    for (int i = 0; i < 12; i++) { const int64_t idx = g * 12 + i; if (idx < 3 * n) out[idx] = v[i]; }
  }
}
__device__ __forceinline__ void load4(const float* __restrict__ in, int64_t g, int64_t n, float (&v)[12]) {
  if ((g + 1) * 4 <= n) {
    const float4* q = reinterpret_cast<const float4*>(in) + 3 * g;
    const float4 a = q[0], b = q[1], c = q[2];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
  } else {
    for (int i = 0; i < 12; i++) { const int64_t idx = g * 12 + i; v[i] = idx < 3 * n ? in[idx] : qnan(); }
  }
}

// ---------------------------------------------------------------------------------------------- F1
// the maps of pixel group g (4 consecutive pixels) of one image: shared by F1 (raw depth, the caller's scale) and F1p (metric depth
// of one pyramid level, scale 1) so that every level is built by the same operations
template <class D>
__device__ __forceinline__ void frame_maps_group(const D* __restrict__ depth, const Camera& cam, float scale, float dmin, float dmax,
                                                 float max_jump, int64_t g, float* __restrict__ vmap, float* __restrict__ nmap,
                                                 float* __restrict__ bmap) {
  const int64_t n = (int64_t)cam.width * cam.height;
  float V[12], N[12], B[12];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t i = g * 4 + k;
    float vx = qnan(), vy = qnan(), vz = qnan(), nx = qnan(), ny = qnan(), nz = qnan(), bx = qnan(), by = qnan(), bz = qnan();
    if (i < n) {
      const int u = (int)(i % cam.width), v = (int)(i / cam.width);
      const float xn = ((float)u - cam.cx) / cam.fx, yn = ((float)v - cam.cy) / cam.fy;
      const float s = sqrtf(xn * xn + yn * yn + 1.0f);
      bx = xn / s; by = yn / s; bz = 1.0f / s;
      const Vtx c = vertex_at(depth, cam, u, v, scale, dmin, dmax);
      if (c.ok) {
        vx = c.x; vy = c.y; vz = c.z;
        if (u > 0 && u < cam.width - 1 && v > 0 && v < cam.height - 1) {
          const Vtx l = vertex_at(depth, cam, u - 1, v, scale, dmin, dmax), r = vertex_at(depth, cam, u + 1, v, scale, dmin, dmax);
          const Vtx t = vertex_at(depth, cam, u, v - 1, scale, dmin, dmax), b = vertex_at(depth, cam, u, v + 1, scale, dmin, dmax);
          const bool smooth = l.ok && r.ok && t.ok && b.ok && fabsf(l.z - c.z) <= max_jump && fabsf(r.z - c.z) <= max_jump &&
                              fabsf(t.z - c.z) <= max_jump && fabsf(b.z - c.z) <= max_jump;
          if (smooth) {
            const float ax = r.x - l.x, ay = r.y - l.y, az = r.z - l.z;   // d/du
            const float ex = b.x - t.x, ey = b.y - t.y, ez = b.z - t.z;   // d/dv
            float cx = ey * az - ez * ay, cy = ez * ax - ex * az, cz = ex * ay - ey * ax;  // (d/dv) x (d/du): towards the camera
            const float len = sqrtf(cx * cx + cy * cy + cz * cz);
            if (len > 0.0f) {
              cx = cx / len; cy = cy / len; cz = cz / len;
              const float facing = cx * c.x + cy * c.y + cz * c.z;
              if (facing > 0.0f) { cx = -cx; cy = -cy; cz = -cz; }
              nx = cx; ny = cy; nz = cz;
            }
          }
        }
      }
    }
    V[3 * k] = vx; V[3 * k + 1] = vy; V[3 * k + 2] = vz;
    N[3 * k] = nx; N[3 * k + 1] = ny; N[3 * k + 2] = nz;
    B[3 * k] = bx; B[3 * k + 1] = by; B[3 * k + 2] = bz;
  }
  store4(vmap, g, n, V);
  store4(nmap, g, n, N);
  store4(bmap, g, n, B);
}

template <class D>
__global__ __launch_bounds__(kFeBlock) void frame_maps_kernel(const D* __restrict__ depth, Camera cam, float scale, float dmin, float dmax,
                             float max_jump, float* __restrict__ vmap, float* __restrict__ nmap, float* __restrict__ bmap) {
  const int64_t n = (int64_t)cam.width * cam.height;
  const int64_t g = (int64_t)blockIdx.x * kFeBlock + threadIdx.x;
  if (g * 4 >= n) return;
  frame_maps_group(depth, cam, scale, dmin, dmax, max_jump, g, vmap, nmap, bmap);
}

// ---------------------------------------------------------------------------------------------- F1p
// Launch one: raw depth -> metric depth of every pyramid level.  A workgroup owns a 32 x 32 tile of level 0 (4 pixels of a row per
// lane, 16-byte stores where the row allows), keeps it in LDS and halves it in place level by level: the tile origin is a multiple
// of 2^(kMaxLevels-1), so the 2 x 2 block of every coarser pixel lies inside the tile.  Level l+1 pixel (u, v), c = level-l depth at
// (2u, 2v): NaN if c is NaN, else the mean of the block's valid depths within max_jump of c, summed in the order (2v,2u) (2v,2u+1)
// (2v+1,2u) (2v+1,2u+1).
constexpr int kPyrTile = 32;

template <class D>
__global__ __launch_bounds__(kFeBlock) void depth_pyramid_kernel(const D* __restrict__ raw, PyramidGeometry P, float scale, float dmin,
                                                                 float dmax, float max_jump, float* __restrict__ out) {
  __shared__ float tile[kPyrTile][kPyrTile + 1];
  const int w = P.cam[0].width, h = P.cam[0].height;
  const int tiles_x = (w + kPyrTile - 1) / kPyrTile;
  const int u0 = (blockIdx.x % tiles_x) * kPyrTile, v0 = (blockIdx.x / tiles_x) * kPyrTile;
  const float nan = qnan();
  {  // level 0: thread t owns row t / 8, columns 4 (t % 8) .. +3 of the tile
    const int r = threadIdx.x / 8, c = 4 * (threadIdx.x % 8);
    const int v = v0 + r, u = u0 + c;
    float z[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      z[k] = nan;
      if (v < h && u + k < w) {
        const float d = (float)raw[(int64_t)v * w + u + k] * scale;
        z[k] = d > dmin && d < dmax ? d : nan;
      }
      tile[r][c + k] = z[k];
    }
    if (v < h) {
      float* o = out + (int64_t)v * w + u;
      if ((w & 3) == 0 && u + 3 < w) *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
      else for (int k = 0; k < 4; k++) if (u + k < w) o[k] = z[k];
    }
  }
  for (int l = 1; l < P.levels; l++) {
    __syncthreads();
    const int side = kPyrTile >> l;                 // tile side at level l
    const int wl = P.cam[l].width, hl = P.cam[l].height;
    const int ul = u0 >> l, vl = v0 >> l;
    float z = nan;
    const int r = threadIdx.x / side, c = threadIdx.x % side;
    const bool mine = r < side;
    if (mine) {
      const float a = tile[2 * r][2 * c], b = tile[2 * r][2 * c + 1], e = tile[2 * r + 1][2 * c], f = tile[2 * r + 1][2 * c + 1];
      if (a == a) {   // (a NaN block centre stays NaN; NaN members fail their gate)
        const bool ka = fabsf(a - a) <= max_jump, kb = fabsf(b - a) <= max_jump, ke = fabsf(e - a) <= max_jump,
                   kf = fabsf(f - a) <= max_jump;
        const float sum = (((ka ? a : 0.0f) + (kb ? b : 0.0f)) + (ke ? e : 0.0f)) + (kf ? f : 0.0f);
        z = sum / (float)((ka ? 1 : 0) + (kb ? 1 : 0) + (ke ? 1 : 0) + (kf ? 1 : 0));
      }
    }
    __syncthreads();
    if (mine) {
      tile[r][c] = z;
      if (vl + r < hl && ul + c < wl) out[P.off[l] + (int64_t)(vl + r) * wl + ul + c] = z;
    }
  }
}

// Launch two: the maps of every level, workgroups partitioned by level (P.block0), each level exactly F1 on its metric depth
__global__ __launch_bounds__(kFeBlock) void pyramid_maps_kernel(const float* __restrict__ depth, PyramidGeometry P, float dmin, float dmax,
                                                                float max_jump, float* __restrict__ vmap, float* __restrict__ nmap,
                                                                float* __restrict__ bmap) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kMaxLevels; k++) l += (k < P.levels && (int)blockIdx.x >= P.block0[k]) ? 1 : 0;
  const Camera cam = P.cam[l];
  const int64_t n = (int64_t)cam.width * cam.height;
  const int64_t g = (int64_t)((int)blockIdx.x - P.block0[l]) * kFeBlock + threadIdx.x;
  if (g * 4 >= n) return;
  const int64_t o = P.off[l];
  frame_maps_group(depth + o, cam, 1.0f, dmin, dmax, max_jump, g, vmap + 3 * o, nmap + 3 * o, bmap + 3 * o);
}

// ---------------------------------------------------------------------------------------------- F2
__global__ __launch_bounds__(kFeBlock) void to_world_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n,
                             PoseF T, float* __restrict__ vw, float* __restrict__ nw) {
  const int64_t g = (int64_t)blockIdx.x * kFeBlock + threadIdx.x;
  if (g * 4 >= n) return;
  float V[12], N[12], OV[12], ON[12];
  load4(vmap, g, n, V);
  load4(nmap, g, n, N);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    to_world(T, V[3 * k], V[3 * k + 1], V[3 * k + 2], OV[3 * k], OV[3 * k + 1], OV[3 * k + 2]);
    rot_to_world(T, N[3 * k], N[3 * k + 1], N[3 * k + 2], ON[3 * k], ON[3 * k + 1], ON[3 * k + 2]);
  }
  store4(vw, g, n, OV);
  store4(nw, g, n, ON);
}

// ---------------------------------------------------------------------------------------------- F2p
// Model pyramid (the KinectFusion resize): level-(l+1) pixel (u, v) from the level-l block a = (2u, 2v), b = (2u+1, 2v),
// c = (2u, 2v+1), d = (2u+1, 2v+1).  Vertex: valid iff all four are (no NaN component), value (((a + b) + c) + d) * 0.25f.  Normal:
// valid iff all four are, the same sum divided by its length sqrtf((x*x + y*y) + z*z), NaN at length 0.  One launch for every
// level: a thread of level l evaluates its quad tree down to level 0 (Resize<l>), whose inner nodes are bit for bit the level-1 ..
// l-1 values other threads write.  A node is valid for the level above iff its value has no NaN component, as that level reads it
// from memory: four valid members can still give a NaN component (Inf + -Inf, Inf / Inf).
template <int LV> struct Resize {
  // the block's four members are summed in a rolled loop above level 1 (the unrolled quad tree of level 3 would hold 64 pixels live)
  static constexpr int kUnroll = LV == 1 ? 4 : 1;
  template <bool NORMAL>
  static __device__ __forceinline__ bool node(const float* __restrict__ m, int w0, int u, int v, float (&o)[3]) {
    float s[3] = {0.f, 0.f, 0.f};
    bool ok = true;
#pragma unroll kUnroll
    for (int q = 0; q < 4; q++) {
      float c[3];
      ok = Resize<LV - 1>::template node<NORMAL>(m, w0, 2 * u + (q & 1), 2 * v + (q >> 1), c) && ok;
#pragma unroll
      for (int k = 0; k < 3; k++) s[k] = q == 0 ? c[k] : s[k] + c[k];
    }
    if (!NORMAL) {
#pragma unroll
      for (int k = 0; k < 3; k++) o[k] = ok ? s[k] * 0.25f : qnan();
      return o[0] == o[0] && o[1] == o[1] && o[2] == o[2];
    }
    const float len = sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const bool good = ok && len > 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = good ? s[k] / len : qnan();
    return o[0] == o[0] && o[1] == o[1] && o[2] == o[2];
  }
};
template <> struct Resize<0> {
  template <bool NORMAL>
  static __device__ __forceinline__ bool node(const float* __restrict__ m, int w0, int u, int v, float (&o)[3]) {
    const int64_t j = 3 * ((int64_t)v * w0 + u);
    o[0] = m[j]; o[1] = m[j + 1]; o[2] = m[j + 2];
    return o[0] == o[0] && o[1] == o[1] && o[2] == o[2];
  }
};

template <int LV>
__device__ __forceinline__ void model_group(const PyramidGeometry& P, int64_t g, float* __restrict__ mv, float* __restrict__ mn) {
  const Camera cam = P.cam[LV];
  const int64_t n = (int64_t)cam.width * cam.height;
  float V[12], N[12];
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    const int64_t i = g * 4 + k;
    float v3[3] = {qnan(), qnan(), qnan()}, n3[3] = {qnan(), qnan(), qnan()};
    if (i < n) {
      const int u = (int)(i % cam.width), v = (int)(i / cam.width);
      (void)Resize<LV>::template node<false>(mv, P.cam[0].width, u, v, v3);
      (void)Resize<LV>::template node<true>(mn, P.cam[0].width, u, v, n3);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) { V[3 * k + q] = v3[q]; N[3 * k + q] = n3[q]; }
  }
  store4(mv + 3 * P.off[LV], g, n, V);
  store4(mn + 3 * P.off[LV], g, n, N);
}

// reads level 0 of mv / mn, writes levels 1 .. P.levels-1; workgroups partitioned by level (P.block0[1] = 0)
__global__ __launch_bounds__(kFeBlock) void model_pyramid_kernel(PyramidGeometry P, float* __restrict__ mv, float* __restrict__ mn) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kMaxLevels; k++) l += (k < P.levels && (int)blockIdx.x >= P.block0[k]) ? 1 : 0;
  const int64_t g = (int64_t)((int)blockIdx.x - P.block0[l]) * kFeBlock + threadIdx.x;
  if (g * 4 >= (int64_t)P.cam[l].width * P.cam[l].height) return;
  if (l == 1) model_group<1>(P, g, mv, mn);
  else if (l == 2) model_group<2>(P, g, mv, mn);
  else if (l == 3) model_group<3>(P, g, mv, mn);
}
static_assert(kMaxLevels == 4, "model_pyramid_kernel dispatches levels 1 .. 3");

// ---------------------------------------------------------------------------------------------- F3
// T: pose guess of the frame (Xc = R Xw + t).  M: pose of the model view (world -> model camera), mcam its intrinsics.
// use_normals = 0: the normal gate is skipped and pairs do not need normals (NW / NC are still written when present).
// pose_dev != null: T is read from HBM (12 doubles, the device-resident Gauss-Newton pose) instead of the argument;
// done != null: the launch returns at once when *done is set (GnState::done of that loop).
__global__ __launch_bounds__(kFeBlock) void associate_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                             const float* __restrict__ bmap, int64_t n, const float* __restrict__ mv,
                                                             const float* __restrict__ mn, PoseF T, AssocParams P, const double* __restrict__ pose_dev,
                                                             const int* __restrict__ done, float* __restrict__ xw, float* __restrict__ xc, float* __restrict__ bv,
                                                             float* __restrict__ nw, float* __restrict__ nc, int* __restrict__ count) {
  const int64_t g = (int64_t)blockIdx.x * kFeBlock + threadIdx.x;
  int matched = 0;
  if (done != nullptr && *done) return;  // device-resident loop already converged: keep the arrays of the last iteration
  if (pose_dev != nullptr) {
#pragma unroll
    for (int k = 0; k < 9; k++) T.R[k] = (float)pose_dev[k];
#pragma unroll
    for (int k = 0; k < 3; k++) T.t[k] = (float)pose_dev[9 + k];
  }
  if (g * 4 < n) {
    float V[12], N[12], B[12], OW[12], OC[12], OB[12], ONW[12], ONC[12];
    load4(vmap, g, n, V);
    load4(nmap, g, n, N);
    load4(bmap, g, n, B);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float x = V[3 * k], y = V[3 * k + 1], z = V[3 * k + 2];
      float mx, my, mz, gx, gy, gz;
      const bool ok = associate_pixel(T, P, mv, mn, x, y, z, N[3 * k], N[3 * k + 1], N[3 * k + 2], mx, my, mz, gx, gy, gz);
      matched += ok ? 1 : 0;
      const float nan = qnan();
      OW[3 * k] = mx; OW[3 * k + 1] = my; OW[3 * k + 2] = mz;
      ONW[3 * k] = gx; ONW[3 * k + 1] = gy; ONW[3 * k + 2] = gz;
      OC[3 * k] = ok ? x : nan; OC[3 * k + 1] = ok ? y : nan; OC[3 * k + 2] = ok ? z : nan;
      ONC[3 * k] = ok ? N[3 * k] : nan; ONC[3 * k + 1] = ok ? N[3 * k + 1] : nan; ONC[3 * k + 2] = ok ? N[3 * k + 2] : nan;
      OB[3 * k] = ok ? B[3 * k] : nan; OB[3 * k + 1] = ok ? B[3 * k + 1] : nan; OB[3 * k + 2] = ok ? B[3 * k + 2] : nan;
    }
    store4(xw, g, n, OW);
    store4(xc, g, n, OC);
    store4(bv, g, n, OB);
    store4(nw, g, n, ONW);
    store4(nc, g, n, ONC);
  }
  if (count != nullptr) {  // integer total: one atomic per wave64
    for (int off = 32; off > 0; off >>= 1) matched += __shfl_down(matched, off, 64);
    if ((threadIdx.x & 63) == 0 && matched) atomicAdd(count, matched);
  }
}

// ---------------------------------------------------------------------------------------------- R0, R1
// The map raycast: V2 (rpe_volume.hip) on the VIRTUAL volume G of a box of world voxels, whose voxel at box index (ix, iy, iz) holds the
// window's bits where the window covers it, the held brick's bits where the grid names a slot, {0, 0} elsewhere.  Bit for bit V2's
// result on a dense copy of the box: the ray rule is V2's (ray_march / ray_normal), the field is F's cell, weight test and lerp chain
// (cell / trilerp), the colour C3's (colour_rgba), all of rpe_volume_field.hpp; only where a corner's 8 bytes come from is stated here.
constexpr int kRayTile = 16;      // as V2: 16 x 16 pixels per workgroup, 8 x 8 per wave

__device__ __forceinline__ int grid_at(const MapRayView& M, int ix, int iy, int iz) {   // box index inside the box: <= 2^24 bricks
  return M.grid[((iz >> 3) * M.nb[1] + (iy >> 3)) * M.nb[0] + (ix >> 3)];
}

// One voxel of the map at box index (ix, iy, iz), inside the box.  The window is the only holder of what it covers and is addressed by
// the voxel's own index in it -- never through the grid, whose window entries R0 may have turned into kMapAbsent: that says "no weight
// > 0 in here", not "all-zero bits", and the colour field reads colour weights.  Anything else is a held brick's slot or absent.  e0 =
// the grid entry of the brick of (bx, by, bz), already read.  No address is formed outside the window's arrays or the pool's capacity
template <bool COLOUR>
__device__ __forceinline__ uint2 map_voxel(const MapRayView& M, int ix, int iy, int iz, int e0, int bx, int by, int bz) {
  const int lx = ix - M.woff[0], ly = iy - M.woff[1], lz = iz - M.woff[2];
  if ((unsigned)lx < (unsigned)M.wdim0 && (unsigned)ly < (unsigned)M.wdim1 && (unsigned)lz < (unsigned)M.wdim2) {
    const unsigned int* p = COLOUR ? M.cvol : M.vol;
    return p ? *reinterpret_cast<const uint2*>(p + 2 * (((int64_t)lz * M.wdim1 + ly) * M.wdim0 + lx)) : make_uint2(0u, 0u);
  }
  // a corner over a brick face, edge or corner: one more grid lookup
  const int s = ((ix >> 3) == bx && (iy >> 3) == by && (iz >> 3) == bz) ? e0 : grid_at(M, ix, iy, iz);
  int64_t w;
  bool pooled;
  const unsigned int* p = COLOUR ? M.cpool : M.pool;
  if (s >= 0 || s == kMapAbsent || !p || !brick_word(M, s, ix & 7, iy & 7, iz & 7, w, pooled)) return make_uint2(0u, 0u);
  return *reinterpret_cast<const uint2*>(p + w);
}

// the eight corners of the cell at i0 (corner n = di + 2 dj + 4 dk): where all eight lie in the window, the dense field's gathers
template <bool COLOUR>
__device__ __forceinline__ void map_corners(const MapRayView& M, const int i0[3], int e0, uint2 (&v)[8]) {
  const int lx = i0[0] - M.woff[0], ly = i0[1] - M.woff[1], lz = i0[2] - M.woff[2];
  const unsigned int* p = COLOUR ? M.cvol : M.vol;
  if (p && (unsigned)lx < (unsigned)(M.wdim0 - 1) && (unsigned)ly < (unsigned)(M.wdim1 - 1) && (unsigned)lz < (unsigned)(M.wdim2 - 1)) {
    const int64_t sy = 2 * (int64_t)M.wdim0, sz = sy * M.wdim1;
    const unsigned int* b = p + (int64_t)lz * sz + (int64_t)ly * sy + 2 * (int64_t)lx;
#pragma unroll
    for (int n = 0; n < 8; n++) v[n] = *reinterpret_cast<const uint2*>(b + ((n & 4) ? sz : 0) + ((n & 2) ? sy : 0) + ((n & 1) ? 2 : 0));
    return;
  }
  const int bx = i0[0] >> 3, by = i0[1] >> 3, bz = i0[2] >> 3;
#pragma unroll
  for (int n = 0; n < 8; n++) v[n] = map_voxel<COLOUR>(M, i0[0] + (n & 1), i0[1] + ((n >> 1) & 1), i0[2] + (n >> 2), e0, bx, by, bz);
}

// F(p) of the virtual volume.  The grid entry of corner 0's brick is read first: absent -- never held, or a window brick R0 found without
// a weight > 0 -- makes corner 0's weight fail the test, so the sample is unknown without a voxel load.  That is the empty-space skip.
__device__ __forceinline__ bool map_field(const MapRayView& M, const VolumeGeometry& G, float px, float py, float pz, float& F) {
  int i0[3];
  float a[3];
  if (!cell(G, px, py, pz, i0, a)) return false;
  const int e0 = grid_at(M, i0[0], i0[1], i0[2]);
  if (e0 == kMapAbsent) return false;
  uint2 v[8];
  map_corners<false>(M, i0, e0, v);
  bool known = true;
#pragma unroll
  for (int n = 0; n < 8; n++) known = known && __uint_as_float(v[n].y) > 0.0f;
  if (!known) return false;
  F = trilerp(__uint_as_float(v[0].x), __uint_as_float(v[1].x), __uint_as_float(v[2].x), __uint_as_float(v[3].x), __uint_as_float(v[4].x),
              __uint_as_float(v[5].x), __uint_as_float(v[6].x), __uint_as_float(v[7].x), a[0], a[1], a[2]);
  return true;
}

// C(p) of the virtual colour volume as RGBA8 (C3 of rpe_color.hip).  The grid is consulted for held bricks only (map_voxel), so R0's
// verdicts on the window's bricks do not reach the colour
__device__ __forceinline__ unsigned map_colour(const MapRayView& M, const VolumeGeometry& G, float px, float py, float pz) {
  int i0[3];
  float a[3];
  if (!cell(G, px, py, pz, i0, a)) return 0u;
  uint2 v[8];
  map_corners<true>(M, i0, grid_at(M, i0[0], i0[1], i0[2]), v);
  return colour_rgba(v, a);
}

__global__ __launch_bounds__(kRayTile * kRayTile) void map_raycast_kernel(MapRayView M, VolumeGeometry G, Camera cam, PoseF T, float dmin,
                                                                          float dmax, float* __restrict__ mv, float* __restrict__ mn,
                                                                          unsigned int* __restrict__ mc) {
  const int tiles_x = (cam.width + kRayTile - 1) / kRayTile;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int u = (blockIdx.x % tiles_x) * kRayTile + (wave % 2) * 8 + lane % 8;
  const int v = (blockIdx.x / tiles_x) * kRayTile + (wave / 2) * 8 + lane / 8;
  if (u >= cam.width || v >= cam.height) return;
  const float xn = ((float)u - cam.cx) / cam.fx, yn = ((float)v - cam.cy) / cam.fy;
  const auto F = [&](float x, float y, float z, float& f) { return map_field(M, G, x, y, z, f); };
  const float zh = ray_march(F, T, xn, yn, G.s, dmin, dmax);
  float ox = qnan(), oy = qnan(), oz = qnan(), nx = qnan(), ny = qnan(), nz = qnan();
  if (zh == zh) {
    to_world(T, xn * zh, yn * zh, zh, ox, oy, oz);
    (void)ray_normal(F, G.s, ox, oy, oz, nx, ny, nz);   // leaves the NaN normal where a sample is unknown
  }
  const int64_t pix = (int64_t)v * cam.width + u, o = 3 * pix;
  mv[o] = ox; mv[o + 1] = oy; mv[o + 2] = oz;
  mn[o] = nx; mn[o + 1] = ny; mn[o + 2] = nz;
  if (mc != nullptr) mc[pix] = zh == zh ? map_colour(M, G, ox, oy, oz) : 0u;   // C of a NaN point: its cell is out of range, 0
}

// R0: one wave per brick of the window inside the box; a lane reads four 16-byte pairs of voxels of the brick's 64 rows of 8.  No weight
// > 0 among the 512 (NaN fails the test) -> kMapAbsent.  The tsdf of such voxels is never read by anyone
constexpr int kOccBlock = 256;
__global__ __launch_bounds__(kOccBlock) void map_occupancy_kernel(MapRayView M) {
  const int b = (int)blockIdx.x * (kOccBlock / 64) + (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  if (b >= M.wbn[0] * M.wbn[1] * M.wbn[2]) return;   // the whole wave
  const int bx = M.wb0[0] + b % M.wbn[0], by = M.wb0[1] + (b / M.wbn[0]) % M.wbn[1], bz = M.wb0[2] + b / (M.wbn[0] * M.wbn[1]);
  bool some = false;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int c = q * 64 + lane, row = c >> 2, x = 2 * (c & 3);   // row = z * 8 + y
    const int64_t vox = ((int64_t)(bz * 8 + (row >> 3)) * M.wdim1 + by * 8 + (row & 7)) * M.wdim0 + bx * 8 + x;
    const uint4 p = *reinterpret_cast<const uint4*>(M.vol + 2 * vox);
    some = some || __uint_as_float(p.y) > 0.0f || __uint_as_float(p.w) > 0.0f;
  }
  if (__ballot(some) == 0ull && lane == 0)
    M.grid[((bz + (M.woff[2] >> 3)) * M.nb[1] + by + (M.woff[1] >> 3)) * M.nb[0] + bx + (M.woff[0] >> 3)] = kMapAbsent;
}

int fe_grid(int64_t n) { return (int)((n + 4 * kFeBlock - 1) / (4 * kFeBlock)); }

}  // namespace

hipError_t launch_frame_maps(const void* d_depth, int depth_type, const Camera& cam, float scale, float dmin, float dmax, float max_jump,
                             float* vmap, float* nmap, float* bmap, hipStream_t s) {
  const int64_t n = (int64_t)cam.width * cam.height;
  if (n == 0) return hipSuccess;
  if (depth_type == 0)
    hipLaunchKernelGGL(frame_maps_kernel<unsigned short>, dim3(fe_grid(n)), dim3(kFeBlock), 0, s, (const unsigned short*)d_depth, cam,
        scale, dmin,
                       dmax, max_jump, vmap, nmap, bmap);
  else
    hipLaunchKernelGGL(frame_maps_kernel<float>, dim3(fe_grid(n)), dim3(kFeBlock), 0, s, (const float*)d_depth, cam, scale, dmin, dmax,
        max_jump,
                       vmap, nmap, bmap);
  return hipGetLastError();
}

hipError_t launch_frame_pyramid(const void* d_depth, int depth_type, const PyramidGeometry& geo, float scale, float dmin, float dmax,
                                float max_jump, float* depth_out, float* vmap, float* nmap, float* bmap, hipStream_t s) {
  PyramidGeometry P = geo;
  const int w = P.cam[0].width, h = P.cam[0].height;
  const int tiles = ((w + kPyrTile - 1) / kPyrTile) * ((h + kPyrTile - 1) / kPyrTile);
  if (depth_type == 0)
    hipLaunchKernelGGL(depth_pyramid_kernel<unsigned short>, dim3(tiles), dim3(kFeBlock), 0, s, (const unsigned short*)d_depth, P, scale,
                       dmin, dmax, max_jump, depth_out);
  else
    hipLaunchKernelGGL(depth_pyramid_kernel<float>, dim3(tiles), dim3(kFeBlock), 0, s, (const float*)d_depth, P, scale, dmin, dmax,
                       max_jump, depth_out);
  int blocks = 0;
  for (int l = 0; l < P.levels; l++) { P.block0[l] = blocks; blocks += fe_grid((int64_t)P.cam[l].width * P.cam[l].height); }
  for (int l = P.levels; l <= kMaxLevels; l++) P.block0[l] = blocks;
  hipLaunchKernelGGL(pyramid_maps_kernel, dim3(blocks), dim3(kFeBlock), 0, s, (const float*)depth_out, P, dmin, dmax, max_jump, vmap, nmap,
                     bmap);
  return hipGetLastError();
}

hipError_t launch_model_pyramid(const PyramidGeometry& geo, float* mv, float* mn, hipStream_t s) {
  PyramidGeometry P = geo;
  if (P.levels < 2) return hipSuccess;
  int blocks = 0;
  P.block0[0] = 0;
  for (int l = 1; l < P.levels; l++) { P.block0[l] = blocks; blocks += fe_grid((int64_t)P.cam[l].width * P.cam[l].height); }
  for (int l = P.levels; l <= kMaxLevels; l++) P.block0[l] = blocks;
  hipLaunchKernelGGL(model_pyramid_kernel, dim3(blocks), dim3(kFeBlock), 0, s, P, mv, mn);
  return hipGetLastError();
}

hipError_t launch_to_world(const float* vmap, const float* nmap, int64_t n, const PoseF& T, float* vw, float* nw, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(to_world_kernel, dim3(fe_grid(n)), dim3(kFeBlock), 0, s, vmap, nmap, n, T, vw, nw);
  return hipGetLastError();
}

hipError_t launch_associate(const float* vmap, const float* nmap, const float* bmap, int64_t n, const float* mv, const float* mn,
                            const Camera& mcam, const PoseF& T, const PoseF& M, float dist_sq, float cos_thr, int use_normals,
                            const double* pose_dev, const int* done, float* xw, float* xc, float* bv, float* nw, float* nc, int* d_count,
                            hipStream_t s) {
  if (n == 0) return hipSuccess;
  AssocParams P;
  P.mcam = mcam; P.M = M; P.dist_sq = dist_sq; P.cos_thr = cos_thr; P.use_normals = use_normals;
  hipLaunchKernelGGL(associate_kernel, dim3(fe_grid(n)), dim3(kFeBlock), 0, s, vmap, nmap, bmap, n, mv, mn, T, P, pose_dev, done, xw,
      xc, bv,
                     nw, nc, d_count);
  return hipGetLastError();
}

hipError_t launch_map_occupancy(const MapRayView& M, hipStream_t s) {
  const int n = M.wbn[0] * M.wbn[1] * M.wbn[2];
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_occupancy_kernel, dim3((n + kOccBlock / 64 - 1) / (kOccBlock / 64)), dim3(kOccBlock), 0, s, M);
  return hipGetLastError();
}

hipError_t launch_map_raycast(const MapRayView& M, const VolumeGeometry& G, const Camera& cam, const PoseF& T, float dmin, float dmax,
                              float* mv, float* mn, unsigned int* mc, hipStream_t s) {
  const int tiles = ((cam.width + kRayTile - 1) / kRayTile) * ((cam.height + kRayTile - 1) / kRayTile);
  hipLaunchKernelGGL(map_raycast_kernel, dim3(tiles), dim3(kRayTile * kRayTile), 0, s, M, G, cam, T, dmin, dmax, mv, mn, mc);
  return hipGetLastError();
}

RPE_PRELOAD(to_world_kernel);

}  // namespace rpe

// ================================================================================================
// THE VOLUME TERM (include/rgbd_pose_hip.h Part 3, "Volume term"): a frame tracked against the TSDF volume itself.  The per-pixel rule
// is sdf_pixel of rpe_sdf_rule.hpp, bit-exact; the sums are those of every Gauss-Newton kernel (rpe_residuals.hpp add_row2,
// rpe_reduce.hpp reduce_and_finish), included here so that the kernels above compile as they did without them.
//   sdf_rows_kernel      {r, J[0..5]} of every frame pixel (NaN where there is no row): the residual image and the tests' hook.
//   icp_sdf_kernel<BLK>  one Gauss-Newton round in one pass over the level's frame pixels: per pixel 12 B of vertex (24 B with the
//                        normal gate) streamed and eight 8-byte corner voxels gathered; add_row2 on pairs of pixels into fp32 partial
//                        sums of one group of 4 pixels, widened to fp64 per group; the 29 sums of every normal-equation record.
// ================================================================================================
#include "rpe_residuals.hpp"
#include "rpe_sdf_rule.hpp"

namespace rpe {

namespace {

constexpr int kSdfRowsBlock = 256;   // one pixel per lane

// One group of 4 pixels into the accumulators (a pixel that is not there has a NaN vertex: no row).  The order is chosen for the
// registers (tests/test_sdf_oracle.py holds the kernel to 128): the four rows first, from the vertices alone; then the normals are
// fetched (normals(N): only with use_normals) and gate them; then the sums.
template <class Normals>
__device__ __forceinline__ void sdf_group(const float* __restrict__ vol, const VolumeGeometry& G, const PoseF& T, const SdfParams& Q,
                                          const float (&V)[12], Normals normals, double (&acc)[28], float& rows) {
  typedef float V2 __attribute__((ext_vector_type(2)));
  const dense_corners corners(vol, G);
  float r[4], J[4][6], len[4];
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; i++) ok[i] = sdf_pixel_row(corners, G, T, Q, V[3 * i], V[3 * i + 1], V[3 * i + 2], r[i], J[i], len[i]);
  if (Q.use_normals) {
    float N[12];
    normals(N);
#pragma unroll
    for (int i = 0; i < 4; i++) ok[i] = ok[i] && sdf_normal_gate(Q, N[3 * i], N[3 * i + 1], N[3 * i + 2], len[i], r[i], J[i]);
  }
  // add_row2 (rpe_residuals.hpp) on the pair of pixels 0, 1 and then on the pair 2, 3, and the group's sums widened to fp64 once --
  // written sum by sum, so that the 28 fp32 pair sums need not all be held at once: for every sum the two fused multiply-adds of
  // add_row2 on a zero start, the addition of the pair's lanes and the widening are the operations add_row2 twice and
  // (double)(s.x + s.y) perform, in their order
  const V2 wa = V2{ok[0] ? 1.f : 0.f, ok[1] ? 1.f : 0.f}, wb = V2{ok[2] ? 1.f : 0.f, ok[3] ? 1.f : 0.f};
  const V2 ra = V2{r[0], r[1]}, rb = V2{r[2], r[3]}, zero = V2{0.f, 0.f};
  V2 Ja[6], Jb[6];
#pragma unroll
  for (int a = 0; a < 6; a++) { Ja[a] = V2{J[0][a], J[1][a]}; Jb[a] = V2{J[2][a], J[3][a]}; }
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const V2 xa = wa * Ja[a], xb = wb * Jb[a];
#pragma unroll
    for (int b = a; b < 6; b++) {
      const V2 t = __builtin_elementwise_fma(xb, Jb[b], __builtin_elementwise_fma(xa, Ja[b], zero));
      acc[k] += (double)(t.x + t.y); k++;
    }
    const V2 t = __builtin_elementwise_fma(xb, rb, __builtin_elementwise_fma(xa, ra, zero));
    acc[21 + a] += (double)(t.x + t.y);
  }
  const V2 t = __builtin_elementwise_fma(wb * rb, rb, __builtin_elementwise_fma(wa * ra, ra, zero));
  acc[27] += (double)(t.x + t.y);
  rows += (wa.x + wa.y) + (wb.x + wb.y);   // (a thread sees fewer than 2^24 pixels: exact)
}

// The kernel's arguments as the kernarg segment lays them out (every argument at its natural alignment, in order), for late_finish
struct SdfRoundArgs { const float* vmap; const float* nmap; int64_t n; const float* vol; VolumeGeometry G; SdfParams Q; PoseF T; Finish fin; };
// (tests/test_sdf_oracle.py reads the same offset and size from the code object's metadata)
static_assert(offsetof(SdfRoundArgs, fin) == 136 && sizeof(Finish) == 136, "late_finish: where the kernarg segment holds the reduction's argument");
// The reduction's argument read from the kernarg segment where it is needed, behind the pixel loop: as a plain argument the compiler
// loads all of it in the kernel's first block and keeps its scalar registers through the loop, beside pose, geometry and gates, which
// is more than the 102 there are.  (The offset goes through an empty asm so that the loads stay below it.)
__device__ __forceinline__ Finish late_finish_at(unsigned off) {
  asm volatile("" : "+s"(off));
  Finish f;
  __builtin_memcpy(&f, (const char*)__builtin_amdgcn_kernarg_segment_ptr() + off, sizeof(Finish));
  return f;
}
__device__ __forceinline__ Finish late_finish() { return late_finish_at((unsigned)offsetof(SdfRoundArgs, fin)); }
// The pose read from the kernarg segment with scalar loads (the segment is constant memory), where a loop trip needs it: for the round
// kernels with one pixel per trip (late_pose, photo_late_pose, map_photo_late_pose name their offsets).  As a plain argument its twelve
// scalars are live through the whole loop beside everything else the trip keeps in scalar registers, which is more than the 102 there
// are.  The offset goes through an empty asm, as late_finish_at's does, so that the loads stay where they are written and the reads of
// one trip are not merged
__device__ __forceinline__ PoseF late_pose_at(unsigned off) {
  typedef const __attribute__((address_space(4))) float* KernargFloats;
  asm volatile("" : "+s"(off));
  KernargFloats p = (KernargFloats)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
  PoseF T;
#pragma unroll
  for (int k = 0; k < 9; k++) T.R[k] = p[k];
#pragma unroll
  for (int k = 0; k < 3; k++) T.t[k] = p[9 + k];
  return T;
}

// four waves per SIMD's worth of registers: 128
template <int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_sdf_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n, const float* __restrict__ vol, VolumeGeometry G, SdfParams Q,
    PoseF T, Finish /* read by late_finish */) {
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; k++) acc[k] = 0.0;
  float rows = 0.f;
  const int full = (int)(n / 4);                  // (n <= 2^28 pixels: rpe_frame_set_depth)
  const int stride = (int)gridDim.x * BLK;
  const float4* __restrict__ v4 = reinterpret_cast<const float4*>(vmap);
  const float4* __restrict__ n4 = reinterpret_cast<const float4*>(nmap);
  for (int g = (int)blockIdx.x * BLK + (int)threadIdx.x; g < full; g += stride) {
    const int64_t q = 3 * (int64_t)g;
    float V[12];
    unpack3(v4[q], v4[q + 1], v4[q + 2], V);
    sdf_group(vol, G, T, Q, V, [&](float (&N)[12]) { unpack3(n4[q], n4[q + 1], n4[q + 2], N); }, acc, rows);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (int64_t)full * 4 < n) {  // leftover pixels
    const int left = (int)(n - (int64_t)full * 4);
    float V[12];
#pragma unroll
    for (int i = 0; i < 12; i++) V[i] = i < 3 * left ? vmap[12 * (int64_t)full + i] : qnan();
    sdf_group(vol, G, T, Q, V, [&](float (&N)[12]) {
#pragma unroll
      for (int i = 0; i < 12; i++) N[i] = i < 3 * left ? nmap[12 * (int64_t)full + i] : qnan();
    }, acc, rows);
  }
  double sums[29];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)rows;
  reduce_and_finish<29, kNeLd, 0, BLK, false>(sums, late_finish());   // host-driven only: no device-side solve in this kernel
}

// the tail of the four rows kernels: {r, J[0..5]} of pixel i into the seven planes of rows, NaN where the pixel has no row
__device__ __forceinline__ void store_row(float* __restrict__ rows, int64_t n, int64_t i, bool ok, float r, const float (&J)[6]) {
  rows[i] = ok ? r : qnan();
#pragma unroll
  for (int k = 0; k < 6; k++) rows[(int64_t)(k + 1) * n + i] = ok ? J[k] : qnan();
}

__global__ __launch_bounds__(kSdfRowsBlock) void sdf_rows_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n,
                                                                 const float* __restrict__ vol, VolumeGeometry G, SdfParams Q, PoseF T,
                                                                 float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kSdfRowsBlock + threadIdx.x;
  if (i >= n) return;
  float r, J[6], nx = 0.f, ny = 0.f, nz = 0.f;
  if (Q.use_normals) { nx = nmap[3 * i]; ny = nmap[3 * i + 1]; nz = nmap[3 * i + 2]; }
  const bool ok = sdf_pixel(dense_corners(vol, G), G, T, Q, vmap[3 * i], vmap[3 * i + 1], vmap[3 * i + 2], nx, ny, nz, r, J);
  store_row(rows, n, i, ok, r, J);
}

SdfParams sdf_params(const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals) {
  SdfParams Q;
  Q.gate = dist_thr; Q.c = cos_thr; Q.k = G.tr / G.s; Q.use_normals = use_normals;
  return Q;
}
// the grid of a round launch of blk threads a workgroup: one item per thread while rt.max_blocks allows it, at least one workgroup
// (an item: a group of 4 pixels for icp_sdf_kernel, a pixel for the round kernels with one pixel per trip)
int round_grid(const ReduceTarget& rt, int64_t items, int blk) {
  const int64_t full = (items + blk - 1) / blk;
  const int grid = (int64_t)rt.max_blocks > full ? (int)full : rt.max_blocks;
  return grid < 1 ? 1 : grid;
}

}  // namespace

hipError_t launch_icp_sdf(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                          float cos_thr, int use_normals, const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  // geometry as the fused ICP round's: one pixel group per thread while the grid allows it
  const int blk = pick_block(rt);
  const int grid = round_grid(rt, (n + 3) / 4, blk);
  if (blk == 512) hipLaunchKernelGGL((icp_sdf_kernel<512>), dim3(grid), dim3(512), 0, s, vmap, nmap, n, vol, G, Q, T, fin);
  else hipLaunchKernelGGL((icp_sdf_kernel<256>), dim3(grid), dim3(256), 0, s, vmap, nmap, n, vol, G, Q, T, fin);
  return hipGetLastError();
}

hipError_t launch_sdf_rows(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                           float cos_thr, int use_normals, const double* pose12, float* rows, hipStream_t s) {
  const int64_t blocks = (n + kSdfRowsBlock - 1) / kSdfRowsBlock;
  hipLaunchKernelGGL(sdf_rows_kernel, dim3((unsigned)blocks), dim3(kSdfRowsBlock), 0, s, vmap, nmap, n, vol, G,
                     sdf_params(G, dist_thr, cos_thr, use_normals), pose_f(pose12), rows);
  return hipGetLastError();
}

// ================================================================================================
// THE MAP VOLUME TERM (include/rgbd_pose_hip.h Part 3, "Map volume term"): the volume term on the virtual volume of a box of the map --
// the window plus the archived bricks.  No new arithmetic: the rule is sdf_pixel with a corner fetch over the brick grid of the map
// raycast (grid_at / map_corners above), so the rows are bit for bit sdf_rows_kernel's on a dense copy of the box.
//   map_sdf_rows_kernel      sdf_rows_kernel with that fetch.
//   icp_map_sdf_kernel<BLK>  one Gauss-Newton round.  ONE pixel per loop trip: the fetch's branches (window, held brick, a grid lookup per
//                            corner over a brick face) cost the registers that sdf_group's four pixels in flight need (462 vector spills
//                            when reused as it is).  A pixel's fp32 row is widened to fp64 and its 28 products are fp64 fused
//                            multiply-adds: a product of two floats is exact in fp64, so a sum carries fp64 accumulation error only.
// ================================================================================================
namespace {

// what the fetch reads of a MapRayView: the kernel argument (16 scalars for the round kernel's loop to keep, not 29)
struct MapSdfView {
  const unsigned int *vol, *pool;
  const int* grid;
  int wdim0, wdim1, wdim2, woff[3], nb0, nb1, capacity;
};
__device__ __forceinline__ MapRayView ray_view(const MapSdfView& S) {
  MapRayView M{};   // no colour; wnb, nb[2], wb0, wbn are not read by grid_at / map_corners<false>
  M.vol = S.vol; M.pool = S.pool; M.grid = const_cast<int*>(S.grid);
  M.wdim0 = S.wdim0; M.wdim1 = S.wdim1; M.wdim2 = S.wdim2; M.capacity = S.capacity;
#pragma unroll
  for (int a = 0; a < 3; a++) M.woff[a] = S.woff[a];
  M.nb[0] = S.nb0; M.nb[1] = S.nb1;
  return M;
}

// The eight corner voxels of the cell i0 of the virtual volume (i0 inside the box, i0 + 1 too: sdf_cell).  The grid entry of corner 0's
// brick is read first: absent -> "no voxels" without a voxel load, which is exact, since corner 0 is then {0, 0} and fails the weight
// test.  Otherwise map_corners: dense gathers when all eight lie in the window, a grid lookup per corner over a brick face.  No address
// is formed outside the window's arrays or the pool's capacity (map_voxel)
struct map_sdf_corners {
  const MapRayView& M;
  __device__ __forceinline__ bool operator()(const int (&i0)[3], float2 (&v)[8]) const {
    const int e0 = grid_at(M, i0[0], i0[1], i0[2]);
    uint2 u[8];
#pragma unroll
    for (int n = 0; n < 8; n++) u[n] = make_uint2(0u, 0u);
    if (e0 != kMapAbsent) map_corners<false>(M, i0, e0, u);
#pragma unroll
    for (int n = 0; n < 8; n++) v[n] = make_float2(__uint_as_float(u[n].x), __uint_as_float(u[n].y));
    return e0 != kMapAbsent;
  }
};

struct MapSdfRoundArgs { const float* vmap; const float* nmap; int64_t n; MapSdfView S; VolumeGeometry G; SdfParams Q; PoseF T; Finish fin; };
// (tests/test_mapsdf_oracle.py reads the same offset and size from the code object's metadata)
static_assert(offsetof(MapSdfRoundArgs, fin) == 192 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(MapSdfRoundArgs, T) == 140 && sizeof(PoseF) == 48, "late_pose: where the kernarg segment holds the pose");

// late_pose_at for this kernel: beside view, geometry, gates and the exec masks of the fetch's nested branches the pose as a plain
// argument costs 4 - 7 scalar spills, however the rest is arranged
__device__ __forceinline__ PoseF late_pose() { return late_pose_at((unsigned)offsetof(MapSdfRoundArgs, T)); }

template <int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(4))) void icp_map_sdf_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, int64_t n, MapSdfView S, VolumeGeometry G, SdfParams Q,
    PoseF /* read by late_pose */, Finish /* read by late_finish_at */) {
  const MapRayView M = ray_view(S);
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; k++) acc[k] = 0.0;
  float rows = 0.f;
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    // sdf_pixel in its parts (sdf_pixel_row's composition, then the normal gate), so that the pose is read once for the cell and once
    // more, behind the fetch, for the row; the normal is fetched behind the corners too (as sdf_group does, for the registers)
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2];
    int i0[3];
    float a[3], r, J[6], len;
    float2 v[8];
    const bool in = sdf_cell(G, late_pose(), x, y, z, i0, a);
    const bool have = map_sdf_corners{M}(i0, v);
    bool ok = sdf_row(v, a, G, late_pose(), Q, x, y, z, r, J, len) && in && have;
    if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
    if (!ok) {
      r = 0.f;
#pragma unroll
      for (int k = 0; k < 6; k++) J[k] = 0.f;
    }
    // a pixel without a row has r = 0 and J = 0: its products add exact zeros
    double Jd[6];
#pragma unroll
    for (int a = 0; a < 6; a++) Jd[a] = (double)J[a];
    const double rd = (double)r;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = a; b < 6; b++) { acc[k] = __builtin_fma(Jd[a], Jd[b], acc[k]); k++; }
      acc[21 + a] = __builtin_fma(Jd[a], rd, acc[21 + a]);
    }
    acc[27] = __builtin_fma(rd, rd, acc[27]);
    rows += ok ? 1.f : 0.f;   // (a thread sees fewer than 2^24 pixels: exact)
  }
  double sums[29];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)rows;
  reduce_and_finish<29, kNeLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(MapSdfRoundArgs, fin)));   // host-driven only
}

__global__ __launch_bounds__(kSdfRowsBlock) void map_sdf_rows_kernel(const float* __restrict__ vmap, const float* __restrict__ nmap,
                                                                     int64_t n, MapSdfView S, VolumeGeometry G, SdfParams Q, PoseF T,
                                                                     float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kSdfRowsBlock + threadIdx.x;
  if (i >= n) return;
  const MapRayView M = ray_view(S);
  float r, J[6], nx = 0.f, ny = 0.f, nz = 0.f;
  if (Q.use_normals) { nx = nmap[3 * i]; ny = nmap[3 * i + 1]; nz = nmap[3 * i + 2]; }
  const bool ok = sdf_pixel(map_sdf_corners{M}, G, T, Q, vmap[3 * i], vmap[3 * i + 1], vmap[3 * i + 2], nx, ny, nz, r, J);
  store_row(rows, n, i, ok, r, J);
}

MapSdfView sdf_view(const MapRayView& M) {
  MapSdfView S;
  S.vol = M.vol; S.pool = M.pool; S.grid = M.grid;
  S.wdim0 = M.wdim0; S.wdim1 = M.wdim1; S.wdim2 = M.wdim2; S.capacity = M.capacity;
  for (int a = 0; a < 3; a++) S.woff[a] = M.woff[a];
  S.nb0 = M.nb[0]; S.nb1 = M.nb[1];
  return S;
}

// a node per new kernel, beside the unit's own (one code object: whichever is touched first loads all of it)
namespace rows_node { RPE_PRELOAD(map_sdf_rows_kernel); }
namespace round_node { RPE_PRELOAD(icp_map_sdf_kernel<256>); }

}  // namespace

hipError_t launch_icp_map_sdf(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G, float dist_thr,
                              float cos_thr, int use_normals, const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const MapSdfView S = sdf_view(M);
  const int blk = pick_block(rt);   // one pixel per thread while the grid allows it
  const int grid = round_grid(rt, n, blk);
  if (blk == 512) hipLaunchKernelGGL((icp_map_sdf_kernel<512>), dim3(grid), dim3(512), 0, s, vmap, nmap, n, S, G, Q, T, fin);
  else hipLaunchKernelGGL((icp_map_sdf_kernel<256>), dim3(grid), dim3(256), 0, s, vmap, nmap, n, S, G, Q, T, fin);
  return hipGetLastError();
}

hipError_t launch_map_sdf_rows(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G, float dist_thr,
                               float cos_thr, int use_normals, const double* pose12, float* rows, hipStream_t s) {
  const int64_t blocks = (n + kSdfRowsBlock - 1) / kSdfRowsBlock;
  hipLaunchKernelGGL(map_sdf_rows_kernel, dim3((unsigned)blocks), dim3(kSdfRowsBlock), 0, s, vmap, nmap, n, sdf_view(M), G,
                     sdf_params(G, dist_thr, cos_thr, use_normals), pose_f(pose12), rows);
  return hipGetLastError();
}

}  // namespace rpe

// ================================================================================================
// THE MAP FUSE (include/rgbd_pose_hip.h Part 3, "Map fuse"): the keyframe list of rpe_rebuild.hip's R2 fused into every brick of a box of the
// map.  The kernel's text is rpe_mapfuse.hpp; it is compiled here, with the map raycast and the map volume term, whose view of a brick
// (brick_word) it shares.
#include "rpe_mapfuse.hpp"

// ================================================================================================
// THE VOLUME COLOUR TERM (include/rgbd_pose_hip.h Part 3, "Volume colour term"): a photometric term against the colour volume, beside the
// volume term and in one launch with it.  The kernels' text is rpe_sdf_photo.hpp; it is compiled here, with the volume term whose cell,
// corner fetch, row and late_finish_at it shares.
#include "rpe_sdf_photo.hpp"
