// Device code shared by the volume's kernels, each rule stated once: voxel projection and update (V1, the tsdf half of C2, R2) and the
// lane's {tsdf, w} pairs of V1 and C2; the field's cell, lerp chain and normal (F(p) of V2 and M4, C(p) of C3, both fields of rpe_mapmesh.hip
// and of the map raycast in rpe_frontend.hip); the ray rule of V2 and the map raycast (ray_march, ray_normal: templates over the field, so
// neither kernel keeps the rule as its own text); where a voxel of a map brick lies (brick_word: the map mesh and the map raycast).
// Followed BIT-EXACTLY (include/rgbd_pose_hip.h Part 3, "TSDF volume"): FMA contraction is off from here to the end of the including unit.
#pragma once
#include "rpe_assoc.h"

#pragma clang fp contract(off)

namespace rpe {
namespace {

// Voxel (i, j, k), centre p = o + ((float)i + 0.5f) * s per axis; camera point pc = R p + t (rows left to right); pixel = nearest
// (floorf(f * x / z + c + 0.5f)); d = z of the level-0 vertex map there (NaN = invalid depth); sdf = d - pc.z; updated iff pc.z > 0,
// the pixel is in the image, d is valid and sdf >= -tr: f = fminf(1, sdf / tr), tsdf = (tsdf * w + f) / (w + 1), w = fminf(w + 1, W).
// voxel_project also hands out sdf and the pixel's index (v * width + u) of an updated voxel.  The depth of pixel `pix` is
// vmap[STRIDE * pix + OFFSET]: the z of a vertex map by default, <1, 0> for a packed depth plane (rpe_rebuild.hip).
template <int STRIDE = 3, int OFFSET = 2>
__device__ __forceinline__ bool voxel_project(const VolumeGeometry& G, const float* __restrict__ vmap, const Camera& cam, const PoseF& T,
                                              int i, int j, int k, float& f, float& sdf, int64_t& pix) {
  const float px = G.o[0] + ((float)i + 0.5f) * G.s, py = G.o[1] + ((float)j + 0.5f) * G.s, pz = G.o[2] + ((float)k + 0.5f) * G.s;
  const float cx = T.R[0] * px + T.R[1] * py + T.R[2] * pz + T.t[0];
  const float cy = T.R[3] * px + T.R[4] * py + T.R[5] * pz + T.t[1];
  const float cz = T.R[6] * px + T.R[7] * py + T.R[8] * pz + T.t[2];
  if (!(cz > 0.0f)) return false;
  const float uf = floorf(cam.fx * (cx / cz) + cam.cx + 0.5f), vf = floorf(cam.fy * (cy / cz) + cam.cy + 0.5f);
  if (!(uf >= 0.0f && uf <= (float)(cam.width - 1) && vf >= 0.0f && vf <= (float)(cam.height - 1))) return false;
  pix = (int64_t)(int)vf * cam.width + (int)uf;
  const float d = vmap[STRIDE * pix + OFFSET];
  if (d != d) return false;
  sdf = d - cz;
  if (!(sdf >= -G.tr)) return false;
  f = fminf(1.0f, sdf / G.tr);
  return true;
}

__device__ __forceinline__ bool voxel_sdf(const VolumeGeometry& G, const float* __restrict__ vmap, const Camera& cam, const PoseF& T, int i,
                                          int j, int k, float& f) {
  float sdf;
  int64_t pix;
  return voxel_project(G, vmap, cam, T, i, j, k, f, sdf, pix);
}

__device__ __forceinline__ void fuse(float& tsdf, float& w, float f, float W) {
  tsdf = (tsdf * w + f) / (w + 1.0f);
  w = fminf(w + 1.0f, W);
}

// THE FUSE'S CULL (R2 of rpe_rebuild.hip, the map fuse of rpe_mapfuse.hpp): can a list entry update any voxel of a brick?
// the cull's margin on a camera coordinate, relative to the sum of the magnitudes that enter it (64 ulp: see box_can_update)
constexpr float kCullEps = 1.0f / 262144.0f;
// Can entry E update ANY voxel whose centre lies in the box [lo, hi] (per axis the centres of the brick's first and last voxel, formed
// with voxel_project's own expression: fp32 rounding is monotonic, so every centre of the brick lies inside)?  false only when every
// centre fails voxel_project: all behind the camera, or all outside the same image edge.
// The box in the camera frame is its centre R c + t with the half extents |R| h.  Exactly, every centre's camera coordinate lies in
// that interval; in fp32 the kernel's own coordinate (three products, three sums) and the interval's ends (c and h: one and two
// roundings; the centre six, the extent five) are each off by a few ulp of M = |R| max(|lo|, |hi|) + |t|, the sum of the magnitudes
// that enter them: fewer than 32 roundings of at most 2^-24 M in all.  The interval is widened by 2^-18 M = 64 ulp on either side.
// The pixel of the interval's extreme ratio is then formed with voxel_project's expression, fx * (x / z) + cx + 0.5f: division,
// product and sums are correctly rounded and so monotonic in x and z, hence no voxel's pixel coordinate passes the extreme one; one
// whole pixel (and 2^-18 of the coordinate) is left on top.  Every comparison is written so that a NaN keeps the entry.
__device__ __forceinline__ bool edge_outside(float xlo, float xhi, float zl, float zh, float f, float c, int size) {
  const float inf = __int_as_float(0x7f800000);
  // the largest and the smallest x / z over the part of the box in front of the camera (0 < z, zl <= z <= zh)
  const float rmax = xhi >= 0.0f ? (zl > 0.0f ? xhi / zl : inf) : xhi / zh;
  const float rmin = xlo <= 0.0f ? (zl > 0.0f ? xlo / zl : -inf) : xlo / zh;
  const float umax = f * rmax + c + 0.5f, umin = f * rmin + c + 0.5f;
  return umax + (1.0f + kCullEps * fabsf(umax)) < 0.0f || umin - (1.0f + kCullEps * fabsf(umin)) > (float)size;
}

__device__ __forceinline__ bool box_can_update(const float* lo, const float* hi, const Camera& cam, const PoseF& T) {
  float c[3], h[3], a[3];
#pragma unroll
  for (int d = 0; d < 3; d++) { c[d] = 0.5f * (lo[d] + hi[d]); h[d] = 0.5f * (hi[d] - lo[d]); a[d] = fmaxf(fabsf(lo[d]), fabsf(hi[d])); }
  float l[3], u[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float R0 = T.R[3 * r], R1 = T.R[3 * r + 1], R2 = T.R[3 * r + 2];
    const float q = R0 * c[0] + R1 * c[1] + R2 * c[2] + T.t[r];
    const float e = fabsf(R0) * h[0] + fabsf(R1) * h[1] + fabsf(R2) * h[2];
    const float m = kCullEps * (fabsf(R0) * a[0] + fabsf(R1) * a[1] + fabsf(R2) * a[2] + fabsf(T.t[r]));
    l[r] = q - e - m; u[r] = q + e + m;
  }
  if (u[2] <= 0.0f) return false;                                                        // every centre behind the camera
  if (edge_outside(l[0], u[0], l[2], u[2], cam.fx, cam.cx, cam.width)) return false;    // all left of column 0 or right of the last
  if (edge_outside(l[1], u[1], l[2], u[2], cam.fy, cam.cy, cam.height)) return false;   // all above row 0 or below the last
  return true;
}

// binary16 <-> fp32.  h(x): round to nearest even, subnormals kept, every NaN to the quiet NaN 0x7e00.
__device__ __forceinline__ float h2f(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
__device__ __forceinline__ unsigned f2h(float x) { return x == x ? (unsigned)__builtin_bit_cast(unsigned short, (_Float16)x) : 0x7e00u; }

// One voxel's colour {r, g, b, wc} as two words (rg = r | g << 16, bw = b | wc << 16) and the observation o (RGBA8): with w = (float)wc
// before the update, each channel c := h(((float)c * w + o) / (w + 1.0f)), then wc := h(fminf(w + 1.0f, W)).  (The colour integrate
// of rpe_color.hip and the keyframe fuse of rpe_rebuild.hip.)
__device__ __forceinline__ void blend(unsigned& rg, unsigned& bw, unsigned o, float W) {
  const float w = h2f(bw >> 16);
  const float r = (h2f(rg & 0xffffu) * w + (float)(o & 0xffu)) / (w + 1.0f);
  const float g = (h2f(rg >> 16) * w + (float)((o >> 8) & 0xffu)) / (w + 1.0f);
  const float b = (h2f(bw & 0xffffu) * w + (float)((o >> 16) & 0xffu)) / (w + 1.0f);
  rg = f2h(r) | f2h(g) << 16;
  bw = f2h(b) | f2h(fminf(w + 1.0f, W)) << 16;
}

// V1, C2: the lane's pair of voxels a, a + 1 (16 bytes), loaded if either is updated (the volume's last voxel alone, as a float2)
__device__ __forceinline__ float4 load_pair(const float* __restrict__ vol, int64_t a, int64_t nvox, bool either) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (either) {
    if (a + 1 < nvox) v = *reinterpret_cast<const float4*>(vol + 2 * a);
    else { const float2 h = *reinterpret_cast<const float2*>(vol + 2 * a); v.x = h.x; v.y = h.y; }
  }
  return v;
}
// ... and each updated voxel (lo: a, hi: a + 1) stored, a pair as one 16-byte store
__device__ __forceinline__ void store_pair(float* __restrict__ vol, int64_t a, float4 v, bool lo, bool hi) {
  if (!lo && !hi) return;
  float* q = vol + 2 * a;
  if (lo && hi) *reinterpret_cast<float4*>(q) = v;
  else if (lo) *reinterpret_cast<float2*>(q) = make_float2(v.x, v.y);
  else *reinterpret_cast<float2*>(q + 2) = make_float2(v.z, v.w);
}

// F(p): g = (p - o) / s - 0.5f, i0 = floorf(g), a = g - i0 per axis; known iff 0 <= i0 <= dim - 2 on every axis and all eight corner
// weights are > 0; trilinear with lerp(x, y, t) = x + (y - x) * t along x for (j, k) = (0,0) (1,0) (0,1) (1,1), then y, then z.
__device__ __forceinline__ float lerp(float x, float y, float t) { return x + (y - x) * t; }
// the cell of p: i0 and a, false when i0 is out of range
__device__ __forceinline__ bool cell(const VolumeGeometry& G, float px, float py, float pz, int i0[3], float a[3]) {
  const float gx = (px - G.o[0]) / G.s - 0.5f, gy = (py - G.o[1]) / G.s - 0.5f, gz = (pz - G.o[2]) / G.s - 0.5f;
  const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
  if (!(fx >= 0.0f && fx <= (float)(G.dim[0] - 2) && fy >= 0.0f && fy <= (float)(G.dim[1] - 2) && fz >= 0.0f &&
        fz <= (float)(G.dim[2] - 2)))
    return false;
  a[0] = gx - fx; a[1] = gy - fy; a[2] = gz - fz;
  i0[0] = (int)fx; i0[1] = (int)fy; i0[2] = (int)fz;
  return true;
}
// the chain's y and z steps on the four x lerps, and the whole chain on the eight corner values vIJK (I along x)
__device__ __forceinline__ float bilerp(float c00, float c10, float c01, float c11, float ay, float az) {
  return lerp(lerp(c00, c10, ay), lerp(c01, c11, ay), az);
}
__device__ __forceinline__ float trilerp(float v000, float v100, float v010, float v110, float v001, float v101, float v011, float v111,
                                         float ax, float ay, float az) {
  return bilerp(lerp(v000, v100, ax), lerp(v010, v110, ax), lerp(v001, v101, ax), lerp(v011, v111, ax), ay, az);
}

// the colour field's RGBA8 byte (rpe_color.hip C3, rpe_mapmesh.hip P3): q(x) = (uint8)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f)
__device__ __forceinline__ unsigned quantise(float x) { return (unsigned)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f); }
// C(p) as RGBA8 from the cell's eight corner voxels v[di + 2 dj + 4 dk] (two words each, as blend's) and a: 0 unless all eight colour
// weights are > 0; each channel with F's lerp chain on (float) of the binary16 values, quantised, A = 255 (C3, the map raycast)
__device__ __forceinline__ unsigned colour_rgba(const uint2 (&v)[8], const float a[3]) {
  unsigned out = 0u;
  bool known = true;
#pragma unroll
  for (int m = 0; m < 8; m++) known = known && h2f(v[m].y >> 16) > 0.0f;
  if (known) {
    float ch[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float x[8];
#pragma unroll
      for (int m = 0; m < 8; m++) x[m] = h2f(c == 0 ? v[m].x & 0xffffu : c == 1 ? v[m].x >> 16 : v[m].y & 0xffffu);
      ch[c] = trilerp(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], a[0], a[1], a[2]);
    }
    out = quantise(ch[0]) | quantise(ch[1]) << 8 | quantise(ch[2]) << 16 | 0xff000000u;
  }
  return out;
}

__device__ __forceinline__ bool field(const float* __restrict__ vol, const VolumeGeometry& G, float px, float py, float pz, float& F) {
  int i0[3];
  float a[3];
  if (!cell(G, px, py, pz, i0, a)) return false;
  const int64_t sy = 2 * (int64_t)G.dim[0], sz = sy * G.dim[1];
  const float* b = vol + (int64_t)i0[2] * sz + (int64_t)i0[1] * sy + 2 * (int64_t)i0[0];
  const float2 v000 = *reinterpret_cast<const float2*>(b), v100 = *reinterpret_cast<const float2*>(b + 2);
  const float2 v010 = *reinterpret_cast<const float2*>(b + sy), v110 = *reinterpret_cast<const float2*>(b + sy + 2);
  const float2 v001 = *reinterpret_cast<const float2*>(b + sz), v101 = *reinterpret_cast<const float2*>(b + sz + 2);
  const float2 v011 = *reinterpret_cast<const float2*>(b + sz + sy), v111 = *reinterpret_cast<const float2*>(b + sz + sy + 2);
  if (!(v000.y > 0.0f && v100.y > 0.0f && v010.y > 0.0f && v110.y > 0.0f && v001.y > 0.0f && v101.y > 0.0f && v011.y > 0.0f &&
        v111.y > 0.0f))
    return false;
  F = trilerp(v000.x, v100.x, v010.x, v110.x, v001.x, v101.x, v011.x, v111.x, a[0], a[1], a[2]);
  return true;
}

// the normal from the central differences g = F(p + s e) - F(p - s e): g / sqrtf(x*x + y*y + z*z); false (NaN stays) if the length is 0
__device__ __forceinline__ bool unit_normal(float gx, float gy, float gz, float& nx, float& ny, float& nz) {
  const float len = sqrtf(gx * gx + gy * gy + gz * gz);
  if (!(len > 0.0f)) return false;
  nx = gx / len; ny = gy / len; nz = gz / len;
  return true;
}

// THE RAY RULE (V2 of rpe_volume.hip, the map raycast of rpe_frontend.hip), over any field F(x, y, z, value) -> known.  Ray of pixel
// (u, v): xn = ((float)u - cx) / fx, yn likewise; samples z_k = dmin + (float)k * s while z_k < dmax, each the camera point (xn z, yn z, z)
// moved to the world (to_world).  Hit: the first k with F(z_k), F(z_k+1) known, F_k > 0 >= F_k+1: z* = z_k + s * (F_k / (F_k - F_k+1));
// NaN without a hit.  The vertex is to_world(xn z*, yn z*, z*).
template <class Field>
__device__ __forceinline__ float ray_march(Field F, const PoseF& T, float xn, float yn, float s, float dmin, float dmax) {
  float zh = qnan();
  bool prev = false;
  float Fp = 0.0f, zp = 0.0f;
  for (int k = 0;; k++) {
    const float z = dmin + (float)k * s;
    if (!(z < dmax)) break;
    float wx, wy, wz, Fk;
    to_world(T, xn * z, yn * z, z, wx, wy, wz);
    const bool known = F(wx, wy, wz, Fk);
    if (known && prev && Fp > 0.0f && Fk <= 0.0f) { zh = zp + s * (Fp / (Fp - Fk)); break; }
    prev = known; Fp = Fk; zp = z;
  }
  return zh;
}

// the normal at world point (px, py, pz) from the six samples F(p +- s e_axis): unit_normal of their differences; false (NaN stays) also
// if any sample is unknown
template <class Field>
__device__ __forceinline__ bool ray_normal(Field F, float s, float px, float py, float pz, float& nx, float& ny, float& nz) {
  float a, b, c, d, e, f;
  const bool ok = F(px + s, py, pz, a) && F(px - s, py, pz, b) && F(px, py + s, pz, c) && F(px, py - s, pz, d) && F(px, py, pz + s, e) &&
                  F(px, py, pz - s, f);
  return ok && unit_normal(a - b, c - d, e - f, nx, ny, nz);
}

// the model normal of a dense volume at world point (px, py, pz)
__device__ __forceinline__ bool field_normal(const float* __restrict__ vol, const VolumeGeometry& G, float px, float py, float pz,
                                             float& nx, float& ny, float& nz) {
  return ray_normal([&](float x, float y, float z, float& F) { return field(vol, G, x, y, z, F); }, G.s, px, py, pz, nx, ny, nz);
}

// A MAP BRICK'S VOXEL (the map mesh of rpe_mapmesh.hip, the map raycast of rpe_frontend.hip).  The word index of voxel (x, y, z), each
// 0 .. 7, of the brick with source s, in the window's arrays (s >= 0: the window brick bx + nb0 * (by + nb1 * bz); pooled = false) or in the
// pool's planes (s < 0: slot ~s, 8 x 8 x 8 voxels in (z, y, x) order); false, and no address, for a brick index outside the window or a
// slot at or above the capacity.  A voxel is two words in either volume ({tsdf, weight} / four binary16).  View: wnb[3], wdim0, wdim1,
// capacity (MapMeshView, MapRayView)
template <class View>
__device__ __forceinline__ bool brick_word(const View& M, int s, int x, int y, int z, int64_t& w, bool& pooled) {
  pooled = s < 0;
  if (pooled) {
    const int slot = ~s;
    if (slot >= M.capacity) return false;
    w = (int64_t)slot * (kArchiveSlotBytes / 4) + 2 * ((z * 8 + y) * 8 + x);
    return true;
  }
  const unsigned nb0 = (unsigned)M.wnb[0], nb1 = (unsigned)M.wnb[1];
  if ((unsigned)s >= nb0 * nb1 * (unsigned)M.wnb[2]) return false;
  const unsigned bx = (unsigned)s % nb0, t = (unsigned)s / nb0, by = t % nb1, bz = t / nb1;
  const unsigned v = ((bz * 8u + (unsigned)z) * (unsigned)M.wdim1 + by * 8u + (unsigned)y) * (unsigned)M.wdim0 + bx * 8u + (unsigned)x;
  w = 2 * (int64_t)v;   // the voxel index fits 32 bits (dims <= 1024), the word index is formed in 64
  return true;
}

}  // namespace
}  // namespace rpe
