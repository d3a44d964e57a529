// gfx950 kernels of the MAP MESH (include/rgbd_pose_hip.h Part 3, "Map mesh"; host side in rpe_mapmesh_api.hip): marching cubes over
// the map -- the window plus the archived bricks -- inside a box of world voxels, bit for bit the mesh rpe_volume_mesh (rpe_mesh.hip)
// gives on a dense volume of the box with the map's content, in brick order.  Only the LISTED bricks are visited (rpe_kernels.h
// MapMeshView: the host lists the window's and the held bricks that lie in the box, ascending by (bz, by, bx), with each brick's 27
// neighbours as list positions); a brick that is not listed is {0, 0} everywhere: weight 0, unknown.  Nothing is placed by atomics.
//
//   P1  map_count_kernel     one workgroup per listed brick.  The brick and its halo are staged from the window's rows or the pool's
//                            slots into LDS through the neighbour table, zeros for an absent neighbour; the cases of the 9^3 cubes at
//                            local -1 .. 7, the used-edge bits of the brick's 512 voxels and its two totals come from LDS.
//   P2  map_scan_kernel      ONE workgroup: exclusive scan of the brick totals, the two grand totals (the host reads those).
//   P3  map_vertex_kernel    per brick with vertices: staged again, to the full reach below; positions, normals and each used
//                            voxel's first id (voxels in (z, y, x) order inside the brick, then axis x < y < z).
//   P3c map_colour_kernel    per brick with vertices, when the map has a colour source: C(p) at each of them.
//   P4  map_triangle_kernel  per brick with triangles: table order per cube; an owner voxel at local 8 belongs to the next brick and
//                            its first id and used bits are read from that brick's workspace through the neighbour table.
//
// EARLY EXIT (P1).  A workgroup whose own 512 voxels have no weight >= wmin emits nothing and leaves before it stages anything: every
// cube this brick emits triangles for (corner 0 at local 0 .. 7) and every cube that can mark an edge one of its voxels owns (the edge
// starts AT that voxel) has a voxel of the brick as a corner, so with none of them known all those cubes are inactive.  The window's
// bricks therefore need no occupancy pass.
//
// THE REACH of a brick, per axis, in local voxel indices (0 .. 7 its own):
//   cases      a cube at local 7 has corners at local 8; the used bits of a voxel at local 0 look at the cubes at local -1: -1 .. 8.
//   vertices   the edge of an own voxel ends at local 8 at most.
//   normals    a vertex of voxel i lies at g = i + t along its edge (g = (p - o) / s - 0.5f, t in [0, 1]) and at g = i across it.  The
//              six samples p +- s e have g in [i - 1, i + 2] exactly, i0 = floorf(g) in i - 1 .. i + 2, corners i0, i0 + 1 in
//              i - 1 .. i + 3.  But t is exactly 0 or 1 when a corner's tsdf is 0 and the sample then sits ON an integer g: the fp32
//              rounding of (p +- s - o) / s - 0.5f can land just below it, so i0 = i - 2 happens (corners from i - 2).  With i in
//              0 .. 7: local -2 .. +10, not -1 .. +9.
//   colours    C(p) at the vertex itself: within the normals' reach.
// That much is staged (13^3 voxels; x in whole 16-byte pairs, so 14 x 13 x 13 = 18.5 KB).  It holds while |o| / s stays small against
// 2^23; for a far origin one ulp of p is a good part of a voxel and a sample can land anywhere.  So NO sample is assumed to stay
// inside: field() tests the staged region and takes everything else from global memory, a corner in one of the 26 neighbours through
// the table, any other by a binary search of the sorted keys.  The field's in-range test is the BOX's (0 <= i0 <= dim - 2 in box
// indices), never the brick's.  The colour field is not staged at all: a brick has few vertices, each takes its eight 8-byte corners
// from global memory as C3 of rpe_color.hip does, through the same table.
//
// WORKSPACE: the case and used bytes of P1 are KEPT (1 KB per listed brick) rather than recomputed: P4 then needs no voxel at all, and
// P3 stages only the bricks that have a vertex.  With the first ids and the counts 3 KB + 40 B per listed brick; nothing scales with
// the box.  No address is formed for an absent neighbour, a slot at or above the capacity or a brick index outside the window.
#include "rpe_volume_field.hpp"
#include "rpe_mc_tables.h"
#include "rpe_mc_rules.hpp"
#include "rpe_scan.hpp"

namespace rpe {

#pragma clang fp contract(off)

namespace {

constexpr int kMapBlock = 256;
constexpr int kMapScanBlock = 1024;
constexpr int kBrickVox = 512;
constexpr int kStY = 13, kStX = 14;                  // staged: local -2 .. 10 on y and z, -2 .. 11 on x
constexpr int kStVox = kStY * kStY * kStX;
constexpr int kCases = 9 * 9 * 9;                    // cubes at local -1 .. 7
constexpr unsigned long long kKeyMask = (1ull << kMapKeyBits) - 1ull;

__device__ __forceinline__ int stage_index(int lx, int ly, int lz) { return ((lz + 2) * kStY + (ly + 2)) * kStX + (lx + 2); }
__device__ __forceinline__ int case_index(int lx, int ly, int lz) { return ((lz + 1) * 9 + (ly + 1)) * 9 + (lx + 1); }

// where voxel (x, y, z) of the brick with source s lies: brick_word (rpe_volume_field.hpp, shared with the map raycast)

// one voxel (8 bytes) of a listed brick's tsdf (COLOUR = false) or colour volume
template <bool COLOUR>
__device__ __forceinline__ uint2 brick_voxel(const MapMeshView& M, int s, int x, int y, int z) {
  int64_t w;
  bool pooled;
  if (!brick_word(M, s, x, y, z, w, pooled)) return make_uint2(0u, 0u);
  const unsigned int* p = pooled ? (COLOUR ? M.cpool : M.pool) : (COLOUR ? M.cvol : M.vol);
  return p ? *reinterpret_cast<const uint2*>(p + w) : make_uint2(0u, 0u);
}

// The voxel at BOX index (ix, iy, iz), inside the box, seen from the brick at box brick (ob[0], ob[1], ob[2]) whose table is in
// s_pos / s_src: its own and its 26 neighbours through the table, anything further by the sorted keys
template <bool COLOUR>
__device__ __forceinline__ uint2 map_voxel(const MapMeshView& M, const int* s_pos, const int* s_src, const int ob[3], int ix, int iy, int iz) {
  const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3;
  const int dx = bx - ob[0], dy = by - ob[1], dz = bz - ob[2];
  int s;
  if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && dz >= -1 && dz <= 1) {
    const int e = (dz + 1) * 9 + (dy + 1) * 3 + dx + 1;
    if (s_pos[e] < 0) return make_uint2(0u, 0u);
    s = s_src[e];
  } else {
    const unsigned long long k = (unsigned long long)bz << (2 * kMapKeyBits) | (unsigned long long)by << kMapKeyBits | (unsigned long long)bx;
    int lo = 0, hi = M.n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (M.key[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo >= M.n || M.key[lo] != k) return make_uint2(0u, 0u);
    s = M.src[lo];
  }
  return brick_voxel<COLOUR>(M, s, ix & 7, iy & 7, iz & 7);
}

// the brick's table into LDS: list positions (-1 = absent) and the sources behind them
__device__ __forceinline__ void load_table(const MapMeshView& M, int pos, int* s_pos, int* s_src) {
  if (threadIdx.x < 27) {
    const int p = M.nbr[(int64_t)pos * 27 + threadIdx.x];
    const bool there = p >= 0 && p < M.n;
    s_pos[threadIdx.x] = there ? p : -1;
    s_src[threadIdx.x] = there ? M.src[p] : 0;
  }
}

// Stage rows (ly, lz) in [R0, R1]^2, NCX 16-byte pairs of voxels each from local x = -2, into st.  A pair never straddles two bricks
// (x is even) and is 16-byte aligned in the window (dim0 is a multiple of 8) and in a slot.
template <int R0, int R1, int NCX>
__device__ __forceinline__ void stage(const MapMeshView& M, const int* s_pos, const int* s_src, uint2* st) {
  constexpr int NR = R1 - R0 + 1, TOTAL = NR * NR * NCX;
  for (int c = (int)threadIdx.x; c < TOTAL; c += kMapBlock) {
    const int cx = c % NCX, r = c / NCX, ly = R0 + r % NR, lz = R0 + r / NR, lx = -2 + 2 * cx;
    const int dx = lx < 0 ? -1 : lx > 7 ? 1 : 0, dy = ly < 0 ? -1 : ly > 7 ? 1 : 0, dz = lz < 0 ? -1 : lz > 7 ? 1 : 0;
    const int e = (dz + 1) * 9 + (dy + 1) * 3 + dx + 1;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    int64_t w;
    bool pooled;
    if (s_pos[e] >= 0 && brick_word(M, s_src[e], lx & 7, ly & 7, lz & 7, w, pooled)) {
      const unsigned int* p = pooled ? M.pool : M.vol;
      v = *reinterpret_cast<const uint4*>(p + w);
    }
    *reinterpret_cast<uint4*>(st + stage_index(lx, ly, lz)) = v;
  }
}

// ---------------------------------------------------------------------------------------------- P1
__global__ __launch_bounds__(kMapBlock) void map_count_kernel(MapMeshView M, float wmin, MapMeshWorkspace W) {
  __shared__ __align__(16) uint2 st[kStVox];
  __shared__ unsigned char cs[kCases];
  __shared__ int s_pos[27], s_src[27];
  __shared__ unsigned red[2][kMapBlock / 64];
  const int pos = (int)blockIdx.x, t = (int)threadIdx.x;
  {   // the early exit (header): the lane's two own voxels, chunk t of the brick as rpe_archive.hip numbers them
    const int row = t >> 2;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    int64_t w;
    bool pooled;
    if (brick_word(M, M.src[pos], 2 * (t & 3), row & 7, row >> 3, w, pooled)) q = *reinterpret_cast<const uint4*>((pooled ? M.pool : M.vol) + w);
    const int some = __uint_as_float(q.y) >= wmin || __uint_as_float(q.w) >= wmin;
    if (!__syncthreads_or(some)) {
      if (t == 0) { W.brick_v[pos] = 0u; W.brick_t[pos] = 0u; }
      return;
    }
  }
  load_table(M, pos, s_pos, s_src);
  __syncthreads();
  stage<-1, 8, 6>(M, s_pos, s_src, st);   // x: -2 .. 9
  __syncthreads();
  // cube at local (x, y, z) in -1 .. 7: corner n = di + 2 dj + 4 dk from the staged region, its case by mc::cube_case (rpe_mc_rules.hpp).
  // A cube that reaches outside the box has an absent corner: weight 0, inactive
  for (int c = t; c < kCases; c += kMapBlock) {
    const int x = c % 9 - 1, y = (c / 9) % 9 - 1, z = c / 81 - 1;
    cs[c] = (unsigned char)mc::cube_case([&](int n) {
      const uint2 v = st[stage_index(x + (n & 1), y + ((n >> 1) & 1), z + (n >> 2))];
      return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
    }, wmin);
  }
  __syncthreads();
  unsigned nv = 0, nt = 0;
#pragma unroll
  for (int r = 0; r < kBrickVox / kMapBlock; r++) {
    const int v = r * kMapBlock + t, x = v & 7, y = (v >> 3) & 7, z = v >> 6;
    // cDDD = the case of the cube at (x - di, y - dj, z - dk)
    const unsigned c000 = cs[case_index(x, y, z)], c100 = cs[case_index(x - 1, y, z)], c010 = cs[case_index(x, y - 1, z)];
    const unsigned c110 = cs[case_index(x - 1, y - 1, z)], c001 = cs[case_index(x, y, z - 1)], c101 = cs[case_index(x - 1, y, z - 1)];
    const unsigned c011 = cs[case_index(x, y - 1, z - 1)];
    const unsigned u = mc::used_edges(c000, c100, c010, c110, c001, c101, c011);
    W.cases[(int64_t)pos * kBrickVox + v] = (unsigned char)c000;
    W.used[(int64_t)pos * kBrickVox + v] = (unsigned char)u;
    nv += __popc(u);
    nt += mc::kTriCount[c000];
  }
  for (int d = 32; d > 0; d >>= 1) { nv += __shfl_down(nv, d, 64); nt += __shfl_down(nt, d, 64); }
  if (t % 64 == 0) { red[0][t / 64] = nv; red[1][t / 64] = nt; }
  __syncthreads();
  if (t == 0) {
    unsigned a = 0, b = 0;
    for (int w = 0; w < kMapBlock / 64; w++) { a += red[0][w]; b += red[1][w]; }
    W.brick_v[pos] = a;
    W.brick_t[pos] = b;
  }
}

// ---------------------------------------------------------------------------------------------- P2
// one workgroup walks the bricks in tiles of 4 per lane (a lane's four are consecutive, so a wave reads 1 KB in one piece): two
// workgroup scans per tile; off_* = exclusive offsets, totals = {vertices, triangles}
__global__ __launch_bounds__(kMapScanBlock) void map_scan_kernel(int n, MapMeshWorkspace W) {
  __shared__ long long lds[kMapScanBlock / 64 + 1];
  long long run_v = 0, run_t = 0;
  for (int base = 0; base < n; base += 4 * kMapScanBlock) {
    const int first = base + 4 * (int)threadIdx.x;
    unsigned v[4], t[4];
    long long sv = 0, st = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] = first + k < n ? W.brick_v[first + k] : 0u;
      t[k] = first + k < n ? W.brick_t[first + k] : 0u;
      sv += v[k]; st += t[k];
    }
    long long tv, tt;
    long long rv = run_v + block_exclusive_scan<kMapScanBlock>(sv, lds, tv);
    long long rt = run_t + block_exclusive_scan<kMapScanBlock>(st, lds, tt);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (first + k < n) { W.off_v[first + k] = rv; W.off_t[first + k] = rt; }
      rv += v[k]; rt += t[k];
    }
    run_v += tv; run_t += tt;
  }
  if (threadIdx.x == 0) { W.totals[0] = run_v; W.totals[1] = run_t; }
}

// ---------------------------------------------------------------------------------------------- P3
// ---- the two fields
// The trilinear value of NCH channels in F's lerp chain (trilerp of rpe_volume_field.hpp: along x for (dj, dk) = (0,0) (1,0) (0,1)
// (1,1), then bilerp along y and z) with the corners taken a pair at a time: corner(di, dj, dk, x) gives a corner's channels and whether its weight is > 0.  The loop is
// NOT unrolled: a corner may come from global memory through the table or a search of the keys (map_voxel), and eight copies of that
// per sample cost more scalar registers than the kernel has
template <int NCH, class Corner>
__device__ __forceinline__ bool trilinear(Corner corner, const float a[3], float out[NCH]) {
  bool known = true;
  float x00[NCH], x10[NCH], x01[NCH], x11[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) x00[c] = x10[c] = x01[c] = x11[c] = 0.0f;
#pragma unroll 1
  for (int jk = 0; jk < 4; jk++) {
    float p[NCH], q[NCH];
    const bool kp = corner(0, jk & 1, jk >> 1, p), kq = corner(1, jk & 1, jk >> 1, q);
    known = known && kp && kq;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      const float x = lerp(p[c], q[c], a[0]);
      if (jk == 0) x00[c] = x; else if (jk == 1) x10[c] = x; else if (jk == 2) x01[c] = x; else x11[c] = x;
    }
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) out[c] = bilerp(x00[c], x10[c], x01[c], x11[c], a[1], a[2]);
  return known;
}

// F(p) of the box's virtual volume (rpe_volume_field.hpp field, bit for bit; the cell is the BOX's): the eight corners from the staged region where they
// all lie in it, from global memory otherwise
__device__ __forceinline__ bool map_field(const uint2* st, const MapMeshView& M, const int* s_pos, const int* s_src,
                                          const VolumeGeometry& G, const int ob[3], float px, float py, float pz, float& F) {
  int i0[3];
  float a[3];
  if (!cell(G, px, py, pz, i0, a)) return false;
  const int lx = i0[0] - 8 * ob[0], ly = i0[1] - 8 * ob[1], lz = i0[2] - 8 * ob[2];
  const bool staged = lx >= -2 && lx <= 9 && ly >= -2 && ly <= 9 && lz >= -2 && lz <= 9;
  float out[1];
  const bool known = trilinear<1>([&](int di, int dj, int dk, float x[1]) {
    const uint2 v = staged ? st[stage_index(lx + di, ly + dj, lz + dk)] : map_voxel<false>(M, s_pos, s_src, ob, i0[0] + di, i0[1] + dj, i0[2] + dk);
    x[0] = __uint_as_float(v.x);
    return __uint_as_float(v.y) > 0.0f;
  }, a, out);
  F = out[0];
  return known;
}

// C(p) of the box's virtual colour volume as RGBA8 (rpe_color.hip C3, bit for bit)
__device__ __forceinline__ unsigned map_colour(const MapMeshView& M, const int* s_pos, const int* s_src, const VolumeGeometry& G,
                                               const int ob[3], float px, float py, float pz) {
  int i0[3];
  float a[3];
  if (!cell(G, px, py, pz, i0, a)) return 0u;
  float ch[3];
  const bool known = trilinear<3>([&](int di, int dj, int dk, float x[3]) {
    const uint2 v = map_voxel<true>(M, s_pos, s_src, ob, i0[0] + di, i0[1] + dj, i0[2] + dk);
    x[0] = h2f(v.x & 0xffffu); x[1] = h2f(v.x >> 16); x[2] = h2f(v.y & 0xffffu);
    return h2f(v.y >> 16) > 0.0f;
  }, a, ch);
  if (!known) return 0u;
  return quantise(ch[0]) | quantise(ch[1]) << 8 | quantise(ch[2]) << 16 | 0xff000000u;
}

// the vertex on a used edge of a voxel: mc::edge_vertex (rpe_mc_rules.hpp) with the voxel's index INSIDE THE BOX.  Normal:
// field_normal's six samples on map_field and its finish, unit_normal (NaN where unknown)
__global__ __launch_bounds__(kMapBlock) void map_vertex_kernel(MapMeshView M, VolumeGeometry G, MapMeshWorkspace W, float* __restrict__ vout,
                                                               float* __restrict__ nout) {
  __shared__ __align__(16) uint2 st[kStVox];
  __shared__ int s_pos[27], s_src[27];
  __shared__ int lds[kMapBlock / 64 + 1];
  const int pos = (int)blockIdx.x, t = (int)threadIdx.x;
  if (W.brick_v[pos] == 0u) return;
  load_table(M, pos, s_pos, s_src);
  __syncthreads();
  stage<-2, 10, 7>(M, s_pos, s_src, st);   // x: -2 .. 11
  __syncthreads();
  const unsigned long long key = M.key[pos];
  const int ob[3] = {(int)(key & kKeyMask), (int)((key >> kMapKeyBits) & kKeyMask), (int)(key >> (2 * kMapKeyBits))};
  int run = (int)W.off_v[pos];
  for (int r = 0; r < kBrickVox / kMapBlock; r++) {
    const int v = r * kMapBlock + t;
    const unsigned u = W.used[(int64_t)pos * kBrickVox + v];
    int total;
    int id = run + block_exclusive_scan<kMapBlock>((int)__popc(u), lds, total);
    run += total;
    if (!u) continue;
    W.first[(int64_t)pos * kBrickVox + v] = id;
    const int l[3] = {v & 7, (v >> 3) & 7, v >> 6};
    const int ijk[3] = {8 * ob[0] + l[0], 8 * ob[1] + l[1], 8 * ob[2] + l[2]};
    const float Fa = __uint_as_float(st[stage_index(l[0], l[1], l[2])].x);
#pragma unroll 1
    for (int a = 0; a < 3; a++) {
      if (!((u >> a) & 1u)) continue;
      const float Fb = __uint_as_float(st[stage_index(l[0] + (a == 0), l[1] + (a == 1), l[2] + (a == 2))].x);
      float p[3];
      mc::edge_vertex(G, ijk, a, Fa, Fb, p);
      // field_normal's differences, an axis per turn: F(p + s e) - F(p - s e)
      float g[3] = {0.0f, 0.0f, 0.0f};
      bool ok = true;
#pragma unroll 1
      for (int q = 0; q < 3; q++) {
        float fp = 0.0f, fm = 0.0f;
        const float px = q == 0 ? p[0] + G.s : p[0], py = q == 1 ? p[1] + G.s : p[1], pz = q == 2 ? p[2] + G.s : p[2];
        const float mx = q == 0 ? p[0] - G.s : p[0], my = q == 1 ? p[1] - G.s : p[1], mz = q == 2 ? p[2] - G.s : p[2];
        const bool kp = map_field(st, M, s_pos, s_src, G, ob, px, py, pz, fp), km = map_field(st, M, s_pos, s_src, G, ob, mx, my, mz, fm);
        ok = ok && kp && km;
        const float d = fp - fm;
        if (q == 0) g[0] = d; else if (q == 1) g[1] = d; else g[2] = d;
      }
      float nx = qnan(), ny = qnan(), nz = qnan();
      if (ok) (void)unit_normal(g[0], g[1], g[2], nx, ny, nz);
      float* o = vout + 3 * (int64_t)id;
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
      float* n = nout + 3 * (int64_t)id;
      n[0] = nx; n[1] = ny; n[2] = nz;
      id++;
    }
  }
}

// P3c, only with a colour source: C(p) at the brick's vertices, a lane per vertex.  A pass of its own -- the positions are read back
// from the vertex buffer -- because inside P3 the two colour planes' pointers are the scalar registers the kernel does not have
__global__ __launch_bounds__(kMapBlock) void map_colour_kernel(MapMeshView M, VolumeGeometry G, MapMeshWorkspace W, const float* __restrict__ vin,
                                                               unsigned int* __restrict__ cout) {
  __shared__ int s_pos[27], s_src[27];
  const int pos = (int)blockIdx.x;
  const unsigned nv = W.brick_v[pos];
  if (nv == 0u) return;
  load_table(M, pos, s_pos, s_src);
  __syncthreads();
  const unsigned long long key = M.key[pos];
  const int ob[3] = {(int)(key & kKeyMask), (int)((key >> kMapKeyBits) & kKeyMask), (int)(key >> (2 * kMapKeyBits))};
  const long long first = W.off_v[pos];
  for (unsigned k = threadIdx.x; k < nv; k += kMapBlock) {
    const float* p = vin + 3 * (first + k);
    cout[first + k] = map_colour(M, s_pos, s_src, G, ob, p[0], p[1], p[2]);
  }
}

// ---------------------------------------------------------------------------------------------- P4
// triangles of the cube at voxel v of the brick, in table order; the vertex of table edge e is on the edge its owner voxel
// v + kEdgeOwner[e] owns along kEdgeAxis[e]: mc::corner_id of the owner's first id and used bits.  An owner at local 8 is a voxel of
// the neighbour brick; the cube is active, so that voxel is known, its brick is listed and P1 / P3 wrote its bytes and its id
__global__ __launch_bounds__(kMapBlock) void map_triangle_kernel(MapMeshView M, MapMeshWorkspace W, int* __restrict__ tout) {
  __shared__ unsigned lds[kMapBlock / 64 + 1];
  __shared__ int s_pos[27], s_src[27];
  const int pos = (int)blockIdx.x, t = (int)threadIdx.x;
  if (W.brick_t[pos] == 0u) return;
  load_table(M, pos, s_pos, s_src);
  __syncthreads();
  long long run = W.off_t[pos];
  for (int r = 0; r < kBrickVox / kMapBlock; r++) {
    const int v = r * kMapBlock + t, x = v & 7, y = (v >> 3) & 7, z = v >> 6;
    const unsigned c = W.cases[(int64_t)pos * kBrickVox + v];
    const unsigned n = mc::kTriCount[c];
    unsigned total;
    const long long t0 = run + block_exclusive_scan<kMapBlock>(n, lds, total);
    run += total;
    for (unsigned q = 0; q < 3 * n; q++) {
      const unsigned e = mc::kTriEdges[c][q];
      const unsigned o = mc::kEdgeOwner[e], axis = mc::kEdgeAxis[e];
      const int ox = x + (int)(o & 1u), oy = y + (int)((o >> 1) & 1u), oz = z + (int)(o >> 2);
      const int p = s_pos[((oz >> 3) + 1) * 9 + ((oy >> 3) + 1) * 3 + (ox >> 3) + 1];
      int id = 0;
      if (p >= 0) {
        const int64_t w = (int64_t)p * kBrickVox + ((oz & 7) * 8 + (oy & 7)) * 8 + (ox & 7);
        id = mc::corner_id(W.first[w], W.used[w], axis);
      }
      tout[3 * t0 + q] = id;
    }
  }
}

}  // namespace

size_t map_mesh_workspace_bytes(int64_t bricks) { return (size_t)bricks * (kBrickVox * 6 + 24) + 16; }

MapMeshWorkspace map_mesh_workspace(void* ws, int64_t bricks) {
  MapMeshWorkspace W;
  const size_t n = (size_t)bricks;
  char* p = static_cast<char*>(ws);
  W.totals = reinterpret_cast<long long*>(p); p += 16;
  W.off_v = reinterpret_cast<long long*>(p); p += 8 * n;
  W.off_t = reinterpret_cast<long long*>(p); p += 8 * n;
  W.first = reinterpret_cast<int*>(p); p += 4 * n * kBrickVox;
  W.brick_v = reinterpret_cast<unsigned*>(p); p += 4 * n;
  W.brick_t = reinterpret_cast<unsigned*>(p); p += 4 * n;
  W.cases = reinterpret_cast<unsigned char*>(p); p += n * kBrickVox;
  W.used = reinterpret_cast<unsigned char*>(p);
  return W;
}

hipError_t launch_map_mesh_count(const MapMeshView& M, float wmin, const MapMeshWorkspace& W, hipStream_t s) {
  if (M.n > 0) hipLaunchKernelGGL(map_count_kernel, dim3((unsigned)M.n), dim3(kMapBlock), 0, s, M, wmin, W);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(kMapScanBlock), 0, s, M.n, W);
  return hipGetLastError();
}

hipError_t launch_map_mesh_emit(const MapMeshView& M, const VolumeGeometry& G, const MapMeshWorkspace& W, float* vertices, float* normals,
                                int* triangles, unsigned int* colours, hipStream_t s) {
  if (M.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(map_vertex_kernel, dim3((unsigned)M.n), dim3(kMapBlock), 0, s, M, G, W, vertices, normals);
  if (colours) hipLaunchKernelGGL(map_colour_kernel, dim3((unsigned)M.n), dim3(kMapBlock), 0, s, M, G, W, vertices, colours);
  hipLaunchKernelGGL(map_triangle_kernel, dim3((unsigned)M.n), dim3(kMapBlock), 0, s, M, W, triangles);
  return hipGetLastError();
}

RPE_PRELOAD(map_count_kernel);

}  // namespace rpe
