// gfx950 kernels of the MESH EXTRACTION (marching cubes over the TSDF volume, rpe_volume_mesh): the zero level set of the context's
// volume becomes an indexed triangle mesh in device buffers.  The output order is fixed by the conventions, so nothing is placed by
// atomics: every vertex and triangle id comes from scans over chunks of kMeshChunk consecutive voxels.
//
//   M1  mesh_classify_kernel   per cube (named by its corner-0 voxel): the 8-bit case of its tsdf <= 0 corners, 0 unless all 8
//                              corners are known.  A lane owns one cube; the corner loads of a wave are contiguous.
//   M2  mesh_count_kernel      per voxel: the used-edge bits of the (at most 3) edges it owns, from the case bytes of the (at most 7)
//                              cubes around it; per chunk: the vertex and triangle totals.  A workgroup owns a chunk.
//   M3  mesh_scan_kernel       ONE workgroup: exclusive scan of the chunk totals and the two grand totals (the host reads those).
//   M4  mesh_vertex_kernel     per chunk: workgroup scan of the per-voxel vertex counts; vertex positions and normals, and each
//                              used voxel's first vertex id.  Chunks without vertices return at once.
//   M5  mesh_triangle_kernel   per chunk: workgroup scan of the per-cube triangle counts; each table edge resolved to its owner voxel's
//                              first id plus the popcount of the owner's lower used-edge bits.
//
// The conventions (include/rgbd_pose_hip.h Part 3, "Mesh") are followed BIT-EXACTLY (fp32, the written order, no FMA contraction);
// tests/mesh_oracle.py is their numpy statement.  Workspace: 6 bytes per voxel (case, used bits, first id) plus 24 per chunk.
#include "rpe_volume_field.hpp"
#include "rpe_mc_tables.h"
#include "rpe_mc_rules.hpp"
#include "rpe_scan.hpp"

namespace rpe {

namespace {

constexpr int kMeshBlock = 256;
constexpr int kMeshRounds = kMeshChunk / kMeshBlock;   // a workgroup walks its chunk in rounds of one voxel per lane
constexpr int kScanBlock = 1024;

// block_exclusive_scan<NT>(x, lds, total): rpe_scan.hpp, shared with rpe_mapmesh.hip

// ---------------------------------------------------------------------------------------------- M1
// cube (i, j, k), 0 <= i <= d0 - 2 etc.: corner n = di + 2 dj + 4 dk is voxel (i + di, j + dj, k + dk); its case by mc::cube_case
// (rpe_mc_rules.hpp), 0 when the cube does not exist
__device__ __forceinline__ unsigned cube_case(const float* __restrict__ vol, const VolumeGeometry& G, float wmin, unsigned flat, int i,
                                              int j, int k) {
  if (i > G.dim[0] - 2 || j > G.dim[1] - 2 || k > G.dim[2] - 2) return 0u;
  const int64_t sy = 2 * (int64_t)G.dim[0], sz = sy * G.dim[1];
  const float* b = vol + 2 * (int64_t)flat;
  return mc::cube_case([&](int n) { return *reinterpret_cast<const float2*>(b + 2 * (n & 1) + ((n >> 1) & 1) * sy + (n >> 2) * sz); }, wmin);
}

// one cube per lane, so that each of the 8 corner loads of a wave reads 512 contiguous bytes; `padded` = the chunks' voxels: the case
// bytes past the volume are written as 0
// a cube outside the box [B.lo, B.hi) has case 0, as an inactive one: it emits nothing and marks no edge (hi <= dim - 1 keeps the
// box's cubes inside cube_case's own range test)
__global__ __launch_bounds__(kMeshBlock) void mesh_classify_kernel(const float* __restrict__ vol, VolumeGeometry G, float wmin, MeshBox B,
                                                                   unsigned padded, unsigned char* __restrict__ cases) {
  const unsigned flat = blockIdx.x * kMeshBlock + threadIdx.x;
  if (flat >= padded) return;
  const unsigned d0 = (unsigned)G.dim[0], d1 = (unsigned)G.dim[1];
  const int i = (int)(flat % d0), j = (int)((flat / d0) % d1), k = (int)(flat / d0 / d1);
  const bool in_box = i >= B.lo[0] && i < B.hi[0] && j >= B.lo[1] && j < B.hi[1] && k >= B.lo[2] && k < B.hi[2];
  cases[flat] = in_box ? (unsigned char)cube_case(vol, G, wmin, flat, i, j, k) : (unsigned char)0;
}

// ---------------------------------------------------------------------------------------------- M2
// the used-edge bits of voxel (i, j, k) = flat (mc::used_edges) from the case bytes of the cubes around it: cDDD = the case of the cube
// at (i - di, j - dj, k - dk), 0 for a missing one
__device__ __forceinline__ unsigned used_bits(const unsigned char* __restrict__ cs, const VolumeGeometry& G, unsigned flat, int i, int j,
                                              int k) {
  const unsigned d0 = (unsigned)G.dim[0], d01 = d0 * (unsigned)G.dim[1];
  const unsigned c000 = cs[flat];
  const unsigned c100 = i > 0 ? cs[flat - 1] : 0u;
  const unsigned c010 = j > 0 ? cs[flat - d0] : 0u;
  const unsigned c110 = i > 0 && j > 0 ? cs[flat - d0 - 1] : 0u;
  const unsigned c001 = k > 0 ? cs[flat - d01] : 0u;
  const unsigned c101 = i > 0 && k > 0 ? cs[flat - d01 - 1] : 0u;
  const unsigned c011 = j > 0 && k > 0 ? cs[flat - d01 - d0] : 0u;
  return mc::used_edges(c000, c100, c010, c110, c001, c101, c011);
}

__global__ __launch_bounds__(kMeshBlock) void mesh_count_kernel(const unsigned char* __restrict__ cs, VolumeGeometry G, unsigned nvox,
                                                                unsigned char* __restrict__ used, unsigned* __restrict__ chunk_v,
                                                                unsigned* __restrict__ chunk_t) {
  __shared__ unsigned red[2][kMeshBlock / 64];
  const unsigned d0 = (unsigned)G.dim[0], d1 = (unsigned)G.dim[1];
  const unsigned base = blockIdx.x * (unsigned)kMeshChunk;
  unsigned nv = 0, nt = 0;
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned v = base + r * kMeshBlock + threadIdx.x;
    unsigned u = 0;
    if (v < nvox) {
      u = used_bits(cs, G, v, (int)(v % d0), (int)((v / d0) % d1), (int)(v / d0 / d1));
      nt += mc::kTriCount[cs[v]];
    }
    used[v] = (unsigned char)u;
    nv += __popc(u);
  }
  for (int d = 32; d > 0; d >>= 1) { nv += __shfl_down(nv, d, 64); nt += __shfl_down(nt, d, 64); }
  if (threadIdx.x % 64 == 0) { red[0][threadIdx.x / 64] = nv; red[1][threadIdx.x / 64] = nt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = 0, b = 0;
    for (int w = 0; w < kMeshBlock / 64; w++) { a += red[0][w]; b += red[1][w]; }
    chunk_v[blockIdx.x] = a;
    chunk_t[blockIdx.x] = b;
  }
}

// ---------------------------------------------------------------------------------------------- M3
// one workgroup: a lane owns a contiguous run of chunks; off_* = exclusive offsets, totals = {vertices, triangles}
__global__ __launch_bounds__(kScanBlock) void mesh_scan_kernel(const unsigned* __restrict__ chunk_v, const unsigned* __restrict__ chunk_t,
                                                               int nchunks, long long* __restrict__ off_v, long long* __restrict__ off_t,
                                                               long long* __restrict__ totals) {
  __shared__ long long lds[kScanBlock / 64 + 1];
  const int per = (nchunks + kScanBlock - 1) / kScanBlock;
  const int lo = min(nchunks, (int)threadIdx.x * per), hi = min(nchunks, lo + per);
  long long sv = 0, st = 0;
  for (int c = lo; c < hi; c++) { sv += chunk_v[c]; st += chunk_t[c]; }
  long long tv, tt;
  long long rv = block_exclusive_scan<kScanBlock>(sv, lds, tv);
  long long rt = block_exclusive_scan<kScanBlock>(st, lds, tt);
  for (int c = lo; c < hi; c++) {
    off_v[c] = rv; off_t[c] = rt;
    rv += chunk_v[c]; rt += chunk_t[c];
  }
  if (threadIdx.x == 0) { totals[0] = tv; totals[1] = tt; }
}

// ---------------------------------------------------------------------------------------------- M4
// the vertex on a used edge of voxel (i, j, k): mc::edge_vertex (rpe_mc_rules.hpp).  Normal: field_normal (NaN where unknown).
__global__ __launch_bounds__(kMeshBlock) void mesh_vertex_kernel(const float* __restrict__ vol, VolumeGeometry G, unsigned nvox,
                                                                 const unsigned char* __restrict__ used, const unsigned* __restrict__ chunk_v,
                                                                 const long long* __restrict__ off_v, int* __restrict__ first_id,
                                                                 float* __restrict__ vout, float* __restrict__ nout) {
  __shared__ int lds[kMeshBlock / 64 + 1];
  if (chunk_v[blockIdx.x] == 0) return;
  const unsigned d0 = (unsigned)G.dim[0], d1 = (unsigned)G.dim[1];
  const unsigned stride[3] = {1u, d0, d0 * d1};
  const unsigned base = blockIdx.x * (unsigned)kMeshChunk;
  int run = (int)off_v[blockIdx.x];
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned v = base + r * kMeshBlock + threadIdx.x;
    const unsigned u = v < nvox ? used[v] : 0u;
    int total;
    int id = run + block_exclusive_scan<kMeshBlock>((int)__popc(u), lds, total);
    run += total;
    if (!u) continue;
    first_id[v] = id;
    const int ijk[3] = {(int)(v % d0), (int)((v / d0) % d1), (int)(v / d0 / d1)};
    const float Fa = vol[2 * (int64_t)v];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (!((u >> a) & 1u)) continue;
      const float Fb = vol[2 * ((int64_t)v + stride[a])];
      float p[3];
      mc::edge_vertex(G, ijk, a, Fa, Fb, p);
      float nx = qnan(), ny = qnan(), nz = qnan();
      (void)field_normal(vol, G, p[0], p[1], p[2], nx, ny, nz);
      float* o = vout + 3 * (int64_t)id;
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
      float* n = nout + 3 * (int64_t)id;
      n[0] = nx; n[1] = ny; n[2] = nz;
      id++;
    }
  }
}

// ---------------------------------------------------------------------------------------------- M5
// triangles of the cube at voxel v in table order; the vertex of table edge e is on the edge its owner voxel v + kEdgeOwner[e] owns
// along kEdgeAxis[e]: mc::corner_id of the owner's first id and used bits
__global__ __launch_bounds__(kMeshBlock) void mesh_triangle_kernel(const unsigned char* __restrict__ cs, const unsigned char* __restrict__ used,
                                                                   const int* __restrict__ first_id, VolumeGeometry G, unsigned nvox,
                                                                   const unsigned* __restrict__ chunk_t, const long long* __restrict__ off_t,
                                                                   int* __restrict__ tout) {
  __shared__ unsigned lds[kMeshBlock / 64 + 1];
  if (chunk_t[blockIdx.x] == 0) return;
  const unsigned d0 = (unsigned)G.dim[0], d01 = d0 * (unsigned)G.dim[1];
  const unsigned base = blockIdx.x * (unsigned)kMeshChunk;
  long long run = off_t[blockIdx.x];
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned v = base + r * kMeshBlock + threadIdx.x;
    const unsigned c = v < nvox ? cs[v] : 0u;
    const unsigned n = mc::kTriCount[c];
    unsigned total;
    const long long t0 = run + block_exclusive_scan<kMeshBlock>(n, lds, total);
    run += total;
    for (unsigned q = 0; q < 3 * n; q++) {
      const unsigned e = mc::kTriEdges[c][q];
      const unsigned o = mc::kEdgeOwner[e], axis = mc::kEdgeAxis[e];
      const unsigned owner = v + (o & 1u) + ((o >> 1) & 1u) * d0 + (o >> 2) * d01;
      tout[3 * t0 + q] = mc::corner_id(first_id[owner], used[owner], axis);
    }
  }
}

}  // namespace

size_t mesh_workspace_bytes(int64_t nvox) {
  const int64_t chunks = (nvox + kMeshChunk - 1) / kMeshChunk;
  return (size_t)chunks * kMeshChunk * 6 + (size_t)chunks * 24 + 16;
}

MeshWorkspace mesh_workspace(void* ws, int64_t nvox) {
  MeshWorkspace W;
  W.chunks = (int)((nvox + kMeshChunk - 1) / kMeshChunk);
  const size_t P = (size_t)W.chunks * kMeshChunk;
  char* p = static_cast<char*>(ws);
  W.first = reinterpret_cast<int*>(p); p += 4 * P;
  W.off_v = reinterpret_cast<long long*>(p); p += 8 * (size_t)W.chunks;
  W.off_t = reinterpret_cast<long long*>(p); p += 8 * (size_t)W.chunks;
  W.totals = reinterpret_cast<long long*>(p); p += 16;
  W.chunk_v = reinterpret_cast<unsigned*>(p); p += 4 * (size_t)W.chunks;
  W.chunk_t = reinterpret_cast<unsigned*>(p); p += 4 * (size_t)W.chunks;
  W.cases = reinterpret_cast<unsigned char*>(p); p += P;
  W.used = reinterpret_cast<unsigned char*>(p);
  return W;
}

hipError_t launch_mesh_count(const float* vol, const VolumeGeometry& G, float wmin, const MeshBox& B, const MeshWorkspace& W,
                             hipStream_t s) {
  const unsigned nvox = (unsigned)((int64_t)G.dim[0] * G.dim[1] * G.dim[2]), padded = (unsigned)W.chunks * kMeshChunk;
  hipLaunchKernelGGL(mesh_classify_kernel, dim3(padded / kMeshBlock), dim3(kMeshBlock), 0, s, vol, G, wmin, B, padded, W.cases);
  hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)W.chunks), dim3(kMeshBlock), 0, s, W.cases, G, nvox, W.used, W.chunk_v, W.chunk_t);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, W.chunk_v, W.chunk_t, W.chunks, W.off_v, W.off_t, W.totals);
  return hipGetLastError();
}

hipError_t launch_mesh_emit(const float* vol, const VolumeGeometry& G, const MeshWorkspace& W, float* vertices, float* normals,
                            int* triangles, hipStream_t s) {
  const unsigned nvox = (unsigned)((int64_t)G.dim[0] * G.dim[1] * G.dim[2]);
  hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)W.chunks), dim3(kMeshBlock), 0, s, vol, G, nvox, W.used, W.chunk_v, W.off_v,
                     W.first, vertices, normals);
  hipLaunchKernelGGL(mesh_triangle_kernel, dim3((unsigned)W.chunks), dim3(kMeshBlock), 0, s, W.cases, W.used, W.first, G, nvox, W.chunk_t,
                     W.off_t, triangles);
  return hipGetLastError();
}

RPE_PRELOAD(mesh_classify_kernel);

}  // namespace rpe
