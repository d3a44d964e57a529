// THE MAP VOLUME COLOUR TERM (include/rgbd_pose_hip.h Part 3, "Map volume colour term"; tests/mapsdf_photo_oracle.py is its numpy
// statement; included by rpe_sdf_photo.hpp at its end, so compiled into rpe_frontend.hip behind the volume colour term): the volume colour term on the virtual volume of a box of the
// map -- the window plus the archived bricks.  No new arithmetic: the photometric rule is sdf_photo_pixel / sdf_photo_row of
// rpe_sdf_photo.hpp, the geometric rule rpe_sdf_rule.hpp's, and both corner sets come through the brick grid of the map raycast
// (grid_at / map_voxel / map_corners<COLOUR> of rpe_frontend.hip), so the rows are bit for bit sdf_photo_rows_kernel's on a dense copy
// of the box and its colour.  The virtual COLOUR volume holds the window's colour bits where the window covers a voxel, the held
// brick's colour plane where the archive holds one, {0, 0} elsewhere -- a brick held without a colour plane and a pool without colour
// (cpool null) included; the window is addressed by position, never through its grid entry: what map_colour reads.
//
//   map_sdf_photo_rows_kernel        sdf_photo_rows_kernel with the map fetch for both corner sets.
//   icp_map_sdf_photo_kernel<GEO, BLK>  one Gauss-Newton round in ONE launch, ONE pixel per loop trip, the record icp_sdf_photo_kernel's.
//                                    The colour corners are fetched BEHIND the TSDF corners' own gates (sdf_photo_gate: a weight > 0 and |tsdf| < 1 at all
//                                    eight, the distance gate): a pixel whose TSDF corners give no row needs no colour, and zeros in their place fail the
//                                    colour-weight test, so the result is the same bits.  With GEO the geometric row is formed and summed
//                                    in front of the colour fetch, so of the TSDF corners one flag crosses it.
#pragma once

namespace rpe {
namespace {

// what both fetches read of a MapRayView: MapSdfView and the two colour sources (null: none)
struct MapSdfPhotoView {
  MapSdfView S;
  const unsigned int *cvol, *cpool;
};
__device__ __forceinline__ MapRayView ray_view(const MapSdfPhotoView& P) {
  MapRayView M = ray_view(P.S);
  M.cvol = P.cvol; M.cpool = P.cpool;
  return M;
}

// The eight colour corners of the cell i0 of the virtual colour volume (i0 inside the box, i0 + 1 too: sdf_cell), as map_colour reads
// them: the window by position, a held brick through the grid, zeros elsewhere.  No address is formed outside the window's arrays or
// the pool's capacity (map_voxel)
struct map_colour_corners {
  const MapRayView& M;
  __device__ __forceinline__ bool operator()(const int (&i0)[3], uint2 (&c)[8]) const {
    map_corners<true>(M, i0, grid_at(M, i0[0], i0[1], i0[2]), c);
    return true;
  }
};

// The round kernel's arguments as the kernarg segment lays them out, for late_finish_at and map_photo_late_pose
struct MapSdfPhotoRoundArgs {
  const float* vmap; const float* nmap; const float* fint; int64_t n; MapSdfPhotoView P; VolumeGeometry G; SdfParams Q; float lam; PoseF T;
  Finish fin;
};
// (tests/test_mapsdf_photo_oracle.py reads the same offsets and sizes from the code object's metadata)
static_assert(offsetof(MapSdfPhotoRoundArgs, fin) == 216 && sizeof(Finish) == 136, "late_finish_at: where the kernarg segment holds the reduction's argument");
static_assert(offsetof(MapSdfPhotoRoundArgs, T) == 168 && sizeof(PoseF) == 48, "map_photo_late_pose: where the kernarg segment holds the pose");
static_assert(offsetof(MapSdfPhotoRoundArgs, P) == 32 && sizeof(MapSdfPhotoView) == 80, "map_photo_late_view: where the kernarg segment holds the view");

// late_pose_at (rpe_frontend.hip) for this kernel, as late_pose and photo_late_pose and for their reason: view, geometry, gates, seven
// pointers and the exec masks of the fetches' nested branches leave no room for twelve more scalars through the whole loop
__device__ __forceinline__ PoseF map_photo_late_pose() { return late_pose_at((unsigned)offsetof(MapSdfPhotoRoundArgs, T)); }

// The view read the same way in front of each of the two fetches: its 24 scalars are then live through one fetch, not through the loop
__device__ __forceinline__ MapRayView map_photo_late_view() {
  unsigned off = (unsigned)offsetof(MapSdfPhotoRoundArgs, P);
  asm volatile("" : "+s"(off));
  MapSdfPhotoView P;
  __builtin_memcpy(&P, (const char*)__builtin_amdgcn_kernarg_segment_ptr() + off, sizeof(MapSdfPhotoView));
  return ray_view(P);
}

template <bool GEO, int BLK>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(GEO ? 2 : 4))) void icp_map_sdf_photo_kernel(
    const float* __restrict__ vmap, const float* __restrict__ nmap, const float* __restrict__ fint, int64_t n,
    MapSdfPhotoView /* read by map_photo_late_view */, VolumeGeometry G, SdfParams Q, float lam, PoseF /* read by map_photo_late_pose */,
    Finish /* read by late_finish_at */) {
  double acc[29];   // 0 .. 26 H | g of both terms, 27 the geometric cost, 28 the photometric cost
#pragma unroll
  for (int k = 0; k < 29; k++) acc[k] = 0.0;
  float grows = 0.f, prows = 0.f;
  const int stride = (int)gridDim.x * BLK;
  for (int i = (int)blockIdx.x * BLK + (int)threadIdx.x; i < (int)n; i += stride) {   // (n <= 2^28 pixels: rpe_frame_set_depth)
    const int64_t q = 3 * (int64_t)i;
    const float x = vmap[q], y = vmap[q + 1], z = vmap[q + 2];
    int i0[3];
    float a[3], r, J[6];
    bool past;
    {
      float2 v[8];
      const bool in = sdf_cell(G, map_photo_late_pose(), x, y, z, i0, a);
      const MapRayView M = map_photo_late_view();
      const bool have = map_sdf_corners{M}(i0, v) && in;
      if (GEO) {
        // the geometric row first, icp_map_sdf_kernel's trip: what the photometric row asks of the TSDF corners is then one flag
        float len;
        bool ok = sdf_row(v, a, G, map_photo_late_pose(), Q, x, y, z, r, J, len) && have;
        if (ok && Q.use_normals) ok = sdf_normal_gate(Q, nmap[q], nmap[q + 1], nmap[q + 2], len, r, J);
        if (!ok) {
          r = 0.f;
#pragma unroll
          for (int k = 0; k < 6; k++) J[k] = 0.f;
        }
        add_row_f64(r, J, acc, 27);   // (a pixel without a row has r = 0 and J = 0: its products add exact zeros)
        grows += ok ? 1.f : 0.f;      // (a thread sees fewer than 2^24 pixels: exact)
      }
      past = sdf_photo_gate(v, a, G, Q.gate, have);
    }
    // the colour corners behind the TSDF corners' gates: zeros in their place have no colour weight > 0, the same "no row"
    uint2 c[8];
#pragma unroll
    for (int m = 0; m < 8; m++) c[m] = make_uint2(0u, 0u);
    if (past) { const MapRayView M = map_photo_late_view(); map_colour_corners{M}(i0, c); }
    float l[8];
    const bool known = colour_lumas(c, l);
    const float If = fint[i];
    const bool okp = sdf_photo_value(past && known && __builtin_isfinite(If), l, a, G, map_photo_late_pose(), x, y, z, If, r, J);
    // step 6: r' = lam r, J' = lam J in fp32 (0 for a pixel without a row)
    r = okp ? lam * r : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = okp ? lam * J[k] : 0.f;
    add_row_f64(r, J, acc, 28);
    prows += okp ? 1.f : 0.f;
  }
  double sums[kSdfPhotoAcc];
#pragma unroll
  for (int k = 0; k < 28; k++) sums[k] = acc[k];
  sums[28] = (double)grows; sums[29] = acc[28]; sums[30] = (double)prows;
  reduce_and_finish<kSdfPhotoAcc, kNlLd, 0, BLK, false>(sums, late_finish_at((unsigned)offsetof(MapSdfPhotoRoundArgs, fin)));   // host-driven only
}

__global__ __launch_bounds__(kSdfRowsBlock) void map_sdf_photo_rows_kernel(const float* __restrict__ vmap, const float* __restrict__ fint,
                                                                           int64_t n, MapSdfPhotoView P, VolumeGeometry G, float gate, PoseF T,
                                                                           float* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kSdfRowsBlock + threadIdx.x;
  if (i >= n) return;
  const MapRayView M = ray_view(P);
  float r, J[6];
  const bool ok = sdf_photo_pixel(map_sdf_corners{M}, map_colour_corners{M}, G, T, gate, vmap[3 * i], vmap[3 * i + 1], vmap[3 * i + 2], fint[i],
                                  r, J);
  store_row(rows, n, i, ok, r, J);
}

MapSdfPhotoView photo_view(const MapRayView& M) {
  MapSdfPhotoView P;
  P.S = sdf_view(M);
  P.cvol = M.cvol; P.cpool = M.cpool;
  return P;
}

// a node per new kernel, beside the unit's own (one code object: whichever is touched first loads all of it)
namespace map_photo_rows_node { RPE_PRELOAD(map_sdf_photo_rows_kernel); }
namespace map_photo_round_node { RPE_PRELOAD(icp_map_sdf_photo_kernel<true, 256>); }

}  // namespace

hipError_t launch_icp_map_sdf_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const MapRayView& M,
                                    const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                    const double* pose12, const ReduceTarget& rt, hipStream_t s) {
  const SdfParams Q = sdf_params(G, dist_thr, cos_thr, use_normals);
  const PoseF T = pose_f(pose12);
  const Finish fin = make_finish(rt);
  const MapSdfPhotoView P = photo_view(M);
  const int blk = pick_block(rt);   // one pixel per thread while the grid allows it
  const int grid = round_grid(rt, n, blk);
#define RPE_MAP_SDF_PHOTO_LAUNCH(GEO, B) \
  hipLaunchKernelGGL((icp_map_sdf_photo_kernel<GEO, B>), dim3(grid), dim3(B), 0, s, vmap, nmap, fint, n, P, G, Q, lam, T, fin)
  if (blk == 512) { if (geometric) RPE_MAP_SDF_PHOTO_LAUNCH(true, 512); else RPE_MAP_SDF_PHOTO_LAUNCH(false, 512); }
  else { if (geometric) RPE_MAP_SDF_PHOTO_LAUNCH(true, 256); else RPE_MAP_SDF_PHOTO_LAUNCH(false, 256); }
#undef RPE_MAP_SDF_PHOTO_LAUNCH
  return hipGetLastError();
}

hipError_t launch_map_sdf_photo_rows(const float* vmap, const float* fint, int64_t n, const MapRayView& M, const VolumeGeometry& G,
                                     float dist_thr, const double* pose12, float* rows, hipStream_t s) {
  const int64_t blocks = (n + kSdfRowsBlock - 1) / kSdfRowsBlock;
  hipLaunchKernelGGL(map_sdf_photo_rows_kernel, dim3((unsigned)blocks), dim3(kSdfRowsBlock), 0, s, vmap, fint, n, photo_view(M), G, dist_thr,
                     pose_f(pose12), rows);
  return hipGetLastError();
}

}  // namespace rpe

// the robust rounds of the four volume terms, as kernels of their own names, and the hook that writes a level's plane of weights
// (include/rgbd_pose_hip.h Part 3, "Robust volume terms"): behind everything whose cell, corner fetches, rows and gates they share
#include "rpe_sdf_robust.hpp"
