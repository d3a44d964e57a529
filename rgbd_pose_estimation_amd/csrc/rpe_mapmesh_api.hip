// Part 3 of include/rgbd_pose_hip.h: the map -- the window plus the archived bricks, a sparse grid of world voxels -- meshed (kernels in
// rpe_mapmesh.hip) and raycast (kernels in rpe_frontend.hip).  A box of it is meshed as rpe_volume_mesh would mesh a dense volume of the
// box, and raycast as rpe_volume_raycast would raycast it; the state check and the box's rules are stated once, for both.  The raycast's
// host part is the BRICK GRID (rpe_kernels.h MapRayView): one int32 per brick of the box, filled from the window's extent and the
// archive's index and uploaded in one copy per call.  For the mesh the host LISTS the
// bricks of the map that lie in the box -- every brick of the window (the kernel's early exit is their occupancy test) and every held
// brick (the index of rpe_archive_api.hip) -- ascending by (bz, by, bx), and gives each its 27 neighbours as list positions: the keys
// are packed integers, so a neighbour's key is the brick's plus a constant and, the list being sorted, one cursor per direction walks
// it once (13 passes, each filling a direction and its opposite; no search).  Keys, sources and table go up in ONE copy; two launches,
// the host's one wait for the two totals, two or three launches.  The result is the context's last mesh; its colours are sampled
// during the extraction.
#include "rpe_frontend_host.hpp"
#include <cmath>
using namespace rpeh;

#pragma clang fp contract(off)   // the box's origin is the header's expression, operation by operation

namespace {

constexpr int64_t kBrick = 8;
constexpr int64_t kMaxBox = (int64_t)1 << 20;     // voxels per axis: the brick coordinates inside the box fit kMapKeyBits
constexpr int64_t kMaxWorld = (int64_t)1 << 40;   // |lo|, |hi|: far beyond any total shift, and nothing below overflows

bool multiples_of_brick(const rpe_context::Volume& V) {
  for (int a = 0; a < 3; a++)
    if (V.g.dim[a] % kBrick || V.total[a] % kBrick) return false;
  return true;
}

void map_bounds(const rpe_context::Volume& V, int64_t lo[3], int64_t hi[3]) {
  for (int a = 0; a < 3; a++) { lo[a] = V.total[a]; hi[a] = V.total[a] + V.g.dim[a]; }
  for (const auto& kv : V.arc.index)
    for (int a = 0; a < 3; a++) {   // the key is (bz, by, bx)
      lo[a] = std::min(lo[a], kBrick * kv.first[2 - a]);
      hi[a] = std::max(hi[a], kBrick * kv.first[2 - a] + kBrick);
    }
}

}  // namespace

// what every entry point asks of the context (`who` names the caller in the messages) ...
int rpeh::map_state(const char* who, const rpe_context::Volume& V) {
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!multiples_of_brick(V))
    return fail(RPE_ERR_STATE, "%s: every dim (%d %d %d) and every component of the total shift (%lld %lld %lld) must be a "
                "multiple of 8", who, V.g.dim[0], V.g.dim[1], V.g.dim[2], (long long)V.total[0], (long long)V.total[1], (long long)V.total[2]);
  return RPE_OK;
}
// ... and the mesh and the raycast of the box.  lo = NULL: the map's bounds.  On success G is the virtual volume's geometry and b0 / nb
// the box in bricks
int rpeh::map_box(const char* who, const rpe_context::Volume& V, const int64_t* lo, const int64_t* hi, rpe::VolumeGeometry& G, int64_t b0[3],
                  int64_t nb[3]) {
  int64_t blo[3], bhi[3];
  if (lo) for (int a = 0; a < 3; a++) { blo[a] = lo[a]; bhi[a] = hi[a]; }
  else map_bounds(V, blo, bhi);
  G = V.g;
  for (int a = 0; a < 3; a++) {
    if (blo[a] < -kMaxWorld || blo[a] > kMaxWorld || bhi[a] < -kMaxWorld || bhi[a] > kMaxWorld || blo[a] % kBrick || bhi[a] % kBrick || bhi[a] - blo[a] < kBrick || bhi[a] - blo[a] > kMaxBox)
      return fail(RPE_ERR_ARG, "%s: the box needs lo and hi in multiples of 8 and 8 <= hi - lo <= 2^20 on every axis (got %lld, "
                  "%lld on axis %d%s)", who, (long long)blo[a], (long long)bhi[a], a, lo ? "" : ": the map's bounds");
    G.dim[a] = (int)(bhi[a] - blo[a]);
    G.o[a] = (float)(V.desc.origin[a] + (double)blo[a] * V.desc.voxel_size);   // rpe_volume_shift's rule: one rounding
    if (!std::isfinite(G.o[a])) return fail(RPE_ERR_ARG, "%s: the box's origin along axis %d is not finite in fp32", who, a);
    b0[a] = blo[a] / kBrick; nb[a] = G.dim[a] / kBrick;
  }
  return RPE_OK;
}

namespace {

inline unsigned long long pack(int64_t bx, int64_t by, int64_t bz) {
  return (unsigned long long)bz << (2 * rpe::kMapKeyBits) | (unsigned long long)by << rpe::kMapKeyBits | (unsigned long long)bx;
}

// the list of the box [b0, b0 + nb) of world bricks into h: keys | sources | table; returns the number of listed bricks
int64_t build_list(const rpe_context::Volume& V, const int64_t b0[3], const int64_t nb[3], std::vector<unsigned char>& h) {
  int64_t w0[3], from[3], to[3];
  for (int a = 0; a < 3; a++) {
    w0[a] = V.total[a] / kBrick;
    from[a] = std::max(w0[a], b0[a]);
    to[a] = std::max(from[a], std::min(w0[a] + V.g.dim[a] / kBrick, b0[a] + nb[a]));
  }
  const int64_t nw = (to[0] - from[0]) * (to[1] - from[1]) * (to[2] - from[2]);
  std::vector<std::pair<unsigned long long, int32_t>> held;
  for (const auto& kv : V.arc.index) {   // (bz, by, bx) ascending: the list's order
    const int64_t x = kv.first[2] - b0[0], y = kv.first[1] - b0[1], z = kv.first[0] - b0[2];
    if (x >= 0 && x < nb[0] && y >= 0 && y < nb[1] && z >= 0 && z < nb[2]) held.emplace_back(pack(x, y, z), ~kv.second);
  }
  const int64_t n = nw + (int64_t)held.size();
  h.resize((size_t)n * rpe::kMapListBytes);   // every byte is written below
  unsigned long long* key = reinterpret_cast<unsigned long long*>(h.data());
  int32_t* src = reinterpret_cast<int32_t*>(h.data() + 8 * (size_t)n);
  int32_t* nbr = src + n;
  // the window's bricks in the box, ascending, merged with the held ones (the window is the only holder of what it covers)
  const int64_t wn0 = V.g.dim[0] / kBrick, wn1 = V.g.dim[1] / kBrick;
  size_t i = 0, k = 0;
  for (int64_t z = from[2]; z < to[2]; z++)
    for (int64_t y = from[1]; y < to[1]; y++)
      for (int64_t x = from[0]; x < to[0]; x++) {
        const unsigned long long kw = pack(x - b0[0], y - b0[1], z - b0[2]);
        for (; k < held.size() && held[k].first < kw; k++, i++) { key[i] = held[k].first; src[i] = held[k].second; }
        key[i] = kw;
        src[i++] = (int32_t)((x - w0[0]) + wn0 * ((y - w0[1]) + wn1 * (z - w0[2])));
      }
  for (; k < held.size(); k++, i++) { key[i] = held[k].first; src[i] = held[k].second; }
  // the table: direction by direction, the neighbour's key = key + a constant, ascending with the list; q is p's neighbour along d
  // exactly when p is q's along -d, so the 13 directions after the centre fill both halves
  const unsigned long long mask = ((unsigned long long)1 << rpe::kMapKeyBits) - 1;
  for (int64_t p = 0; p < n; p++) {
    for (int e = 0; e < 27; e++) nbr[27 * p + e] = -1;
    nbr[27 * p + 13] = (int32_t)p;
  }
  for (int e = 14; e < 27; e++) {
    const int64_t dx = e % 3 - 1, dy = (e / 3) % 3 - 1, dz = e / 9 - 1;
    int64_t cur = 0;
    for (int64_t p = 0; p < n; p++) {
      const int64_t x = (int64_t)(key[p] & mask) + dx, y = (int64_t)((key[p] >> rpe::kMapKeyBits) & mask) + dy,
                    z = (int64_t)(key[p] >> (2 * rpe::kMapKeyBits)) + dz;
      if (x < 0 || x >= nb[0] || y < 0 || y >= nb[1] || z < 0 || z >= nb[2]) continue;
      const unsigned long long want = pack(x, y, z);
      while (cur < n && key[cur] < want) cur++;
      if (cur < n && key[cur] == want) { nbr[27 * p + e] = (int32_t)cur; nbr[27 * cur + 26 - e] = (int32_t)p; }
    }
  }
  return n;
}

// The brick grid of the box [b0, b0 + nb) of world bricks into h, x fastest, every entry written: kMapAbsent, then the window's bricks
// by their linear index, then the held ones as ~slot (the window is the only holder of what it covers: they do not meet).  Also M's
// description of window and box
// (rpe_frontend_host.hpp: kMaxGrid, the most bricks a caller lets a box have)
}  // namespace

void rpeh::build_grid(const rpe_context::Volume& V, const int64_t b0[3], const int64_t nb[3], std::vector<unsigned char>& h, rpe::MapRayView& M) {
  const int64_t n = nb[0] * nb[1] * nb[2];
  h.resize((size_t)n * sizeof(int32_t));
  int32_t* g = reinterpret_cast<int32_t*>(h.data());
  std::fill(g, g + n, (int32_t)rpe::kMapAbsent);
  int64_t w0[3], from[3], to[3];
  for (int a = 0; a < 3; a++) {
    w0[a] = V.total[a] / kBrick;
    M.wnb[a] = V.g.dim[a] / (int)kBrick;
    from[a] = std::max(w0[a], b0[a]);
    to[a] = std::max(from[a], std::min(w0[a] + M.wnb[a], b0[a] + nb[a]));
    M.nb[a] = (int)nb[a];
    M.wb0[a] = (int)(from[a] - w0[a]); M.wbn[a] = (int)(to[a] - from[a]);
    M.woff[a] = (int)std::max<int64_t>(-(kMaxBox << 1), std::min<int64_t>(kMaxBox << 1, kBrick * (w0[a] - b0[a])));
  }
  M.wdim0 = V.g.dim[0]; M.wdim1 = V.g.dim[1]; M.wdim2 = V.g.dim[2];
  for (int64_t z = from[2]; z < to[2]; z++)
    for (int64_t y = from[1]; y < to[1]; y++)
      for (int64_t x = from[0]; x < to[0]; x++)
        g[(x - b0[0]) + nb[0] * ((y - b0[1]) + nb[1] * (z - b0[2]))] = (int32_t)((x - w0[0]) + M.wnb[0] * ((y - w0[1]) + M.wnb[1] * (z - w0[2])));
  for (const auto& kv : V.arc.index) {   // the key is (bz, by, bx)
    const int64_t x = kv.first[2] - b0[0], y = kv.first[1] - b0[1], z = kv.first[0] - b0[2];
    if (x >= 0 && x < nb[0] && y >= 0 && y < nb[1] && z >= 0 && z < nb[2]) g[x + nb[0] * (y + nb[1] * z)] = ~kv.second;
  }
}

int rpeh::map_field(rpe_context* c, const char* who, const int64_t* lo, const int64_t* hi, rpe::VolumeGeometry& G, rpe::MapRayView& M) {
  auto& V = c->vol;
  int64_t b0[3], nb[3];
  int rc;
  if ((rc = map_state(who, V)) || (rc = map_box(who, V, lo, hi, G, b0, nb))) return rc;
  const int64_t n = nb[0] * nb[1] * nb[2];   // <= 2^51
  if (n > kMaxGrid) return fail(RPE_ERR_ARG, "%s: %lld bricks in the box; the brick grid holds at most 2^24", who, (long long)n);
  if ((rc = V.map_list.reserve(c, (size_t)n * sizeof(int32_t)))) return rc;
  build_grid(V, b0, nb, V.h_map_list, M);
  HIP_TRY(hipMemcpyAsync(V.map_list, V.h_map_list.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  M.vol = reinterpret_cast<const unsigned int*>(V.d.get());
  M.cvol = V.have_color ? reinterpret_cast<const unsigned int*>(V.cd.get()) : nullptr;
  M.pool = V.arc.pool; M.cpool = V.arc.cpool;
  M.capacity = (int)V.arc.capacity;
  M.grid = static_cast<int*>(V.map_list.get());
  return RPE_OK;
}

extern "C" {

int rpe_volume_map_bounds(rpe_context* c, int64_t lo[3], int64_t hi[3]) {
  session_end(c);
  if (!c || !lo || !hi) return fail(RPE_ERR_ARG, "rpe_volume_map_bounds: bad argument");
  const auto& V = c->vol;
  if (int rc = map_state("rpe_volume_map_bounds", V)) return rc;
  map_bounds(V, lo, hi);
  return RPE_OK;
}

int rpe_volume_map_mesh(rpe_context* c, double min_weight, const int64_t lo[3], const int64_t hi[3], int64_t* n_vertices,
                        int64_t* n_triangles) {
  session_end(c);
  if (c) c->vol.have_mesh = false;   // the last mesh lives until this call, whatever it returns
  if (!c || !n_vertices || !n_triangles || !lo != !hi) return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: bad argument");
  auto& V = c->vol;
  int rc = map_state("rpe_volume_map_mesh", V);
  if (rc) return rc;
  const float wmin = (float)min_weight;
  if (!(min_weight > 0) || !std::isfinite(min_weight) || !(wmin > 0))
    return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: min_weight must be finite and > 0, also in fp32 (got %g)", min_weight);
  int64_t b0[3], nb[3];
  rpe::VolumeGeometry G;
  if ((rc = map_box("rpe_volume_map_mesh", V, lo, hi, G, b0, nb))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = build_list(V, b0, nb, V.h_map_list);
  if (n >= ((int64_t)1 << 31) / 27) return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: %lld bricks in the box; the table holds fewer than 2^31 / 27", (long long)n);
  if ((rc = V.map_list.reserve(c, (size_t)n * rpe::kMapListBytes)) || (rc = V.ws.reserve(c, rpe::map_mesh_workspace_bytes(n)))) return rc;
  if (n) HIP_TRY(hipMemcpyAsync(V.map_list, V.h_map_list.data(), (size_t)n * rpe::kMapListBytes, hipMemcpyHostToDevice, c->stream));
  const bool colour = V.have_color || V.arc.cpool;
  rpe::MapMeshView M{};
  M.vol = reinterpret_cast<const unsigned int*>(V.d.get());
  M.cvol = V.have_color ? reinterpret_cast<const unsigned int*>(V.cd.get()) : nullptr;
  M.pool = V.arc.pool; M.cpool = V.arc.cpool;
  M.wdim0 = V.g.dim[0]; M.wdim1 = V.g.dim[1];
  for (int a = 0; a < 3; a++) M.wnb[a] = V.g.dim[a] / (int)kBrick;
  M.capacity = (int)V.arc.capacity;
  M.n = (int)n;
  M.key = static_cast<const unsigned long long*>(V.map_list.get());
  M.src = reinterpret_cast<const int*>(static_cast<const char*>(V.map_list.get()) + 8 * (size_t)n);
  M.nbr = M.src + n;
  const rpe::MapMeshWorkspace W = rpe::map_mesh_workspace(V.ws, n);
  HIP_TRY(rpe::launch_map_mesh_count(M, wmin, W, c->stream));
  long long tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, W.totals, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (tot[0] >= ((long long)1 << 31))
    return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: %lld vertices; the int32 triangle ids hold fewer than 2^31", tot[0]);
  const size_t vb = (size_t)tot[0] * 3 * sizeof(float), tb = (size_t)tot[1] * 3 * sizeof(int32_t);
  if (vb && ((rc = V.mv.reserve(c, vb)) || (rc = V.mn.reserve(c, vb)))) return rc;   // (an empty mesh asks for nothing)
  if (vb && colour && (rc = V.mc.reserve(c, (size_t)tot[0] * 4))) return rc;
  if (tb && (rc = V.mt.reserve(c, tb))) return rc;
  if (tot[0] > 0) HIP_TRY(rpe::launch_map_mesh_emit(M, G, W, V.mv, V.mn, V.mt, colour ? V.mc.get() : nullptr, c->stream));
  V.nv = tot[0]; V.nt = tot[1];
  V.have_mesh = true; V.mesh_is_map = true; V.map_color = colour;
  *n_vertices = V.nv; *n_triangles = V.nt;
  return RPE_OK;
}

int rpe_volume_map_raycast(rpe_context* c, const double* pose12, const rpe_camera* cam, double dmin, double dmax, const int64_t lo[3],
                           const int64_t hi[3], int flags) {
  session_end(c);
  if (!c || !pose12 || !lo != !hi || (flags & ~(RPE_MAPRAY_COLOR | RPE_MAPRAY_NO_SKIP))) return fail(RPE_ERR_ARG, "rpe_volume_map_raycast: bad argument");
  rpe::Camera k;
  int rc = camera_of(cam, &k);
  if (rc) return rc;
  auto& V = c->vol;
  int64_t b0[3], nb[3];
  rpe::VolumeGeometry G;
  if ((rc = map_state("rpe_volume_map_raycast", V)) || (rc = map_box("rpe_volume_map_raycast", V, lo, hi, G, b0, nb))) return rc;
  const int64_t n = nb[0] * nb[1] * nb[2];   // <= 2^51
  if (n > kMaxGrid)
    return fail(RPE_ERR_ARG, "rpe_volume_map_raycast: %lld bricks in the box; the brick grid holds at most 2^24", (long long)n);
  if (!(dmin >= 0) || !(dmax > dmin) || !std::isfinite(dmax))
    return fail(RPE_ERR_ARG, "rpe_volume_map_raycast: need 0 <= dmin < dmax, both finite (got %g, %g)", dmin, dmax);
  const double samples = ((double)(float)dmax - (double)(float)dmin) / (double)G.s;
  if (!(samples <= (double)(1 << 22)))
    return fail(RPE_ERR_ARG, "rpe_volume_map_raycast: %.0f samples per ray ((dmax - dmin) / voxel_size) exceed 2^22", samples);
  const bool colour = flags & RPE_MAPRAY_COLOR;
  if (colour && !V.have_color && !V.arc.cpool)
    return fail(RPE_ERR_STATE, "rpe_volume_map_raycast: RPE_MAPRAY_COLOR needs a colour volume or a colour plane in the archive");
  HIP_TRY(hipSetDevice(c->device));
  auto& F = c->fe;
  const int64_t pixels = (int64_t)k.width * k.height;
  if ((rc = V.map_list.reserve(c, (size_t)n * sizeof(int32_t))) || (rc = model_room(c, pixels))) return rc;
  if (colour && (rc = F.mcolor.reserve(c, (size_t)pixels * 4))) return rc;
  rpe::MapRayView M{};
  build_grid(V, b0, nb, V.h_map_list, M);
  HIP_TRY(hipMemcpyAsync(V.map_list, V.h_map_list.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  M.vol = reinterpret_cast<const unsigned int*>(V.d.get());
  M.cvol = V.have_color ? reinterpret_cast<const unsigned int*>(V.cd.get()) : nullptr;
  M.pool = V.arc.pool; M.cpool = V.arc.cpool;
  M.capacity = (int)V.arc.capacity;
  M.grid = static_cast<int*>(V.map_list.get());
  F.have_model = false;
  F.have_mcolor = false; F.feat[1].have = false; F.photo_levels = 0;
  if (!(flags & RPE_MAPRAY_NO_SKIP)) HIP_TRY(rpe::launch_map_occupancy(M, c->stream));
  HIP_TRY(rpe::launch_map_raycast(M, G, k, pose_f(pose12), (float)dmin, (float)dmax, F.mmap[0], F.mmap[1], colour ? F.mcolor.get() : nullptr,
                                  c->stream));
  F.mcam = k;
  one_level(*cam, k, F.mkcam, &F.mgeo);
  std::memcpy(F.mpose, pose12, sizeof(F.mpose));
  F.have_model = true;
  F.have_mcolor = colour;
  return RPE_OK;
}

}  // extern "C"
