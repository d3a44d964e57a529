// Part 3 of include/rgbd_pose_hip.h: the map mesh (kernels in rpe_mapmesh.hip).  The map is the window plus the archived bricks, a
// sparse grid of world voxels; a box of it is meshed as rpe_volume_mesh would mesh a dense volume of the box.  The host LISTS the
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

}  // namespace

extern "C" {

int rpe_volume_map_bounds(rpe_context* c, int64_t lo[3], int64_t hi[3]) {
  session_end(c);
  if (!c || !lo || !hi) return fail(RPE_ERR_ARG, "rpe_volume_map_bounds: bad argument");
  const auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!multiples_of_brick(V))
    return fail(RPE_ERR_STATE, "rpe_volume_map_bounds: every dim (%d %d %d) and every component of the total shift (%lld %lld %lld) must be a "
                "multiple of 8", V.g.dim[0], V.g.dim[1], V.g.dim[2], (long long)V.total[0], (long long)V.total[1], (long long)V.total[2]);
  map_bounds(V, lo, hi);
  return RPE_OK;
}

int rpe_volume_map_mesh(rpe_context* c, double min_weight, const int64_t lo[3], const int64_t hi[3], int64_t* n_vertices,
                        int64_t* n_triangles) {
  session_end(c);
  if (c) c->vol.have_mesh = false;   // the last mesh lives until this call, whatever it returns
  if (!c || !n_vertices || !n_triangles || !lo != !hi) return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: bad argument");
  auto& V = c->vol;
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!multiples_of_brick(V))
    return fail(RPE_ERR_STATE, "rpe_volume_map_mesh: every dim (%d %d %d) and every component of the total shift (%lld %lld %lld) must be a "
                "multiple of 8", V.g.dim[0], V.g.dim[1], V.g.dim[2], (long long)V.total[0], (long long)V.total[1], (long long)V.total[2]);
  const float wmin = (float)min_weight;
  if (!(min_weight > 0) || !std::isfinite(min_weight) || !(wmin > 0))
    return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: min_weight must be finite and > 0, also in fp32 (got %g)", min_weight);
  int64_t blo[3], bhi[3], b0[3], nb[3];
  if (lo) for (int a = 0; a < 3; a++) { blo[a] = lo[a]; bhi[a] = hi[a]; }
  else map_bounds(V, blo, bhi);
  rpe::VolumeGeometry G = V.g;
  for (int a = 0; a < 3; a++) {
    if (blo[a] < -kMaxWorld || blo[a] > kMaxWorld || bhi[a] < -kMaxWorld || bhi[a] > kMaxWorld || blo[a] % kBrick || bhi[a] % kBrick || bhi[a] - blo[a] < kBrick || bhi[a] - blo[a] > kMaxBox)
      return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: the box needs lo and hi in multiples of 8 and 8 <= hi - lo <= 2^20 on every axis (got %lld, "
                  "%lld on axis %d%s)", (long long)blo[a], (long long)bhi[a], a, lo ? "" : ": the map's bounds");
    G.dim[a] = (int)(bhi[a] - blo[a]);
    G.o[a] = (float)(V.desc.origin[a] + (double)blo[a] * V.desc.voxel_size);   // rpe_volume_shift's rule: one rounding
    if (!std::isfinite(G.o[a])) return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: the box's origin along axis %d is not finite in fp32", a);
    b0[a] = blo[a] / kBrick; nb[a] = G.dim[a] / kBrick;
  }
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = build_list(V, b0, nb, V.h_map_list);
  if (n >= ((int64_t)1 << 31) / 27) return fail(RPE_ERR_ARG, "rpe_volume_map_mesh: %lld bricks in the box; the table holds fewer than 2^31 / 27", (long long)n);
  int rc;
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

}  // extern "C"
