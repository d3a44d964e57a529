// Part 3 of include/rgbd_pose_hip.h: the map REBUILT from the keyframes (kernel in rpe_mapfuse.hpp, compiled into rpe_frontend.hip).  A list
// of keyframes is fused into every brick of a box of world voxels, in the window or not, leaving bit for bit what
// rpe_volume_fuse_keyframes leaves in a dense volume of the box.  Two passes, so that the archive's capacity is checked before anything
// is written (as a shift does) without a staging pool of the box's size: pass 1 runs the fuse from zeros on every brick of the box and
// keeps one flag word per brick; the host -- which holds the index -- then decides which absent bricks take a slot, which held bricks
// are released and which bricks pass 2 writes; pass 2 runs on that list only.  The flags' copy is the call's one host wait.
#include "rpe_frontend_host.hpp"
#include <utility>
using namespace rpeh;

namespace {
constexpr size_t kSlot = (size_t)rpe::kArchiveSlotBytes;
using Key = std::array<int64_t, 3>;   // (bz, by, bx), the index's key
}  // namespace

extern "C" {

int rpe_volume_map_fuse_keyframes(rpe_context* c, const int32_t* ids, int count, const double* poses12, int flags, const int64_t lo[3],
                                  const int64_t hi[3], int64_t stats[4]) {
  static const char* who = "rpe_volume_map_fuse_keyframes";
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (flags & ~(RPE_FUSE_CLEAR | RPE_FUSE_COLOR | RPE_FUSE_NO_CULL)) return fail(RPE_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
  if (!lo != !hi) return fail(RPE_ERR_ARG, "%s: lo and hi come together", who);
  const bool clear = flags & RPE_FUSE_CLEAR, color = flags & RPE_FUSE_COLOR, cull = !(flags & RPE_FUSE_NO_CULL);
  auto& V = c->vol;
  auto& A = V.arc;
  auto& K = c->kf;
  int rc = map_state(who, V);
  if (rc) return rc;
  std::vector<rpe::FuseEntry> table;
  if ((rc = fuse_list(c, who, ids, count, poses12, color, table))) return rc;
  int64_t b0[3], nb[3];
  rpe::VolumeGeometry G;
  if ((rc = map_box(who, V, lo, hi, G, b0, nb))) return rc;
  const int64_t n = nb[0] * nb[1] * nb[2];   // <= 2^51
  if (n > kMaxGrid) return fail(RPE_ERR_ARG, "%s: %lld bricks in the box; the brick grid holds at most 2^24", who, (long long)n);
  rpe::MapRayView R{};
  build_grid(V, b0, nb, V.h_map_list, R);    // the host's copy is all this call needs: pass 1 reads no brick
  const int32_t* grid = reinterpret_cast<const int32_t*>(V.h_map_list.data());
  if (!A.on && (int64_t)R.wbn[0] * R.wbn[1] * R.wbn[2] != n)
    return fail(RPE_ERR_STATE, "%s: the box reaches outside the window and the archive is off (rpe_volume_archive)", who);
  HIP_TRY(hipSetDevice(c->device));

  // ---- pass 1: the table up, a flag word per brick down (the wait)
  if ((rc = K.d_table.once(c, RPE_MAX_KEYFRAMES * sizeof(rpe::FuseEntry))) || (rc = A.flags.reserve(c, (size_t)n * sizeof(unsigned int)))) return rc;
  HIP_TRY(hipMemcpyAsync(K.d_table, table.data(), table.size() * sizeof(rpe::FuseEntry), hipMemcpyHostToDevice, c->stream));
  rpe::MapFuseView M{};
  M.wdim0 = V.g.dim[0]; M.wdim1 = V.g.dim[1];
  for (int a = 0; a < 3; a++) { M.wnb[a] = V.g.dim[a] / 8; M.nb[a] = (int)nb[a]; }
  M.capacity = (int)A.capacity;
  M.table = K.d_table; M.count = (int)table.size(); M.cull = cull ? 1 : 0;
  M.n = (int)n; M.flags = A.flags;
  HIP_TRY(rpe::launch_map_fuse_mark(M, G, color, c->stream));
  A.h_flags.resize((size_t)n);
  if ((rc = copy_to_host(c, A.h_flags.data(), A.flags, (size_t)n * sizeof(unsigned int)))) return rc;

  // ---- the host's part: pass 2's list, the slots that change hands; nothing is written before the capacity is known to suffice
  auto& list = A.h_pairs;   // {box brick, source, fresh}; the upload may read it until the next wait on the stream
  list.clear();
  std::vector<int32_t> fresh_at;    // positions in `list` of the absent bricks that take a slot (source filled in below)
  std::vector<Key> taken, released;
  std::vector<int32_t> released_slot;
  auto key_of = [&](int64_t b) { return Key{b0[2] + b / (nb[0] * nb[1]), b0[1] + (b / nb[0]) % nb[1], b0[0] + b % nb[0]}; };
  for (int64_t b = 0; b < n; b++) {
    const int32_t src = grid[b];
    const unsigned f = A.h_flags[(size_t)b];
    const bool absent = src == (int32_t)rpe::kMapAbsent, held = src < 0 && !absent;
    if (absent) {
      if (!(f & 1u)) continue;
      fresh_at.push_back((int32_t)list.size());
      taken.push_back(key_of(b));
      list.insert(list.end(), {(int32_t)b, src, 1});
    } else if (clear) {
      if (held && !(f & 1u)) { released.push_back(key_of(b)); released_slot.push_back(~src); }   // all zero after the fuse: no device work
      else list.insert(list.end(), {(int32_t)b, src, 1});
    } else if (f & 2u) {   // (an updated voxel has a weight >= 1, max_weight being >= 1: a present brick never ends all zero here)
      list.insert(list.end(), {(int32_t)b, src, 0});
    }
  }
  const size_t n_new = taken.size(), n_rel = released.size();
  if (n_new > A.free.size() + n_rel)
    return fail(RPE_ERR_STATE, "%s: the archive needs %lld free slots for the bricks that become non-empty and has %lld (capacity %lld, "
                "held %lld): grow it with rpe_volume_archive", who, (long long)n_new, (long long)(A.free.size() + n_rel),
                (long long)A.capacity, (long long)A.index.size());
  // the free list as it will stand -- the released slots behind the free ones -- hands out from its tail, as a shift does
  for (size_t i = 0; i < n_new; i++)
    list[(size_t)fresh_at[i] + 1] = ~(i < n_rel ? released_slot[n_rel - 1 - i] : A.free[A.free.size() - 1 - (i - n_rel)]);

  // ---- pass 2
  if (clear) V.have_mesh = false;   // as rpe_volume_fuse_keyframes: the mesh of a cleared volume is gone
  if (color && (rc = ensure_color_volume(c, true))) return rc;
  bool pooled = false;
  for (size_t i = 1; i < list.size() && !pooled; i += 3) pooled = list[i] < 0;
  if (color && pooled && !A.cpool) {   // as archive_leave: the first colour brick in the pool; the bricks held so far have none
    if ((rc = A.cpool.reserve(c, (size_t)A.capacity * kSlot))) return rc;
    HIP_TRY(hipMemsetAsync(A.cpool, 0, (size_t)A.capacity * kSlot, c->stream));
  }
  if (!list.empty()) {
    if ((rc = A.pairs.reserve(c, list.size() * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(A.pairs, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    M.vol = reinterpret_cast<unsigned int*>(V.d.get());
    M.cvol = V.have_color ? reinterpret_cast<unsigned int*>(V.cd.get()) : nullptr;
    M.pool = A.pool; M.cpool = A.cpool;
    M.n = (int)(list.size() / 3); M.list = A.pairs; M.flags = nullptr;
    HIP_TRY(rpe::launch_map_fuse(M, G, clear, color, c->stream));
  }
  // the index follows: a released slot goes back to the free list, a taken one leaves it
  for (size_t i = 0; i < n_rel; i++) { A.index.erase(released[i]); A.free.push_back(released_slot[i]); }
  for (size_t i = 0; i < n_new; i++) { A.index[taken[i]] = A.free.back(); A.free.pop_back(); }
  if (stats) { stats[0] = n; stats[1] = (int64_t)(list.size() / 3); stats[2] = (int64_t)n_new; stats[3] = (int64_t)n_rel; }
  return RPE_OK;
}

}  // extern "C"
