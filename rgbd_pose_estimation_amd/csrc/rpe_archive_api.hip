// Part 3 of include/rgbd_pose_hip.h: the volume archive (kernels in rpe_archive.hip).  The voxels a shift of the moving volume pushes
// out of the window are kept, brick by brick (8 x 8 x 8 voxels, aligned in WORLD voxel coordinates: world voxel = total shift + window
// index, world brick = world voxel / 8), in a pool of 4-KB slots on the device and written back when the window returns over them.
// The INDEX lives on the host: a std::map world brick -> slot, keyed (bz, by, bx), and a list of free slots.  A shift asks the device
// which leaving bricks hold a non-zero word (A1, the shift's one host wait), the host then checks the capacity before anything is
// written, hands out slots, looks the entering bricks up and uploads the two (window brick, slot) lists; A2 gathers, the existing
// shift runs, A2 scatters.  A device-side index (a hash table the kernels probe and update) would save the wait and cost atomics, a
// failure mode in the middle of a shift and a sort for the download; at a few thousand bricks per shift the host does this in
// microseconds.  rpe_shift_api.hip calls archive_leave / archive_enter; with the archive off it does not come here at all.
#include "rpe_frontend_host.hpp"
#include <utility>
using namespace rpeh;

namespace {

constexpr int64_t kBrick = 8;
constexpr size_t kSlot = (size_t)rpe::kArchiveSlotBytes;
constexpr int64_t kMaxCapacity = (int64_t)1 << 24;   // 64 GB of tsdf bricks: beyond any device, and slot numbers stay far inside 32 bits

using Key = std::array<int64_t, 3>;   // (bz, by, bx): the map iterates in the download's order

// The bricks of a window of nb bricks that have no place after a move by s bricks (new index = old index - s), as at most three
// disjoint boxes: axis by axis, the slab that leaves along the axis, restricted on the axes before it to what stays there
// (tests/archive_oracle.py leaving_boxes).  Per axis only one of the two slabs is non-empty
rpe::ArchiveBoxes leaving_boxes(const int nb[3], const int64_t s[3]) {
  rpe::ArchiveBoxes B{};
  int64_t keep[3][2];
  for (int a = 0; a < 3; a++) {
    keep[a][0] = std::min<int64_t>(std::max<int64_t>(0, s[a]), nb[a]);
    keep[a][1] = std::max<int64_t>(keep[a][0], std::min<int64_t>(nb[a], nb[a] + s[a]));
  }
  int k = 0, count = 0;
  for (int a = 0; a < 3; a++) {
    const int64_t slab[2][2] = {{0, keep[a][0]}, {keep[a][1], nb[a]}};
    for (const auto& sl : slab) {
      if (sl[0] >= sl[1]) continue;
      int lo[3], n[3];
      bool some = true;
      for (int b = 0; b < 3; b++) {
        const int64_t l = b == a ? sl[0] : b < a ? keep[b][0] : 0, h = b == a ? sl[1] : b < a ? keep[b][1] : nb[b];
        lo[b] = (int)l; n[b] = (int)(h - l);
        some = some && h > l;
      }
      if (!some) continue;
      for (int b = 0; b < 3; b++) { B.lo[k][b] = lo[b]; B.n[k][b] = n[b]; }
      B.first[k] = count;
      count += n[0] * n[1] * n[2];
      k++;
    }
  }
  for (; k <= 3; k++) B.first[k] = count;
  return B;
}

// brick g of the boxes -> (bx, by, bz) in the window, in A1's order
template <class F> void for_each_brick(const rpe::ArchiveBoxes& B, F f) {
  int g = 0;
  for (int b = 0; b < 3; b++) {
    if (B.first[b + 1] == B.first[b]) continue;
    for (int z = 0; z < B.n[b][2]; z++)
      for (int y = 0; y < B.n[b][1]; y++)
        for (int x = 0; x < B.n[b][0]; x++) f(g++, B.lo[b][0] + x, B.lo[b][1] + y, B.lo[b][2] + z);
  }
}

bool multiples_of_brick(const rpe_context::Volume& V) {
  for (int a = 0; a < 3; a++)
    if (V.g.dim[a] % kBrick || V.total[a] % kBrick) return false;
  return true;
}

}  // namespace

namespace rpeh {

int archive_drop(rpe_context* c) {
  auto& A = c->vol.arc;
  if (A.pool) HIP_TRY(hipStreamSynchronize(c->stream));   // a kernel in flight may still use the pool, an upload the host lists
  A = rpe_context::Volume::Archive();
  return RPE_OK;
}

int archive_leave(rpe_context* c, const int32_t shift[3], const int64_t total_new[3], ArchivePlan* plan) {
  auto& V = c->vol;
  auto& A = V.arc;
  for (int a = 0; a < 3; a++)
    if (shift[a] % kBrick)
      return fail(RPE_ERR_ARG, "rpe_volume_shift: with the archive on every component of the shift must be a multiple of 8 (got %d along axis %d)",
                  shift[a], a);
  int nb[3];
  int64_t s[3], sneg[3], b_old[3], b_new[3];
  for (int a = 0; a < 3; a++) {
    nb[a] = V.g.dim[a] / (int)kBrick;
    s[a] = shift[a] / kBrick; sneg[a] = -s[a];
    b_old[a] = V.total[a] / kBrick; b_new[a] = total_new[a] / kBrick;
  }
  // A1 over the leaving bricks, and the one wait
  const rpe::ArchiveBoxes L = leaving_boxes(nb, s);
  const int n_leaving = L.first[3];
  if (int rc = A.flags.reserve(c, (size_t)n_leaving * sizeof(unsigned int))) return rc;
  HIP_TRY(rpe::launch_brick_occupancy(V.d, V.have_color ? V.cd.get() : nullptr, V.g.dim, L, A.flags, c->stream));
  A.h_flags.resize((size_t)n_leaving);
  if (int rc = copy_to_host(c, A.h_flags.data(), A.flags, (size_t)n_leaving * sizeof(unsigned int))) return rc;
  // capacity, before anything is written
  int64_t needed = 0;
  for (int g = 0; g < n_leaving; g++) needed += A.h_flags[g] != 0;
  if (needed > (int64_t)A.free.size())
    return fail(RPE_ERR_STATE, "rpe_volume_shift: the archive needs %lld free slots for the bricks that leave and has %lld (capacity %lld, "
                "held %lld): grow it with rpe_volume_archive", (long long)needed, (long long)A.free.size(), (long long)A.capacity,
                (long long)A.index.size());
  // slots for the leaving bricks (from the tail of the free list, taken for good only by archive_enter), the entering bricks' slots
  plan->leave_key.clear(); plan->enter_key.clear(); plan->enter_slot.clear();
  A.h_pairs.clear();
  for_each_brick(L, [&](int g, int x, int y, int z) {
    if (!A.h_flags[g]) return;
    const size_t i = plan->leave_key.size();
    plan->leave_key.push_back(Key{b_old[2] + z, b_old[1] + y, b_old[0] + x});
    A.h_pairs.push_back(x + nb[0] * (y + nb[1] * z));
    A.h_pairs.push_back(A.free[A.free.size() - 1 - i]);
  });
  if (!A.index.empty()) {
    const rpe::ArchiveBoxes E = leaving_boxes(nb, sneg);   // the new window's bricks that were not in the old one
    for_each_brick(E, [&](int, int x, int y, int z) {
      const Key key{b_new[2] + z, b_new[1] + y, b_new[0] + x};
      const auto it = A.index.find(key);
      if (it == A.index.end()) return;
      plan->enter_key.push_back(key);
      plan->enter_slot.push_back(it->second);
      A.h_pairs.push_back(x + nb[0] * (y + nb[1] * z));
      A.h_pairs.push_back(it->second);
    });
  }
  const int n_out = (int)plan->leave_key.size();
  if (A.h_pairs.empty()) return RPE_OK;
  if (int rc = A.pairs.reserve(c, A.h_pairs.size() * sizeof(int32_t))) return rc;
  HIP_TRY(hipMemcpyAsync(A.pairs, A.h_pairs.data(), A.h_pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (n_out == 0) return RPE_OK;
  if (V.have_color && !A.cpool) {   // the first brick archived while a colour volume exists: the bricks held so far restore zeros
    if (int rc = A.cpool.reserve(c, (size_t)A.capacity * kSlot)) return rc;
    HIP_TRY(hipMemsetAsync(A.cpool, 0, (size_t)A.capacity * kSlot, c->stream));
  }
  HIP_TRY(rpe::launch_brick_copy(true, V.d, V.have_color ? V.cd.get() : nullptr, A.pool, A.cpool, V.g.dim, A.pairs, n_out, (int)A.capacity,
                                 c->stream));
  return RPE_OK;
}

int archive_enter(rpe_context* c, const ArchivePlan& plan) {
  auto& V = c->vol;
  auto& A = V.arc;
  const size_t n_out = plan.leave_key.size(), n_in = plan.enter_key.size();
  if (n_in)
    HIP_TRY(rpe::launch_brick_copy(false, V.d, V.have_color ? V.cd.get() : nullptr, A.pool, A.cpool, V.g.dim, A.pairs.get() + 2 * n_out, (int)n_in,
                                   (int)A.capacity, c->stream));
  // the index follows: the window is the only holder of what it covers
  for (size_t i = 0; i < n_out; i++) A.index[plan.leave_key[i]] = A.free[A.free.size() - 1 - i];
  A.free.resize(A.free.size() - n_out);
  for (size_t i = 0; i < n_in; i++) { A.index.erase(plan.enter_key[i]); A.free.push_back(plan.enter_slot[i]); }
  return RPE_OK;
}

}  // namespace rpeh

extern "C" {

int rpe_volume_archive(rpe_context* c, int64_t capacity_bricks) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_archive: bad argument");
  if (capacity_bricks < 0 || capacity_bricks > kMaxCapacity)
    return fail(RPE_ERR_ARG, "rpe_volume_archive: capacity 0 .. 2^24 bricks (got %lld)", (long long)capacity_bricks);
  auto& V = c->vol;
  auto& A = V.arc;
  HIP_TRY(hipSetDevice(c->device));
  if (capacity_bricks == 0) return archive_drop(c);
  if (!V.have) return fail(RPE_ERR_STATE, "no volume: call rpe_volume_init first");
  if (!multiples_of_brick(V))
    return fail(RPE_ERR_STATE, "rpe_volume_archive: every dim (%d %d %d) and every component of the total shift (%lld %lld %lld) must be a "
                "multiple of 8", V.g.dim[0], V.g.dim[1], V.g.dim[2], (long long)V.total[0], (long long)V.total[1], (long long)V.total[2]);
  if (A.on && capacity_bricks < (int64_t)A.index.size())
    return fail(RPE_ERR_ARG, "rpe_volume_archive: capacity %lld is below the %lld bricks held", (long long)capacity_bricks, (long long)A.index.size());
  if (A.on && capacity_bricks <= A.capacity) return RPE_OK;   // the pool does not shrink (capacity 0 frees it)
  const size_t bytes = (size_t)capacity_bricks * kSlot, keep = (size_t)A.capacity * kSlot;
  if (!A.on) {
    if (int rc = A.pool.reserve(c, bytes)) return rc;
  } else if (A.cpool) {
    const DevMem::Grow g[2] = {{&A.pool, keep, bytes}, {&A.cpool, keep, bytes}};
    if (int rc = DevMem::regrow(c, "rpe_volume_archive", g)) return rc;
  } else {
    const DevMem::Grow g[1] = {{&A.pool, keep, bytes}};
    if (int rc = DevMem::regrow(c, "rpe_volume_archive", g)) return rc;
  }
  for (int64_t slot = capacity_bricks - 1; slot >= A.capacity; slot--) A.free.push_back((int32_t)slot);   // the lowest new slot goes first
  A.capacity = capacity_bricks;
  A.on = true;
  return RPE_OK;
}

int rpe_volume_archive_info(rpe_context* c, int64_t* held, int64_t* capacity) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_archive_info: bad argument");
  if (held) *held = (int64_t)c->vol.arc.index.size();
  if (capacity) *capacity = c->vol.arc.capacity;
  return RPE_OK;
}

int rpe_volume_archive_download(rpe_context* c, int64_t* coords, float* tsdf, uint16_t* colour) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_archive_download: bad argument");
  auto& A = c->vol.arc;
  if (A.index.empty()) return RPE_OK;
  if (!coords || !tsdf) return fail(RPE_ERR_ARG, "rpe_volume_archive_download: coords and tsdf are required while bricks are held");
  HIP_TRY(hipSetDevice(c->device));
  size_t n = 0;
  for (const auto& kv : A.index) {
    coords[3 * n + 0] = kv.first[2]; coords[3 * n + 1] = kv.first[1]; coords[3 * n + 2] = kv.first[0];
    const size_t slot_words = (size_t)kv.second * (kSlot / 4);
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(tsdf) + n * kSlot, A.pool.get() + slot_words, kSlot, hipMemcpyDeviceToHost, c->stream));
    if (colour) {
      if (A.cpool) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(colour) + n * kSlot, A.cpool.get() + slot_words, kSlot, hipMemcpyDeviceToHost, c->stream));
      else std::memset(reinterpret_cast<char*>(colour) + n * kSlot, 0, kSlot);
    }
    n++;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

int rpe_volume_archive_clear(rpe_context* c) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "rpe_volume_archive_clear: bad argument");
  auto& A = c->vol.arc;
  A.index.clear();
  A.free.clear();
  for (int64_t slot = A.capacity - 1; slot >= 0; slot--) A.free.push_back((int32_t)slot);
  return RPE_OK;
}

}  // extern "C"
