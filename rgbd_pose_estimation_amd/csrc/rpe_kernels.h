// Internal launcher interface between the host units (rpe_host.hpp: rpe_capi.hip, rpe_refine.hip ...) and the gfx950 kernel units (rpe_normal_eq.hip,
// rpe_icp.hip, rpe_joint.hip, rpe_score.hip, rpe_nl.hip; shared device code: rpe_reduce.hpp, rpe_residuals.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rpe {

constexpr int kBlock = 256;          // 4 wave64 per workgroup
constexpr int kNeLd = 32;            // doubles per normal-equation / moment partial record
constexpr int kNlLd = 64;            // doubles per nl_round partial record
constexpr int kMaxScoreH = 8192;     // hypotheses per scoring launch (LDS vote table = 32 KiB)
// run records of a collecting launch kept on the device for a collective (ReduceTarget: rows > 0 with d_out set): kRunSlots slots of
// kRunLd doubles; a launch of <= 256 workgroups has at most 8 runs (rpe_reduce.hpp collect_and_send), absent ones are zero
constexpr int kRunSlots = 8;
constexpr int kRunLd = 32;

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }   // what the front end writes for "invalid"

// Correspondence arrays resident in HBM.  3 x n column-major (xyz interleaved), dtype 0 = f32, 1 = f64.
struct DeviceArrays {
  const void* a[5];        // RPE_XW, RPE_XC, RPE_BV, RPE_NW, RPE_NC
  short* mask[3];          // RPE_MOD_23 / 33 / NN (n shorts each) or null
  const void* weight[3];   // n Tp each or null
  int64_t n;
  int dtype;
};

// State of a device-resident Gauss-Newton loop (lives in HBM next to the pose; one launch per iteration, no host round trip).
struct GnState {
  double tol;        // stop when |delta| < tol
  double step, cost; // of the last iteration
  int max_iters;     // stop after this many iterations
  int iters;         // iterations done
  int done;          // 1: converged / failed / max_iters reached -> later launches of the same batch return at once
  int status;        // 0 ok, 1 normal equations not positive definite
};

// Peer-to-peer all-reduce of the 32-double record over xGMI, inside the reduction kernel (one process per GPU, <= 8 ranks).
// Every rank owns a mailbox in fine-grained HBM that all peers map through HIP IPC:
//   mailbox[parity 2][source rank kP2PMaxWorld][64 words], word = { lo 32 bits: one half of a double, hi 32 bits: step tag }.
// The tag travels WITH the data in one 8-byte store (the "LL" flag-in-data protocol), so no ordering between stores is assumed.
constexpr int kP2PMaxWorld = 8;
constexpr int kP2PWords = 64;                                  // 32 doubles = 64 halves
constexpr size_t kP2PRecordWords = (size_t)2 * kP2PMaxWorld * kP2PWords;             // [parity][source rank][64]
constexpr size_t kP2PVoteWords = (size_t)2 * kP2PMaxWorld * kMaxScoreH;              // [parity][source rank][hypothesis]
constexpr size_t kP2PMailboxBytes = (kP2PRecordWords + kP2PVoteWords) * 8;           // records first, vote counters behind
struct P2PDesc {
  int world, rank;
  unsigned long long* peer[kP2PMaxWorld];   // every rank's mailbox as mapped in THIS process; peer[rank] is the own one
};

// Where a reduction kernel leaves its result (both stages run inside one launch, see reduce_and_finish).
struct ReduceTarget {
  double* d_partials;          // max_blocks * kNlLd doubles of scratch
  unsigned int* d_ticket;      // 9 arrival counters 128 B apart (8 shards + top), zero between launches
  int max_blocks;              // cap on workgroups (= partial records)
  int block;                   // workgroup size 256 / 512 / 1024, 0 = default
  double* d_out;               // record in HBM (for a collective), or null
  double* h_out;               // record in pinned host memory + sequence word at [LD], or null
  unsigned long long seq;      // sequence value published after the record
  double* gn_pose = nullptr;   // device-resident GN: 12 doubles in HBM, read at kernel start, updated by the last workgroup
  GnState* gn = nullptr;       // its state (null = ordinary launch: pose from the kernel argument, record published)
  const P2PDesc* p2p = nullptr;   // multi-GPU: exchange + sum the record with the peers before publishing (h_out path only)
  unsigned long long p2p_step = 0;   // collective step counter, identical on every rank (tag + mailbox parity)
  int tail = -1;               // cross-workgroup stage of the ordinary kernels: -1 = default / RPE_TAIL
  // resident kernels: wait for the host's next pose at most this long (100 MHz ticks; 2 s)
  unsigned long long pose_wait_ticks = 200000000ull;
  unsigned long long fault_tag = 0;                    // test hook: see Finish
  double pivot_floor = 1e-12;  // device-side 6x6 solves: relative pivot floor (rpe::pivot_floor of the arrays' dtype, rpe/linalg.hpp)
  // > 0: collecting workgroups + host-side final sum -- runs of up to `rows` workgroups are added by the first workgroup of
  int rows = 0;
  // normal-equation kernels (one launch and resident): the flavour WITHOUT NaN guards.  Only for arrays known or about to be verified
  // to hold finite values: the shim launches it first and repeats the launch in the guarded flavour if the record comes back
  // non-finite (rpe_receive.hip clean-first protocol); results nobody on the host inspects use it only for arrays already verified
  bool clean = false;
  int solver = 0;              // autonomous resident loops: 1 = launch_auto_solver's workgroup sums, solves and hands the poses out
  const double* chain_runs = nullptr;   // chained sharded steps: see Finish (rpe_reduce.hpp)
  double* chain_pose_out = nullptr;
  int stride = 0;              // resident kernels: > 1 = strided runs (see Finish)
                               // the run, the run records go to h_out as tagged pairs (ordinary kernels: behind a header pair; h_out
                               // must hold
                               // 1 + ceil(grid / run length) x sums pairs), and the host adds them in order. Host-consumed, single-GPU
                               // results only
};
// ev_begin / ev_end (optional): the launch goes through hipExtLaunchKernelGGL and the two events receive the dispatch's own begin /
// end timestamps -- what rocprofv3 reports for the kernel (bench roofline timing)
#define RPE_LAUNCH_EV(KERNEL, GRID, BLOCK, SHMEM, STREAM, EV0, EV1, ...)                                              \
  do {                                                                                                                \
    if ((EV0) && (EV1)) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, EV0, EV1, 0, __VA_ARGS__);            \
    else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);                                         \
  } while (0)
hipError_t launch_normal_eq(const DeviceArrays& A, int kind, int flags, const double* pose12, const ReduceTarget& rt, hipStream_t s,
                            hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// RESIDENT form of the same kernels: one launch serves up to max_iters Gauss-Newton iterations; between iterations every workgroup
// waits for the next pose in `ctl` (16 words in fine-grained device memory written by the host: layout in rpe_residuals.hpp), tagged
// first_tag + i; the run records of iteration i (rt.rows) are published with sequence value rt.seq + i.  Needs host-writable device
// memory (large BAR).
constexpr unsigned long long kResidentStopBit = 1ull << 63;
// = kLostMarker (rpe_reduce.hpp): a run whose granules never arrived
constexpr unsigned long long kResidentLostMarker = 0x7ff8dead00c0ffeeull;
// How many 512-thread workgroups of the resident kernels the CURRENT device holds at once (occupancy of the heaviest instances x
// compute
// units, at most 256; 0 = none fits: no resident loops). Every resident launcher caps its grid with it: a collecting workgroup waits
// for
// workgroups of its own launch, so all of them must be on the compute units together.
int resident_cap_device();
// Each kernel unit is a code object of its own that the runtime loads on the first launch out of it (a few milliseconds, once per
// process and device).  rpe_create touches one kernel of every unit so that the first frame does not pay for it in the middle of a run.
// Every kernel unit ends with RPE_PRELOAD(<one of its kernels>): a node that links itself into a list when the library is loaded.  The
// head is a plain pointer, zero before any constructor runs, so the order in which the units' nodes are built does not matter;
// rpe_context.hip defines the constructor and walks the list (a unit without the line fails tests/test_isa_resources.py).
struct PreloadNode {
  const void* kernel;
  const PreloadNode* next;
  explicit PreloadNode(const void* kernel);
};
#define RPE_PRELOAD(...) static const ::rpe::PreloadNode unit_kernel((const void*)(__VA_ARGS__))
void resident_geometry(const DeviceArrays& A, int kind, int max_blocks, int* grid, int* nacc, int* max_rows, int* rows_auto);
// The solving workgroup of an autonomous resident loop (rpe_residuals.hpp solver_loop): ONE workgroup, launched on a stream of its own
// BEFORE the workers' kernel (launch_normal_eq_resident / launch_normal_eq_joint_resident with rt.solver = 1, same rt otherwise); nacc =
// 17 (point-to-point) or 29; workers = the grid of the workers' kernel (resident_geometry).  auto_solver_workers: that grid if the
// solving workgroup applies to it (enough workers, one compute unit to spare, RPE_AUTO_SOLVER != 0), else 0.
int auto_solver_workers(int grid);
int auto_solver_cap();   // the largest workers' grid that leaves the solving workgroup its compute unit
hipError_t launch_auto_solver(int nacc, int workers, unsigned long long first_tag, int max_iters, const ReduceTarget& rt, hipStream_t s);
// false: no resident instance serves this problem (fp64 arrays, 2D-3D kinds, more than one group per thread): one launch per iteration
bool normal_eq_resident_fits(const DeviceArrays& A, int kind, int max_blocks, bool autonomous_no_solver = false);
hipError_t launch_normal_eq_resident(const DeviceArrays& A, int kind, int flags, const unsigned long long* ctl,
    unsigned long long first_tag,
                                     int max_iters, const ReduceTarget& rt, hipStream_t s, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// test hook: one application of the device-resident loop's 6x6 LDL^T solve + SE(3) exp-map update (d_step_ok: |delta|, ok flag)
hipError_t launch_gn_update_probe(const double* d_rec32, double* d_pose12, double* d_step_ok, double pivot_floor, hipStream_t s);
hipError_t launch_moments(const DeviceArrays& A, int flags, const ReduceTarget& rt, hipStream_t s, hipEvent_t ev_begin = nullptr,
                          hipEvent_t ev_end = nullptr);
// chained sharded steps: the LAST solve + update (all-reduced run records of the final step, its pose) and the result to the host as
// tagged pairs: pose (12) | |delta| | cost | iterations | status
hipError_t launch_chain_finish(int kind, const double* d_runs, const double* d_pose, GnState* d_state, double pivot_floor, double* h_pairs,
                               unsigned long long seq, hipStream_t s);
// R1 lsq_pnp: sum of the sine residuals at pose7 (quaternion | t), arrays XW and BV; record = sum | count
hipError_t launch_sine_error(const DeviceArrays& A, const double* pose7, const ReduceTarget& rt, hipStream_t s, hipEvent_t ev_begin = nullptr,
                             hipEvent_t ev_end = nullptr);
// fused joint normal equations: terms = bit set over residual kinds (1 << kind); scale / robust / robust_k indexed by kind
hipError_t launch_normal_eq_joint(const DeviceArrays& A, int terms, int flags, const double* pose12, const double* scale4,
                                  const int* robust4, const double* robust_k4, const ReduceTarget& rt, hipStream_t s,
                                  hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// RESIDENT form of the joint kernel (one launch per refinement; control block, tags and run records as launch_normal_eq_resident;
// geometry = resident_geometry of a 29-sum kind)
// the resident form serves frame-sized problems only (one group per thread, the workgroup's slice staged in its LDS): true if this
// term set / size / mask-and-weight use fits; otherwise the refinement runs one launch of the joint kernel per iteration
bool joint_resident_fits(const DeviceArrays& A, int terms, int flags, int max_blocks, bool autonomous, bool clean);
// does the joint kernel of this term set have a CLEAN flavour (no NaN guards)?  rt.clean is ignored where it has none
bool joint_has_clean_flavour(int dtype, int terms);
hipError_t launch_normal_eq_joint_resident(const DeviceArrays& A, int terms, int flags, const double* scale4, const int* robust4,
                                           const double* robust_k4, const unsigned long long* ctl, unsigned long long first_tag, int max_iters,
                                           const ReduceTarget& rt, hipStream_t s);
// d_poses: H x 12 (fast: R row-major, t) or H x 8 (exact: qw qx qy qz tx ty tz pad) values of the array dtype.
// thr: {thre_3d (fast: squared), cos_thr, cos_nl} as doubles holding values of the array dtype.
// d_votes[0..H) must be zero on entry (launch_publish_votes leaves them so)
hipError_t launch_score(const DeviceArrays& A, int kind, int exact, const void* d_poses, int H, const double* thr3, int* d_votes,
                        int max_blocks, hipStream_t s);
// single-launch form for short lists (H <= score_small_cap): the hypotheses, staged in HOST memory in the layout above, travel as a
// kernel
// argument (h_poses), or are read from HBM (d_poses: a device-generated batch; exactly one of the two is non-null); rt must be a
// collecting target (rt.rows > 0); record[h] of the result = votes of hypothesis h
int score_small_cap(int dtype, int exact);
hipError_t launch_score_small(const DeviceArrays& A, int kind, int exact, const void* h_poses, const void* d_poses, int H,
    const double* thr3,
                              const ReduceTarget& rt, hipStream_t s);
// RESIDENT scoring (K4r): one launch serves a whole RANSAC run on resident arrays -- batches of up to kSessionHyps hypotheses (op 0) and
// the winner's masks (op 1) handed over through the control block (layout in rpe_score.hip), the counts back as run records of
// kSessionHyps sums each, published with sequence value rt.seq + batch number.  grid = score_resident_grid (0: not frame-sized).
constexpr int kSessionHypsMax = 32;
constexpr int kSessionCtlWordsMax = 512;   // = the context's 4-KB control block
int score_resident_grid(const DeviceArrays& A, int max_blocks);
hipError_t launch_score_resident(const DeviceArrays& A, int kind, int exact, const unsigned long long* ctl, unsigned long long first_tag,
                                 const double* thr3, int grid, const ReduceTarget& rt, hipStream_t s);
// pose12: fast = R row-major (9) t (3); exact = qw qx qy qz tx ty tz (rest ignored).  The vote total is record[0] of rt.
hipError_t launch_mask(const DeviceArrays& A, int kind, int exact, const double* pose12, const double* thr3, const ReduceTarget& rt,
                       hipStream_t s, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// params24 = c_opt(3) Cw(3) Cc(3) Rwc(9) pad; record = 64 doubles
hipError_t launch_nl_round(const DeviceArrays& A, const double* params24, const ReduceTarget& rt, hipStream_t s,
                           hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// copy `count` reduced values from HBM to pinned host memory and then store `seq` to *h_flag (the host spins on it)
hipError_t launch_publish_pairs(const double* d_src, int count, double* h_pairs, unsigned long long seq, hipStream_t s);   // {value, seq} pairs, no flag
// sharded scoring: exchange the `count` vote counters with the peers (same mailbox protocol as the records, one word per
// hypothesis), add them in rank order, publish the totals, zero the counters.  *h_status is set to 1 if a peer timed out.
hipError_t launch_publish_votes_p2p(int* d_votes, int count, const P2PDesc* p2p, unsigned long long step, int* h_dst, int* h_status,
                                    unsigned long long* h_flag, unsigned long long seq, hipStream_t s);
// publish the vote counters to pinned host memory, raise the sequence word, and zero the counters for the next launch_score
hipError_t launch_publish_votes(int* d_votes, int count, int* h_dst, unsigned long long* h_flag, unsigned long long seq, hipStream_t s);
hipError_t launch_publish_i32(const int* d_src, int count, int* h_dst, unsigned long long* h_flag, unsigned long long seq,
    hipStream_t s);

// ---- batched hypothesis generation (rpe_hypotheses.hip): `iters` RANSAC iterations of the 3-point closed form, sampled from the
// PCG32 stream (state, inc) exactly as the host sampler would; poses to d_poses in the scoring layout of `exact`, and to
// h_q7 (pinned, 8 values of the array dtype per iteration: qw qx qy qz tx ty tz valid) for the host's replay
hipError_t launch_gen_shinji(const DeviceArrays& A, unsigned long long state, unsigned long long inc, int iters, int exact,
    void* d_poses,
                             void* h_q7, hipStream_t s);

// FAST-mode generator of the plain-RANSAC solvers with a 4-point sample (tolerance parity): solver 0 = kneip_ransac (P3P), 1 =
// shinji_kneip_ransac (3-point fit, P3P), 2 = nl_kneip_ransac (P3P), 3 = nl_shinji_ransac (3-point fit, nl_2p), 4 =
// nl_shinji_kneip_ransac (3-point fit, P3P, nl_2p): gen_p3p_slots(solver) slots per iteration; same sample stream as the host (4 draws
// per iteration); d_poses in the FAST scoring layout (12 values per slot), h_q7 pinned, 8 values per slot (qw qx qy qz tx ty tz valid)
int gen_p3p_slots(int solver);
hipError_t launch_gen_p3p(const DeviceArrays& A, int solver, unsigned long long state, unsigned long long inc, int iters,
    void* d_poses, void* h_q7,
                          hipStream_t s);

// ---- PROSAC order (rpe_prosac.hip): the first top_k (<= kProsacMaxTopK) positions of "indices by weight descending, ties to the lower
// index" for n float weights in HBM.  d_hist: 2048 uints, zero on entry and on exit; d_ctl: 8 uints; d_cand: kProsacSortCap keys;
// d_status: 0 ok, 1 = more candidates than the LDS sort holds (heavy ties around the cut): use the host order.
constexpr int kProsacSortCap = 8192;
constexpr int kProsacMaxTopK = 4096;
hipError_t launch_prosac_order(const float* d_w, int n, int top_k, unsigned int* d_hist, unsigned int* d_ctl,
    unsigned long long* d_cand, int* d_order,
                               int* d_status, hipStream_t s);

// ---- front end (rpe_frontend.hip): depth frame -> maps -> projective association; fp32 throughout
struct Camera { float fx, fy, cx, cy; int width, height; };
struct PoseF { float R[9]; float t[3]; };   // Xc = R Xw + t, R row-major
// the C ABI's pose12 (R row-major | t, doubles) rounded to the kernels' fp32 pose: host units and launchers that take a pose12
inline PoseF pose_f(const double* p12) {
  PoseF T;
  for (int i = 0; i < 9; i++) T.R[i] = (float)p12[i];
  for (int i = 0; i < 3; i++) T.t[i] = (float)p12[9 + i];
  return T;
}
// coarse-to-fine pyramid: level l is (width >> l) x (height >> l) pixels, stored at pixel offset off[l] of the concatenated maps
// (off[l] is a multiple of 4: every level starts 16-byte aligned); block0 is set by the launchers
constexpr int kMaxLevels = 4;
struct PyramidGeometry { Camera cam[kMaxLevels]; int64_t off[kMaxLevels + 1]; int block0[kMaxLevels + 1]; int levels; };
// F1p (two launches): depth_out := metric depth of every level, vmap / nmap / bmap := F1's maps of every level
hipError_t launch_frame_pyramid(const void* d_depth, int depth_type, const PyramidGeometry& P, float scale, float dmin, float dmax,
                                float max_jump, float* depth_out, float* vmap, float* nmap, float* bmap, hipStream_t s);
// F2p (one launch): levels 1 .. P.levels-1 of the model maps from their level 0
hipError_t launch_model_pyramid(const PyramidGeometry& P, float* mv, float* mn, hipStream_t s);
// depth_type 0 = uint16 (metres = value * scale), 1 = float32 (metres = value * scale); maps are 3 x (width*height) floats
hipError_t launch_frame_maps(const void* d_depth, int depth_type, const Camera& cam, float scale, float dmin, float dmax,
    float max_jump,
                             float* vmap, float* nmap, float* bmap, hipStream_t s);
hipError_t launch_to_world(const float* vmap, const float* nmap, int64_t n, const PoseF& T, float* vw, float* nw, hipStream_t s);
// d_count (may be null): incremented by the number of associated pixels.  pose_dev (may be null): T read from HBM (12 doubles).
// done (may be null): device flag; when set the launch does nothing.
hipError_t launch_associate(const float* vmap, const float* nmap, const float* bmap, int64_t n, const float* mv, const float* mn,
                            const Camera& mcam, const PoseF& T, const PoseF& M, float dist_sq, float cos_thr, int use_normals,
                            const double* pose_dev, const int* done, float* xw, float* xc, float* bv, float* nw, float* nc, int* d_count,
                            hipStream_t s);
// ---- depth filter (rpe_filter.hip): F0, the optional stage in front of F1 / F1p.  ws = the (2 radius + 1)^2 spatial weights in row
// order (dy outer, dx inner), a / b = the range cut-off a + b z^2; all cast by the host once (include/rgbd_pose_hip.h Part 3)
constexpr int kFilterMaxRadius = 4;
struct FilterParams { int radius; float a, b; float ws[(2 * kFilterMaxRadius + 1) * (2 * kFilterMaxRadius + 1)]; };
// out := the filtered metric depth of the width x height image (NaN = invalid), what F1 / F1p then read as float32 with scale 1
hipError_t launch_depth_filter(const void* d_depth, int depth_type, int width, int height, float scale, float dmin, float dmax,
                               const FilterParams& P, float* out, hipStream_t s);
// ---- TSDF volume (rpe_volume.hip): voxels are float2 {tsdf, weight} at (k * dim1 + j) * dim0 + i; geometry cast from the descriptor's
// doubles once (include/rgbd_pose_hip.h Part 3)
struct VolumeGeometry { int dim[3]; float o[3]; float s, tr, W; };
// V1: fuse the level-0 vertex map (its z = metric depth, NaN = invalid) of camera `cam` under T (Xc = R Xw + t)
hipError_t launch_volume_integrate(float* vol, const VolumeGeometry& G, const float* vmap, const Camera& cam, const PoseF& T, hipStream_t s);
// V2: world vertex / normal maps (3 x width*height floats) of the view T with intrinsics cam, samples in (dmin, dmax)
hipError_t launch_volume_raycast(const float* vol, const VolumeGeometry& G, const Camera& cam, const PoseF& T, float dmin, float dmax,
                                 float* mv, float* mn, hipStream_t s);
// ---- mesh extraction (rpe_mesh.hip): marching cubes over the volume, ids placed by scans over chunks of kMeshChunk voxels.  The
// workspace is one allocation of mesh_workspace_bytes(nvox) (6 bytes per voxel plus 24 per chunk), cut by mesh_workspace.
constexpr int kMeshChunk = 4096;
struct MeshWorkspace {
  int chunks = 0;
  unsigned char *cases = nullptr, *used = nullptr;   // per voxel: the case of its cube, its used-edge bits
  int* first = nullptr;                              // per voxel with used edges: its first vertex id
  unsigned *chunk_v = nullptr, *chunk_t = nullptr;   // per chunk: vertex and triangle counts
  long long *off_v = nullptr, *off_t = nullptr;      // per chunk: their exclusive offsets
  long long* totals = nullptr;                       // {vertices, triangles}
};
size_t mesh_workspace_bytes(int64_t nvox);
MeshWorkspace mesh_workspace(void* ws, int64_t nvox);
// M1-M3: cases, used edges, chunk counts, their scan and the totals (min weight wmin > 0).  Only the cubes with lo <= (i, j, k) < hi per
// axis take part (rpe_volume_mesh_box); the full box is lo = 0, hi = dim - 1
struct MeshBox { int lo[3], hi[3]; };
hipError_t launch_mesh_count(const float* vol, const VolumeGeometry& G, float wmin, const MeshBox& B, const MeshWorkspace& W, hipStream_t s);
// M4-M5 after launch_mesh_count: 3 x V vertex and normal floats, 3 x T int32 triangle ids
hipError_t launch_mesh_emit(const float* vol, const VolumeGeometry& G, const MeshWorkspace& W, float* vertices, float* normals,
                            int* triangles, hipStream_t s);
// ---- colour (rpe_color.hip): frame colour RGBA8 per pixel; colour volume 4 binary16 {r, g, b, wc} per voxel, the tsdf's voxel index
// C1: n pixels of 3 bytes (bgr = 1: B, G, R order) -> RGBA8 with A = 255
hipError_t launch_frame_color(const unsigned char* rgb, int64_t n, int bgr, unsigned int* rgba, hipStream_t s);
// C2: V1 on vol plus the colour update of the band voxels (updated and sdf <= tr) from the frame colour rgba (level-0 pixels)
hipError_t launch_volume_integrate_color(float* vol, unsigned short* cvol, const VolumeGeometry& G, const float* vmap,
                                         const unsigned int* rgba, const Camera& cam, const PoseF& T, hipStream_t s);
// C3: RGBA8 of the colour field C at n world points (stride 3 floats)
hipError_t launch_color_sample(const unsigned short* cvol, const VolumeGeometry& G, const float* pts, int64_t n, unsigned int* rgba,
                               hipStream_t s);
// ---- colour registration (rpe_register.hip): a separate colour camera reprojected onto the depth frame.  Everything cast by the host
// once (include/rgbd_pose_hip.h Part 3): the colour camera, T = depth camera -> colour camera, the distortion k1 k2 p1 p2 k3, r2_max
// (0 = no limit), the z-buffer cell in colour pixels (0 = no occlusion test) with its grid gw x gh, the tolerance a + b zmin^2
struct RegisterRig { Camera cam; PoseF T; float k1, k2, p1, p2, k3, r2_max; int cell, gw, gh; float a, b; };
// R1: the z-buffer in its factored form ((gw + 1) * (gh + 1) words of base-cell minima, cleared to 0xffffffff by the caller; a cell's
// value is the minimum of four of them, rpe_register.hip) takes the bits of Xk.z of the n depth pixels of vmap
hipError_t launch_register_splat(const float* vmap, int64_t n, const RegisterRig& G, unsigned int* zbuf, hipStream_t s);
// R2: out[i] = RGBA8 of depth pixel i from the colour camera's RGBA8 image crgba, 0 where it has none; count (may be null):
// kRegCountWords words, cleared by the caller, whose SUM grows by the pixels with A = 255.  zbuf is not read with cell = 0
constexpr int kRegCountWords = 64;
hipError_t launch_register_gather(const float* vmap, int64_t n, const RegisterRig& G, const unsigned int* zbuf, const unsigned int* crgba,
                                  unsigned int* out, unsigned int* count, hipStream_t s);
// ---- photometric term (rpe_photo.hip).  P1: the frame's intensity pyramid (one float per pixel, levels concatenated as G says) from
// its level-0 RGBA8 colour.  P2: the model's photometric map (float4 {I, gx, gy, zm} per pixel, levels concatenated) from its level-0
// RGBA8 colour and its world vertex / normal maps; M = world -> model camera
hipError_t launch_frame_intensity(const unsigned int* rgba, const PyramidGeometry& G, float* out, hipStream_t s);
hipError_t launch_model_photo(const unsigned int* rgba, const PyramidGeometry& G, const float* mv, const float* mn, const PoseF& M,
                              float* out4, hipStream_t s);
// P3: one round of one level in one kernel -- the photometric rows (weight lam, gate dist_thr) and, geometric != 0, the point-to-plane
// rows of launch_icp_fused (use_normals = 1).  Record of kNlLd doubles: H (21) | g (6) of both terms | geometric cost | geometric
// pairs | photometric cost | photometric pairs
hipError_t launch_icp_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* mv, const float* mn,
                            const float* pmap4, const Camera& mcam, const PoseF& M, float dist_thr, float cos_thr, float lam, int geometric,
                            const double* pose12, const ReduceTarget& rt, hipStream_t s);
// P4: rows[k * n + i], k = 0 .. 6: {r, J[0..5]} (unscaled) of frame pixel i, NaN where it has no pair
hipError_t launch_photo_rows(const float* vmap, const float* fint, int64_t n, const float* pmap4, const Camera& mcam, const PoseF& M,
                             float dist_thr, const double* pose12, float* rows, hipStream_t s);
// ---- features (rpe_feature.hip): keypoints, descriptors, matches.  All integer arithmetic; ids come from scans, never from atomics.
constexpr int kMaxKeypoints = 4096;     // RPE_MAX_KEYPOINTS
constexpr int kFeatScoreBins = 4096;    // a score is at most 16 * 255
enum { kFeatCtlSurvivors = 0, kFeatCtlCut = 1, kFeatCtlTies = 2, kFeatCtlCount = 3, kFeatCtlMatches = 4, kFeatCtlWords = 8 };
// the detector's workspace for an image of n pixels: score (n ints), box sums (n u16), per-chunk survivor counts -> offsets
// (n / 256 + 2 ints), the score histogram, the control words above and the survivors' pixel indices ((n + w + h + 1) / 4 + 1 ints)
// (scale levels only: lum = Y | K << 8 of every level's pixels, kidx = the kept survivors' indices in the levels' index space)
struct FeatureWork { int* score; unsigned short* box; int* chunk; unsigned int* hist; int* ctl; int* spix; unsigned short* lum; int* kidx; };
// F1: detect + describe one view.  rgba / vmap / nmap: the view's RGBA8 colour, vertex and normal maps (w x h).  Leaves the number of
// keypoints in W.ctl[kFeatCtlCount] and pixel index, score, xy and descriptor of keypoint k at slot k, in pixel order.  Six kernels, no
// host wait.  kind = kDescUpright: D6, kp_bin untouched; kDescOriented: the sixth kernel is launch_feature_describe_oriented, which
// leaves the angle bin of keypoint k in kp_bin[k] too.
enum { kDescUpright = 0, kDescOriented = 1 };   // RPE_DESC_*
hipError_t launch_feature_detect(const unsigned int* rgba, const float* vmap, const float* nmap, int w, int h, int threshold, int max_keypoints,
                                 const FeatureWork& W, int kind, int* kp_pix, int* kp_score, int* kp_xy, unsigned int* kp_desc, int* kp_bin,
                                 hipStream_t s);
// D6o (rpe_feature_oriented.hip): xy, the oriented descriptor and the angle bin of the keypoints D5 left in kp_pix / ctl[kFeatCtlCount]
hipError_t launch_feature_describe_oriented(const unsigned int* rgba, const unsigned short* box, int w, int h, int max_keypoints,
                                            const int* ctl, const int* kp_pix, int* kp_xy, unsigned int* kp_desc, int* kp_bin,
                                            hipStream_t s);
// D3 / D5 on their own (rpe_feature.hip), for a detection whose other stages are not launch_feature_detect's: both work on a linear
// index -- chunk counts of nchunks chunks and W.hist in, W.ctl and the kept survivors' indices (in W.spix's order) and scores out
hipError_t launch_feature_scan(const FeatureWork& W, int nchunks, int max_keypoints, hipStream_t s);
hipError_t launch_feature_select(const FeatureWork& W, int max_keypoints, int* kp_idx, int* kp_score, hipStream_t s);
// ---- scale levels (rpe_feature_scale.hip): the detector on a fixed ladder of up to four levels of scale p / q = 1, 2/3, 1/2, 1/3, the
// levels' pixels laid end to end in ONE index space: index = base[l] + v * w[l] + u.  tile[l] = the first 32 x 8 tile of level l in
// D1s' grid, tiles_x[l] its tiles per row; entries from n on are empty levels (w = h = 0, base = base[4] = all pixels, tile = tile[4])
constexpr int kFeatMaxLevels = 4;
struct FeatLevels { int n; int w[kFeatMaxLevels], h[kFeatMaxLevels], base[kFeatMaxLevels + 1], tile[kFeatMaxLevels + 1], tiles_x[kFeatMaxLevels]; };
inline FeatLevels feature_levels(int w, int h, int n) {
  constexpr int P[kFeatMaxLevels] = {1, 2, 1, 1}, Q[kFeatMaxLevels] = {1, 3, 2, 3};
  FeatLevels L{};
  L.n = n;
  for (int l = 0; l < kFeatMaxLevels; l++) {
    L.w[l] = l < n ? w * P[l] / Q[l] : 0;
    L.h[l] = l < n ? h * P[l] / Q[l] : 0;
    L.tiles_x[l] = (L.w[l] + 31) / 32;
    L.base[l + 1] = L.base[l] + L.w[l] * L.h[l];
    L.tile[l + 1] = L.tile[l] + L.tiles_x[l] * ((L.h[l] + 7) / 8);
  }
  return L;
}
// F1 with L.n > 1 levels: eight launches (the histogram's memset, D0 resample, D1s, D2s, D3, D4s, D5, D6s or D6os), every stage once
// over all levels, no host wait.  Leaves what launch_feature_detect leaves -- the keypoints in (level, level pixel) order, kp_pix /
// kp_xy = the LEVEL-0 pixel a keypoint stands at -- and per keypoint its level and level pixel (kp_level, kp_lxy)
hipError_t launch_feature_detect_levels(const unsigned int* rgba, const float* vmap, const float* nmap, const FeatLevels& L, int threshold,
                                        int max_keypoints, const FeatureWork& W, int kind, int* kp_pix, int* kp_score, int* kp_xy,
                                        unsigned int* kp_desc, int* kp_bin, int* kp_level, int* kp_lxy, hipStream_t s);
// per keypoint of the list A: d1, index and d2 over the list B (ties to the lower index; d1 = d2 = 257, index -1 without any)
struct MatchLists { int *d1, *idx, *d2, *back; int *mf, *mm, *md1, *md2; float* mw; };
hipError_t launch_feature_best(const unsigned int* desc_a, int na, const unsigned int* desc_b, int nb, int* d1, int* idx, int* d2, hipStream_t s);
// the accepted matches of the nf frame keypoints, in frame-keypoint order (L.mf mm md1 md2 mw), their number in ctl[kFeatCtlMatches]
hipError_t launch_feature_accept(const MatchLists& L, int nf, int max_dist, int ratio_num, int ratio_den, int cross_check, int* ctl, hipStream_t s);
// the five solver slots of `matches` matches (3 floats per match each)
hipError_t launch_feature_gather(const MatchLists& L, int matches, const int* fpix, const int* mpix, const float* fv, const float* fn,
                                 const float* fb, const float* mv, const float* mn, float* xw, float* xc, float* bv, float* nw, float* nc,
                                 hipStream_t s);
// ---- keyframes (rpe_keyframe.hip): the features of many model views in one packed store, CSR-style -- keyframe k owns the keypoints
// off[k] .. off[k + 1] - 1 of desc (8 u32 each), xw / nw (3 floats each: the world vertex / normal at the keypoint) and xy (2 ints)
constexpr int kMaxKeyframes = 256;      // RPE_MAX_KEYFRAMES
struct KeyframeStore { int* off; unsigned int* desc; float* xw; float* nw; int* xy; };
// the acceptance test of rpe_features_match as the counting pass applies it; back = per store keypoint the frame keypoint that is its
// best (the cross-check), or nullptr
struct KeyframeAccept { int max_dist, ratio_num, ratio_den; const int* back; };
// K1: the model side's `count` keypoints (pix, xy, desc) and the model's vertex / normal maps at them, to the store from keypoint `base`
hipError_t launch_keyframe_snapshot(int count, const int* pix, const int* xy, const unsigned int* desc, const float* mv, const float* mn,
                                    const KeyframeStore& S, int base, hipStream_t s);
// K2: per keypoint q of list A (na of them) and segment g = 0 .. segments - 1 of list B: d1, index inside the segment and d2 at
// [g * na + q] (rules of launch_feature_best; d1 / d2 may be nullptr).  Segment g = keyframe seg0 + g of the store whose offsets are
// `off`, or, off == nullptr, the one list of one_n descriptors from one_lo.  counts != nullptr: counts[seg0 + g] += the pairs that
// pass `acc` (clear it first).
hipError_t launch_keyframe_best(const unsigned int* desc_a, int na, const unsigned int* desc_b, const int* off, int seg0, int segments,
                                int one_lo, int one_n, const KeyframeAccept& acc, int* d1, int* idx, int* d2, int* counts, hipStream_t s);
// K3: order[r] = the keyframe of rank r by (count descending, id ascending), K <= kMaxKeyframes
hipError_t launch_keyframe_rank(const int* counts, int K, int* order, hipStream_t s);
// K4: the five solver slots of `matches` matches (frame keypoint mf, keypoint mm of the keyframe that starts at `base`)
hipError_t launch_keyframe_gather(const int* mf, const int* mm, int matches, const int* fpix, const float* fv, const float* fn,
                                  const float* fb, const KeyframeStore& S, int base, float* xw, float* xc, float* bv, float* nw, float* nc,
                                  hipStream_t s);
// ---- keyframe graph (rpe_graph.hip): edges of keyframe-to-keyframe matches beside the store, and the joint Gauss-Newton round over
// all of them.  An edge (j, i), j > i, owns `count` pairs from `off` of the pair arrays a / b (positions inside keyframe j / keyframe
// i); `out` = the pairs of the edges before it in (j, i) order (where the row kernel writes).
struct GraphEdgeDev { int j, i, off, count, out, pad; };
constexpr int kGraphRaw = 40;           // doubles per edge the round kernel leaves (38 sums, layout in rpe_graph.hip)
constexpr int kGraphCorr = 12;          // floats per keyframe: C row-major (9) | c (3), X = C x + c
// G1: the accepted pairs of keyframe j's keypoints (na of them; d1 / idx / d2 = K2's rows over the segments 0 .. segs - 1), segment s
// written from pair base.v[s] in the order of j's keypoints, at most counts[s] of them (base.v[s] < 0: the segment is dropped).
// The bases travel as a kernel argument (1 KB)
struct GraphBases { int v[kMaxKeyframes]; };
hipError_t launch_graph_pack(const int* d1, const int* idx, const int* d2, int na, int segs, const int* off, const KeyframeAccept& acc,
                             const int* counts, const GraphBases& base, int* a, int* b, hipStream_t s);
// G2: one launch for every edge: the raw record of edge e at raw[e * kGraphRaw]
hipError_t launch_graph_round(const GraphEdgeDev* edges, int n_edges, const int* a, const int* b, const KeyframeStore& S, const float* corr,
                              float gate2, double* raw, hipStream_t s);
// G3: r of every pair at rows[3 * (out + k)], NaN where the pair does not count
hipError_t launch_graph_rows(const GraphEdgeDev* edges, int n_edges, const int* a, const int* b, const KeyframeStore& S, const float* corr,
                             float gate2, float* rows, hipStream_t s);
// G4: xw <- C_k xw + c_k, nw <- C_k nw for every keypoint of the K keyframes (`used` keypoints)
hipError_t launch_graph_apply(const KeyframeStore& S, int K, int used, const float* corr, hipStream_t s);
// ---- rebuilding the volume from keyframes (rpe_rebuild.hip).  A keyframe's attachment is its level-0 depth as a packed plane (one fp32
// per pixel, NaN = invalid) and, optionally, its RGBA8 colour; a list entry of the fuse is one attachment with the camera it was taken
// with and the pose it is fused at.  The table of a call lives in device memory (count <= kMaxKeyframes entries)
struct FuseEntry { const float* z; const unsigned int* rgba; Camera cam; PoseF T; };
// R1: z[i] = vmap[3 i + 2] for the n pixels of a vertex map; fcolor != nullptr: rgba[i] = fcolor[i] too
hipError_t launch_attach_pack(const float* vmap, const unsigned int* fcolor, int64_t n, float* z, unsigned int* rgba, hipStream_t s);
// R2: the entries fused in list order in one pass over the volume, each as V1 (color: as C2, cvol written too) would fuse it.  clear:
// the volume (and cvol) is taken as all zero and every voxel is written; cull = false switches the per-workgroup cull off
hipError_t launch_volume_fuse(float* vol, unsigned short* cvol, const VolumeGeometry& G, const FuseEntry* table, int count, bool clear,
                              bool color, bool cull, hipStream_t s);
// ---- moving the volume (rpe_shift.hip).  S1: out voxel (i, j, k) := voxel (i + shift[0], j + shift[1], k + shift[2]) of vol where that
// lies inside dim, zero bits elsewhere; cvol != nullptr: the colour volume likewise into cvol_out, in the same launch.  Out of place:
// vol_out / cvol_out must not overlap vol / cvol.  |shift[a]| <= dim[a] (the caller clears the volume itself for a larger one)
hipError_t launch_volume_shift(const float* vol, float* vol_out, const unsigned short* cvol, unsigned short* cvol_out, const int dim[3],
                               const int shift[3], hipStream_t s);
// ---- the volume archive (rpe_archive.hip): bricks of 8 x 8 x 8 voxels kept in a pool of slots, kArchiveSlotBytes per slot and volume,
// a brick's 64 rows of 8 voxels back to back in (z, y, x) order.  Every dim is a multiple of 8.
constexpr int kArchiveSlotBytes = 4096;
// up to three disjoint boxes of bricks: box b covers lo[b][a] .. lo[b][a] + n[b][a] - 1 on axis a; its bricks are numbered from
// first[b], x fastest; first[3] = the number of bricks of all boxes
struct ArchiveBoxes { int lo[3][3], n[3][3], first[4]; };
// A1: flags[g] = 1 if any 32-bit word of brick g of the boxes is non-zero in vol or (cvol != nullptr) in cvol, else 0
hipError_t launch_brick_occupancy(const float* vol, const unsigned short* cvol, const int dim[3], const ArchiveBoxes& B, unsigned int* flags,
                                  hipStream_t s);
// A2: n pairs {window brick = bx + nb0 * (by + nb1 * bz), slot}.  to_pool: slot := brick (cpool without cvol: the slot's colour is
// zeroed); else brick := slot (the colour only where cvol and cpool both exist).  A pair whose brick is not in the window or whose slot
// is not below capacity is skipped
hipError_t launch_brick_copy(bool to_pool, float* vol, unsigned short* cvol, unsigned int* pool, unsigned int* cpool, const int dim[3],
                             const int* pairs, int n, int capacity, hipStream_t s);
// ---- the map mesh (rpe_mapmesh.hip): marching cubes over the LISTED bricks of the map -- the window's and the archive's that lie in a
// box of world voxels -- one workgroup per brick.  The list is one upload of kMapListBytes per brick: key (ascending: the brick's
// coordinates in the box, bz << 34 | by << 17 | bx), src (>= 0: the window brick bx + nb0 * (by + nb1 * bz); < 0: ~slot of the pool)
// and nbr (27 list positions, entry (dz + 1) * 9 + (dy + 1) * 3 + dx + 1, -1 = absent).
constexpr int kMapKeyBits = 17;
constexpr size_t kMapListBytes = 8 + 4 + 27 * 4;
struct MapMeshView {
  const unsigned int *vol, *cvol, *pool, *cpool;   // the window's two volumes and the pool's two planes as words; null = all zeros
  int wdim0, wdim1, wnb[3], capacity;              // the window's row and plane lengths, its bricks per axis, the pool's slots
  int n;                                           // listed bricks
  const unsigned long long* key; const int* src; const int* nbr;
};
// per listed brick: 512 case bytes, 512 used-edge bytes, 512 first ids, the two counts and their offsets; totals behind
struct MapMeshWorkspace {
  unsigned char *cases = nullptr, *used = nullptr;
  int* first = nullptr;
  unsigned *brick_v = nullptr, *brick_t = nullptr;
  long long *off_v = nullptr, *off_t = nullptr, *totals = nullptr;
};
size_t map_mesh_workspace_bytes(int64_t bricks);
MapMeshWorkspace map_mesh_workspace(void* ws, int64_t bricks);
// P1-P2: the counts per listed brick (min weight wmin > 0), their scan, the totals
hipError_t launch_map_mesh_count(const MapMeshView& M, float wmin, const MapMeshWorkspace& W, hipStream_t s);
// P3-P4 after launch_map_mesh_count: G = the geometry of the box (dim = its voxels, o = its fp32 origin); colours (may be null: not
// sampled) = one RGBA8 per vertex
hipError_t launch_map_mesh_emit(const MapMeshView& M, const VolumeGeometry& G, const MapMeshWorkspace& W, float* vertices, float* normals,
                                int* triangles, unsigned int* colours, hipStream_t s);
// ---- the map raycast (kernels in rpe_frontend.hip): V2's rays through the map inside a box of world voxels.  The BRICK GRID is one int32
// per brick of the box, x fastest, in the codes of the map mesh's sources: >= 0 the window brick bx + nb0 * (by + nb1 * bz), < 0 the pool's
// slot ~slot, kMapAbsent (no ~slot equals it: capacity <= 2^24) for a brick the map does not hold
constexpr int kMapAbsent = -2147483647 - 1;
struct MapRayView {
  const unsigned int *vol, *cvol, *pool, *cpool;   // as MapMeshView
  int wdim0, wdim1, wdim2, wnb[3], capacity;       // the window's dims, its bricks per axis, the pool's slots
  int woff[3];                                     // the window's voxel (0, 0, 0) as an index of the box (clamped to +-2^21: far outside)
  int nb[3];                                       // the box's bricks per axis
  int wb0[3], wbn[3];                              // the window's bricks that lie in the box: the first, in window bricks, and how many
  int* grid;
};
// R0: the window's bricks in the box that hold no weight > 0 become kMapAbsent in the grid (exact: F is known only with eight weights > 0)
hipError_t launch_map_occupancy(const MapRayView& M, hipStream_t s);
// R1: world vertex / normal maps as launch_volume_raycast leaves them on the dense virtual volume G of the box; mc (may be null) = the
// RGBA8 colour field at each vertex, as launch_color_sample would leave it
hipError_t launch_map_raycast(const MapRayView& M, const VolumeGeometry& G, const Camera& cam, const PoseF& T, float dmin, float dmax,
                              float* mv, float* mn, unsigned int* mc, hipStream_t s);
// ---- the map fuse (kernel in rpe_mapfuse.hpp, compiled into rpe_frontend.hip): R2's list of keyframes fused into the bricks of a box of
// the map, wherever they lie.  Sources as in the brick grid: >= 0 the window brick, < 0 the pool's slot ~slot
struct MapFuseView {
  unsigned int *vol, *cvol, *pool, *cpool;         // the window's two volumes and the pool's two planes as words; null = none
  int wdim0, wdim1, wnb[3], capacity;              // as MapMeshView
  int nb[3];                                       // the box's bricks per axis
  const FuseEntry* table; int count, cull;         // R2's table
  int n;                                           // workgroups: every brick of the box (pass 1) or the list's entries (pass 2)
  const int* list;                                 // pass 2: {box brick (x fastest), source, fresh} per entry
  unsigned int* flags;                             // pass 1: per box brick, 1 = non-zero after the fuse from zeros | 2 = some voxel updated
};
// pass 1 over every brick of the box (G = the box's virtual volume), no volume access; M.list is not read
hipError_t launch_map_fuse_mark(const MapFuseView& M, const VolumeGeometry& G, bool color, hipStream_t s);
// pass 2 over M.list; clear: every entry is fresh.  M.flags is not read
hipError_t launch_map_fuse(const MapFuseView& M, const VolumeGeometry& G, bool clear, bool color, hipStream_t s);
// one ICP round in one kernel: association + normal equations of kind 0 (p2p) / 1 (p2plane, frame normals); record as launch_normal_eq
hipError_t launch_icp_fused(const float* vmap, const float* nmap, int64_t n, const float* mv, const float* mn, const Camera& mcam,
                            const PoseF& M, float dist_sq, float cos_thr, int use_normals, int kind, const double* pose12, const ReduceTarget& rt,
                            hipStream_t s);

// resident ICP loop (one launch; poses through the control block, run records to the host -- as launch_normal_eq_resident)
void icp_resident_geometry(int64_t n, int kind, int max_blocks, int* grid, int* nacc, int* max_rows, int* rows_auto);
hipError_t launch_icp_resident(const float* vmap, const float* nmap, int64_t n, const float* mv, const float* mn, const Camera& mcam,
    const PoseF& M,
                               float dist_sq, float cos_thr, int use_normals, int kind, const unsigned long long* ctl, unsigned long long first_tag,
                               int max_iters, const ReduceTarget& rt, hipStream_t s);

// ---- the volume term (rpe_frontend.hip; rule in rpe_sdf_rule.hpp): the frame level's vertices (and, with use_normals, normals) in the
// field of the dense volume `vol` under pose12.  One round in one kernel, record as launch_normal_eq's (H (21) | g (6) | sum r^2 | rows)
hipError_t launch_icp_sdf(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                          float cos_thr, int use_normals, const double* pose12, const ReduceTarget& rt, hipStream_t s);
// rows[k * n + i], k = 0 .. 6: {r, J[0..5]} of frame pixel i, NaN where it has no row
hipError_t launch_sdf_rows(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                           float cos_thr, int use_normals, const double* pose12, float* rows, hipStream_t s);
// ---- the map volume term (rpe_frontend.hip): the same two on the virtual volume G of a box of the map, through the brick grid of M
// (as launch_map_raycast takes them; the colour planes, wnb, wb0, wbn are not read).  Rows bit for bit launch_sdf_rows' on a dense copy
hipError_t launch_icp_map_sdf(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G, float dist_thr,
                              float cos_thr, int use_normals, const double* pose12, const ReduceTarget& rt, hipStream_t s);
hipError_t launch_map_sdf_rows(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G, float dist_thr,
                               float cos_thr, int use_normals, const double* pose12, float* rows, hipStream_t s);

// ---- the volume colour term (rpe_sdf_photo.hpp, compiled into rpe_frontend.hip): the photometric rows of a frame against the colour
// volume cvol (4 binary16 per voxel at the tsdf's index) beside the volume term's, one round in one kernel.  fint: the level's frame
// intensity.  geometric != 0: the volume term's rows (weight 1) as well.  Record of kNlLd doubles laid out as launch_icp_photo's
hipError_t launch_icp_sdf_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol, const unsigned short* cvol,
                                const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                const double* pose12, const ReduceTarget& rt, hipStream_t s);
// rows[k * n + i], k = 0 .. 6: {r, J[0..5]} (unscaled) of the photometric row of frame pixel i, NaN where it has no row
hipError_t launch_sdf_photo_rows(const float* vmap, const float* fint, int64_t n, const float* vol, const unsigned short* cvol,
                                 const VolumeGeometry& G, float dist_thr, const double* pose12, float* rows, hipStream_t s);
// ---- the map volume colour term (rpe_map_sdf_photo.hpp, compiled into rpe_frontend.hip): the same two on the virtual volume G of a box
// of the map and its virtual colour volume, through the brick grid of M (as launch_map_raycast takes them, the colour sources M.cvol /
// M.cpool included, either may be null; wnb, wb0, wbn are not read).  Rows bit for bit launch_sdf_photo_rows' on dense copies
hipError_t launch_icp_map_sdf_photo(const float* vmap, const float* nmap, const float* fint, int64_t n, const MapRayView& M,
                                    const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                    const double* pose12, const ReduceTarget& rt, hipStream_t s);
hipError_t launch_map_sdf_photo_rows(const float* vmap, const float* fint, int64_t n, const MapRayView& M, const VolumeGeometry& G,
                                     float dist_thr, const double* pose12, float* rows, hipStream_t s);
// ---- the robust volume terms (rpe_sdf_robust.hpp, compiled into rpe_frontend.hip; the weight's rule in rpe_sdf_robust_rule.hpp): the
// four round launchers above with a robust weight on every row -- kind 1 (Huber) or 3 (Tukey), k the geometric row's scale [m], photo_k
// the photometric row's [unscaled levels; 0: weight 1].  Records laid out as the unweighted launchers'; the row counts count every row
constexpr int kRobustNone = 0, kRobustHuber = 1, kRobustTukey = 3;   // RPE_ROBUST_NONE / _HUBER / _TUKEY (rpe_sdf_api.hip asserts it)
hipError_t launch_icp_sdf_robust(const float* vmap, const float* nmap, int64_t n, const float* vol, const VolumeGeometry& G, float dist_thr,
                                 float cos_thr, int use_normals, int kind, float k, const double* pose12, const ReduceTarget& rt, hipStream_t s);
hipError_t launch_icp_map_sdf_robust(const float* vmap, const float* nmap, int64_t n, const MapRayView& M, const VolumeGeometry& G,
                                     float dist_thr, float cos_thr, int use_normals, int kind, float k, const double* pose12,
                                     const ReduceTarget& rt, hipStream_t s);
hipError_t launch_icp_sdf_photo_robust(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol,
                                       const unsigned short* cvol, const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals,
                                       float lam, int geometric, int kind, float k, float photo_k, const double* pose12, const ReduceTarget& rt,
                                       hipStream_t s);
hipError_t launch_icp_map_sdf_photo_robust(const float* vmap, const float* nmap, const float* fint, int64_t n, const MapRayView& M,
                                           const VolumeGeometry& G, float dist_thr, float cos_thr, int use_normals, float lam, int geometric,
                                           int kind, float k, float photo_k, const double* pose12, const ReduceTarget& rt, hipStream_t s);
// the tests' hook: out[i] = the weight of frame pixel i's row (photo != 0: the photometric row's; fint, cvol and the colour sources of M
// are read only then), NaN where it has no row.  M = null: the dense window vol / cvol; else the map through M.  kind 0 or scale 0: 1
hipError_t launch_sdf_robust_weights(const float* vmap, const float* nmap, const float* fint, int64_t n, const float* vol,
                                     const unsigned short* cvol, const MapRayView* M, const VolumeGeometry& G, float dist_thr, float cos_thr,
                                     int use_normals, int photo, int kind, float scale, const double* pose12, float* out, hipStream_t s);
}  // namespace rpe
