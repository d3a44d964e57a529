/* rgbd_pose_hip.h -- C ABI of librgbdpose_hip.so, the MI355X (gfx950) backend of the RGB-D absolute-pose
 * hot path of ShudaLi/rgbd_pose_estimation.  Plain pointers and sizes only; no C++ / torch types.
 *
 * Part 1 is the reference's own FFI, byte for byte (reference Library.cpp:15-82 -> libabsolute.so).
 * Part 2 is additive: a handle-based API over correspondence arrays that stay resident in HBM, one entry
 * point per hot loop of the reference plus the Gauss-Newton formulation the north
 * star asks for.  Every function returns 0 on success or a negative rpe_status; rpe_last_error() explains.
 *
 * Conventions (same as the reference): Xc = R_cw * Xw + t (pose/AbsoluteOrientation.hpp:51); 3 x N arrays
 * are column-major = N packed xyz triples (Eigen Map<MatrixXf>(p,3,n), Library.cpp:20-22); rotation
 * matrices cross this boundary ROW-major (Library.cpp:35-39); masks are short 0/1 (N x cols column-major,
 * column 0 = 2D-3D, 1 = 3D-3D, 2 = normal-normal: pose/NormalAOPoseAdapter.hpp:179-195).
 */
#ifndef RGBD_POSE_HIP_H
#define RGBD_POSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Part 1 -- drop-in replacements for libabsolute.so
 * ---------------------------------------------------------------------------------------------- */

/* Replaces ao() (Library.cpp:17-45): closed-form 3D-3D absolute orientation over ALL n correspondences
 * (AOOnlyPoseAdapter + shinji_ls2, pose/AbsoluteOrientation.hpp:322-342).  x_w_, x_c_: n xyz float triples
 * (host).  R_cw_[9] row-major, t_[3].  The moment sums run on the GPU with fp64 accumulation; the 3x3 SVD
 * on the host.  Prints "ao()" like the reference unless RPE_QUIET=1.  Aborts like the reference
 * (SOPHUS_ENSURE) only if no HIP device is usable: then it prints the reason and calls abort(). */
void ao(float* x_w_, float* x_c_, int n_, float* R_cw_, float* t_);

/* Replaces ao_ransac() (Library.cpp:47-75): shinji_ransac2 (Iter=1000, thre_3d=0.1, confidence=0.99999,
 * pose/AbsoluteOrientation.hpp:158-213) with the vote loop scored on the GPU in hypothesis batches, then
 * shinji_ls1 over the inliers (:298-320).  Sampling uses the documented Rand31 stream (seed RPE_SEED, default 1)
 * instead of the reference's unseeded rand(). */
void ao_ransac(float* x_w_, float* x_c_, int n_, float* R_cw_, float* t_);

/* Replaces py2c() (Library.cpp:77-81): prints N floats, one per line. */
void py2c(float* array, int N);

/* ------------------------------------------------------------------------------------------------
 * Part 2 -- additive handle-based API
 * ---------------------------------------------------------------------------------------------- */

typedef enum {
  RPE_OK = 0,
  RPE_ERR_NO_DEVICE = -1,     /* no HIP device / HIP runtime error: the product has NO CPU fallback */
  RPE_ERR_HIP = -2,
  RPE_ERR_ARG = -3,
  RPE_ERR_STATE = -4,         /* a required array was never uploaded / bound */
  RPE_ERR_DEGENERATE = -5,    /* normal equations not positive definite, or NaN result.  A pivot at or below 16 eps of the ARRAYS' dtype x its
                               * diagonal entry (9.5e-7 for fp32 arrays, 1e-12 for fp64) counts: the cancelled pivots of rank-deficient sets -- one
                               * repeated point, a line, a single plane seen point-to-plane -- are rounding noise of the products, of either sign */
  RPE_ERR_ALIGN = -6          /* bound device pointer not 16-byte aligned */
} rpe_status;

typedef struct rpe_context rpe_context;

int rpe_abi_version(void);
const char* rpe_last_error(void);
int rpe_device_count(void);            /* number of usable HIP devices (0 on a CPU-only host) */

/* stream: a hipStream_t the caller owns (e.g. torch's current stream), or NULL for a private stream. */
int rpe_create(rpe_context** out, int device, void* stream);
void rpe_destroy(rpe_context* ctx);
int rpe_synchronize(rpe_context* ctx);

/* dtype of the correspondence arrays: Tp of the reference's templates */
enum { RPE_F32 = 0, RPE_F64 = 1 };
/* array slots.  Names follow the adapters' members. */
enum {
  RPE_XW = 0,   /* points_g       world points         PnPPoseAdapter.hpp:100        */
  RPE_XC = 1,   /* points_c       camera points        AOPoseAdapter.hpp:95 (NaN column = invalid, :147-152) */
  RPE_BV = 2,   /* bearingVectors unit bearings        PnPPoseAdapter.hpp:98         */
  RPE_NW = 3,   /* normal_g       world normals        NormalAOPoseAdapter.hpp:95    */
  RPE_NC = 4,   /* normal_c       camera normals       NormalAOPoseAdapter.hpp:94    */
  RPE_NUM_ARRAYS = 5
};
/* per-modality inlier masks (short) and weights (Tp), index = mask column */
enum { RPE_MOD_23 = 0, RPE_MOD_33 = 1, RPE_MOD_NN = 2 };

/* Declare the correspondence count and dtype; (re)allocates nothing until an upload. */
int rpe_set_problem(rpe_context* ctx, int64_t n, int dtype);
/* Copy a host array (3 x n, dtype of the problem) into HBM.  Asynchronous on the context stream. */
int rpe_upload(rpe_context* ctx, int slot, const void* host);
/* Copy array `slot` back to the host (3 x n of the problem's dtype); synchronises.  For arrays produced on the device
 * (rpe_associate) and for tests. */
int rpe_download(rpe_context* ctx, int slot, void* host);
/* Use a buffer that already lives in HBM (must be 16-byte aligned, 3*n elements); no copy, not owned. */
int rpe_bind(rpe_context* ctx, int slot, const void* device_ptr);
/* n shorts (0/1) / n weights for one modality; host pointers, NULL clears. */
int rpe_upload_mask(rpe_context* ctx, int modality, const short* host_mask);
int rpe_upload_weight(rpe_context* ctx, int modality, const void* host_weight);
/* Copy the device mask written by rpe_inlier_mask back to the host (n shorts). */
int rpe_download_mask(rpe_context* ctx, int modality, short* host_mask);

/* ---- K1' closed-form moments: the two passes of shinji() (AbsoluteOrientation.hpp:56-73) fused into ONE
 * pass.  out[18] = { sum w, sum w*Xw (3), sum w*Xc (3), sum w*Xc*Xw^T (9, row-major), sum w*|Xc|^2, count of
 * contributing correspondences }.
 * flags: RPE_USE_MASK -> only mask33 == 1 (shinji_ls/shinji_ls1 inlier set, :279-288); RPE_USE_WEIGHT ->
 * w = weight33 (nl_shinji_kneip_ls centroid pass, AbsoluteOrientationNormal.hpp:457-469);
 * RPE_SKIP_INVALID -> skip NaN columns (isValid).  fp32 inputs are widened, all arithmetic is fp64. */
enum { RPE_USE_MASK = 1, RPE_USE_WEIGHT = 2, RPE_SKIP_INVALID = 4 };
int rpe_p2p_moments(rpe_context* ctx, int flags, double* out18);
/* Closed-form pose from the moments (host: 3x3 SVD, det fix, t = Cc - R*Cw; AbsoluteOrientation.hpp:75-95). */
int rpe_pose_from_moments(const double* m18, double* R9, double* t3);

/* ---- R1 lsq_pnp (P3P.hpp:472-502): the sum over ALL correspondences of the sine of the angle between predicted and observed
 * bearing, sum_i | normalize(R*Xw_i + t) x bv_i | (what PnPPoseAdapter::getError(i) returns, PnPPoseAdapter.hpp:204-210).
 * pose7 = unit quaternion (w, x, y, z) | t, rounded to the array dtype; every term is evaluated in the array dtype by the
 * reference's own operation sequence (the reference's bits), the terms are added in fp64 -- the reference adds them one after
 * the other in Tp, so its printed total differs from *sum_out by its own accumulated rounding only.  Arrays XW, BV (24 B/corr fp32).
 * count_out (optional): the number of terms. */
int rpe_sine_error_sum(rpe_context* ctx, const double* pose7, double* sum_out, int64_t* count_out);

/* ---- K1/K2/K3 Gauss-Newton normal equations (new formulation; objective of K1 == shinji()).
 * kind: residual.  pose12 = R row-major (9) | t (3).  out32: H upper triangle row-major (21) | g (6) |
 * sum w r^2 | sum w | 3 pad.  Tangent order (upsilon, omega), update T <- exp(delta)*T (sophus/se3.hpp:314-342).
 * The pose enters the kernel in fp64; p = R*Xw + t and the residual are formed in fp64 (the subtraction
 * cancels ~3 digits), the products in the array dtype, the sums in fp64. */
enum {
  RPE_RES_P2P = 0,      /* r = R*Xw + t - Xc                         (3)  arrays XW, XC      24 B/corr fp32 */
  RPE_RES_P2PLANE = 1,  /* r = Nc . (R*Xw + t - Xc)                  (1)  arrays XW, XC, NC  36 B/corr      */
  RPE_RES_BEARING = 2,  /* r = normalize(R*Xw + t) x bv  (P3P.hpp:482-485) (3)  arrays XW, BV  24 B/corr      */
  RPE_RES_NORMAL = 3,   /* r = R*Nw - Nc   (alignment scored at AbsoluteOrientationNormal.hpp:248) (3)  arrays NW, NC  24 B/corr;
                           rotation only.  Served by the joint kernel (rpe_normal_eq_joint); mask / weight of modality NN */
  RPE_RES_REPROJ = 4    /* 2D-3D pixel reprojection, r = (p_x/p_z - bv_x/bv_z, p_y/p_z - bv_y/bv_z), p = R*Xw + t   (2)  arrays XW, BV
                           24 B/corr; mask / weight of modality 23.  The pixel conversion of TestMain.cpp:35-36 with the principal point at
                           the origin (PoseAdapterBase.hpp:44), in NORMALISED image coordinates: the focal length multiplies r and J alike,
                           so the step does not depend on it -- scale the term by f^2 (rpe_term.scale, `scales` of rpe_gn_refine) for H, g
                           and the cost in pixels.  Correspondences with p_z <= 1e-6 or bv_z <= 1e-6 (not in front of the camera) contribute
                           nothing and do not count.  Alternative to RPE_RES_BEARING for the 2D-3D term of the joint kernel. */
};
int rpe_normal_eq(rpe_context* ctx, int kind, int flags, const double* pose12, double* out32);
/* Same, result left in HBM at d_out32 (32 doubles, must not be NULL) for a caller-side collective (RCCL
 * all-reduce); asynchronous on the context's stream. */
int rpe_normal_eq_device(rpe_context* ctx, int kind, int flags, const double* pose12, double* d_out32);
/* Host: solve H*delta = -g (LDL^T); RPE_ERR_DEGENERATE if H is not positive definite.  ne32[29], as rpe_normal_eq* fill it in, is the
 * relative pivot floor that goes with the record's product dtype (0 = 1e-12). */
int rpe_gn_solve(const double* ne32, double* delta6);
/* Host: pose <- exp(delta) * pose  (Sophus SE3::exp, sophus/se3.hpp:321-342). */
int rpe_gn_apply(const double* delta6, double* pose12);
/* ---- fused joint normal equations: up to four residual kinds (at most one of P2P / P2PLANE) in ONE pass over the arrays,
 * each term with its modality's inlier mask (RPE_USE_MASK) and weights (RPE_USE_WEIGHT), a scale, and an optional robust
 * IRLS weight on the residual-block norm s: Huber min(1, k/s) or Cauchy 1/(1 + (s/k)^2).  out32 as rpe_normal_eq, with
 * cost = sum scale*w*r^2 and the last entry = number-weighted count over all terms.  This is the single-kernel form of the
 * joint 2D-3D + 3D-3D + N-N objective the reference's nl_shinji_kneip_ls alternates over (:484-510). */
enum { RPE_ROBUST_NONE = 0, RPE_ROBUST_HUBER = 1, RPE_ROBUST_CAUCHY = 2,
       RPE_ROBUST_TUKEY = 3 /* the volume terms only (rpe_sdf_set_robust): a term of this list with it is RPE_ERR_ARG */ };
typedef struct { int kind; double scale; int robust; double robust_k; } rpe_term;
int rpe_normal_eq_joint(rpe_context* ctx, int nterms, const rpe_term* terms, int flags, const double* pose12, double* out32);
int rpe_gn_refine_joint(rpe_context* ctx, int nterms, const rpe_term* terms, int flags, double* pose12, int max_iter, double tol,
                        int* iters_out, double* last_step, double* final_cost);

/* Device-resident variant of rpe_gn_refine_joint: pose and loop state stay on the GPU, which solves the 6x6 system (LDL^T) and
 * applies the SE(3) exp-map update itself; the host waits once.  One GPU and a single plain point-to-point or point-to-plane term
 * (scale 1, no robust weight): ONE launch whose resident grid iterates by itself until |delta| < tol or max_iter.  Otherwise one
 * launch per iteration whose last workgroup solves (the host enqueues max_iter launches; those after convergence return
 * immediately).  Same arithmetic as the host loop.  RPE_DEVICE_LOOP_RESIDENT=0 selects the per-iteration form everywhere.
 * After rpe_p2p_init the loop is SHARDED: every launch's last workgroup first exchanges and sums the record with its peers, so
 * the refinement stays one launch per iteration on any number of GPUs of a node (collective: all ranks call it alike). */
int rpe_gn_refine_device(rpe_context* ctx, int nterms, const rpe_term* terms, int flags, double* pose12, int max_iter, double tol,
                         int* iters_out, double* last_step, double* final_cost);

/* Test hook for the device-resident loop: ONE application, ON THE GPU, of what its last workgroup does with a record -- the register
 * LDL^T solve of H delta = -g and pose <- exp(delta) * pose with the kernel's own SE(3) exponential (sophus/se3.hpp:321-342) -- to a
 * record and pose of the caller's.  RPE_ERR_DEGENERATE where the device solve refuses the system. */
int rpe_debug_device_gn_update(rpe_context* ctx, const double* ne32, double* pose12, double* step_norm);

/* One Gauss-Newton step on one GPU (kernel -> D2H of the 32-double record -> solve -> exp-map update of pose12).
 * ne32_out / step_norm may be NULL. */
int rpe_gn_step(rpe_context* ctx, int kind, int flags, double* pose12, double* ne32_out, double* step_norm);
/* ---- multi-GPU: one process per GPU, correspondences sharded by contiguous index ranges, pose replicated.
 * rank 0 obtains a 128-byte id (rpe_comm_unique_id) and hands it to every rank by any means (MPI, torch.distributed,
 * a file); each rank then calls rpe_comm_init on its context (RCCL communicator on that context's device; librccl is
 * resolved at run time).  rpe_gn_step_dist = rpe_gn_step with ONE in-place all-reduce(sum) of the 32-double record over
 * RCCL/xGMI between the kernel and the host solve; every rank ends the step with the same pose.  With a communicator set,
 * rpe_score all-reduces the H int32 vote counters the same way. */
int rpe_comm_unique_id(void* id128);
int rpe_comm_init(rpe_context* ctx, int world, int rank, const void* id128);
int rpe_comm_destroy(rpe_context* ctx);
/* ranks of the context's RCCL communicator as the communicator reports them (ncclCommCount; 0 = none), and the PCI bus id of the
 * context's GPU (one process per GPU: every rank of a node reports a different one) */
int rpe_comm_count(rpe_context* ctx, int* ranks);
int rpe_device_bus_id(rpe_context* ctx, char* buf, int len);
int rpe_gn_step_dist(rpe_context* ctx, int kind, int flags, double* pose12, double* ne32_out, double* step_norm);
/* `steps` such steps in one call (every rank passes the same count). */
int rpe_gn_steps_dist(rpe_context* ctx, int kind, int flags, double* pose12, int steps, double* last_step_norm);
/* The same `steps` steps over the RCCL communicator with the HOST OUT OF THE LOOP: every launch takes its pose from the launch before
 * it (each workgroup adds that step's all-reduced run records, solves the 6x6 system and applies the exp-map itself), so the calling
 * thread enqueues steps x {kernel, ncclAllReduce} plus one finishing kernel and waits once -- a launch's latency overlaps the kernels
 * in front of it instead of adding to every step.  The SE(3) update runs on the device (the device-resident loops' solve, equal to the
 * host's to 1e-13); rpe_gn_steps_dist is the form with the exp-map on the host.  Needs rpe_comm_init; every rank passes the same
 * arguments and ends with the same pose.  RPE_ERR_DEGENERATE if a step's normal equations are not positive definite. */
int rpe_gn_steps_dist_device(rpe_context* ctx, int kind, int flags, double* pose12, int steps, double* last_step_norm);
/* Peer-to-peer variant of the collective for ONE node (<= 8 ranks): instead of RCCL, the normal-equation kernel's last
 * workgroup writes the 32-double record straight into a mailbox of every peer over xGMI (HIP IPC mappings, flag-in-data
 * words), waits for the peers' records in its own mailbox, adds them in rank order and publishes the sum -- the whole sharded
 * step is ONE kernel launch, and every rank gets bitwise the same record.  Each rank calls rpe_p2p_export (64-byte IPC handle),
 * all handles are gathered by any means (world x 64 bytes, rank order), each rank calls rpe_p2p_init; rpe_gn_step_dist then
 * uses this path (it takes precedence over an RCCL communicator), and rpe_score exchanges and sums its vote counters the same
 * way.  A rank that waits more than 10 s for a peer fails the step with RPE_ERR_HIP instead of hanging; ranks should therefore
 * enter their first exchange together (one local launch + a barrier).  Callers barrier before rpe_p2p_destroy. */
int rpe_p2p_export(rpe_context* ctx, void* handle64);
int rpe_p2p_init(rpe_context* ctx, int world, int rank, const void* handles);
/* pause = 1 keeps the mailboxes but routes rpe_gn_step_dist / rpe_score through the RCCL communicator (stand-by); 0 resumes. */
int rpe_p2p_pause(rpe_context* ctx, int pause);
int rpe_p2p_destroy(rpe_context* ctx);
/* What the exact scoring kernels compare the SQUARED 3D residual with (dtype RPE_F32: evaluated in float): the smallest value whose
 * correctly rounded square root reaches thre_3d, so that  sqrt(s) < thre_3d  <=>  s < cut  for every s (test hook; no GPU involved). */
double rpe_host_sqrt_cut(int dtype, double thre_3d);
/* Host-side exchange for ONE node (the third way to all-reduce; csrc/rpe_hostex.cpp): on one GPU a reduction's final sum already
 * happens on the host (a few run records per launch, added by the calling thread), so with sharded correspondences every rank's host
 * thread holds its shard's record microseconds after its kernel -- and the rank processes share the node's memory.  The records are
 * exchanged between the host threads through a POSIX shared-memory segment and added in RANK ORDER (bitwise the same sums on every
 * rank): no collective kernel, no GPU-side wait for a peer.  rpe_hostex_init(ctx, world, rank, name, create): `name` ("/...") is
 * agreed by any means; exactly one rank passes create = 1 and must do so before the others open (they wait up to the time-out for the
 * segment to appear).  With an exchange set,
 * rpe_gn_step_dist / rpe_gn_steps_dist / rpe_gn_refine are sharded steps (the exchange takes precedence over rpe_p2p_* and
 * rpe_comm_*), rpe_gn_refine keeps its RESIDENT kernel per rank (one GPU per rank; ranks that share a GPU fall back to one launch per
 * iteration, because two resident grids that wait for each other's hosts cannot both be resident), and rpe_score adds the vote counters
 * the same way.  Every wait is bounded (10 s): a missing peer fails the call with RPE_ERR_STATE. */
int rpe_hostex_init(rpe_context* ctx, int world, int rank, const char* name, int create);
int rpe_hostex_destroy(rpe_context* ctx);
/* The exchange by itself (no GPU involved; what the two calls above wrap): */
typedef struct rpe_host_exchange rpe_host_exchange;
int rpe_host_exchange_open(const char* name, int world, int rank, int create, double timeout_s, rpe_host_exchange** out);
int rpe_host_exchange_allreduce_f64(rpe_host_exchange* h, double* v, int n);   /* in place, 1 <= n <= 64, sums in rank order */
int rpe_host_exchange_allreduce_i32(rpe_host_exchange* h, int* v, int n);      /* in place, 1 <= n <= 8192 */
int rpe_host_exchange_set_label(rpe_host_exchange* h, const char* label);      /* e.g. the rank's GPU (PCI bus id) */
int rpe_host_exchange_labels_collide(rpe_host_exchange* h);                    /* after an exchange: do two ranks carry the same label? */
int rpe_host_exchange_unlink(rpe_host_exchange* h);                            /* drop the name once every rank has opened it */
void rpe_host_exchange_close(rpe_host_exchange* h);
/* Whole refinement loop on one GPU: up to 3 residual kinds summed with scales; stops when |delta| < tol.
 * iters_out = iterations run; returns RPE_ERR_DEGENERATE if a solve failed. */
int rpe_gn_refine(rpe_context* ctx, int nterms, const int* kinds, const double* scales, int flags, double* pose12, int max_iter,
                  double tol, int* iters_out, double* last_step, double* final_cost);

/* Host-clock profile of rpe_gn_refine's resident loop (one GPU): enable = 1 clears and starts; enable = 0 stops and returns the sums, in
 * microseconds over `steps` steady-state iterations, of the host's WAIT for a record (pose hand-over in flight + one iteration of the
 * resident kernel + record in flight) and of the host's own turn (6x6 solve + SE(3) update + hand-over stores). */
int rpe_debug_loop_profile(rpe_context* ctx, int enable, double* wait_us, double* host_us, long long* steps);

/* State of a context's RESIDENT loops (rpe_gn_refine, rpe_gn_refine_joint, rpe_icp, rpe_gn_refine_device run as ONE launch whose grid
 * must be on the compute units all at once).  enabled: large-BAR device, at least one workgroup of the resident kernels per compute
 * unit, and fewer than two lost grids so far; lost: refinements whose grid lost a workgroup's sums (another process on the GPU, a
 * partition smaller than the occupancy query promised) and that were FINISHED with one launch per iteration -- such a call still
 * succeeds, a context that sees it twice stops using resident loops; cap: workgroups of a resident kernel the device holds at once
 * (occupancy x compute units, at most 256; RPE_RESIDENT_CAP lowers it).  enabled is a bit set: 1 resident loops, 2 host-driven ones
 * (large BAR), 4 the autonomous loops still ask for their solving workgroup (cleared once the two kernels did not meet). */
int rpe_debug_resident_state(rpe_context* ctx, int* enabled, int* lost, int* cap);
/* Test hook, per context: the last workgroup of the next host-driven resident loops withholds its sums of `iteration` (> 0), and the
 * workgroups wait `pose_wait_s` seconds (0.5 .. 60; 0 = default 2 s) for the next pose.  (0, 0) = off.  Nothing in the library reads
 * a fault from the environment. */
int rpe_debug_inject_resident_fault(rpe_context* ctx, int iteration, double pose_wait_s);

/* Which CPU should the thread that drives the resident Gauss-Newton loop sit on?  (It spins on every iteration's records and writes
 * every pose through the PCIe BAR: the choice is worth 5-10 % of a step.)  Measures a handful of candidates -- the current CPU, three
 * spread over the GPU-local CPUs (sysfs local_cpulist of the device), two over the others, one SMT sibling -- with `reps` refinements of
 * `steps` iterations each over the context's OWN arrays (kind / flags as rpe_gn_refine, tol = 0, from pose12, which is not modified),
 * then leaves the CALLING THREAD pinned to the fastest (sched_setaffinity, this thread only) and reports it: best_cpu / best_us (us per
 * iteration), and up to `cap` (cpu, us) trials.  Opt-in; the environment RPE_HOST_CPU=auto makes the first host-driven resident
 * refinement of every context do this by itself (200 iterations x 5 per candidate), RPE_HOST_CPU=<cpu> pins without measuring.
 * HSA_ENABLE_INTERRUPT=0 in the process environment (a ROCm runtime knob: completion signals polled instead of interrupt-driven,
 * -0.25 us per step of a short refinement) is the caller's choice: it must be set before the runtime initialises. */
int rpe_tune_host_thread(rpe_context* ctx, int kind, int flags, const double* pose12, int steps, int reps, int* best_cpu, double* best_us,
                         int* trial_cpus, double* trial_us, int cap, int* ntrials);

/* HIP-event timing of the one-launch reduction kernels (rpe_normal_eq*, rpe_p2p_moments, rpe_nl_round, rpe_inlier_mask), on the
 * context's stream: after enable(max_records, stride) every stride-th such call launches its kernel with an event pair that receives the dispatch's own begin / end
 * timestamps (hipExtLaunchKernelGGL: what rocprofv3 reports for the kernel, no marker packets); collect() synchronises,
 * returns the number of pairs and their total / minimum elapsed milliseconds, and rearms.  enable(0, 1) = off. */
int rpe_timing_enable(rpe_context* ctx, int max_records, int stride);
int rpe_timing_collect(rpe_context* ctx, int* count, double* total_ms, double* min_ms);
/* Elapsed time an EMPTY event pair reports on this context's stream (average and minimum over `pairs` pairs): what the pair
 * itself adds to every interval rpe_timing_collect returns (2-5 us on MI355X), so that event-based kernel times can be
 * compared with rocprofv3's dispatch timestamps. */
int rpe_timing_calibrate(rpe_context* ctx, int pairs, double* avg_ms, double* min_ms);

/* ---- K4 batched hypothesis scoring: the vote loops V1..V8.
 * kind selects the modality set exactly as the reference's loops combine them. */
enum {
  RPE_VOTE_33 = 0,        /* shinji_ransac / ransac2 / prosac      AbsoluteOrientation.hpp:133-143,190-200,248-258 */
  RPE_VOTE_23 = 1,        /* kneip_ransac / prosac                 P3P.hpp:362-376,439-453                         */
  RPE_VOTE_33_23 = 2,     /* shinji_kneip_ransac / prosac          AbsoluteOrientation.hpp:403-422,480-499         */
  RPE_VOTE_NN_23 = 3,     /* nl_kneip_ransac                       AbsoluteOrientationNormal.hpp:245-264           */
  RPE_VOTE_NN_33 = 4,     /* nl_shinji_ransac                      :322-337                                        */
  RPE_VOTE_NN_33_23 = 5,  /* nl_shinji_kneip_ransac                :397-423                                        */
  RPE_VOTE_23_MATRIX = 6  /* kneip_ransac multiplies by so3().matrix() (P3P.hpp:365) where kneip_prosac uses so3()*x (:442):
                             differs from RPE_VOTE_23 only in RPE_SCORE_EXACT arithmetic                     */
};
/* arithmetic: RPE_SCORE_FAST = rotation-matrix FMA form, squared-distance compare (results can differ from
 * the reference only for correspondences within rounding of a threshold); RPE_SCORE_EXACT = the reference's
 * own operation sequence in Tp (quaternion rotate, sqrt, divide, no FMA contraction): votes bit-identical
 * to the CPU path. */
enum { RPE_SCORE_FAST = 0, RPE_SCORE_EXACT = 1 };
/* poses7: H x (qw qx qy qz tx ty tz) doubles holding Tp-representable values (a Sophus::SE3<Tp>).
 * thre_3d in metres; cos_thr = cos(atan(thre_2d/f)); cos_nl = cos(nl_thre), already evaluated in Tp.
 * votes_out[H]: total votes per hypothesis (sum over the modalities of `kind`). */
int rpe_score(rpe_context* ctx, int kind, int mode, const double* poses7, int H, double thre_3d, double cos_thr, double cos_nl,
              int* votes_out);
/* One batch of `iters` 3D-3D RANSAC iterations entirely on the device: per iteration a thread draws the 3-point sample from the
 * PCG32 stream (rng_state, rng_inc: rpe::Rand31's state, Utility.hpp) at its own position (3 draws per iteration, skip-ahead), runs
 * the closed-form fit shinji() (AbsoluteOrientation.hpp:47-99) on the resident arrays, and the batch is scored by K4 without the
 * poses ever leaving HBM.  Bitwise the hypotheses, in the order, the host sampler + solver would have produced (same functions,
 * no FMA contraction).  votes_out[iters]; q7_out[iters x 7] = qw qx qy qz tx ty tz holding Tp values; valid_out[i] = 0 where the
 * sample hit an invalid (all-NaN) camera point and the reference skips the iteration.  The caller advances its stream by 3*iters. */
int rpe_ransac33_batch(rpe_context* ctx, uint64_t rng_state, uint64_t rng_inc, int iters, int mode, double thre_3d, int* votes_out,
                       double* q7_out, unsigned char* valid_out);
/* The same for the plain-RANSAC solvers with a 4-point sample, FAST scoring mode only (the device solvers agree with
 * the host's to rounding, not bit for bit -- the vote-exact default keeps the host generators).  solver: 0 = kneip_ransac (one slot
 * per iteration: the P3P branch that best reprojects the 4th sample), 1 = shinji_kneip_ransac (3-point fit, P3P), 2 = nl_kneip_ransac
 * (P3P), 3 = nl_shinji_ransac (3-point fit, nl_2p), 4 = nl_shinji_kneip_ransac (3-point fit, P3P, nl_2p).  The sample of iteration i is
 * the host sampler's (4 draws per iteration from (rng_state, rng_inc)).  votes_out / valid_out: iters x slots, q7_out: x 7.
 * cos_thr = cos(atan(thre_2d / f)), cos_nl = cos(nl_thre). */
int rpe_ransac_p3p_batch(rpe_context* ctx, int solver, uint64_t rng_state, uint64_t rng_inc, int iters, double thre_3d, double cos_thr,
                         double cos_nl, int* votes_out, double* q7_out, unsigned char* valid_out);
/* K4b: write the winner's inlier masks into the context's device masks (all modalities of `kind`; others
 * untouched) -- what setInlier() stores; returns the vote total. */
int rpe_inlier_mask(rpe_context* ctx, int kind, int mode, const double* pose7, double thre_3d, double cos_thr, double cos_nl,
                    int* votes_out);
/* K4r -- resident scoring session: between _begin and _end, rpe_score calls of at most 128 hypotheses and rpe_inlier_mask calls with
 * exactly these parameters are served by ONE resident launch (the hypotheses travel through the context's control block, the vote
 * counts return as run records): a whole RANSAC run of the reference (pose/AbsoluteOrientation.hpp:169-209: sample, score, keep the
 * best, shrink Iter, finally the winner's mask) costs one kernel launch instead of one per batch and one for the masks.  Results are
 * those of the calls outside a session, bit for bit.  RPE_ERR_STATE when the context cannot hold one (resident kernels unavailable,
 * a sharded context, more correspondences than one group per thread of a co-resident grid): the caller goes on without.  Any other
 * call on the context -- and a longer hypothesis list, or other parameters -- ends the session implicitly; _end is idempotent.  One
 * session per host thread; while it is open, resident loops of other contexts on the same GPU wait for it. */
int rpe_score_session_begin(rpe_context* ctx, int kind, int mode, double thre_3d, double cos_thr, double cos_nl);
int rpe_score_session_end(rpe_context* ctx);

/* ---- PROSAC order: the first top_k (<= 4096) entries of "indices sorted by weight, descending" (pose/Utility.hpp:107-118 sortIndexes as
 * PROSAC consumes it through getSortedIdx, pose/AOOnlyPoseAdapter.hpp:233-254) for n float weights (host pointer), computed on the GPU:
 * two-level radix select of the cut + LDS bitonic sort of the candidates.  Equal weights are ordered by index (the reference's
 * comparator leaves their order to std::sort), which makes the order unique and the prefix well defined.  RPE_ERR_STATE when more than
 * 8192 (near-)equal weights surround the cut: the caller then sorts on the host (the C++ adapters do). */
int rpe_prosac_order(rpe_context* ctx, const float* weights, int n, int top_k, int* order_out);

/* ---- K5 one round of nl_shinji_kneip_ls (AbsoluteOrientationNormal.hpp:484-505) + find_opt_cc (:24-39),
 * fused into one pass over up to 60 B/corr.  in: c_opt[3], Cw[3], Cc[3], Rwc9 (row-major, rotation used by
 * find_opt_cc).  out44: M23 (9) TW K | M33 (9) sigma | MNN (9) TL M | AA (6: xx xy xz yy yz zz) bb (3) | pad.
 * Sums are the FRESH contributions of this round; the host applies the reference's accumulate-across-rounds
 * recurrences.  Masks/weights of all three modalities are honoured (weights optional, scaled as the adapters do). */
int rpe_nl_round(rpe_context* ctx, const double* c_opt3, const double* Cw3, const double* Cc3, const double* Rwc9, double* out44);

/* ---- adapter-level pipelines, for hosts that cannot include the C++ headers (and for the parity tests): builds the
 * adapter the reference's demos would build for the arrays given (AOOnly / PnP / AO / NormalAO), runs one solver of
 * pose/ *.hpp on it, optionally a least-squares stage, and returns pose, votes, adapted Iter and the inlier masks.
 * method: 0 shinji_ransac  1 shinji_ransac2  2 shinji_prosac  3 kneip_ransac  4 kneip_prosac  5 shinji_kneip_ransac
 *         6 shinji_kneip_prosac  7 nl_kneip_ransac  8 nl_shinji_ransac  9 nl_shinji_kneip_ransac
 *         10 none (pose R9/t3 and mask_in are INPUTS: least-squares stage only)
 * ls:     0 none  1 shinji_ls / shinji_ls1 (inliers)  2 nl_shinji_kneip_ls (bug-compatible)  3 nl_shinji_kneip_ls (fixed)
 *         4 shinji_ls2 (all)  5 gn_refine_p2p  6 gn_refine_joint  7 gn_refine_p2plane  8 gn_refine_bearing  9 gn_refine_reproj
 * mask_in / mask_out: 3 x n shorts, row 0 = 2D-3D, 1 = 3D-3D, 2 = normal-normal.  seed: sampler stream.
 * RE-ENTRANT: every call builds its own random stream from `seed` and carries `score_mode` as a per-call option (rpe::RunOptions,
 * rpe/device.hpp); nothing process-wide is written, so concurrent calls from several threads -- different seeds, different modes --
 * each produce exactly what the same call produces alone (tests/cpp/reentrancy_host.cpp under ThreadSanitizer,
 * tests/test_gpu_pipelines.py::test_concurrent_runs_with_different_seeds_and_modes).  The reference's samplers share the process-global
 * rand() (pose/Utility.hpp:148,212,229; Library.cpp ao_ransac) and are not thread-safe; ao_ransac() here owns its stream too.  The
 * C++ free functions (shinji_ransac2<Tp>(adapter, thr, Iter, conf) ...) keep the reference's semantics when called as the reference
 * calls them -- one process-global stream, rpe::seed() in place of srand() -- and take the same options as a last, defaulted argument. */
typedef struct {
  int n;
  int dtype;              /* RPE_F32 / RPE_F64 */
  const void* bv;         /* host pointers, 3 x n, or NULL */
  const void* xc;
  const void* nc;
  const void* xw;
  const void* nw;
  const void* weights;    /* n x wcols column-major or NULL */
  int wcols;
  double fx, fy;
} rpe_problem;
int rpe_run(int method, const rpe_problem* p, double thre_3d, double thre_2d, double thre_nl, int* iter_io, double confidence,
            uint64_t seed, int ls, int score_mode, const short* mask_in, double* R9, double* t3, int* max_votes, short* mask_out);

/* The hypothesis stream of a solver made explicit ("both CPU restatement and GPU consume the same sample
 * list").  rpe_host_hypotheses runs `method`'s sampler (seeded as rpe_run does) and minimal solvers -- shinji K = 3
 * (AbsoluteOrientation.hpp:47-99), kneip (P3P.hpp:63-294), nl_2p (AbsoluteOrientationNormal.hpp:77-142), in the order the solver's
 * loop tries them -- for `iters` iterations WITHOUT scoring anything: no GPU is needed.  q7_out[cap x 7] = qw qx qy qz tx ty tz
 * (Tp values), first_out[iters + 1]: the hypotheses of iteration i are first_out[i] .. first_out[i+1].  Returns their number.
 * rpe_run_replay is rpe_run with the hypotheses of iteration i TAKEN from poses7[first[i] .. first[i+1]) instead of being sampled:
 * scoring on the GPU, best-so-far on strict '>', adaptive Iter, winner's masks and the optional least-squares stage as in rpe_run. */
int rpe_host_hypotheses(int method, const rpe_problem* p, int iters, uint64_t seed, double* q7_out, int cap, int* first_out);
int rpe_run_replay(int method, const rpe_problem* p, const double* poses7, const int* first, int list_iters, double thre_3d,
    double thre_2d,
                   double thre_nl, int* iter_io, double confidence, int ls, int score_mode, double* R9, double* t3, int* max_votes,
                   short* mask_out);

/* ------------------------------------------------------------------------------------------------
 * Part 3 -- front end (additive): the step BEFORE the hot path.  A depth frame becomes
 * the adapters' arrays directly in HBM: points_c / normal_c / bearingVectors of the frame, points_g / normal_g of the
 * model it is registered against.  Camera model = the reference simulator's pinhole (u - cx = fx * X / Z,
 * pose/Simulator.hpp:150-162; defaults f = 585, 640 x 480, principal point at the centre).  All fp32.
 * The reference has no counterpart of this stage; its contract is the numpy statement the parity tests hold.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { double fx, fy, cx, cy; int width, height; } rpe_camera;
enum { RPE_DEPTH_U16 = 0, RPE_DEPTH_F32 = 1 };
/* F1: upload one depth image (host, row-major, width*height values; metres = value * depth_scale) and build the frame's
 * maps: vertex map (NaN where depth is 0 / NaN / outside (dmin, dmax)), unit bearing vectors (every pixel), normal map
 * (central differences, towards the camera; NaN on the border, next to invalid depth, or where a neighbour's depth
 * differs by more than max_jump metres). */
int rpe_frame_set_depth(rpe_context* ctx, const void* depth, int depth_type, const rpe_camera* cam, double depth_scale, double dmin,
                        double dmax, double max_jump);
enum { RPE_MAP_VERTEX = 0, RPE_MAP_NORMAL = 1, RPE_MAP_BEARING = 2, RPE_MAP_MODEL_VERTEX = 3, RPE_MAP_MODEL_NORMAL = 4 };
/* copy one map (3 x width*height floats) to the host */
int rpe_frame_download(rpe_context* ctx, int which, float* out);
/* F2: the model := this frame's maps moved to the world frame under pose12 (Xw = R^T (Xc - t)); the model view's pose
 * and camera := pose12 and the frame's camera.  Device to device. */
int rpe_model_from_frame(rpe_context* ctx, const double* pose12);
/* ... or a model rendered elsewhere: world-frame vertex / normal maps (host, 3 x width*height floats, NaN = empty)
 * as seen from the view `pose12` (world -> model camera) with intrinsics `cam`. */
int rpe_model_upload(rpe_context* ctx, const float* vertex_w, const float* normal_w, const rpe_camera* cam, const double* pose12);
/* F3: projective data association of the frame against the model under the pose guess pose12 (frame: Xc = R Xw + t).
 * Each frame vertex is moved to the world, projected into the model view (nearest pixel), and paired with the model
 * vertex there if it lies within dist_thr metres and (use_normals) the normals agree to cos_thr.  Declares the problem
 * (n = width*height, RPE_F32) and fills XW, XC, BV, NW, NC in place, index = frame pixel; pixels without a partner get a
 * NaN column in XC / BV / NC (the reference's isValid convention, AOPoseAdapter.hpp:147-152) which every kernel skips.
 * matched (may be NULL: no host synchronisation) = number of pairs. */
int rpe_associate(rpe_context* ctx, const double* pose12, double dist_thr, double cos_thr, int use_normals, int64_t* matched);
/* ICP: max_iter rounds of { rpe_associate under the current pose ; one Gauss-Newton step of residual `kind`
 * (RPE_RES_P2PLANE uses the FRAME's normals, RPE_RES_P2P none) }.
 * device_resident = 1 keeps pose, solve and exp-map on the GPU (one host wait at the end; with fused = 1 ONE launch whose resident grid
 * iterates by itself), 0 solves on the host each round
 * (with fused = 1 that is ONE resident launch for the whole loop: the frame's pixels stay in registers and the host hands a pose to
 * the waiting grid every round, as rpe_gn_refine does -- the fastest form, needs a large-BAR device).
 * fused = 1 pairs and accumulates in ONE kernel per round (the pairs never exist in HBM: 48 B/pixel instead of 156); same
 * pairing function and per-pixel arithmetic as the two-kernel path, the sums differ in rounding only.  On return XW XC BV NW NC hold the pairs under the
 * RETURNED pose when fused, under the pose of the last round otherwise. */
typedef struct { int kind; int max_iter; double tol; double dist_thr; double cos_thr; int use_normals; int device_resident; int fused;
    } rpe_icp_options;
int rpe_icp(rpe_context* ctx, const rpe_icp_options* opt, double* pose12, int* iters_out, double* last_step, double* final_cost,
            int64_t* matched);

/* ---- coarse-to-fine pyramids of frame and model (KinectFusion-style ICP).  Conventions, followed bit for bit:
 * Levels l = 0 .. L-1, L <= RPE_MAX_LEVELS; level l is (width >> l) x (height >> l) pixels and every level must have one
 * (RPE_ERR_ARG otherwise).  Level camera, computed in double and cast to fp32 like the level-0 camera: level 0 is the camera itself,
 * level l >= 1 has fx / 2^l, fy / 2^l, cx_l = (cx + 0.5) / 2^l - 0.5, cy_l likewise (level-1 pixel u is centred on level-0
 * coordinate 2u + 0.5).  Frame depth pyramid (fp32 metres, NaN = invalid): level 0 = depth * depth_scale, NaN outside (dmin, dmax);
 * level l+1 pixel (u, v) with c = level-l depth at (2u, 2v): NaN if c is, else the mean of the 2 x 2 block's valid depths d with
 * |d - c| <= max_jump, summed in the order (2v,2u) (2v,2u+1) (2v+1,2u) (2v+1,2u+1) with 0 for an excluded pixel and divided by their
 * count (fp32, no FMA contraction).  Frame maps of level l = F1's arithmetic on the level's metric depth (scale 1, same dmin / dmax /
 * max_jump) with the level camera; level 0 is bitwise what rpe_frame_set_depth builds.  Model levels: rpe_model_from_frame moves
 * every level of the frame (F2 on each); rpe_model_build_pyramid resizes an uploaded level 0 (KinectFusion): block a = (2u,2v),
 * b = (2u+1,2v), c = (2u,2v+1), d = (2u+1,2v+1) of level l; a vertex is valid iff all four level-l values have no NaN component, value
 * (((a + b) + c) + d) * 0.25f; a normal is valid iff all four are, the same sum divided by sqrtf(x*x + y*y + z*z), NaN at length 0;
 * vertices and normals independently. */
enum { RPE_MAX_LEVELS = 4, RPE_MAP_DEPTH = 5 };
/* F1p: rpe_frame_set_depth plus the frame's pyramid of `levels` levels (metric depth and maps of every level; two launches).
 * rpe_frame_set_depth resets the frame to one level (and keeps no metric depth). */
int rpe_frame_set_depth_pyramid(rpe_context* ctx, const void* depth, int depth_type, const rpe_camera* cam, double depth_scale,
                                double dmin, double dmax, double max_jump, int levels);
/* one map of one level: which = RPE_MAP_* (3 x w_l*h_l floats; model maps: the model's level) or RPE_MAP_DEPTH (w_l*h_l floats of
 * metric depth, frames set by rpe_frame_set_depth_pyramid only).  rpe_frame_download keeps rejecting RPE_MAP_DEPTH. */
int rpe_frame_download_level(rpe_context* ctx, int which, int level, float* out);
/* the fp64 camera of a level of the frame (model = 0) or of the model (model = 1): the values the kernels' fp32 camera was cast from */
int rpe_frame_level_camera(rpe_context* ctx, int level, int model, rpe_camera* out);
/* F2p: levels 1 .. levels-1 of the model from its level 0 (one launch); rpe_model_upload resets the model to one level */
int rpe_model_build_pyramid(rpe_context* ctx, int levels);
/* coarse-to-fine ICP: levels L-1 .. 0, each rpe_icp's loop (every execution form of opt, opt->tol ending the level early) on that
 * level's frame and model maps, from the pose the coarser level returned.  iters_per_level[l] rounds at level l (0 = finest; coarse
 * levels may have 0, level 0 needs >= 1; opt->max_iter is not used), dist_thr_per_level[l] its distance gate (NULL: opt->dist_thr
 * everywhere).  One host wait per level.  iters_out[l] = rounds run at level l; last_step / final_cost / matched and the solver
 * slots (XW XC BV NW NC, n = width*height) are level 0's, as rpe_icp leaves them.  RPE_ERR_STATE when the frame or the model has
 * fewer than `levels` levels. */
int rpe_icp_pyramid(rpe_context* ctx, const rpe_icp_options* opt, int levels, const int* iters_per_level, const double* dist_thr_per_level,
                    double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched);

/* ---- Depth filter (optional, off by default): a bilateral filter on the frame's metric depth in front of F1 / F1p, the first kernel
 * of a KinectFusion pipeline.  A depth camera's noise grows with the square of the range and is centimetres at room distances, more
 * than the spacing of neighbouring pixels' rays: the central-difference normals of raw depth are then mostly noise, and with them the
 * point-to-plane residual, the cos_thr gate and the stored normals.  Conventions, followed bit for bit (fp32, the written order, no FMA
 * contraction; tests/filter_oracle.py states them in numpy):
 * Cast once: r = radius (1 .. RPE_FILTER_MAX_RADIUS), a = (float)depth_cut, b = (float)depth_cut_z2.  m(u, v) = the metric depth of
 * level 0 as above: d = (float)raw * scale, NaN unless d > dmin && d < dmax.  Spatial weights, made on the host:
 * ws[dy][dx] = (float)exp(-(double)(dx*dx + dy*dy) / (2 * sigma_space * sigma_space)), double, libm's exp.  Pixel (u, v): c = m(u, v);
 * c NaN gives NaN (holes are not filled).  cut = a + b * (c * c), inv = 1.0f / cut.  For dy = -r .. r (outer), dx = -r .. r (inner),
 * neighbours inside the image only: d = m(u + dx, v + dy), t = (d - c) * inv, x = t * t; the neighbour counts iff x < 1.0f (a NaN one
 * does not), with wr = (1.0f - x) * (1.0f - x), wgt = ws[dy][dx] * wr, num += wgt * d, den += wgt.  out = num / den (den >= 1: the
 * centre).  The range kernel is the biweight, a polynomial with support `cut`: the depth difference at which a neighbour stops
 * counting is depth_cut + depth_cut_z2 z^2 metres, the z^2 term following the sensor's noise law (a constant cut cannot be right at
 * 1 m and at 5 m at once).  Nothing bleeds across a depth step larger than cut.
 * The filtered image is handed, as RPE_DEPTH_F32 with scale 1, to the kernels of rpe_frame_set_depth / rpe_frame_set_depth_pyramid,
 * which re-apply (dmin, dmax): level 0 of the frame is F1 on the filtered depth, coarser levels follow from it by the block rule
 * above, RPE_MAP_DEPTH level 0 downloads the filtered depth, and rpe_volume_integrate fuses the filtered vertex map.  Fusing the raw
 * depth beside filtered tracking is out of scope: a caller who wants that builds the frame twice.
 * The setting belongs to the context and applies to the NEXT rpe_frame_set_depth*; the current frame is not touched.  A frame build
 * with the filter on is one launch more (2 for rpe_frame_set_depth, 3 for the pyramid) and no extra host wait; the filtered buffer
 * is allocated on first use and reused.  With the filter off every function returns the bits it returned without it. */
enum { RPE_FILTER_MAX_RADIUS = 4 };
typedef struct { int radius; double sigma_space, depth_cut, depth_cut_z2; } rpe_depth_filter;
/* radius 0 or filter = NULL: off (the other fields are then not looked at).  RPE_ERR_ARG for a radius outside 0 .. RPE_FILTER_MAX_RADIUS,
 * sigma_space or depth_cut not finite and > 0, depth_cut_z2 not finite or < 0; the setting is then unchanged. */
int rpe_frame_set_filter(rpe_context* ctx, const rpe_depth_filter* filter);
/* the current setting: {0, 0, 0, 0} while off */
int rpe_frame_get_filter(rpe_context* ctx, rpe_depth_filter* out);

/* ---- TSDF volume (KinectFusion): frames fused into a truncated signed distance volume, raycast into the model.  With it,
 * rpe_frame_set_depth_pyramid -> rpe_volume_raycast -> rpe_model_build_pyramid -> rpe_icp_pyramid -> rpe_volume_integrate tracks
 * frame to model with every map on the GPU.  Conventions, followed bit for bit (fp32, the written order, no FMA contraction):
 * Geometry is cast once: o = (float)origin, s = (float)voxel_size, tr = (float)trunc, W = (float)max_weight; poses as everywhere in
 * Part 3 (each of the 12 doubles cast to fp32).  One volume per context: dim[0] x dim[1] x dim[2] voxels, each {tsdf, weight} (two
 * floats) at index (k * dim[1] + j) * dim[0] + i; weight 0 = unobserved (rpe_volume_init clears everything to 0); the centre of
 * voxel (i, j, k) is o + ((float)i + 0.5f) * s per axis.
 * Integrate (the frame's level-0 vertex map under pose12, Xc = R Xw + t), per voxel: pc = R p + t, each row summed left to right;
 * skipped unless pc.z > 0; pixel uf = floorf(fx * (pc.x / pc.z) + cx + 0.5f), vf likewise, skipped unless inside the image;
 * d = z of the frame's level-0 vertex map there (the metric depth, NaN where invalid: skipped); sdf = d - pc.z, skipped unless
 * sdf >= -tr; f = fminf(1.0f, sdf / tr); tsdf := (tsdf * w + f) / (w + 1.0f), w := fminf(w + 1.0f, W).  A skipped voxel is never
 * stored (its 16-byte pair may be loaded): its bits stay.
 * Field F(p): g = (p - o) / s - 0.5f per axis, i0 = floorf(g), a = g - i0; known iff 0 <= i0 <= dim - 2 on every axis and all 8
 * corner weights are > 0; with lerp(x, y, t) = x + (y - x) * t it is: lerps along x for the (j, k) corner pairs (0,0) (1,0) (0,1)
 * (1,1), then along y ((0,0) with (1,0), (0,1) with (1,1)), then along z.
 * Raycast (pose12, camera cam, range (dmin, dmax)), ray of pixel (u, v): xn = ((float)u - cx) / fx, yn likewise; samples at camera
 * depths z_k = dmin + (float)k * s while z_k < dmax, each the camera point (xn * z, yn * z, z) moved to the world (Xw = R^T (Xc - t),
 * as rpe_model_from_frame).  Hit: the first k where F(z_k) and F(z_k+1) are both known with F_k > 0 and F_k+1 <= 0;
 * z* = z_k + s * (F_k / (F_k - F_k+1)); model vertex = world point of (xn * z*, yn * z*, z*).  Model normal at that world point pw:
 * the central differences F(pw + s e) - F(pw - s e) per axis (pw.x + s etc. in fp32), divided by sqrtf(x*x + y*y + z*z); NaN if any
 * of the six samples is unknown or the length is 0 (the vertex stays).  The gradient points towards free space (the camera), as the
 * frame normals do.  No hit: NaN vertex and normal.  The model after a raycast is exactly what rpe_model_upload of those maps with
 * (cam, pose12) leaves: one level, model pose pose12, model camera cam (rpe_model_build_pyramid adds levels). */
typedef struct { int dim[3]; double voxel_size; double origin[3]; double trunc; int max_weight; } rpe_volume_desc;
/* (re)allocate and clear the context's volume: dims 2 .. 1024, voxel_size and trunc > 0, origin finite, max_weight >= 1 */
int rpe_volume_init(rpe_context* ctx, const rpe_volume_desc* desc);
/* fuse the current frame (level 0) seen from pose12 into the volume; RPE_ERR_STATE without a volume or a frame */
int rpe_volume_integrate(rpe_context* ctx, const double* pose12);
/* the model := the volume raycast from pose12 with intrinsics cam over camera depths (dmin, dmax): 0 <= dmin < dmax, both finite,
 * at most 2^22 samples per ray ((dmax - dmin) / voxel_size); RPE_ERR_STATE without a volume */
int rpe_volume_raycast(rpe_context* ctx, const double* pose12, const rpe_camera* cam, double dmin, double dmax);
/* copy the volume to the host: 2 x voxels floats {tsdf, weight} in voxel index order */
int rpe_volume_download(rpe_context* ctx, float* tsdf_weight);
/* copy 2 x voxels floats {tsdf, weight}, in voxel index order, into the context's volume (the inverse of rpe_volume_download);
 * RPE_ERR_STATE without a volume.  The bits are taken as given. */
int rpe_volume_upload(rpe_context* ctx, const float* tsdf_weight);

/* ---- Mesh: marching cubes over the volume, the triangle mesh of its zero level set, built in device buffers the context owns.
 * Conventions, followed bit for bit (fp32, the written order, no FMA contraction; tests/mesh_oracle.py states them in numpy):
 * Cubes: cube (i, j, k) exists for 0 <= i <= d0-2, 0 <= j <= d1-2, 0 <= k <= d2-2; its corner n = di + 2*dj + 4*dk is voxel
 * (i+di, j+dj, k+dk).  wmin = (float)min_weight (min_weight finite and > 0, also in fp32).  A corner is known iff weight >= wmin and
 * its tsdf is finite; a cube is active iff all 8 corners are known.  Case = the 8-bit mask of the corners with tsdf <= 0 (the
 * raycast's split: F > 0 is free space).  Edges: 0-3 the x-edges for (dj, dk) = (0,0) (1,0) (0,1) (1,1), 4-7 the y-edges for (di, dk),
 * 8-11 the z-edges for (di, dj); the edge from corner a to b = a + e_axis is crossed iff (Fa > 0) != (Fb > 0) and belongs to voxel a
 * with that axis (each voxel owns at most 3 potential vertices).
 * Vertices: one on every crossed edge that at least one active cube contains, ordered by the owning voxel's index
 * (k*d1 + j)*d0 + i, then by axis x < y < z.  Position: t = Fa / (Fa - Fb) (never 0 / 0; t in [0, 1]); along the edge's axis
 * o + (((float)ia + 0.5f) + t) * s, on the other two axes the voxel centre o + ((float)i + 0.5f) * s.  Normal: exactly the raycast's
 * model normal at the vertex (six F(p +- s e) samples, F with weight > 0, not wmin; NaN if a sample is unknown or the length is 0).
 * Triangles: emitted by active cubes with case != 0, 255, ordered by cube index (k*d1 + j)*d0 + i, then in table order; three int32
 * vertex ids each, wound so that (v1 - v0) x (v2 - v0) points to the free side (tsdf > 0), the side of the normal.
 * Table (csrc/rpe_mc_tables.h, generated by scripts/gen_mc_tables.py): on each cube face the crossed edges are joined into segments;
 * on an ambiguous face (four crossed edges) the two tsdf <= 0 corners are joined across the diagonal (a rule of the face's four values
 * alone, so neighbouring cubes agree and the mesh has no cracks).  Segments chain into closed loops; each loop is fan-triangulated
 * from its vertex with the lowest edge number, in the direction the winding requires; loops in the order of that edge.  At most 5
 * triangles per case.
 * The mesh lives until the next rpe_volume_mesh / rpe_volume_mesh_box (whether or not it succeeds), rpe_volume_init or a non-zero
 * rpe_volume_shift.  Workspace: 6 bytes per voxel,
 * allocated on the first extraction and kept with the volume. */
/* marching cubes over the volume: builds the mesh in device buffers the context owns and returns its size (one host wait);
 * RPE_ERR_STATE without a volume, RPE_ERR_ARG for a bad min_weight or a mesh of 2^31 or more vertices (the ids are int32) */
int rpe_volume_mesh(rpe_context* ctx, double min_weight, int64_t* n_vertices, int64_t* n_triangles);
/* copy the last extracted mesh out: vertices and normals 3 x n_vertices floats (normals may be NULL), triangles 3 x n_triangles int32;
 * RPE_ERR_STATE before any extraction or after rpe_volume_init */
int rpe_volume_mesh_download(rpe_context* ctx, float* vertices, float* normals, int32_t* triangles);

/* ---- Colour: a registered RGB image fused beside the depth, and the fused colour sampled at the model's and the mesh's vertices.
 * Conventions, followed bit for bit (fp32, the written order, no FMA contraction; tests/color_oracle.py states them in numpy).
 * h(x) = fp32 -> IEEE binary16, round to nearest even, subnormals kept, overflow to +-Inf, every NaN to the quiet NaN 0x7e00.
 * Frame colour: width*height*3 bytes, row-major, at the current frame's level-0 size, REGISTERED to the depth image: pixel (u, v) of
 * both images sees the same ray (a separate colour camera: rpe_frame_register_color, "Colour registration" below).  Stored on the
 * device as RGBA8 with A = 255; A = 0 (only rpe_frame_register_color writes it) means "this pixel has no colour".  rpe_frame_set_depth
 * and rpe_frame_set_depth_pyramid drop it.
 * Colour volume: beside {tsdf, weight}, at the same voxel index; a voxel is four binary16 {r, g, b, wc} (8 bytes, channels on the
 * 0..255 scale), wc = 0: no colour observed.  It comes into being, all zeros, on the first rpe_volume_integrate_color or
 * rpe_volume_color_upload after rpe_volume_init; rpe_volume_init drops it; the plain rpe_volume_integrate never touches it.
 * Integrate with colour (pose12): {tsdf, weight} are updated exactly as rpe_volume_integrate does it (same voxels, same bits).  A voxel
 * that this rule updates AND whose sdf <= tr (inside the truncation band) AND whose frame pixel (uf, vf) has A != 0 also gets a colour
 * update (the same gate in rpe_volume_fuse_keyframes; the tsdf update does not look at A): the observation o = the frame
 * colour at the same (uf, vf), each channel (float)byte; with w = (float)wc before the update, each channel
 * c := h(((float)c * w + o) / (w + 1.0f)), then wc := h(fminf(w + 1.0f, W)) (for W > 2048 the weight stops at 2048: 2049 rounds to
 * 2048; a NaN weight becomes W, as in the tsdf rule).  A voxel without a colour update is never stored (its 16-byte pair may be loaded).
 * Colour field C(p): F's g, i0, a and in-range rule; known iff in range and all 8 corner COLOUR weights are > 0 (the tsdf weights
 * play no part); each channel with F's lerp order on (float) of the binary16 values.  q(x) = (uint8)floorf(fminf(fmaxf(x, 0.0f),
 * 255.0f) + 0.5f) (a NaN channel gives 0, +Inf 255).  Output RGBA8: (q(r), q(g), q(b), 255) when known, (0, 0, 0, 0) when unknown or
 * at a NaN point.
 * Model colour = C at the level-0 model vertex of each pixel; mesh colour = C at each vertex of the last mesh.  So a mesh colour is bit
 * for bit the model colour at the same point.  Any call that replaces the model (rpe_volume_raycast, rpe_model_upload,
 * rpe_model_from_frame) drops the model colour.  Colour calls without the colour state they need return RPE_ERR_STATE. */
enum { RPE_COLOR_RGB8 = 0, RPE_COLOR_BGR8 = 1 };
enum { RPE_COLOR_FRAME = 0, RPE_COLOR_MODEL = 1 };
/* the current frame's colour: width*height*3 bytes in `format` order (RPE_COLOR_*8); RPE_ERR_STATE without a frame */
int rpe_frame_set_color(rpe_context* ctx, const uint8_t* pixels, int format);
/* rpe_volume_integrate plus the colour update of the band voxels; RPE_ERR_STATE without a volume, a frame or a frame colour */
int rpe_volume_integrate_color(rpe_context* ctx, const double* pose12);
/* the model colour map := C at the model's level-0 vertices (after rpe_volume_raycast, rpe_model_upload or rpe_model_from_frame);
 * RPE_ERR_STATE without a model or a colour volume */
int rpe_model_sample_color(rpe_context* ctx);
/* copy the frame colour (which = RPE_COLOR_FRAME) or the model colour (RPE_COLOR_MODEL) out: 4 x width*height bytes RGBA8 */
int rpe_color_download(rpe_context* ctx, int which, uint8_t* rgba);
/* RGBA8 colours of the last mesh's vertices, 4 x n_vertices bytes (nothing for an empty mesh); RPE_ERR_STATE without a mesh or a
 * colour volume */
int rpe_volume_mesh_colors(rpe_context* ctx, uint8_t* rgba);
/* copy the colour volume out: 4 x voxels binary16 bit patterns {r, g, b, wc} in voxel index order; RPE_ERR_STATE without one */
int rpe_volume_color_download(rpe_context* ctx, uint16_t* rgbw);
/* the inverse of rpe_volume_color_download (the bits are taken as given); RPE_ERR_STATE without a volume */
int rpe_volume_color_upload(rpe_context* ctx, const uint16_t* rgbw);

/* ---- Colour registration: a SEPARATE colour camera reprojected onto the depth frame on the device.  An RGB-D sensor's colour camera
 * sits a few centimetres beside the depth camera, with its own resolution, focal length and lens distortion, and sees around foreground
 * objects differently.  rpe_frame_register_color takes its image as delivered and leaves the current frame's colour where
 * rpe_frame_set_color leaves it (same buffer, same state changes): RGBA8 at the depth frame's level-0 size, A = 255 where a colour was
 * found and 0x00000000 elsewhere -- outside the colour image, without depth, or HIDDEN from the colour camera by something nearer (the
 * naive per-pixel lookup paints the occluder's colour there).  Everywhere colour is consumed, A = 0 means "no colour".
 * Conventions, followed bit for bit (fp32, the written order, no FMA contraction; tests/register_oracle.py states them in numpy).
 * Casts, once: the colour camera (fx fy cx cy; wc x hc pixels), dist = k1 k2 p1 p2 k3, pose12 = (R, t) as every pose12 is cast,
 * a = (float)occl_tol, b = (float)occl_tol_z2, r2_max.  Grid: gw = (wc + cell - 1) / cell, gh = (hc + cell - 1) / cell.
 * Projection of depth pixel i with the level-0 vertex X (all three components finite):
 *   Xk = R X + t, each row summed left to right; needs Xk.z > 0.  x = Xk.x / Xk.z, y = Xk.y / Xk.z, r2 = x*x + y*y; needs
 *   r2 <= r2_max when r2_max > 0.  rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
 *   xd = x * rad + ((2.0f * p1) * (x * y) + p2 * (r2 + 2.0f * (x * x)));  yd = y * rad + (p1 * (r2 + 2.0f * (y * y)) + (2.0f * p2) * (x * y));
 *   px = fx * xd + cx, py = fy * yd + cy, both finite; x0 = floorf(px), y0 = floorf(py); needs 0 <= x0 <= wc - 2, 0 <= y0 <= hc - 2.
 *   A pixel that fails any of these has no colour and casts no shadow.
 * Z-buffer (cell >= 1): gw x gh unsigned words, cleared to 0xffffffff per call.  gx = (px + 0.5f) / (float)cell - 0.5f, i0 = floorf(gx);
 *   gy, j0 likewise.  The pixel takes the minimum of the bits of Xk.z (a positive float: ordered as unsigned) into those of the four
 *   cells (i0 + di, j0 + dj), di, dj = 0, 1, that lie inside the grid.  Its own cell is ci = floorf(gx + 0.5f), cj = floorf(gy + 0.5f):
 *   one of the four, inside the grid.  With zmin that cell's value after ALL pixels have written, the pixel is visible iff
 *   (Xk.z - zmin) <= a + b * (zmin * zmin).  An integer minimum does not depend on arrival order: the output is repeatable bit for bit.
 *   (The device keeps the minima per base cell (i0, j0) and takes the minimum of four of them when it reads a cell: the same value.)
 *   (The z^2 term, as in rpe_depth_filter: one constant cannot fit a floor at a grazing angle at 4 m and a table edge at 1 m.)
 * Sample (visible pixels; with cell = 0 every pixel that passed the projection): s = px - x0, u = py - y0; each channel on (float)byte
 *   with lerp(p, q, s) = p + (q - p) * s along x for the rows y0 and y0 + 1, then along y by u; then the colour block's q(x); A = 255.
 * Out of scope: depth registered INTO the colour camera, rolling-shutter or time offsets, distortion of the DEPTH camera, distortion
 * models other than the five coefficients, and the fold-over of a strongly distorted model beyond r2_max when no limit is given. */
typedef struct {
  rpe_camera cam;        /* the colour camera: its own width x height and pinhole */
  double dist[5];        /* k1 k2 p1 p2 k3 (Brown-Conrady, the usual order); all 0 = none */
  double pose12[12];     /* depth camera -> colour camera, Xk = R Xd + t, the layout of every pose12 */
  double r2_max;         /* skip points with x^2 + y^2 > r2_max before distortion; 0 = no limit */
  int cell;              /* z-buffer cell in colour pixels, 1 .. 16; 0 = no occlusion test */
  double occl_tol, occl_tol_z2;   /* hidden iff z - zmin > occl_tol + occl_tol_z2 * zmin^2 (metres) */
} rpe_color_rig;
/* the current frame's colour from a separate colour camera: `pixels` = rig->cam.width * height * 3 bytes in `format` order
 * (RPE_COLOR_*8).  known may be NULL (no host wait); otherwise it receives the number of A = 255 pixels (one host wait).
 * RPE_ERR_STATE without a frame; RPE_ERR_ARG for a bad format, cell outside 0 .. 16, a colour camera of fewer than 2 x 2 pixels or
 * with a non-finite or non-positive focal length or a non-finite centre, non-finite dist, pose or tolerances, negative tolerances or
 * r2_max.  After an error the frame colour is what it was */
int rpe_frame_register_color(rpe_context* ctx, const uint8_t* pixels, int format, const rpe_color_rig* rig, int64_t* known);

/* ---- Photometric term: tracking against the model's colour beside its geometry.  Point-to-plane ICP has nothing to hold three of
 * the six degrees of freedom with wherever the view is one plane (a wall, a floor, a corridor); the intensity of a textured plane
 * does.  Conventions, followed bit for bit for everything per pixel (fp32, the written order, no FMA contraction;
 * tests/photo_oracle.py states them in numpy); the sums are held to a rounding bound.
 * Model colour without a volume: rpe_model_color_upload (the companion of rpe_model_upload) and rpe_model_color_from_frame (for
 * rpe_model_from_frame users: frame-to-frame RGB-D odometry).  As before, any call that replaces the model drops the model colour.
 * Intensity of an RGBA8 pixel: I = ((0.299f * r + 0.587f * g) + 0.114f * b) on the 0..255 scale, NaN when A = 0.
 * Frame intensity pyramid (one float per pixel per level; level sizes and cameras are the depth pyramid's): level 0 from the frame
 * colour; level l+1 = (((a + b) + c) + d) * 0.25f over the 2 x 2 block a = (2u,2v), b = (2u+1,2v), c = (2u,2v+1), d = (2u+1,2v+1) of
 * level l (the order of rpe_model_build_pyramid), NaN if any of the four is.
 * Model photometric map, one float4 {I, gx, gy, zm} per model pixel per level: I as above (level 0 from the model colour, coarser
 * levels by the same block mean); gx = 0.5f * (I(u+1,v) - I(u-1,v)), gy = 0.5f * (I(u,v+1) - I(u,v-1)) (NaN on the border or beside
 * a NaN); zm = z of the level's model vertex in the MODEL camera's frame, ((R_m[6] * X + R_m[7] * Y) + R_m[8] * Z) + t_m[2], and NaN
 * wherever the level's model normal has a NaN component.  The model normals are NaN across depth jumps, so this one poison keeps
 * every bilinear and gradient stencil off the occlusion edges.
 * The term, per frame pixel of level l under the pose (R, t) (Xc = R Xw + t), with Xc the frame vertex, If the frame intensity,
 * (R_m, t_m) and (fx, fy, cx, cy, w, h) the model view's pose and camera at that level:
 *  1. Xw = R^T (Xc - t) and Xm = R_m Xw + t_m exactly as rpe_associate forms them; needs Xc and If finite and Xm.z > 0.
 *  2. x = fx * (Xm.x / Xm.z) + cx, y likewise; x0 = floorf(x), y0 = floorf(y); needs 0 <= x0 <= w - 2 and 0 <= y0 <= h - 2;
 *     a = x - x0, b = y - y0.
 *  3. The four map entries at (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1): all sixteen floats finite, and |zm - Xm.z| <= dist_thr
 *     for each of the four (the occlusion gate; dist_thr in fp32).
 *  4. Is, Gx, Gy = bilinear of I, gx, gy with lerp(p, q, s) = p + (q - p) * s: along x for both rows, then along y.
 *  5. r = Is - If.  With z = Xm.z, u = Gx * fx, v = Gy * fy:  q = (u / z, v / z, -((u * Xm.x + v * Xm.y) / (z * z)));
 *     A = -(R_m R^T), A[i][j] = -((R_m[3i] * R[3j] + R_m[3i+1] * R[3j+1]) + R_m[3i+2] * R[3j+2]) on the fp32 poses;
 *     a3[j] = (q[0] * A[0][j] + q[1] * A[1][j]) + q[2] * A[2][j];  J = [a3 | Xc x a3] with (Xc x a3)[0] = Xc.y * a3[2] - Xc.z * a3[1]
 *     and cyclic, in the tangent order (upsilon, omega) of rpe_normal_eq, update T <- exp(delta) T.
 *  6. r' = lam * r, J' = lam * J, lam = (float)weight in metres per intensity level, accumulated the way every Gauss-Newton kernel
 *     here accumulates a row: fp32 fused multiply-adds into partial sums of one group of 4 consecutive pixels, widened to fp64 per
 *     group.  Steps 1-5 are bit for bit the oracle's; every sum is within 8 * 2^-24 of the sum of the magnitudes of its products.
 * Whatever replaces the frame's depth or colour, the model or the model colour drops the prepared maps. */
enum { RPE_PHOTO_FRAME = 0, RPE_PHOTO_MODEL = 1 };
/* the model colour map given by the caller: 4 x width*height bytes RGBA8 at the model's level-0 size, A = 0: unknown;
 * RPE_ERR_STATE without a model */
int rpe_model_color_upload(rpe_context* ctx, const uint8_t* rgba);
/* model colour := the current frame colour (device to device); RPE_ERR_STATE unless the model's level 0 has the frame's size and
 * the frame has a colour */
int rpe_model_color_from_frame(rpe_context* ctx);
/* the frame intensity pyramid and the model photometric map of `levels` levels (two launches); RPE_ERR_STATE without a frame colour,
 * a model colour, or `levels` levels of both the frame (rpe_frame_set_depth_pyramid) and the model */
int rpe_photo_prepare(rpe_context* ctx, int levels);
/* one prepared map of one level: RPE_PHOTO_FRAME (w_l*h_l floats) or RPE_PHOTO_MODEL (4 x w_l*h_l floats {I, gx, gy, zm} per pixel) */
int rpe_photo_download(rpe_context* ctx, int which, int level, float* out);
/* the photometric normal equations of one level alone, for callers who combine terms themselves: the 32 doubles of rpe_normal_eq --
 * H upper triangle (21) | g (6) | [27] cost = sum r'^2 | [28] photometric pairs | [29] pivot floor.  weight finite and > 0 */
int rpe_photo_normal_eq(rpe_context* ctx, int level, const double* pose12, double dist_thr, double weight, double* out32);
/* {r, J[0..5]} (unscaled) of every frame pixel of the level, as 7 planes of w_l*h_l floats (rows[k * w_l*h_l + pixel]), NaN where the
 * pixel has no pair.  Plane 0 is the residual image. */
int rpe_photo_rows(rpe_context* ctx, int level, const double* pose12, double dist_thr, float* rows);
/* rpe_icp / rpe_icp_pyramid with the photometric term beside the geometric one: per round ONE launch that forms the point-to-plane
 * row exactly as the fused ICP round does and the photometric row above, one record (H and g the sums of both terms, the two costs
 * and the two pair counts apart), one host wait, the host solve and left update of rpe_icp; opt->tol ends a level early.  Host-driven
 * only: opt->device_resident = 1 is RPE_ERR_ARG, opt->fused is not consulted, opt->kind must be RPE_RES_P2PLANE with use_normals = 1
 * (RPE_ERR_ARG otherwise); photo_weight finite and > 0; RPE_ERR_STATE when the maps are not prepared for the levels asked.
 * final_cost / matched are the geometric cost and pairs of the last round as rpe_icp reports them, photo_cost / photo_matched (may be
 * NULL) the photometric ones; the pyramid form reports level 0's.  On return the solver slots hold the pairs under the returned pose. */
int rpe_icp_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, double* pose12, int* iters_out, double* last_step,
                 double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched);
int rpe_icp_pyramid_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, int levels, const int* iters_per_level,
                         const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                         int64_t* matched, double* photo_cost, int64_t* photo_matched);

/* ---- Volume term: a frame tracked against the TSDF volume ITSELF (Bylow et al., RSS 2013; Canelhas' SDF tracker).  No raycast, no
 * model view, no model pyramid and no projective association: each frame vertex is moved to the world under the current pose, the
 * trilinear TSDF there is the residual and the gradient of the same eight corners is the row.  A round reads the frame's pixels and
 * one 8-corner gather per pixel; a tracked frame needs rpe_volume_raycast only when someone wants to look at the model.
 * Conventions, followed bit for bit for everything per pixel (fp32, the written order, no FMA contraction; tests/sdf_oracle.py
 * states them in numpy); the sums are held to a rounding bound.  Casts are made once: (R, t) as every pose12 (Xc = R Xw + t); the
 * volume's o, s, tr as rpe_volume_init cast them; gate = (float)dist_thr, c = (float)cos_thr, k = tr / s.
 * The term, per frame pixel of level l with vertex Xc and normal Nc (frame camera coordinates):
 *  1. Xc has three finite components.  Xw = R^T (Xc - t) exactly as rpe_associate forms it.
 *  2. The field's cell of Xw: g = (Xw - o) / s - 0.5f, i0 = floorf(g), a = g - i0 per axis; needs 0 <= i0 <= dim - 2 on every axis.
 *  3. The eight corner voxels v[di][dj][dk] = voxel (i0 + (di, dj, dk)): all eight weights > 0 (the field's "known"), and all eight
 *     tsdf values with fabsf(v) < 1.0f -- no corner saturated, so the point is inside the truncation band on every side (a NaN tsdf
 *     fails this test).
 *  4. D = the field's trilinear value (lerp(x, y, t) = x + (y - x) * t along x, then y, then z); r = D * tr [m]; needs fabsf(r) <= gate.
 *  5. The gradient of the same interpolant, in tsdf per voxel, from corner differences through the same lerp:
 *       gx = lerp(lerp(v100 - v000, v110 - v010, ay), lerp(v101 - v001, v111 - v011, ay), az)
 *       gy = lerp(lerp(v010 - v000, v110 - v100, ax), lerp(v011 - v001, v111 - v101, ax), az)
 *       gz = lerp(lerp(v001 - v000, v101 - v100, ax), lerp(v011 - v010, v111 - v110, ax), ay)
 *     len = sqrtf((gx * gx + gy * gy) + gz * gz), needs len > 0;  n = (gx * k, gy * k, gz * k), metres per metre, about unit length
 *     on a clean surface.
 *  6. a[i] = -((R[3i] * n.x + R[3i+1] * n.y) + R[3i+2] * n.z): the gradient turned into the camera frame and negated.
 *  7. With use_normals: Nc finite and (-((a[0] * Nc.x + a[1] * Nc.y) + a[2] * Nc.z)) / (len * k) >= c -- the frame normal agrees with
 *     the field's gradient, as ICP's cos_thr demands of the model normal.
 *  8. Residual r, J = [a | Xc x a] with (Xc x a)[0] = Xc.y * a[2] - Xc.z * a[1] and cyclic, in the tangent order (upsilon, omega) of
 *     rpe_normal_eq, update T <- exp(delta) T (dXw = -R^T (upsilon + omega x Xc)).
 *  9. Accumulated the way every Gauss-Newton row here is: fp32 fused multiply-adds on pairs of pixels into partial sums of one group
 *     of 4 consecutive pixels, widened to fp64 once per group, then the fixed order of every reduction here.  Steps 1-8 are bit for
 *     bit the oracle's; every sum is within 8 * 2^-24 of the sum of the magnitudes of its products.
 * What the term is NOT.  Its basin is the truncation band: a point further than trunc from the fused surface gives no row, so a
 * start more than a few voxels off wants a coarse level or rpe_icp first.  Rows are not weighted by voxel weight.  It reads the
 * dense window only: voxels in the archive's bricks give no row (the map form over the brick grid of rpe_volume_map_raycast is the
 * follow-up).
 * The calls need a frame (with the levels asked) and a volume, RPE_ERR_STATE otherwise; they need NO model, and neither read nor
 * replace the model, the solver slots or the prepared photometric maps. */
/* {r, J[0..5]} of every frame pixel of the level, as 7 planes of w_l*h_l floats (rows[k * w_l*h_l + pixel]), NaN where the pixel has
 * no row.  Plane 0 is the residual image in metres.  level >= 0, dist_thr >= 0 */
int rpe_sdf_rows(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, float* rows);
/* the normal equations of one level: the 32 doubles of rpe_normal_eq -- H upper triangle (21) | g (6) | [27] sum r^2 | [28] rows |
 * [29] pivot floor (the rows' products are fp32) */
int rpe_sdf_normal_eq(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, double* out32);
/* rpe_icp / rpe_icp_pyramid on the volume term: per round ONE launch, one host wait, the host solve and left update of rpe_icp;
 * opt->tol ends a level early.  Of opt, max_iter (>= 1; the pyramid form takes iters_per_level), tol, dist_thr, cos_thr and
 * use_normals are read; kind and fused are not consulted; host-driven only: device_resident = 1 is RPE_ERR_ARG.  final_cost is the
 * sum of r^2 and matched the rows of the last round; the pyramid form reports level 0's.  A round whose normal equations are not
 * positive definite returns RPE_ERR_DEGENERATE with iters_out the rounds completed, as rpe_icp does. */
int rpe_icp_sdf(rpe_context* ctx, const rpe_icp_options* opt, double* pose12, int* iters_out, double* last_step, double* final_cost,
                int64_t* matched);
int rpe_icp_pyramid_sdf(rpe_context* ctx, const rpe_icp_options* opt, int levels, const int* iters_per_level,
                        const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                        int64_t* matched);

/* ---- Volume colour term: a photometric term beside the volume term, against the COLOUR VOLUME itself.  The volume term is geometry
 * only: where geometry does not hold all six degrees of freedom -- a wall, a floor, a corridor -- it has nothing to hold the in-plane
 * motion with.  The colour that does is already in the volume, beside the TSDF (rpe_volume_integrate_color): in the cell a frame vertex
 * lands in, the trilinear luma of the eight colour voxels against the frame's intensity is the residual, and the gradient of the same
 * eight lumas is the row.  No raycast, no model, no model colour, no rpe_photo_prepare; a round is ONE launch that forms both rows.
 * Conventions, followed bit for bit for everything per pixel (fp32, the written order, no FMA contraction; tests/sdf_photo_oracle.py
 * states them in numpy); the sums are held to a rounding bound.  (R, t) as every pose12 (Xc = R Xw + t); the frame's level-l vertex Xc
 * and level-l intensity If (the photometric term's intensity pyramid of the frame's colour: NaN where A = 0); the volume's o, s, tr as
 * rpe_volume_init cast them; gate = (float)dist_thr; lam = (float)weight, in metres per intensity level.
 * The term, per frame pixel of level l:
 *  1. Xc has three finite components and If is finite.  Xw and the field's cell (i0, a) are steps 1-2 of the volume term.
 *  2. The eight TSDF corners are known and unsaturated and fabsf(D * tr) <= gate: the volume term's steps 3-4.  Its slope and normal
 *     gates are NOT asked: a photometric row stands wherever the point lies on the fused surface within the gate.
 *  3. The eight colour-volume corners of the same cell all have colour weight > 0 (the colour field's "known").  Each corner's luma
 *     y = ((0.299f * r + 0.587f * g) + 0.114f * b), on its binary16 channels widened exactly to fp32: the photometric term's
 *     intensity, on the 0 .. 255 scale.  A channel that is NaN or Inf under a weight > 0 is NOT gated: it goes through steps 4-6 as
 *     any value does, into the row and into the sums.
 *  4. Iv = the trilinear value of the eight y through the field's lerp chain (x, then y, then z).  The gradient (gx, gy, gz) of the
 *     same eight y by exactly the three corner-difference expressions of the volume term's step 5, in levels per voxel;
 *     m = (gx / s, gy / s, gz / s).
 *  5. a[i] = -((R[3i] * m.x + R[3i+1] * m.y) + R[3i+2] * m.z); r = Iv - If; J = [a | Xc x a], the cross product as in the volume
 *     term's step 8; tangent order and update are those of rpe_normal_eq.
 *  6. r' = lam * r and J' = lam * J (fp32), accumulated beside the geometric row of the same pixel -- the volume term's, unchanged,
 *     normal gate included, weight 1.  Both fp32 rows are widened to fp64 and their products added with fp64 fused multiply-adds
 *     (a product of two floats is exact in fp64), then the fixed order of every reduction here: every sum is within 8 * 2^-24 of the
 *     sum of the magnitudes of its products.
 * What the term is NOT.  The colour is the volume's voxel-size blend: a coarser, noisier measurement than a frame's own pixels.  It
 * reads the dense window only: voxels in the archive's bricks give no row here -- "Map volume colour term" below is the same term over
 * the window AND the archived bricks (rpe_map_sdf_photo_rows ... rpe_icp_pyramid_map_sdf_rgbd).  Rows are not weighted by voxel weight.  Its basin is still the truncation band: a point further than trunc
 * from the fused surface gives neither row.
 * The calls need a frame (with the levels asked), a frame colour, a volume and a colour volume, RPE_ERR_STATE otherwise; they need NO
 * model and NO rpe_photo_prepare.  They build the frame's intensity pyramid themselves (one launch, into a buffer of their own, kept
 * until the frame's depth or colour is replaced) and neither read nor replace the model, the model colour, the prepared photometric
 * maps, the solver slots, the volumes or the archive. */
/* {r, J[0..5]} of the photometric row of every frame pixel of the level, UNSCALED as rpe_photo_rows gives them, as 7 planes of
 * w_l*h_l floats, NaN where the pixel has no row.  level >= 0, dist_thr >= 0 */
int rpe_sdf_photo_rows(rpe_context* ctx, int level, const double* pose12, double dist_thr, float* rows);
/* the photometric normal equations ALONE, laid out as rpe_photo_normal_eq: H upper triangle (21) | g (6) of the rows scaled by
 * weight | [27] sum r'^2 | [28] rows | [29] pivot floor.  weight finite and > 0 */
int rpe_sdf_photo_normal_eq(rpe_context* ctx, int level, const double* pose12, double dist_thr, double weight, double* out32);
/* rpe_icp_sdf / rpe_icp_pyramid_sdf with the photometric rows beside the geometric ones: the same conventions (of opt, max_iter, tol,
 * dist_thr, cos_thr and use_normals are read; host-driven only: device_resident = 1 is RPE_ERR_ARG; RPE_ERR_DEGENERATE as rpe_icp_sdf)
 * and photo_weight, finite and > 0 (RPE_ERR_ARG otherwise).  final_cost / matched are the geometric sum of r^2 and rows of the last
 * round, photo_cost / photo_matched the photometric sum of r'^2 and rows; the pyramid form reports level 0's. */
int rpe_icp_sdf_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, double* pose12, int* iters_out, double* last_step,
                     double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched);
int rpe_icp_pyramid_sdf_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, int levels, const int* iters_per_level,
                             const double* dist_thr_per_level, double* pose12, int* iters_out, double* last_step, double* final_cost,
                             int64_t* matched, double* photo_cost, int64_t* photo_matched);

/* ---- Features and relocalisation: correspondences WITHOUT a pose guess.  rpe_associate pairs under a guess, so every entry above
 * that produces a pose from images needs a start inside ICP's basin; a lost tracker has none.  Here keypoints of the frame's colour
 * and of the model view's colour are described and matched by appearance, the matched pixels' vertices, normals and bearings go into
 * the five solver slots, and the RANSAC / PROSAC solvers of rpe_run produce the pose that ICP then refines.  Conventions, followed
 * bit for bit -- everything is integer arithmetic or a comparison (tests/feature_oracle.py states them in numpy):
 * Sides: RPE_FEAT_FRAME = the frame colour (RGBA8) with the frame's level-0 vertex / normal / bearing maps; RPE_FEAT_MODEL = the model
 * colour (rpe_model_sample_color, rpe_model_color_upload, rpe_model_color_from_frame) with the model's level-0 world vertex / normal
 * maps.  rpe_photo_prepare is not needed.  Whatever replaces the frame's depth or colour drops the frame's features, whatever
 * replaces the model or its colour the model's; a new detection on either side drops the match list.
 * Luma: Y = (77 r + 150 g + 29 b + 128) >> 8, and 0 where A = 0.  Pixels outside the image count as Y = 0, A = 0.
 * Detector: segment test on the 16-pixel ring of radius 3, offsets (dx, dy), y down, clockwise from the top: (0,-3) (1,-3) (2,-2)
 * (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).  A pixel is a corner iff nine
 * contiguous ring pixels (cyclically) are all > Y + t or all < Y - t (t = threshold, 1 .. 255, default 12), it lies at least 16 pixels
 * from every image edge, A != 0 at the centre and on all 16 ring pixels, and the view's vertex and normal at the centre are finite
 * (normals are NaN across depth jumps: silhouette corners stay out).  Score = sum over the ring of max(|Y_ring - Y| - t, 0).
 * Suppression, 3 x 3: a corner survives iff its score beats all 8 neighbours' (a non-corner scores 0), a tie going to the lower pixel
 * index v * width + u.  At most max_keypoints (1 .. RPE_MAX_KEYPOINTS, the top_k limit of rpe_prosac_order) are kept: the strongest
 * by (score descending, pixel index ascending).  The kept ones are LISTED IN PIXEL-INDEX ORDER; a keypoint's id is its list position.
 * Descriptor: upright, fixed scale, 256 bits over S = the 5 x 5 box sum of Y around a pixel (<= 6375).  Bit i is
 * S(p + a_i) < S(p + b_i); the 256 offset pairs lie within +-13 (patch plus box stay inside the 16-pixel border) and are
 * csrc/rpe_brief_table.h, generated by scripts/gen_brief_table.py from the project's PCG32 stream by the rule stated there.  Bit i is
 * bit i % 32 of word i / 32; eight uint32 per keypoint.
 * Oriented descriptor (RPE_DESC_ORIENTED; RPE_DESC_UPRIGHT, the one above, is the default): the same tests on offsets turned into the
 * patch's own orientation, so that a camera rolled about its axis sees the same bits (tests/oriented_oracle.py states it in numpy).
 * The detector -- luma, segment test, score, suppression, cap, keypoint order -- is the same for both kinds.  Moments over the disc
 * D = {(dx, dy): dx^2 + dy^2 <= 169} (529 offsets; a keypoint lies 16 pixels inside, so D is in the image): m10 = sum_D dx Y(p + d),
 * m01 = sum_D dy Y(p + d), Y the luma above (0 where A = 0); |m| <= 2914 * 255 fits int32.  Angle bin, 32 bins: with
 * C[k] = round(1024 cos(2 pi k / 32)) = 1024 1004 946 851 724 569 392 200 0 -200 -392 -569 -724 -851 -946 -1004 -1024 -1004 -946
 * -851 -724 -569 -392 -200 0 200 392 569 724 851 946 1004 and S[k] = C[(k + 24) % 32] (tabulated, never computed on the device),
 * bin = the k that maximises m10 C[k] + m01 S[k] in int64, a tie going to the lowest k (m10 = m01 = 0 gives bin 0).  Steering: an
 * offset (x, y) of the table becomes x' = (x C[bin] - y S[bin] + 512) >> 10, y' = (x S[bin] + y C[bin] + 512) >> 10, the shift
 * arithmetic (floor); bin 0 is the identity, bins 8, 16 and 24 are exact quarter turns; over the table the steered offsets reach
 * +-17, which with the box's 2 passes the 16-pixel border.  Bit i is S(p + a'_i) < S(p + b'_i) over the same box sums, a sample
 * position outside the image reading S = 0 (box sums inside the image count outside pixels as 0 already); the packing is unchanged.
 * An oriented descriptor whose bin is 0 equals the upright descriptor of the same keypoint.  The kind belongs to the context
 * (rpe_features_set_descriptor) and applies to every later detection on either side, rpe_relocalize*'s own included; descriptors of
 * the two kinds are never matched against each other.
 * Matching: for frame keypoint q, d1 / d2 = the smallest / second smallest Hamming distance over the model keypoints (the second
 * over all others, so a duplicate gives d2 = d1), the index that of the first smallest; d2 = 257 with one model keypoint; no match
 * without any.  Accepted iff d1 <= max_dist and d1 * ratio_den < d2 * ratio_num (ints; defaults 64 and 8 / 10; max_dist 0 .. 256,
 * ratio terms 1 .. 65536) and, with cross_check = 1, q is in turn the best of its model keypoint under the same tie rule.  Matches
 * are listed in frame-keypoint order.
 * Slots: rpe_features_match declares the problem (n = matches, RPE_F32) and fills, per match, XW / NW = the model vertex / normal at
 * the model keypoint, XC / NC / BV = the frame's vertex / normal / bearing at the frame keypoint.  The match quality 256 - d1 is the
 * float weight of the match (rpe_matches_download): what a PROSAC solver sorts.
 * Scale levels (rpe_features_set_levels(n), n = 1 .. 4; 1, the stage above on the image itself, is the default): the detector and the
 * descriptor on a fixed ladder of levels l = 0 .. n - 1 of scale p / q = 1 / 1, 2 / 3, 1 / 2, 1 / 3 (steps of 1.5, 1.33, 1.5), so
 * that a camera that has moved CLOSER to what it mapped finds the corners it mapped (tests/scale_oracle.py states it in numpy).  For
 * a side of w x h: w_l = floor(w p / q), h_l = floor(h p / q).  Luma: Y_0 is the luma above; Y_l(u, v) = floor((sum over j, i = 0 ..
 * q - 1 of Y_0(floor((q u + i) / p), floor((q v + j) / p)) + floor(q^2 / 2)) / q^2) -- the image repeated p times per axis, averaged
 * over q x q blocks: weights (2, 1) and (1, 2) alternating over two source pixels per axis at 2 / 3, the rounded 2 x 2 mean at 1 / 2,
 * the rounded 3 x 3 mean at 1 / 3; every source index lies in the image.  Known: K_l(u, v) iff every source pixel of that sum has
 * A != 0 (K_0 = A != 0).  Centre: level pixel u stands at level-0 pixel c(u) = floor(((2 u + 1) q - p) / (2 p)) -- 2 u at 1 / 2,
 * 3 u + 1 at 1 / 3, floor((6 u + 1) / 4) at 2 / 3 -- and v likewise; a level keypoint's vertex, normal, bearing and "finite" test are
 * those of level-0 pixel (c(u), c(v)).  Detector per level: the one above on (Y_l, K_l) with K_l in A's place -- ring of radius 3,
 * border of 16 and the 3 x 3 suppression all IN LEVEL PIXELS, nothing suppressed across levels; a level with w_l <= 32 or h_l <= 32
 * has no keypoint.  Order and cap: the survivors of all levels form one list in (level ascending, level pixel index v w_l + u
 * ascending) order; of more than max_keypoints the strongest stay by (score descending, then that order), listed in that order; a
 * keypoint's id is its list position; RPE_MAX_KEYPOINTS bounds the total.  Descriptor: either kind, unchanged, ON THE KEYPOINT'S OWN
 * LEVEL -- box sums and moments of Y_l (not zeroed where K_l fails), the steered offsets' out-of-image rule against w_l x h_l.  A
 * keypoint REPORTS xy = (c(u), c(v)), the level-0 pixel (two keypoints of different levels may share it: both stay), so matching, the
 * slots, the keyframe store and the graph take a multi-level detection unchanged, and a store filled at one number of levels may be
 * queried at another: the descriptors are comparable, only the yield differs.  rpe_features_scale gives the level and the level
 * pixel.  The bearing of a level-l keypoint is that of its level-0 pixel, up to q / (2 p) pixels (1.5 at level 3) from the level
 * pixel's true centre: thre_2d of a solver that scores bearings (rpe_relocalize's) has to leave room for it.  What the levels cost
 * on a pair that has NOT changed scale: more matches, a smaller share of them correct (the 320 x 240 `narrow` pair of the tests: 919
 * matches, 0.973 correct at 1 level; 2105, 0.939 at 4).  What they do not do: no level above scale 1 (a camera that moved AWAY is
 * served only as far as the keyframe's own coarser levels meet the frame's finer ones), no suppression across levels, bearings
 * quantised to level-0 pixels, no gate on a match by depth ratio against level difference.
 * Scope: descriptors are compared at the levels of the fixed ladder only (no patch scaled by the keypoint's depth).  The model is ONE view; a caller who keeps many adds each to the keyframe store
 * below ("Keyframes") and relocalises against all of them at once -- nothing is re-uploaded or re-detected. */
typedef struct { int threshold; int max_keypoints; } rpe_feature_options;                       /* NULL: {12, RPE_MAX_KEYPOINTS} */
typedef struct { int max_dist; int ratio_num, ratio_den; int cross_check; } rpe_match_options;  /* NULL: {64, 8, 10, 0} */
enum { RPE_FEAT_FRAME = 0, RPE_FEAT_MODEL = 1, RPE_MAX_KEYPOINTS = 4096 };
enum { RPE_DESC_UPRIGHT = 0, RPE_DESC_ORIENTED = 1 };
/* the descriptor kind of every later detection of this context.  A change of kind drops both sides' features and the match list;
 * setting the current kind again drops nothing.  RPE_ERR_ARG for any other kind */
int rpe_features_set_descriptor(rpe_context* ctx, int kind);
int rpe_features_get_descriptor(rpe_context* ctx, int* kind);
/* the number of scale levels (1 .. 4, "Scale levels" above) of every later detection of this context, rpe_relocalize*'s own included.
 * A change drops both sides' features and the match list; setting the current number again drops nothing.  The keyframe store is not
 * touched and sets no condition.  RPE_ERR_ARG for any other number */
int rpe_features_set_levels(rpe_context* ctx, int levels);
int rpe_features_get_levels(rpe_context* ctx, int* levels);
/* detect and describe the keypoints of one side (six launches, eight with more than one level; one host wait for the count either way); RPE_ERR_STATE without the side's depth
 * or model and colour, RPE_ERR_ARG for options out of range */
int rpe_features_detect(rpe_context* ctx, int which, const rpe_feature_options* opt, int* count);
/* the side's keypoints: xy 2 x count int32 (u, v per keypoint), score count int32, desc 8 x count uint32 (any may be NULL);
 * RPE_ERR_STATE before a detection or after its features were dropped */
int rpe_features_download(rpe_context* ctx, int which, int32_t* xy, int32_t* score, uint32_t* desc);
/* the angle bins (0 .. 31) of the side's keypoints, count int32: all 0 for an upright detection; RPE_ERR_STATE as rpe_features_download */
int rpe_features_angles(rpe_context* ctx, int which, int32_t* bins);
/* the level (0 .. levels - 1) and the level pixel (u, v) of the side's keypoints: count int32 and 2 x count int32 (either may be NULL);
 * with one level all levels are 0 and lxy = xy; RPE_ERR_STATE as rpe_features_download */
int rpe_features_scale(rpe_context* ctx, int which, int32_t* level, int32_t* lxy);
/* match the frame's keypoints against the model's and fill XW XC BV NW NC (n = matches; 0 matches leave an empty problem);
 * RPE_ERR_STATE unless both sides have features */
int rpe_features_match(rpe_context* ctx, const rpe_match_options* opt, int* matches);
/* the last match list: frame / model keypoint ids, d1, d2 and the weight 256 - d1, `matches` values each (any may be NULL) */
int rpe_matches_download(rpe_context* ctx, int32_t* frame_idx, int32_t* model_idx, int32_t* d1, int32_t* d2, float* weight);
/* relocalise the frame against the model: detects on each side whose features are missing (or were made with other options or another
 * descriptor kind), matches,
 * and runs rpe_run's solver `method` (0 .. 9) with stage `ls` on the matches -- rpe_run itself, on the downloaded arrays, weights =
 * the match quality for every modality, focal lengths of the frame's camera, RPE_SCORE_EXACT, the stream of `seed`.  iter_io,
 * confidence, the thresholds, max_votes and mask_out (3 x matches shorts; give room for 3 x RPE_MAX_KEYPOINTS) are rpe_run's.
 * pose12 = the solver's pose (Xc = R Xw + t), the start for rpe_icp_pyramid(_rgbd).  RPE_ERR_DEGENERATE with fewer than min_matches
 * (>= 4) matches: *matches is set, pose12 is left untouched.  The slots keep the matches. */
int rpe_relocalize(rpe_context* ctx, const rpe_feature_options* fopt, const rpe_match_options* mopt, int method, double thre_3d,
                   double thre_2d, double thre_nl, int* iter_io, double confidence, uint64_t seed, int ls, int min_matches,
                   double* pose12, int* matches, int* max_votes, short* mask_out);

/* ---- Keyframes: the model side's features kept on the device, and a frame relocalised against all of them at once.  A lost tracker
 * does not know which of its keyframes the camera sees; what the solvers need from a keyframe is small -- per keypoint the descriptor
 * and the world vertex and normal (at most 64 B x RPE_MAX_KEYPOINTS) -- so the context keeps it, and the frame's keypoints are matched
 * against every keyframe in one pass.  Conventions, bit for bit (tests/keyframe_oracle.py states them in numpy):
 * Store: a keyframe = the model side's current detection: xy and desc of rpe_features_download(RPE_FEAT_MODEL) and, per keypoint, the
 * model's level-0 world vertex xw and normal nw at its pixel (count x 3 floats each), with the model's pose (rpe_model_upload's /
 * rpe_model_from_frame's pose12, informative) and level-0 width and height.  A keyframe made from a tracked frame goes through
 * rpe_model_from_frame + rpe_model_color_from_frame + rpe_features_detect(RPE_FEAT_MODEL) first.  Ids are 0, 1, ... in insertion order;
 * at most RPE_MAX_KEYFRAMES.  The store belongs to the context: it survives new frames, new models, rpe_volume_init and new detections
 * and is freed with the context; its memory grows in steps as keyframes are added.  Removing ONE keyframe is out of scope:
 * rpe_keyframes_clear empties the store and drops its graph (a saved map comes back through rpe_keyframe_add_host).  Keyframes of different cameras may
 * share a store.  A store has ONE descriptor kind, that of its first keyframe (rpe_keyframe_add: the kind of the model's detection;
 * rpe_keyframe_add_host: the context's current kind); rpe_keyframes_clear forgets it.  RPE_ERR_STATE for a keyframe of the other kind
 * added to a non-empty store, for rpe_keyframes_query / rpe_keyframe_match with frame features of the other kind, and for
 * rpe_relocalize_keyframes while the context's kind differs from the store's.  Matching, ranking and the solver runs do not depend on
 * the kind.
 * Query: per keyframe k, count[k] = the number of matches rpe_features_match would accept with keyframe k's keypoints as the model's
 * (the rules of "Matching" above, over the keypoints of k ALONE: d2 = 257 with one keypoint, no match against an empty keyframe; the
 * cross-check is per keyframe too).  order = the ids sorted by (count descending, id ascending).  One host wait.
 * Match: rpe_keyframe_match(id) is rpe_features_match with keyframe id in the model's place: the problem is declared, XW / NW come
 * from the store, XC / NC / BV from the frame's maps, and rpe_matches_download gives the list (model_idx = the keypoint's position
 * inside the keyframe).  A new detection on the frame, rpe_keyframes_clear or any later match call drops that list.  Cost: the store's
 * matcher gives one keyframe a few workgroups only, so ONE such call takes about twice rpe_features_match's time against the same
 * keypoints as the model; the store pays from the query on, where the keyframes share one launch.
 * Relocalise: rpe_relocalize_keyframes detects on the frame (if its features are missing or were made with other options), queries,
 * and walks the ranking over the first `candidates` (>= 1) keyframes, stopping at the first with fewer than min_matches (>= 4)
 * matches.  Each candidate gets exactly rpe_relocalize's run: the downloaded slots through rpe_run, weights = the match quality for
 * every modality, the frame's focal lengths, RPE_SCORE_EXACT, the same seed and the same incoming *iter_io; a candidate rpe_run
 * refuses with RPE_ERR_DEGENERATE is skipped.  The candidate with the most max_votes wins, a tie going to the better rank.  On return
 * pose12, *keyframe, *matches, *iter_io, *max_votes, mask_out (3 x matches shorts; give room for 3 x RPE_MAX_KEYPOINTS), the slots and
 * the match list are the winner's.  RPE_ERR_DEGENERATE when the best-ranked keyframe has fewer than min_matches matches (or every
 * candidate was refused): *keyframe = the best-ranked id, *matches = its count, pose12 is left untouched. */
enum { RPE_MAX_KEYFRAMES = 256 };
/* the model side's current features become keyframe *id (may be NULL); RPE_ERR_STATE without a model detection or with a full store */
int rpe_keyframe_add(rpe_context* ctx, int* id);
/* the same from host arrays (count 0 .. RPE_MAX_KEYPOINTS; xy 2 x count int32 inside width x height, desc 8 x count uint32, xw / nw
 * 3 x count floats, NULL allowed for count = 0); RPE_ERR_ARG for bad arguments, RPE_ERR_STATE with a full store */
int rpe_keyframe_add_host(rpe_context* ctx, int count, const int32_t* xy, const uint32_t* desc, const float* xw, const float* nw,
                          const double* pose12, int width, int height, int* id);
/* what the store knows of keyframe id (any output may be NULL); RPE_ERR_ARG for an id that is not in the store */
int rpe_keyframe_info(rpe_context* ctx, int id, int* count, double* pose12, int* width, int* height);
/* keyframe id's arrays, shaped as rpe_keyframe_add_host takes them (any may be NULL) */
int rpe_keyframe_download(rpe_context* ctx, int id, int32_t* xy, uint32_t* desc, float* xw, float* nw);
int rpe_keyframes_count(rpe_context* ctx, int* count);
/* the store's descriptor kind (RPE_DESC_*), -1 while it is empty */
int rpe_keyframes_descriptor(rpe_context* ctx, int* kind);
/* empties the store (its memory is kept for the next keyframes) */
int rpe_keyframes_clear(rpe_context* ctx);
/* counts[k] and order[r] for the K keyframes of the store (K ints each); RPE_ERR_STATE without frame features or with an empty store */
int rpe_keyframes_query(rpe_context* ctx, const rpe_match_options* mopt, int* counts, int* order);
/* rpe_features_match against keyframe id; RPE_ERR_STATE as rpe_keyframes_query, RPE_ERR_ARG for an id that is not in the store */
int rpe_keyframe_match(rpe_context* ctx, int id, const rpe_match_options* mopt, int* matches);
int rpe_relocalize_keyframes(rpe_context* ctx, const rpe_feature_options* fopt, const rpe_match_options* mopt, int candidates, int method,
                             double thre_3d, double thre_2d, double thre_nl, int* iter_io, double confidence, uint64_t seed, int ls,
                             int min_matches, double* pose12, int* keyframe, int* matches, int* max_votes, short* mask_out);

/* ---- Keyframe graph: close loops -- every keyframe pose of the store refined jointly from keyframe-to-keyframe matches.  The pose
 * kept with a keyframe is the tracker's at the time; after a long path the keyframes around a loop disagree by the accumulated drift.
 * Here the keyframes are linked by the matches of their own keypoints (nothing new is detected or uploaded), and a gated Gauss-Newton
 * over ALL poses makes the matched world points agree.  tests/graph_oracle.py states every rule in numpy.
 * Graph: an edge (j, i), j > i, is the match list rpe_features_match would give with keyframe j's descriptors as the frame's and
 * keyframe i's as the model's (cross-check per pair of keyframes), kept when it has >= min_matches (>= 3) pairs.  Edges are ordered
 * by (j, i), the pairs of an edge by j's keypoints; a pair is (a, b) = positions inside keyframe j / keyframe i.  rpe_keyframes_link
 * drops the edges whose newer keyframe is >= first and builds them again (first = a new keyframe's id links it; first = 0 rebuilds
 * all): per j one launch of the store's matcher against the keyframes 0 .. j - 1 and ONE host wait.  rpe_graph_add_edge_host puts a
 * caller's own pairs (a solver's inliers) in an edge's place.  The graph lives beside the store, grows in steps as it does, and
 * rpe_keyframes_clear drops it.
 * Round: poses are Xc = R Xw + t; keyframe k sits in the store at T0_k with fp32 world points x.  At trial poses T_k a point's world
 * position is X_k(x) = C_k x + c_k, C_k = R_k^T R0_k, c_k = R_k^T (t0_k - t_k): computed on the host in fp64 and handed to the device
 * as 12 floats per keyframe (a pose with the store's own bits gives the identity exactly).  In fp32, every product and sum rounded on
 * its own: X[r] = (((C[3r] x[0]) + (C[3r+1] x[1])) + (C[3r+2] x[2])) + c[r].  A pair's residual is r = X_j(x_a) - X_i(x_b); it counts
 * iff the six coordinates are finite and ((r0 r0) + (r1 r1)) + (r2 r2) < gate^2, gate cast to fp32 and squared in fp32.  The update is
 * T_k <- exp(delta_k) T_k as rpe_gn_apply does it, tangent order (upsilon, omega): dX_k/d upsilon = -R_k^T, dX_k/d omega =
 * R_k^T [p]x, p = R_k X_k + t_k; the residual's row by keyframe i has the other sign.  ONE launch serves every edge (one workgroup per
 * edge); behind the fp32 rows all arithmetic is fp64 in a fixed order (no atomics): the same call gives the same bits.
 * Record, RPE_GRAPH_RECORD doubles per edge: [0] counted pairs | [1] cost = sum |r|^2 | [2..7] g_j | [8..13] g_i | [14..34] H_jj upper
 * triangle row-major | [35..55] H_ii upper triangle | [56..91] H_ji row-major (rows: keyframe j's tangent).  The system is H delta = -g.
 * Optimise: per round the corrections, the launch, one copy of the records to the host, rpe_graph_solve, the left update; it ends
 * early when |delta| < tol.  Fixed: `anchor`, and the lowest id of every other connected component -- components over the edges with
 * >= 1 counted pair in the FIRST round; a keyframe without such an edge keeps its pose.  RPE_ERR_STATE without an edge;
 * RPE_ERR_DEGENERATE (nothing is changed) when the joint system is not positive definite.  With apply != 0 the store takes the result:
 * rpe_keyframe_info's poses are the new ones and every keypoint's xw <- C_k xw + c_k, nw <- C_k nw in the fp32 order above (nw without
 * the + c), so that relocalisation answers in the corrected world; edges are indices and stay valid.
 * The TSDF and colour volume follow through rpe_volume_fuse_keyframes ("Keyframe depth and rebuilding the volume" below): keyframes
 * that carry their depth are fused again at the corrected poses in one launch.
 * Out of scope: relative-pose (odometry) edges; robust kernels other than the gate; removing a keyframe; a sparse or device-side
 * solve (rpe_graph_solve is dense, K <= RPE_MAX_KEYFRAMES). */
enum { RPE_GRAPH_RECORD = 92 };
/* (re)build the edges of the keyframes >= first (0 .. the store's count); *edges / *pairs (may be NULL) = the graph's totals.
 * RPE_ERR_STATE with an empty store, RPE_ERR_ARG for first out of range, min_matches outside 3 .. RPE_MAX_KEYPOINTS or bad options */
int rpe_keyframes_link(rpe_context* ctx, int first, const rpe_match_options* mopt, int min_matches, int* edges, int64_t* pairs);
/* edge (j, i) := the caller's `count` (1 .. RPE_MAX_KEYPOINTS) pairs, replacing an existing edge (j, i); RPE_ERR_ARG for j <= i, ids
 * that are not in the store and positions outside the keyframes.  A replacement that fits reuses the old pairs' place; dead pairs of
 * replaced edges are compacted away once they outweigh the live ones */
int rpe_graph_add_edge_host(rpe_context* ctx, int j, int i, int count, const int32_t* a, const int32_t* b);
int rpe_graph_info(rpe_context* ctx, int* edges, int64_t* pairs);
/* (j, i, count) per edge: 3 x edges int32 */
int rpe_graph_edges(rpe_context* ctx, int32_t* jic);
/* the pairs of edge number `edge` (its position in rpe_graph_edges' order): `count` int32 each (either may be NULL) */
int rpe_graph_edge_download(rpe_context* ctx, int edge, int32_t* a, int32_t* b);
/* r of every pair at poses12 (K x 12 doubles; NULL = the store's), edges in order: pairs x 3 floats, NaN where the pair does not count */
int rpe_graph_residuals(rpe_context* ctx, const double* poses12, double gate, float* r);
/* the records of one round: edges x RPE_GRAPH_RECORD doubles */
int rpe_graph_normal_eq(rpe_context* ctx, const double* poses12, double gate, double* records);
/* gates: one per round; stats (may be NULL): 3 x rounds doubles, per round run {counted pairs, cost, |delta|}; *rounds_out (may be
 * NULL) = the rounds run; poses12_out (may be NULL): K x 12 doubles */
int rpe_keyframes_optimize(rpe_context* ctx, int anchor, int rounds, const double* gates, double tol, int apply, double* poses12_out,
                           double* stats, int* rounds_out);

/* ---- Keyframe depth and rebuilding the volume: after rpe_keyframes_optimize(apply = 1) the store answers in the corrected world, but
 * the TSDF and colour volume still hold every frame fused at its drifted pose.  A keyframe may therefore carry an ATTACHMENT -- its
 * level-0 metric depth, the camera it was taken with and, optionally, its colour -- and rpe_volume_fuse_keyframes fuses a list of
 * attachments into the context's volume in ONE pass over the voxels.  tests/rebuild_oracle.py states the result in numpy.
 * Attachment: the depth is a packed plane, one fp32 per pixel, NaN = invalid: exactly the values rpe_volume_integrate reads from the
 * frame, the z of its level-0 vertex map (so an attached keyframe fuses as the frame itself would have, depth filter included); the
 * colour is the frame's RGBA8 map.  The camera is kept as the rpe_camera given and as the fp32 camera the kernels use.  The memory
 * belongs to the store: rpe_keyframes_clear drops every attachment (and keeps the memory for the next keyframes), rpe_destroy frees
 * it.  Cost: 4 B per pixel for the depth plus 4 B per pixel for the colour -- 2.4 MB per keyframe at 640 x 480, about 630 MB for a
 * full store of RPE_MAX_KEYFRAMES.  Attachments do not take part in rpe_keyframes_optimize, rpe_keyframes_link, rpe_keyframes_query
 * or rpe_relocalize_keyframes: their outputs are the same bits with and without.
 * Fuse, THE CONTRACT: after rpe_volume_fuse_keyframes the volume, the colour volume and every piece of volume state are, bit for
 * bit, what this sequence leaves:
 *   1. with RPE_FUSE_CLEAR: rpe_volume_init with the volume's own descriptor;
 *   2. for each list entry in order: that keyframe's depth (and colour) as the current frame, then rpe_volume_integrate(pose) or,
 *      with RPE_FUSE_COLOR, rpe_volume_integrate_color(pose), the pose cast to fp32 as every integrate casts it.
 * The state this covers: a mesh extracted before stays valid without RPE_FUSE_CLEAR and is dropped with it; with RPE_FUSE_CLEAR
 * but without RPE_FUSE_COLOR the colour volume is dropped, as rpe_volume_init drops it; with both it exists and untouched voxels are
 * zero; without RPE_FUSE_CLEAR, RPE_FUSE_COLOR makes (and clears) a colour volume if there is none.  A voxel that no keyframe updates
 * keeps its bits (without RPE_FUSE_CLEAR) or is zero (with it).  The current frame, the model and the store are not touched.  The
 * host waits once, for the upload of the list's descriptor table.
 * Cull: a workgroup of the kernel owns a brick of 32 x 8 x 4 voxels and skips the list entries that cannot update any of them (every
 * voxel centre behind the camera, or all outside the same image edge).  The test is conservative: the result has the same bits
 * with RPE_FUSE_NO_CULL, which switches it off (tests, timing).
 * Out of scope: the frames BETWEEN keyframes (the rebuilt volume holds the keyframes only); de-integrating a single frame; fusing
 * in any order but the list's; compressing the stored depth (16-bit or binary16 depth would break the bit contract); removing a
 * keyframe; rpe_keyframe_add attaching by itself.  (Moving the volume: "Moving volume" below.)
 * The volume archive ("Volume archive" below) is not touched by this call: bricks archived before a correction keep the old poses'
 * surface; rpe_volume_archive_clear forgets them. */
enum { RPE_FUSE_CLEAR = 1, RPE_FUSE_COLOR = 2, RPE_FUSE_NO_CULL = 4 };
/* the CURRENT frame's level-0 depth (z of its vertex map), its camera and, if it has one, its colour become keyframe id's attachment
 * (replacing an earlier one).  RPE_ERR_STATE without a frame; RPE_ERR_ARG for an id not in the store or a frame whose level-0 size is
 * not the keyframe's width x height */
int rpe_keyframe_attach_frame(rpe_context* ctx, int id);
/* the same from host arrays: z = width*height floats (NaN = invalid; the bits are taken as given), rgba = 4*width*height bytes or NULL,
 * cam as everywhere in Part 3 (its size must be the keyframe's) */
int rpe_keyframe_attach_host(rpe_context* ctx, int id, const float* z, const uint8_t* rgba, const rpe_camera* cam);
/* what is attached (any output may be NULL): *have_depth, *have_color 0 / 1, the camera (all zero without an attachment) */
int rpe_keyframe_attachment_info(rpe_context* ctx, int id, int* have_depth, int* have_color, rpe_camera* cam);
/* copy the attachment out (either may be NULL); RPE_ERR_STATE for what is not attached */
int rpe_keyframe_attachment_download(rpe_context* ctx, int id, float* z, uint8_t* rgba);
/* fuse the attachments of `count` (1 .. RPE_MAX_KEYFRAMES) keyframes into the context's volume, in list order; ids = NULL: every
 * keyframe that has a depth attachment, by ascending id (count ignored).  poses12 = NULL: the store's poses (rpe_keyframe_info's);
 * else one pose per LIST ENTRY (count x 12 doubles).  Repeated ids are allowed.
 * RPE_ERR_STATE without a volume, for a listed keyframe without depth, with RPE_FUSE_COLOR for one without colour, and with ids = NULL
 * when no keyframe has depth; RPE_ERR_ARG for ids not in the store, bad count or unknown flags. */
int rpe_volume_fuse_keyframes(rpe_context* ctx, const int32_t* ids, int count, const double* poses12, int flags);

/* ---- Moving volume: the window of the TSDF and colour volume follows the camera.  rpe_volume_init fixes a cube; a camera that walks
 * out of it gets no raycast hits and the session is over.  rpe_volume_shift moves the window by WHOLE VOXELS on the device,
 * rpe_volume_follow proposes the shift that re-centres it in front of the camera, rpe_volume_geometry says where it is now, and
 * rpe_volume_mesh_box extracts the surface of the cubes that are about to leave.  tests/shift_oracle.py states all four in numpy.
 * Shift by (di, dj, dk) voxels along +x, +y, +z.  Content: new voxel (i, j, k) := old voxel (i+di, j+dj, k+dk) where that lies inside
 * the old window, with the bits as they are (NaN payloads, -0 and denormals stay); every other voxel is cleared to {0, 0}.  A colour
 * volume, if there is one, moves by the same rule and its cleared voxels are all-zero bits; if there is none, none comes into being.
 * Geometry: the context keeps the descriptor rpe_volume_init was given (origin and voxel_size as doubles) and an int64 total shift per
 * axis, zeroed by rpe_volume_init.  After a shift origin_now[a] = origin[a] + (double)total[a] * voxel_size, in double as written,
 * and the kernels' fp32 origin is o[a] = (float)origin_now[a]: ONE rounding from the exact value every time, so nothing drifts over
 * many shifts, and at total 0 the origin is the init's again.  Every other call (integrate, raycast, mesh, colour, the keyframe fuse)
 * then sees an ordinary volume at that origin: the shifted context behaves, bit for bit, like a fresh rpe_volume_init at origin_now
 * followed by rpe_volume_upload / rpe_volume_color_upload of the moved content.
 * Edge rules: shift = (0, 0, 0) changes nothing at all (the last mesh stays).  |shift[a]| >= dim[a] on any axis is legal and clears
 * the whole window.  A total shift beyond 2^30 voxels either way on any axis, or an o[a] that is not finite, is RPE_ERR_ARG and
 * nothing has changed.  Any non-zero shift drops the last mesh (rpe_volume_mesh_download and rpe_volume_mesh_colors then return
 * RPE_ERR_STATE).  The frame, the model, the model colour, the keyframes and the graph are in world coordinates and are not touched.
 * Memory: the shift is out of place.  The context keeps a spare of the tsdf volume and, if there is a colour volume, of that too,
 * reserved on the first shift and swapped with the live arrays by each one: 8 B + 8 B per voxel more, 2 GB at 512^3 with colour.
 * rpe_volume_init drops the spares when the volume grows.  The host does not wait.
 * Follow (pose12 with Xc = R Xw + t, look_ahead metres, granule voxels), all in double, in this order: p = (0, 0, look_ahead) - t;
 * c[a] = R[0][a]*p[0] + R[1][a]*p[1] + R[2][a]*p[2], summed left to right (the world point look_ahead metres in front of the camera);
 * centre[a] = origin_now[a] + 0.5 * dim[a] * voxel_size; v[a] = (c[a] - centre[a]) / voxel_size;
 * shift[a] = granule * (int)trunc(v[a] / granule).  So an axis moves only when the target is at least granule voxels off centre, and
 * in multiples of granule.  The shift is computed, not applied.
 * Mesh of a box: exactly rpe_volume_mesh with one more condition on a cube: cube (i, j, k) takes part only if lo[a] <= index[a] <
 * hi[a] on every axis; a cube outside has case 0.  Vertex rule and order (owner voxel index, then axis), triangle order, the normals
 * (the raycast's normal from the field of the WHOLE volume, not of the box), the mesh's lifetime, rpe_volume_mesh_download and
 * rpe_volume_mesh_colors are unchanged; rpe_volume_mesh is the full box (0, dim-1).  Cubes partition along a cut: for a shift di > 0
 * the cubes with i < di are exactly those whose surface is lost and the cubes with i >= di exactly the cubes of the window after the
 * shift, so mesh_box of what leaves, download, shift loses or doubles no triangle.  The extraction still sweeps the whole volume.
 * The tracking loop: follow -> if non-zero: mesh_box of what leaves, download, shift -> raycast -> ICP -> integrate.  What comes IN
 * is empty until frames are fused into it; rpe_volume_fuse_keyframes with RPE_FUSE_CLEAR rebuilds the new window from the store. */
/* move the window by shift[0..2] voxels; RPE_ERR_STATE without a volume, RPE_ERR_ARG for a total beyond 2^30 or a non-finite origin */
int rpe_volume_shift(rpe_context* ctx, const int32_t shift[3]);
/* the init-time descriptor with origin replaced by origin_now; total_shift (may be NULL) = the voxels moved since rpe_volume_init;
 * RPE_ERR_STATE without a volume */
int rpe_volume_geometry(rpe_context* ctx, rpe_volume_desc* desc, int64_t total_shift[3]);
/* the shift that re-centres the window on the point look_ahead metres in front of the camera at pose12; granule >= 1 and a finite
 * look_ahead >= 0 are required and |v[a]| <= 2^30, otherwise RPE_ERR_ARG; RPE_ERR_STATE without a volume */
int rpe_volume_follow(rpe_context* ctx, const double* pose12, double look_ahead, int granule, int32_t shift[3]);
/* rpe_volume_mesh over the cubes lo <= (i, j, k) < hi only: 0 <= lo[a] <= hi[a] <= dim[a] - 1, otherwise RPE_ERR_ARG; an empty box
 * gives an empty mesh */
int rpe_volume_mesh_box(rpe_context* ctx, double min_weight, const int32_t lo[3], const int32_t hi[3], int64_t* n_vertices,
                        int64_t* n_triangles);

/* ---- Volume archive: what leaves the moving window is kept, bit for bit, on the device, and put back when the window returns over it.
 * Without it a voxel that a shift pushes out is destroyed ("What comes IN is empty", above); with it the window plus the archive is a
 * map.  tests/archive_oracle.py states the section in numpy.
 * Brick: 8 x 8 x 8 voxels, aligned in WORLD voxel coordinates.  World voxel = total shift + window index, per axis; world brick =
 * world voxel / 8, an int64 triple (bx, by, bz).  The archive therefore requires every dim and every component of the total shift,
 * and with it on of every shift, to be a multiple of 8 (rpe_volume_follow with granule = 8 proposes such shifts).
 * THE INVARIANT: there is one unbounded store of bricks, keyed by world brick.  A shift (1) writes into it every LEAVING brick -- a
 * brick of the window that has no destination inside the window after the move; for |shift[a]| >= dim[a] on any axis that is every
 * brick -- of which ANY 32-bit word is non-zero in the tsdf or the colour volume, (2) moves the window as rpe_volume_shift always does,
 * (3) takes out of the store every ENTERING brick -- a brick of the new window that was not in the old one -- that the store holds,
 * and writes it over the zeros step 2 left there.  After any sequence of shifts, uploads and integrates, the window and the archive
 * (rpe_volume_archive_download) are what this model gives, bit for bit; the window is always the only holder of what it covers; and
 * shift(d) followed by shift(-d) is the identity on both volumes.  The occupancy rule of step 1 is about BITS, not weights: NaN
 * payloads, -0, and a voxel of weight 0 that has a tsdf all make their brick non-zero, so the round trip is exact for any content.
 * An all-zero brick is not kept, and restores as the zeros it was.
 * Colour: a brick is archived with the colour volume's brick if there is a colour volume, with all-zero colour otherwise, and restores
 * its colour into the colour volume if there is one at that time (into a window without a colour volume only the tsdf brick returns).
 * Memory: a slot is 4 KB for {tsdf, weight} plus 4 KB for colour; the colour plane of the pool is reserved (and zeroed) the first time
 * a brick is archived while a colour volume exists.  The index world brick -> slot lives on the host.
 * Shift with the archive on: a component that is not a multiple of 8 is RPE_ERR_ARG; more non-zero leaving bricks than free slots
 * (capacity - held; the slots of the bricks that enter in the same shift do not count) is RPE_ERR_STATE with both numbers in the
 * message.  Both are decided before anything is written: window, archive and geometry are unchanged.  The host waits ONCE per shift,
 * for the flags that say which leaving bricks are non-zero.  With the archive off rpe_volume_shift is what it was, call for call, and
 * does not wait.
 * Lifetimes: rpe_volume_init drops the archive (pool and content).  rpe_volume_fuse_keyframes does not touch it: after a loop closure
 * has rebuilt the window at corrected poses, the archived bricks still hold the OLD poses' surface -- rebuild window and archive
 * together with rpe_volume_map_fuse_keyframes ("Map fuse", below) instead, or forget the bricks with rpe_volume_archive_clear.
 * rpe_volume_upload, rpe_volume_integrate and the colour calls write the window only.
 * The tracking loop: follow(granule = 8) -> if non-zero: shift -> map raycast ("Map raycast", below: raycasting the archive directly,
 * beside the window) -> ICP -> integrate; with rpe_volume_raycast in its place the model shows the window only.
 * Out of scope: shifts or dims that are not multiples of 8 with the archive on; a device-side index (no host wait); spilling the pool
 * to host memory; moving the archived bricks under a loop-closure correction (they are rebuilt instead: "Map fuse"). */
/* capacity_bricks > 0: switch the archive on with a pool of that many slots, or grow the pool to it (the content stays; a capacity
 * between the number of held bricks and the current capacity changes nothing: the pool does not shrink); 0: switch it off and free
 * everything.  RPE_ERR_ARG for a capacity below the number of held bricks, negative or above 2^24; RPE_ERR_STATE (nothing changed)
 * without a volume or when a dim or a component of the total shift is not a multiple of 8 */
int rpe_volume_archive(rpe_context* ctx, int64_t capacity_bricks);
/* the number of held bricks and the capacity (0 and 0 with the archive off); either may be NULL */
int rpe_volume_archive_info(rpe_context* ctx, int64_t* held, int64_t* capacity);
/* the held bricks sorted by (bz, by, bx): coords = held x 3 int64 (bx, by, bz); tsdf = held x 8 x 8 x 8 x 2 floats in (z, y, x) order,
 * as rpe_volume_download lays a window out; colour (may be NULL) = held x 8 x 8 x 8 x 4 binary16, zeros where none was kept.  Slot
 * numbers are not part of the contract.  With nothing held nothing is written */
int rpe_volume_archive_download(rpe_context* ctx, int64_t* coords, float* tsdf, uint16_t* colour);
/* forget every brick, keep the pool.  (To CORRECT the archived bricks after a loop closure, rather than lose them, rebuild the map
 * with rpe_volume_map_fuse_keyframes.) */
int rpe_volume_archive_clear(rpe_context* ctx);

/* ---- Map mesh: the window and the archived bricks meshed in one extraction.  The MAP is a sparse grid of world voxels (world voxel =
 * total shift + window index, as above): a voxel holds the window's bits where the window covers it, the held brick's bits where the
 * archive holds its world brick, and {0, 0} with all-zero colour -- weight 0, unknown -- everywhere else.  The colour of a window voxel
 * is the colour volume's (zeros without one), of a held voxel the pool's colour plane's (zeros without one).
 * A box of world voxels lo <= w < hi (int64 per axis, multiples of 8, 8 <= hi - lo <= 2^20) defines a VIRTUAL VOLUME: dim = hi - lo,
 * origin = origin_init + (double)lo * voxel_size in double as written, o = (float) of that (rpe_volume_shift's single rounding);
 * voxel_size, trunc and max_weight are the init descriptor's.
 * THE CONTRACT: rpe_volume_map_mesh gives the mesh rpe_volume_mesh gives on a fresh rpe_volume_init of the virtual volume with the
 * map's content uploaded into it, with the same min_weight: the same cubes, known and active rules, cases and tables, the vertex rule
 * o + (((float)i + 0.5f) + t) * s with i the index inside the box, normals from the field of the whole virtual volume (weight > 0,
 * 0 <= i0 <= dim - 2 of the box), winding, and colours C(p) of the virtual colour volume -- the same bits.  Only the ORDER differs,
 * and it is fixed: bricks ascend by (bz, by, bx), as rpe_volume_archive_download sorts them; inside a brick voxels go in (z, y, x)
 * order, x fastest; vertices follow their owner voxel in that order, then axis x < y < z; triangles follow their cube (named by its
 * corner-0 voxel) in that order, then table order.  So the map mesh is a stated permutation of the dense one; with the box equal to
 * the window's extent it is a permutation of rpe_volume_mesh's mesh of the window.  tests/mapmesh_oracle.py states it in numpy.
 * A brick outside the box is absent: cubes that reach over the box's faces are inactive, as at the faces of any volume.
 * The archive does not have to be on: without it the map is the window.  Every dim and every component of the total shift must be a
 * multiple of 8 (the archive's own precondition).  Nothing is written to the window, the archive or the geometry.
 * The result is the last mesh: rpe_volume_mesh_download serves it and it has the same lifetime (dropped by the next extraction of
 * either kind, rpe_volume_init and a non-zero rpe_volume_shift).  Colours are sampled DURING the extraction, when the window has a
 * colour volume or the pool a colour plane; rpe_volume_mesh_colors returns them for a map mesh, RPE_ERR_STATE if neither existed at
 * extraction time (for a window mesh it is unchanged).  Only the bricks of the map that lie in the box are visited, one workgroup per
 * brick; the workspace is 3 KB per such brick, nothing scales with the box.  The host waits once, for the two totals.
 * Out of scope: boxes that are not multiples of 8; simplifying or welding the mesh; a device-side brick index; dense order for the map
 * mesh. */
/* the world-voxel bounding box of the window and every held brick, in multiples of 8; RPE_ERR_STATE without a volume or when a dim or
 * a component of the total shift is not a multiple of 8 */
int rpe_volume_map_bounds(rpe_context* ctx, int64_t lo[3], int64_t hi[3]);
/* marching cubes over the map inside the box lo <= w < hi (lo = hi = NULL: the bounds); min_weight, n_vertices and n_triangles as in
 * rpe_volume_mesh.  RPE_ERR_STATE as rpe_volume_map_bounds; RPE_ERR_ARG for a box that is unaligned, empty or larger than 2^20 voxels
 * on an axis, a bad min_weight, or 2^31 or more vertices */
int rpe_volume_map_mesh(rpe_context* ctx, double min_weight, const int64_t lo[3], const int64_t hi[3], int64_t* n_vertices,
                        int64_t* n_triangles);

/* ---- Map raycast: the window and the archived bricks as ONE model.  rpe_volume_raycast marches through the window's dense array, so a
 * surface the map knows but the window no longer covers gives no model point; this call marches through the map.  The box lo <= w < hi
 * of world voxels defines the VIRTUAL VOLUME that "Map mesh" defines (lo = hi = NULL: rpe_volume_map_bounds): dim = hi - lo,
 * o = (float)(origin_init + (double)lo * voxel_size); voxel size, trunc and max weight are the init call's.  A map voxel holds the
 * window's bits where the window covers it, the held brick's bits where the archive holds its world brick, {0, 0} elsewhere.
 * THE CONTRACT: after the call the model -- vertex map, normal map, model pose and camera, one level -- is, bit for bit, what
 * rpe_volume_raycast(pose12, cam, dmin, dmax) leaves on a fresh rpe_volume_init of that virtual volume with the map's content uploaded.
 * The sample positions z_k = dmin + (float)k * s, the hit rule, z*, the six-sample normal and the NaN rules are the raycast's
 * ("TSDF volume"); tests/mapray_oracle.py states the composition in numpy.  With the box equal to the window's extent o is the window's
 * own o and the result is rpe_volume_raycast's.
 * Colour: with RPE_MAPRAY_COLOR the model colour map is written too, and equals what rpe_model_sample_color would then leave: C(p) of
 * the virtual colour volume -- the window's colour volume where it covers, the pool's colour plane for held bricks, zeros elsewhere.
 * Without the flag the model colour is dropped, as after any raycast.  RPE_ERR_STATE if the flag is set and neither a colour volume
 * nor a colour plane exists.
 * Rules: nothing is written to the window, the archive, the geometry or the last mesh.  The archive need not be on.  Every dim and
 * every component of the total shift must be a multiple of 8 (RPE_ERR_STATE, as rpe_volume_map_bounds); the box rules are the map
 * mesh's (multiples of 8, 8 <= hi - lo <= 2^20), and the box may hold at most 2^24 bricks (RPE_ERR_ARG with the count in the
 * message, decided before anything is reserved); dmin, dmax and the 2^22 samples per ray are rpe_volume_raycast's.
 * How: the host writes a BRICK GRID, one int32 per brick of the box (x fastest; >= 0 a window brick, ~slot a held one, a sentinel for
 * absent), from the window's extent and the archive's index, and uploads it in one copy per call: 4 B per brick of the BOX, 64 MB at
 * the limit.  A sample whose cell starts in an absent brick is unknown without a voxel load.  An occupancy pre-pass first marks every
 * window brick without a weight > 0 absent: exact, since F is known only where all eight corner weights are > 0, and it is the
 * empty-space skip the window raycast does not have.  It reads the whole window once; RPE_MAPRAY_NO_SKIP switches it off and changes
 * no bit of the result.  As measured the pre-pass does not pay in a fused room, where free space in front of a
 * surface has a weight too: break-even at 256^3, 0.25 ms lost at 512^3; the Python and C++ wrappers pass RPE_MAPRAY_NO_SKIP unless
 * asked.  The host does not wait.
 * Out of scope: a device-side brick index; caching the grid between calls; boxes that are not multiples of 8; strides longer than one
 * sample through absent space. */
enum { RPE_MAPRAY_COLOR = 1, RPE_MAPRAY_NO_SKIP = 2 };
/* the model := the map inside the box raycast from pose12 with camera cam over camera depths (dmin, dmax).  RPE_ERR_STATE without a
 * volume, for unaligned dims or total shift, or for RPE_MAPRAY_COLOR without any colour; RPE_ERR_ARG for a NULL pose or camera, lo
 * without hi, unknown flags, a bad box, more than 2^24 bricks, bad dmin / dmax: the model is as before */
int rpe_volume_map_raycast(rpe_context* ctx, const double* pose12, const rpe_camera* cam, double dmin, double dmax,
                           const int64_t lo[3], const int64_t hi[3], int flags);

/* ---- Map volume term: a frame tracked against the TSDF of the whole MAP -- the window and the archived bricks.  "Volume term" reads the
 * window's dense array, so a surface the map knows but the window no longer covers gives no row; these calls read the map.  No new
 * arithmetic: the box lo <= w < hi of world voxels defines the VIRTUAL VOLUME that "Map mesh" and "Map raycast" define (lo = hi = NULL:
 * rpe_volume_map_bounds): dim = hi - lo, o = (float)(origin_init + (double)lo * voxel_size), one rounding; voxel size, trunc and max
 * weight are the init call's.  A map voxel holds the window's bits where the window covers it, the held brick's bits where the archive
 * holds its world brick, {0, 0} elsewhere.
 * THE CONTRACT: rpe_map_sdf_rows returns, bit for bit, what rpe_sdf_rows returns in a second context whose volume is a fresh
 * rpe_volume_init of that virtual volume with the map's content uploaded: steps 1-8 of "Volume term" on the virtual volume
 * (tests/mapsdf_oracle.py states the composition in numpy).  With the box equal to the window's extent o is the window's own o and the
 * rows are rpe_sdf_rows' of the same context.  The record of rpe_map_sdf_normal_eq is the one rpe_sdf_normal_eq returns -- the same 32
 * doubles, the row count exact, every sum within 8 * 2^-24 of the sum of the magnitudes of its products; it need not equal
 * rpe_sdf_normal_eq's to the bit, because the sums are formed otherwise: a pixel's fp32 row is widened to fp64 and its products are
 * accumulated in fp64 (a product of two floats is exact there), one pixel per thread and loop trip, then the fixed order of every
 * reduction here.  The loops are rpe_icp_sdf's and rpe_icp_pyramid_sdf's, round for round, with that record.
 * Rules: a frame (with the levels asked) and a volume, as "Volume term"; every dim and every component of the total shift a multiple of
 * 8 (RPE_ERR_STATE, as rpe_volume_map_bounds); the box rules are the map mesh's (multiples of 8, 8 <= hi - lo <= 2^20), lo and hi both
 * given or both NULL, and the box may hold at most 2^24 bricks (RPE_ERR_ARG with the count in the message).  The archive need not be on:
 * the map is then the window.  The calls read the frame's maps, the window, the pool and the archive's index, and write nothing but the
 * uploaded grid and the reduction's scratch: the model, the model colour, the prepared photometric maps, the solver slots, the last
 * mesh, both volumes and the archive stay as they were.
 * How: the BRICK GRID of "Map raycast" (one int32 per brick of the box) is built on the host and uploaded ONCE per call -- the map cannot
 * change inside a call, so every round of a loop reads the same grid.  A pixel whose cell starts in an absent brick has no row without a
 * voxel load; a cell inside the window is gathered as the window term gathers it; a cell across a brick face costs one grid lookup per
 * corner beyond it.
 * What it is NOT: rows are still not weighted by voxel weight; the grid is rebuilt and uploaded on every call (4 B per brick of the
 * box), not kept between calls; the occupancy pre-pass of the raycast is not run. */
/* rpe_sdf_rows / rpe_sdf_normal_eq / rpe_icp_sdf / rpe_icp_pyramid_sdf on the map inside the box; every other argument as theirs.
 * RPE_ERR_STATE without a frame, a volume or the levels asked, or for unaligned dims or total shift; RPE_ERR_ARG for what the window
 * forms refuse, lo without hi, a bad box, or more than 2^24 bricks */
int rpe_map_sdf_rows(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals,
                     const int64_t lo[3], const int64_t hi[3], float* rows);
int rpe_map_sdf_normal_eq(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals,
                          const int64_t lo[3], const int64_t hi[3], double* out32);
int rpe_icp_map_sdf(rpe_context* ctx, const rpe_icp_options* opt, const int64_t lo[3], const int64_t hi[3], double* pose12,
                    int* iters_out, double* last_step, double* final_cost, int64_t* matched);
int rpe_icp_pyramid_map_sdf(rpe_context* ctx, const rpe_icp_options* opt, int levels, const int* iters_per_level,
                            const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                            double* last_step, double* final_cost, int64_t* matched);

/* ---- Map volume colour term: a frame tracked with colour against the whole MAP -- the TSDF AND the colour of the window and the
 * archived bricks.  "Volume colour term" reads the window's two dense arrays, so a textured surface the map knows but the window no longer
 * covers gives no photometric row, and "Map volume term" is geometry only; these calls read both of the map.  No new arithmetic: the box
 * lo <= w < hi of world voxels (lo = hi = NULL: rpe_volume_map_bounds) defines the VIRTUAL VOLUME of "Map volume term" and, beside it,
 * the VIRTUAL COLOUR VOLUME that "Map raycast" and "Map mesh" sample: a voxel holds the window's colour bits where the window covers
 * it, the held brick's colour plane where the archive holds its world brick, {0, 0} elsewhere -- also for a brick archived before the
 * colour volume existed (held without a colour plane: the archive restores zeros for those) and while the pool has no colour plane at
 * all.  Zeros have no colour weight > 0: such a cell gives a geometric row and no photometric one.
 * THE CONTRACT: rpe_map_sdf_photo_rows returns, bit for bit, what rpe_sdf_photo_rows returns in a second context whose volume is a
 * fresh rpe_volume_init of the virtual volume with the map's TSDF and colour uploaded (rpe_volume_upload, rpe_volume_color_upload) and
 * the same frame: steps 1-5 of "Volume colour term" on the two virtual volumes (tests/mapsdf_photo_oracle.py states the composition in
 * numpy).  With the box equal to the window's extent the rows are rpe_sdf_photo_rows' of the same context.  The records are laid out as
 * the window calls', the row counts exact, every sum within 8 * 2^-24 of the sum of the magnitudes of its products (both rows widened
 * to fp64, fp64 fused multiply-adds, one pixel per thread and loop trip, in the combined round the geometric row before the photometric
 * one); the loops are rpe_icp_sdf_rgbd's and rpe_icp_pyramid_sdf_rgbd's, round for round, with that record.
 * Rules: the union of the two terms'.  A frame (with the levels asked), a frame colour, a volume and a colour volume, and every dim and
 * every component of the total shift a multiple of 8 (RPE_ERR_STATE); weight / photo_weight finite and > 0, the box rules of "Map
 * volume term" (multiples of 8, 8 <= hi - lo <= 2^20, lo and hi both given or both NULL, at most 2^24 bricks), host-driven only
 * (RPE_ERR_ARG).  The archive need not be on: the map is then the window.  The calls write nothing but the uploaded grid, their own
 * intensity pyramid and the reduction's scratch: the model, the model colour, the prepared photometric maps, the solver slots, the last
 * mesh, both volumes and the archive stay as they were.
 * How: the brick grid is built and uploaded ONCE per call and serves both fetches and every round.  The colour corners are fetched
 * behind the TSDF corners' gates (a pixel whose TSDF corners give no row needs no colour; the result is the same bits); a cell whose
 * corner-0 brick is absent costs no voxel load.
 * What it is NOT: as "Map volume term" -- rows not weighted by voxel weight, the grid rebuilt on every call, no device-side brick index,
 * no device-resident loop. */
/* rpe_sdf_photo_rows / rpe_sdf_photo_normal_eq / rpe_icp_sdf_rgbd / rpe_icp_pyramid_sdf_rgbd on the map inside the box; every other
 * argument as theirs */
int rpe_map_sdf_photo_rows(rpe_context* ctx, int level, const double* pose12, double dist_thr, const int64_t lo[3], const int64_t hi[3],
                           float* rows);
int rpe_map_sdf_photo_normal_eq(rpe_context* ctx, int level, const double* pose12, double dist_thr, double weight, const int64_t lo[3],
                                const int64_t hi[3], double* out32);
int rpe_icp_map_sdf_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, const int64_t lo[3], const int64_t hi[3],
                         double* pose12, int* iters_out, double* last_step, double* final_cost, int64_t* matched, double* photo_cost,
                         int64_t* photo_matched);
int rpe_icp_pyramid_map_sdf_rgbd(rpe_context* ctx, const rpe_icp_options* opt, double photo_weight, int levels, const int* iters_per_level,
                                 const double* dist_thr_per_level, const int64_t lo[3], const int64_t hi[3], double* pose12, int* iters_out,
                                 double* last_step, double* final_cost, int64_t* matched, double* photo_cost, int64_t* photo_matched);

/* ---- Robust volume terms: an optional IRLS weight on the rows of the four volume terms ("Volume term", "Volume colour term", "Map volume
 * term", "Map volume colour term").  Their gates are the only defence against depth the map does not explain -- a person, a moved chair,
 * a door that has opened: a row 8 cm off passes a 10 cm gate at full weight and pulls the pose.  OFF by default; set once per context
 * and then used by the four normal-equation calls and the eight loops.  The four rows calls are not affected: they return the
 * unweighted r and J.
 * The rule (csrc/rpe_sdf_robust_rule.hpp; tests/sdf_robust_oracle.py states it in numpy), followed bit for bit: fp32, the written
 * order, no FMA contraction.  The weight w of a row with residual r and scale k -- r in metres for the geometric row, in UNSCALED
 * intensity levels (before the photometric weight lam) for the photometric row:
 *   RPE_ROBUST_HUBER:  s = fabsf(r);  w = s <= k ? 1.0f : k / s
 *   RPE_ROBUST_TUKEY:  u = r / k;  q = 1.0f - u * u;  w = fabsf(r) < k ? q * q : 0.0f
 * A weighted row contributes w J J^T to H, w J r to g and w r^2 to the cost entry of its term; a pixel without a row has no weight (0 in
 * the sums, NaN in the hook below).  The row count still counts EVERY row that passed the gates, weight 0 included.  In the colour
 * calls the geometric row is weighted with k; the photometric row with photo_k on its unscaled residual and then scaled by lam as
 * before; photo_k = 0 leaves the photometric rows at weight 1.  The photometric-only record of rpe_sdf_photo_normal_eq /
 * rpe_map_sdf_photo_normal_eq is weighted with photo_k.  The records' layout is unchanged, every sum is within 8 * 2^-24 of the sum of
 * the magnitudes of its (weighted) products and the row counts are exact: the row and its weight are widened to fp64 (w J is exact
 * there) and added with fp64 fused multiply-adds, one pixel per thread and loop trip, on the window too.  A round whose weights are all
 * 0 ends as any round whose normal equations are not positive definite ends: RPE_ERR_DEGENERATE.
 * With kind RPE_ROBUST_NONE every call launches exactly the kernels it launched before there was a weight and returns the same bits.
 * What it is NOT.  No confidence weighting: rows are still not weighted by voxel weight (tried in the oracles: min(w, 4) / 4 moved a
 * tracked pose by less than 3 % either way).  No scale estimation: k is the caller's, in the units of r, and does not follow the
 * level or the round.  No Cauchy kernel.  The front-end ICP (rpe_icp, rpe_icp_rgbd and their pyramid forms) and the keyframe graph stay
 * unweighted. */
/* kind: RPE_ROBUST_NONE (off; k and photo_k are not read and read back as 0), RPE_ROBUST_HUBER or RPE_ROBUST_TUKEY; with a kind other
 * than NONE k finite and >= 1e-6, photo_k 0 or finite and >= 1e-6.  RPE_ROBUST_CAUCHY, any other kind and any other scale are
 * RPE_ERR_ARG and leave the setting as it was.  The setting is the context's: it survives new frames, volumes and shifts */
int rpe_sdf_set_robust(rpe_context* ctx, int kind, double k, double photo_k);
int rpe_sdf_robust(rpe_context* ctx, int* kind, double* k, double* photo_k);
/* The tests' hook and a way to look at what the weight does: the plane of weights of the level, w_l*h_l floats, under the context's
 * setting -- of the geometric rows (photo = 0: scale k, gates as rpe_sdf_rows') or of the photometric rows (photo = 1: scale photo_k,
 * gate as rpe_sdf_photo_rows'; cos_thr and use_normals are not read; needs what the colour calls need).  NaN where the pixel has no
 * row; 1 for every row with kind NONE or with photo = 1 and photo_k = 0.  The map form reads the map inside the box, as
 * rpe_map_sdf_rows / rpe_map_sdf_photo_rows do.  Arguments, states and their codes are those of the rows calls */
int rpe_sdf_robust_weights(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals, int photo,
                           float* weights);
int rpe_map_sdf_robust_weights(rpe_context* ctx, int level, const double* pose12, double dist_thr, double cos_thr, int use_normals,
                               int photo, const int64_t lo[3], const int64_t hi[3], float* weights);

/* ---- Map fuse: the whole MAP rebuilt from the keyframes -- the window and the archived bricks.  rpe_volume_fuse_keyframes writes the
 * dense window only: after a loop closure the archived bricks, most of a walked map, would keep the surface fused at the drifted poses.
 * This call fuses a list of keyframes into every brick of a box of world voxels, in the window or not, takes archive slots for the
 * bricks that become non-empty and releases the slots of bricks that become empty.  No new arithmetic: the box lo <= w < hi defines the
 * VIRTUAL VOLUME that "Map mesh" defines (lo = hi = NULL: rpe_volume_map_bounds): dim = hi - lo, o = (float)(origin_init + (double)lo *
 * voxel_size), one rounding; voxel size, trunc and max weight are the init call's; its content is the map's (the window's bits where
 * the window covers, the held brick's where the archive holds one, zeros elsewhere; colour likewise).
 * THE CONTRACT: after the call the map holds inside the box, bit for bit, what rpe_volume_fuse_keyframes(ids, count, poses12, flags)
 * leaves in a second context whose volume is a fresh rpe_volume_init of that virtual volume with the map's content uploaded: voxel
 * centre o + ((float)i + 0.5f) * s with i the index inside the box, projection, update, colour blend and list order are those of
 * "Keyframe depth and rebuilding the volume" (tests/mapfuse_oracle.py states the composition in numpy).  A brick of the box that the
 * window covers holds its part of the result in the window.  A brick of the box outside the window is held by the archive afterwards
 * if and only if any 32-bit word of its tsdf or colour brick is non-zero -- the archive's own rule for a leaving brick.  Nothing outside
 * the box changes: window voxels outside it keep their bits, held bricks outside it keep their slots.  With the box equal to the
 * window's extent o is the window's own o and the window holds what rpe_volume_fuse_keyframes would leave in it.
 * Flags are rpe_volume_fuse_keyframes' (RPE_FUSE_CLEAR | RPE_FUSE_COLOR | RPE_FUSE_NO_CULL).  RPE_FUSE_CLEAR: the box starts from zeros
 * in both volumes; where a colour volume or a colour plane of the pool exists it is zeroed inside the box even without RPE_FUSE_COLOR;
 * a held brick of the box that ends all zero is released (its slot returns to the free list, no device work); whether a colour volume
 * exists does not change.  Without it window and held bricks are loaded, updated and stored, and an absent brick starts from zeros.
 * RPE_FUSE_COLOR creates the colour volume, zero-filled, if there is none, and the pool's colour plane, zeroed, when a brick of the
 * pool is written and there is none.  The last mesh is treated as rpe_volume_fuse_keyframes treats it (dropped with RPE_FUSE_CLEAR);
 * the model, the solver slots and the photometric maps stay.
 * Refusals, all before anything is written: the list's are rpe_volume_fuse_keyframes', code for code; the box rules are the map
 * mesh's, and the box may hold at most 2^24 bricks (RPE_ERR_ARG); unaligned dims or total shift are RPE_ERR_STATE, as
 * rpe_volume_map_bounds; a box that reaches outside the window while the archive is off is RPE_ERR_STATE; and CAPACITY: if the absent
 * bricks that become non-zero need more slots than are free (counting those RPE_FUSE_CLEAR releases) the call returns RPE_ERR_STATE
 * with both numbers in the message and window, pool, index and free list are exactly as before.
 * How: two passes of one kernel, a workgroup per brick.  Pass 1 runs the fuse from zeros on every brick of the box without touching a
 * voxel and leaves one flag word per brick (non-zero after the fuse; some voxel updated); the host waits ONCE, for the flags, checks
 * the capacity, hands slots out and lists the bricks to write; pass 2 loads, fuses and stores the listed bricks only.  The projection
 * is computed twice: the price of refusing before writing without a staging pool of the box's size.
 * stats (may be NULL) = {bricks in the box, bricks written, slots newly taken, slots released}.
 * Out of scope: the default box is the current map's bounds -- surfaces the corrected poses see beyond it are fused only if the caller
 * widens the box; only keyframes are fused, not the frames between them; the index stays on the host; no per-frame integrate into
 * archived bricks. */
int rpe_volume_map_fuse_keyframes(rpe_context* ctx, const int32_t* ids, int count, const double* poses12, int flags,
                                  const int64_t lo[3], const int64_t hi[3], int64_t stats[4]);

/* ---- host-side pieces of the solvers (no GPU needed): sampling, minimal solvers, small algebra.  They exist so that
 * hosts in other languages do not have to re-implement them, and so that the host logic can be tested on a CPU box.
 * 3 x K inputs are column-major doubles whose values are rounded to dtype before use. */
void rpe_host_random_elements(int n, int m, uint64_t seed, int draws, int* out);                 /* Utility.hpp:124-156 */
void rpe_host_prosac_samples(int dtype, int m, int n, uint64_t seed, int draws, int* out);       /* Utility.hpp:161-250 */
int rpe_host_update_num_iters(int dtype, double p, double ep, int model_points, int max_iters);  /* P3P.hpp:296-318    */
void rpe_host_sort_indexes(const double* w, int n, int* out);                                     /* Utility.hpp:107-118 */
int rpe_host_kneip_main(int dtype, const double* xw4, const double* bv4, double* sols12);         /* P3P.hpp:63-232     */
int rpe_host_kneip(int dtype, const double* xw4, const double* bv4, double* R9, double* t3);      /* P3P.hpp:250-294    */
void rpe_host_nl_2p(int dtype, const double* v18, double* R9,
    double* t3);                        /* AbsoluteOrientationNormal.hpp:77-142 */
void rpe_host_shinji(int dtype, const double* xw, const double* xc, int K, double* R9, double* t3); /* AbsoluteOrientation.hpp:47-99 */
void rpe_host_se3_exp(const double* a6, double* R9, double* t3);                                  /* sophus/se3.hpp:321-342 */
void rpe_host_svd3(const double* A9, double* U9, double* s3, double* V9);
void rpe_host_calc_err(const double* Rgt9, const double* tgt3, const double* Rse9, const double* tse3, double* err2, double* pct2);
/* the joint system of a keyframe graph: K poses, `edges` records of RPE_GRAPH_RECORD doubles, ji = (j, i) per edge (2 x edges int32),
 * fixed_mask (K bytes, may be NULL) != 0 for the keyframes that stay.  Assembles the 6K x 6K system, removes the fixed keyframes and
 * solves H delta = -g by a dense Cholesky factorisation; delta = 6 x K doubles, 0 for a fixed keyframe and for one on no edge.
 * RPE_ERR_DEGENERATE when the matrix is not positive definite (a pivot at or below 1e-12 of its diagonal entry) */
int rpe_graph_solve(int K, int edges, const int32_t* ji, const double* records, const uint8_t* fixed_mask, double* delta);

#ifdef __cplusplus
}
#endif
#endif /* RGBD_POSE_HIP_H */
