#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path (BASELINE.json metric: correspondence-residuals/s + pose error vs the CPU path).

A "step" is ONE Gauss-Newton iteration of the point-to-point absolute-orientation refinement over one batch of synthetic
correspondences resident in HBM: normal-equation kernel (K1: residuals + 6-DoF Jacobians + two-stage reduction to the 27
scalars), [all-reduce of the 32-double record over RCCL when --gpus > 1], record to the host, 6x6 solve and SE(3) exp-map
update ON THE HOST (north star), next pose back to the GPU.

  N = 1   workload = BASELINE.json configs[1]: 640x480 dense depth = 307 200 3D-3D correspondences, fp32, refinement over
          the RANSAC inlier mask.  The host loop is rpe_gn_refine (C++, inside the library); on one GPU its kernel is RESIDENT:
          ONE launch serves all steps of a refinement, every new pose reaches the waiting grid through device memory.
  N > 1   workload = configs[4]: 10 000 000 correspondences sharded N ways (contiguous ranges), one all-reduce(sum) of the
          32-double record per iteration over RCCL (library-owned communicator); strong scaling.  `python bench.py --gpus N`
          starts its own N rank processes (no GPU is touched by the parent); under torch.distributed.run it is one rank.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what the headline needs and nothing else: set up, pre-warm, pick the host CPU, W warm-up steps, SETTLE_REGIONS
untimed regions, ONE timed region of exactly K steps (barrier + synchronize, K steps, synchronize + barrier, MAX over ranks), the
outputs, the JSON line.
--full adds everything reported beside the headline: --repeats timed regions (default 50; ms_per_step is then the MEDIAN
repetition, p10 / p90 beside it) with HIP events on some of them (roofline), the untuned figure, the pose against the CPU oracle,
the CPU baseline, the bandwidth-bound and reference-API kernels, fp64, the other legs and, for N > 1, the collectives timed beside
the headline's.  --dump-outputs DIR writes the last timed step's result (the pose a caller of rpe_gn_refine receives, with the
step norm and cost where the path returns them) as DIR/<name>.npy; the inputs are seeded, the same on every run.
Rank 0 prints ONE JSON line.  Nothing here reads the reference project.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_FRAME = 307200             # 640 x 480 (configs[1])
N_SHARDED = 10_000_000       # configs[4]
BYTES_PER_CORR = 24 + 2      # Xw 12 + Xc 12 + short inlier mask 2 (p2p fp32 + mask)
HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
THRE_3D = 0.2                # Parameters.yml thre_3d
PROFILE_INDEX = "profiles/r06_bench_profiles.json"   # rocprofv3 / PMC summaries of THIS command, one entry per steps-per-launch
PREWARM_MAX_STEPS = 2000     # steps per launch of the pre-warm, of each host-CPU trial and of the settle regions (the default --steps)
SETTLE_REGIONS = 24          # untimed regions right before a plain run's one timed region


# ------------------------------------------------------------------------------------------------ launcher (no GPU, no torch)
def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rank_env(base: dict, rank: int, world: int, port: int) -> dict:
    env = dict(base)
    env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=base.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return env


def launch_children(argv: list[str], gpus: int) -> int:
    """`python bench.py --gpus N` from a bare shell: N fresh rank processes (one per GPU), started BEFORE anything in this process
    has touched HIP -- this parent never does.  Rank 0's stdout is forwarded (its last line is the JSON line); any failing child
    fails the run."""
    port = free_port()
    procs = []
    for r in range(gpus):
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=rank_env(os.environ, r, gpus, port),
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=None, text=True))
    out0, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out0 or "")
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        print(f"bench.py: rank(s) failed: {bad}", file=sys.stderr)
        return 1
    return 0


def pin_to_gpu_numa_node(local_rank: int, world_size: int = 1):
    """The host thread that waits for every record and hands every pose over should sit next to the GPU's PCIe root.  Plain
    sched_setaffinity on this process, before any GPU call (no exec, no wrapper).  Best effort: returns what it did."""
    global ORIG_AFFINITY
    try:
        allowed = sorted(os.sched_getaffinity(0))
        ORIG_AFFINITY = set(allowed)
        cards = []
        base = "/sys/class/drm"
        for name in sorted(os.listdir(base)):
            if not name.startswith("renderD"):
                continue
            dev = os.path.join(base, name, "device")
            try:
                if open(os.path.join(dev, "vendor")).read().strip() != "0x1002":
                    continue
                cards.append(dev)
            except OSError:
                continue
        if not cards:
            return {"pinned": False, "reason": "no amdgpu render node in sysfs"}
        dev = cards[min(local_rank, len(cards) - 1)]
        cpus = []
        for part in open(os.path.join(dev, "local_cpulist")).read().strip().split(","):
            if not part:
                continue
            lo, _, hi = part.partition("-")
            cpus += list(range(int(lo), int(hi or lo) + 1))
        cand = [c for c in cpus if c in allowed] or allowed
        # away from CPU 0 (interrupts).  One GPU: one CPU for the polling thread.  Several ranks: four CPUs each, disjoint between the
        # ranks -- threads created later (RCCL's, torch's) inherit the mask and must not share a single core with a thread that spins
        # (the first cores of a socket take the interrupts and poll 3-4 % slower: start at the 17th, scripts/core_sweep.py)
        skip = 16 if len(cand) >= 64 else 1
        if world_size > 1:
            first = (skip + 4 * local_rank) % len(cand)
            mine = {cand[(first + k) % len(cand)] for k in range(4)}
        else:
            mine = {cand[skip % len(cand)]}
        os.sched_setaffinity(0, mine)
        return {"pinned": True, "cpu": sorted(mine)[0] if len(mine) == 1 else sorted(mine), "numa_node": open(os.path.join(dev, "numa_node")).read().strip(),
                "gpu_local_cpus": len(cpus), "gpu_local_cpu_ids": cpus}
    except Exception as e:  # noqa: BLE001
        return {"pinned": False, "reason": repr(e)}


# ------------------------------------------------------------------------------------------------ workload
def make_shard(rank: int, n: int):
    """Same ground-truth pose on every rank, different points per rank (Simulator.hpp model, Parameters.yml values)."""
    import numpy as np
    from rgbd_pose_estimation_amd import simulator as S
    R, t = S.random_pose(np.random.default_rng(20260101))
    rng = np.random.default_rng(1000 + rank)
    return S.simulate_3d_3d_correspondences(rng, R, t, n, 0.05, 0.1).astype(np.float32)


def initial_pose(sc):
    """Start 0.02 rad / 5 cm away from the truth (what a RANSAC winner looks like)."""
    import numpy as np
    w = np.array([0.012, -0.010, 0.0125]); th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K
    return dR @ sc.R, sc.t + np.array([0.03, -0.03, 0.03])


def rot_err(Ra, Rb):
    import numpy as np
    D = Ra @ Rb.T
    s = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2
    return math.atan2(s, (np.trace(D) - 1) / 2)


def dump_outputs(out_dir: str, pose, last: dict):
    """--dump-outputs: what the timed path returned after its last step, as float64 .npy files -- pose.npy (12: R row-major, then t,
    as rpe_gn_refine writes it back), step_norm.npy (|delta| of the last step) and, where the path returns it, cost.npy (the last
    step's cost).  The inputs are seeded (make_shard, initial_pose), so two builds run with the same arguments can be compared."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"pose": np.asarray(pose, np.float64).reshape(12)}
    arrays.update({k: np.array([v], np.float64) for k, v in last.items() if v is not None})
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


ORIG_AFFINITY = None


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sc, seconds: float):
    """Oracle (CPU restatement of the reference; the reference itself needs Eigen + OpenCV and cannot be built here) timed on this
    host, SURVEY.md 8(d): shinji_ls2<float> through AOOnlyPoseAdapter's virtual getters -- exactly what Library.cpp ao() runs -- and
    the shinji_ransac2 vote loop; 1 thread because the reference is single-threaded, and an all-core variant of the SAME restatement
    beside it; every figure is the MEDIAN of >= 20 timed runs after a warm-up run.  Bounded: about `seconds` of CPU work in all."""
    import numpy as np
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ctypes as C
        import oracle_lib as O
        lib = O.lib()
        for fn in ("orc_time_ao", "orc_time_ao_threads", "orc_time_gn_p2p", "orc_time_gn_p2p_threads", "orc_time_votes33", "orc_time_votes33_threads"):
            getattr(lib, fn).restype = C.c_double
        xw, xc = np.ascontiguousarray(sc.Q, np.float32), np.ascontiguousarray(sc.P, np.float32)
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        n = len(xw)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def median_runs(f, budget_s, min_runs=20, max_runs=400):
            f()   # warm-up
            ts, spent = [], 0.0
            while len(ts) < min_runs or (spent < budget_s and len(ts) < max_runs):
                dt = f(); ts.append(dt); spent += dt
            return percentile(ts, 0.5), len(ts), spent

        # the bench's host thread is pinned to one CPU; the worker threads of the all-core legs get the process's original CPU set back
        pinned = os.sched_getaffinity(0)
        wide = ORIG_AFFINITY or pinned
        try:   # a job given fewer CPUs than it can see says so in OMP_NUM_THREADS
            granted = int(os.environ.get("OMP_NUM_THREADS", "").split(",")[0])
        except ValueError:
            granted = 64
        threads = max(1, min(64, len(wide), granted))

        def all_cores(f):
            os.sched_setaffinity(0, wide)
            try:
                return f()
            finally:
                os.sched_setaffinity(0, pinned)

        share = seconds / 4.0
        ao1, ao1_runs, ao1_spent = median_runs(lambda: lib.orc_time_ao(p(xw), p(xc), n, 1, p(R), p(t)), share * 1.6)
        # all-core figure of the SAME restatement: 10 repetitions per call on ONE pool of threads (the spawn / join of the pool and the
        # first touch of the four 3 x n work matrices are amortised over them -- with one repetition per call they were most of a 2 ms
        # call), swept over thread counts: on a two-socket host the best count is rarely "all of them"; the best is reported with its count
        AO_REPS = 10
        sweep = sorted({k for k in (4, 8, 16, 32, 64, 128, threads) if 1 < k <= threads} or {threads})
        ao_sweep = {}
        for k in sweep:
            med, runs_k, _ = all_cores(lambda k=k: median_runs(lambda: lib.orc_time_ao_threads(p(xw), p(xc), n, AO_REPS, k, p(R), p(t)) / AO_REPS,
                                                                share * 0.4 / len(sweep), min_runs=5, max_runs=100))
            ao_sweep[k] = (med, runs_k)
        ao_threads = min(ao_sweep, key=lambda k: ao_sweep[k][0])
        aoN, aoN_runs = ao_sweep[ao_threads]
        pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
        out = np.zeros(29)
        g1, g1_runs, _ = median_runs(lambda: lib.orc_time_gn_p2p(p(xw), p(xc), C.c_long(n), 1, p(pose), p(out)), share * 0.6)
        gN, gN_runs, _ = all_cores(lambda: median_runs(lambda: lib.orc_time_gn_p2p_threads(p(xw), p(xc), C.c_long(n), 10, p(pose), p(out), threads) / 10, share * 0.2))
        # vote loop (V2, 3D-3D): one hypothesis per run, at the scene's true pose
        from rgbd_pose_estimation_amd.api import pose7_from_Rt
        q7 = np.ascontiguousarray(pose7_from_Rt(sc.R, sc.t, 0), np.float64).reshape(1, 7)
        v = np.zeros(1, np.int32)
        v1, v1_runs, _ = median_runs(lambda: lib.orc_time_votes33(p(xw), p(xc), n, p(q7), 1, C.c_float(THRE_3D), p(v)), share * 0.6)
        votes_1 = int(v[0])
        q8 = np.ascontiguousarray(np.tile(q7, (8, 1)))
        v8 = np.zeros(8, np.int32)
        vN, vN_runs, _ = all_cores(lambda: median_runs(lambda: lib.orc_time_votes33_threads(p(xw), p(xc), n, p(q8), 8, C.c_float(THRE_3D), p(v8), threads) / 8, share * 0.2))
        # the reference's own default build has no optimisation flag at all (CMakeLists.txt:13-15): the same port compiled that way
        o0 = None
        try:
            o0_path = os.path.join(ROOT, "oracle", "liboracle_O0.so")
            if os.path.exists(o0_path):
                lib0 = C.CDLL(o0_path)
                lib0.orc_time_ao.restype = C.c_double
                o0m, _, _ = median_runs(lambda: lib0.orc_time_ao(p(xw), p(xc), n, 1, p(R), p(t)), min(1.5, share * 0.4), min_runs=5)
                o0 = n / o0m
        except Exception:
            o0 = None
        return {"value": n / ao1, "unit": "correspondence-residuals/s", "cores": 1, "kind": "port", "statistic": "median of the timed runs (one warm-up run before)",
                "runs": ao1_runs, "no_O_flag_value": o0,
                "sample_short": f"{ao1_runs} calls of oracle shinji_ls2<float> (=Library.cpp ao(), alloc+copy-in timed as :20-26) on the same {n}-corr scene, g++ -O2, 1 thread, {ao1_spent:.1f} s; median",
                "sample": f"{ao1_runs} calls of the oracle's shinji_ls2<float> (AOOnlyPoseAdapter virtual getters, gather + centroid + covariance "
                          f"passes + 3x3 SVD = Library.cpp ao()) on the same {n}-correspondence scene, g++ -O2, 1 thread, {ao1_spent:.1f} s",
                "all_cores": {"value": n / aoN, "threads": ao_threads, "runs": aoN_runs, "reps_per_call": AO_REPS,
                              "sweep": {str(k): n / v[0] for k, v in sorted(ao_sweep.items())},
                              "what": "the same shinji_ls2<float> restatement, its O(N) loops over contiguous index ranges on one pool of std::threads "
                                      "per call of %d repetitions (spin barriers between the phases); best of the swept thread counts; the 3 x n work "
                                      "matrices are allocated once per call outside the timed region, the copy-in of Library.cpp:20-22 is inside every "
                                      "repetition; the 1-thread figure allocates inside every call exactly as Library.cpp:20-26 does" % AO_REPS},
                "vote_loop": {"value": n / v1, "unit": "corr*hyp/s", "cores": 1, "runs": v1_runs, "votes": votes_1,
                              "what": "shinji_ransac2 vote loop (AbsoluteOrientation.hpp:190-200), one hypothesis per run",
                              "all_cores": {"value": n / vN, "threads": threads, "runs": vN_runs, "votes_equal": bool(np.all(v8 == votes_1))}},
                "gn_pass_fp64_value": n / g1, "gn_pass_fp64_runs": g1_runs,
                "gn_pass_fp64_all_cores": {"value": n / gN, "threads": threads, "runs": gN_runs},
                "host_cpus": os.cpu_count(), "cpu_model": cpu_model()}
    except Exception as e:  # the baseline is a reported number, never a dependency of the GPU path
        return {"value": None, "unit": "correspondence-residuals/s", "cores": 1, "kind": "port", "sample": f"unavailable: {e!r}", "cpu_model": cpu_model()}


def record_close(rec, ref, tol):
    """Two packed normal-equation records (H upper triangle 21 | g 6 | cost | weight) agree entry by entry, each entry judged on its OWN
    natural scale: H_ij against sqrt(H_ii H_jj), g_i against sqrt(H_ii cost) (Cauchy-Schwarz bounds of the sums they are), cost and
    weight against themselves -- so a wrong gradient cannot hide behind the largest entry of H."""
    import numpy as np
    idx, k = {}, 0
    for i in range(6):
        for j in range(i, 6):
            idx[(i, j)] = k; k += 1
    diag = np.array([abs(ref[idx[(i, i)]]) for i in range(6)])
    cost = abs(ref[27])
    for (i, j), k in idx.items():
        if abs(rec[k] - ref[k]) > tol * math.sqrt(diag[i] * diag[j]) + 1e-300:
            return False
    for i in range(6):
        if abs(rec[21 + i] - ref[21 + i]) > tol * math.sqrt(diag[i] * cost) + 1e-300:
            return False
    return abs(rec[27] - ref[27]) <= tol * cost + 1e-300 and abs(rec[28] - ref[28]) <= tol * abs(ref[28]) + 1e-300


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]


def collective_plan(world: int, want: str, share_gpu: bool, full: bool = True) -> dict:
    """What `bench.py --gpus N` does about the per-iteration all-reduce, decided BEFORE any GPU is touched (the dry-run launcher test
    prints it).  The north star's collective -- one RCCL all-reduce of the normal-equation scalars per Gauss-Newton iteration over xGMI,
    here on a communicator the library owns -- is the headline whenever RCCL can be set up; with --full (`full`), other ways of adding
    the 32-double records are timed beside it.  RPE_BENCH_COLLECTIVE = auto (default: RCCL headline, host-side exchange beside) | rccl |
    host | p2p (the in-kernel mailboxes as headline) | auto_p2p (RCCL headline, mailboxes beside)."""
    if want not in ("auto", "rccl", "host", "p2p", "auto_p2p"):
        sys.exit(f"bench.py: unknown RPE_BENCH_COLLECTIVE={want}")
    if world <= 1:
        return {"headline": "none", "timed_beside": [], "rccl_init": False, "rccl_ranks_expected": 0, "distinct_gpu_check": False,
                "scaling": "weak", "weak_scaling_extra": False}
    headline = {"auto": "rccl", "rccl": "rccl", "host": "host", "p2p": "p2p", "auto_p2p": "rccl"}[want]
    beside = {"auto": ["host"], "rccl": [], "host": [], "p2p": [], "auto_p2p": ["p2p"]}[want] if full else []
    rccl_init = want != "host" and not (want == "p2p" and os.environ.get("RPE_BENCH_STRICT_COLLECTIVE") == "1")
    return {"headline": headline, "timed_beside": beside, "rccl_init": rccl_init, "rccl_ranks_expected": world if rccl_init else 0,
            "fallback": "host-side exchange, then torch.distributed, if RCCL cannot be set up", "distinct_gpu_check": not share_gpu,
            "scaling": "strong", "weak_scaling_extra": True,
            "json_fields": ["config.collective", "config.rccl_ranks", "config.rccl_verified", "config.collective_step_us", "config.pci_bus_ids", "weak_scaling"]}


def profile_entries():
    """profiles/r05_bench_profiles.json: what rocprofv3 --kernel-trace --stats and the two --pmc passes recorded for bench.py's own
    command, keyed by the steps one launch of the resident kernel served.  File-derived numbers enter the JSON line only next to the
    steps_per_launch they were recorded with."""
    try:
        return json.load(open(os.path.join(ROOT, PROFILE_INDEX)))
    except Exception:
        return {}


KERNEL_SOURCES = ("rpe_normal_eq.hip", "rpe_reduce.hpp", "rpe_residuals.hpp", "rpe_kernels.h")


def kernel_source_hash():
    """sha256 over the sources the dominant kernel (normal_eq_resident_kernel / normal_eq_kernel) is compiled from.  The profile index
    records the hash its rocprofv3 / PMC runs were taken on; a file-derived `traffic` enters the line only while the hashes agree."""
    import hashlib
    h = hashlib.sha256()
    try:
        for name in KERNEL_SOURCES:
            with open(os.path.join(ROOT, "rgbd_pose_estimation_amd", "csrc", name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    except OSError:
        return None
    return h.hexdigest()[:16]


def library_hash():
    import hashlib
    try:
        with open(os.path.join(ROOT, "rgbd_pose_estimation_amd", "lib", "librgbdpose_hip.so"), "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return None


def cheap_scene(n, seed=4):
    """n correspondences with normals for bandwidth runs: a 250 000-point simulated scene tiled (the bytes streamed are what matters)."""
    import numpy as np
    from rgbd_pose_estimation_amd import simulator as S
    rng = np.random.default_rng(seed)
    R, t = S.random_pose(rng)
    base = S.simulate_3d_3d_correspondences(rng, R, t, min(n, 250000), 0.02, 0.0).astype(np.float32)
    nrm = rng.standard_normal((len(base.Q), 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    reps = (n + len(base.Q) - 1) // len(base.Q)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:n])
    return R, t, tile(base.Q), tile(base.P), tile(nrm)


def hbm_roofline(local_rank):
    """LIVE bandwidth-bound figures, event-timed in this run (SURVEY 8d 'Config 4', 'Roofline'): configs[3] -- 1 M correspondences with
    normals, point-to-plane, 36 B each -- steady (the 36 MB set stays in the 256 MiB Infinity Cache between launches) and cold (a
    480 MB stream evicts it before every launch), and the point-to-point kernel on 10 M and 20 M correspondences (240 / 480 MB: at and
    past the Infinity Cache).  One launch per call (normal_eq_kernel), HIP events = the dispatch's begin / end timestamps."""
    from rgbd_pose_estimation_amd import _lib as L, api
    out = {"peak_GBs": HBM_PEAK_GBS, "timing": "HIP events on the kernel's stream (hipExtLaunchKernelGGL begin / end), mean over the launches"}
    R, t, Q20, P20, _ = cheap_scene(20_000_000)
    pose = api.pose12(R, t)
    big = api.Context(local_rank).load(L.F32, xw=Q20, xc=P20)
    ten = api.Context(local_rank).load(L.F32, xw=Q20[:10_000_000], xc=P20[:10_000_000])
    del Q20, P20

    def timed(ctx, kind, launches, before=None):
        for _ in range(5):
            ctx.normal_eq(kind, pose)
        ctx.timing_enable(launches, 1)
        for _ in range(launches):
            if before:
                before()
            ctx.normal_eq(kind, pose)
        cnt, tot_ms, mn_ms = ctx.timing_collect()
        ctx.timing_enable(0, 1)
        return tot_ms / max(cnt, 1) * 1e-3, mn_ms * 1e-3, cnt

    def row(n, bpc, avg, mn, cnt, **kw):
        return dict(n=n, bytes_per_corr=bpc, working_set_MB=bpc * n / 1e6, launches=cnt, avg_launch_us=avg * 1e6, min_launch_us=mn * 1e6,
                    achieved_GBs=bpc * n / avg / 1e9, frac_of_peak=bpc * n / avg / 1e9 / HBM_PEAK_GBS, **kw)

    _, _, Q1, P1, N1 = cheap_scene(1_000_000)
    c3 = api.Context(local_rank).load(L.F32, xw=Q1, xc=P1, nc=N1)
    avg, mn, cnt = timed(c3, L.RES_P2PLANE, 60)
    out["config3_p2plane_1M_steady"] = row(1_000_000, 36, avg, mn, cnt, kernel="rpe::normal_eq_kernel<float, 1, 256, false, false>")
    avg, mn, cnt = timed(c3, L.RES_P2PLANE, 40, before=lambda: big.p2p_moments())
    out["config3_p2plane_1M_cold"] = row(1_000_000, 36, avg, mn, cnt, evicted_by="a 480 MB moments pass of another context before every launch")
    c3.close()
    avg, mn, cnt = timed(big, L.RES_P2P, 30)
    out["p2p_20M"] = row(20_000_000, 24, avg, mn, cnt, note="480 MB > 256 MiB Infinity Cache: HBM streaming")
    avg, mn, cnt = timed(ten, L.RES_P2P, 30)
    out["p2p_10M"] = row(10_000_000, 24, avg, mn, cnt, note="240 MB <= Infinity Cache: the steady state is served on-die, above the HBM read ceiling")
    big.close(); ten.close()
    # PMC traffic of exactly these launches (same kernels, same sizes, one launch per call), from the committed profile
    prof = profile_entries().get("hbm_stream", {})
    for case, e in prof.items():
        if case in out and isinstance(out[case], dict):
            out[case]["traffic"] = e.get("traffic_bytes_per_launch")
            out[case]["traffic_over_algorithmic"] = e.get("traffic_over_algorithmic")
            out[case]["traffic_source"] = PROFILE_INDEX + " hbm_stream (2 x FETCH_SIZE + WRITE_SIZE, separate --pmc passes over scripts/hbm_stream_probe.py)"
    return out


def reference_api_roofline(local_rank, sizes=(307200, 1_000_000, 10_000_000), launches=30):
    """LIVE event-timed launches of the kernels behind the REFERENCE'S OWN least-squares API (round-3 review, item 2): K1' moments_kernel
    (shinji / shinji_ls* / ao(): pose/AbsoluteOrientation.hpp:56-73; 24 B per correspondence), K5 nl_round_kernel (nl_shinji_kneip_ls +
    find_opt_cc: pose/AbsoluteOrientationNormal.hpp:457-505; five arrays + three short masks = 66 B) and K4b mask_kernel of the 3D-3D
    vote (the winner's mask; two arrays + one short written = 26 B), at 307 200 / 1 M / 10 M correspondences, steady (the set left in
    the Infinity Cache by the previous launch) and cold (a 480 MB pass of another context before every launch; skipped where the set
    exceeds the cache anyway).  HIP events = the dispatch's own begin / end timestamps (rpe_timing_enable)."""
    import numpy as np
    from rgbd_pose_estimation_amd import _lib as L, api
    out = {"peak_GBs": HBM_PEAK_GBS, "timing": "HIP events on the kernel's stream (hipExtLaunchKernelGGL begin / end), mean over the launches",
           "bytes_per_corr": {"K1p_moments": 24, "K5_nl_round": 66, "K4b_mask_33": 26}}
    Re, te, Qe, Pe, _ = cheap_scene(20_000_000, seed=9)
    evictor = api.Context(local_rank).load(L.F32, xw=Qe, xc=Pe)
    del Qe, Pe
    rng = np.random.default_rng(11)
    for n in sizes:
        R, t, Q, P, Nc = cheap_scene(n)
        bv = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32)
        Nw = np.ascontiguousarray((Nc.astype(np.float64) @ R).astype(np.float32))
        ctx = api.Context(local_rank).load(L.F32, xw=Q, xc=P, bv=bv, nw=Nw, nc=Nc)
        for m in range(3):
            ctx.upload_mask(m, (rng.random(n) < 0.8).astype(np.int16))
        q7 = api.pose7_from_Rt(R, t, L.F32)
        Rwc, c_opt = R.T, -(R.T @ t)
        Cw, Cc = Q[:1000].mean(0), P[:1000].mean(0)
        cases = (("K1p_moments", 24, "rpe::moments_kernel<float, 256, true, false>", lambda: ctx.p2p_moments(L.USE_MASK), 26),
                 ("K5_nl_round", 66, "rpe::nl_round_full_kernel<float, 256, false>", lambda: ctx.nl_round(c_opt, Cw, Cc, Rwc), 66),
                 ("K4b_mask_33", 26, "rpe::mask_kernel<float, 0, true>", lambda: ctx.inlier_mask(L.VOTE_33, q7, thre_3d=THRE_3D), 26))
        for name, _, kernel, fn, bpc in cases:
            for state in ("steady", "cold"):
                if state == "cold" and bpc * n > 400e6:
                    continue
                for _ in range(5):
                    fn()
                k = launches if state == "steady" else max(10, launches // 2)
                ctx.timing_enable(k, 1)
                for _ in range(k):
                    if state == "cold":
                        evictor.p2p_moments()
                    fn()
                cnt, tot_ms, mn_ms = ctx.timing_collect()
                ctx.timing_enable(0, 1)
                avg = tot_ms / max(cnt, 1) * 1e-3
                out["%s_%d_%s" % (name, n, state)] = dict(kernel=kernel, n=n, bytes_per_corr=bpc, working_set_MB=bpc * n / 1e6, launches=cnt, avg_launch_us=avg * 1e6,
                                                          min_launch_us=mn_ms * 1e3, achieved_GBs=bpc * n / avg / 1e9, frac_of_peak=bpc * n / avg / 1e9 / HBM_PEAK_GBS)
        ctx.close()
    evictor.close()
    prof = profile_entries().get("reference_api_kernels", {})
    for key, e in out.items():
        if isinstance(e, dict) and "kernel" in e and key.endswith("_steady"):
            pe = prof.get(key[: -len("_steady")])
            if pe:
                e["traffic"] = pe.get("traffic_bytes_per_launch")
                e["traffic_over_algorithmic"] = pe.get("traffic_over_algorithmic")
                e["rocprofv3_avg_launch_us"] = pe.get("rocprofv3_avg_launch_us")
                e["traffic_source"] = PROFILE_INDEX + " reference_api_kernels (separate --pmc passes over scripts/reference_api_probe.py)"
    out["note"] = ("K1' is timed with the 3D-3D inlier mask (shinji_ls / shinji_ls1: 24 B + 2 B); K4b re-writes the mask it reads next, so its masks are "
                   "restored by nothing -- the masked kernels run before it at every size")
    return out


def fp64_lines(local_rank):
    """Tp = double (what TestMain.cpp:52-326 instantiates): event-timed K1 / K2 launches (48 / 72 B per correspondence) and the exact
    3D-3D scoring rate at 307 200 and 1 M correspondences."""
    import numpy as np
    from rgbd_pose_estimation_amd import _lib as L, api
    out = {}
    for n in (307200, 1_000_000):
        R, t, Q, P, Nn = cheap_scene(n, seed=5)
        ctx = api.Context(local_rank).load(L.F64, xw=Q.astype(np.float64), xc=P.astype(np.float64), nc=Nn.astype(np.float64))
        pose = api.pose12(R, t)
        rows = {}
        for name, kind, bpc in (("K1_p2p", L.RES_P2P, 48), ("K2_p2plane", L.RES_P2PLANE, 72)):
            for _ in range(5):
                ctx.normal_eq(kind, pose)
            batch = []   # five batches of 20 event-timed launches, median batch average: one stalled launch (seen: 10 ms once) must not set the figure
            for _ in range(5):
                ctx.timing_enable(20, 1)
                for _ in range(20):
                    ctx.normal_eq(kind, pose)
                cnt, tot_ms, mn_ms = ctx.timing_collect()
                batch.append(tot_ms / max(cnt, 1) * 1e-3)
            ctx.timing_enable(0, 1)
            avg = sorted(batch)[len(batch) // 2]
            rows[name] = {"bytes_per_corr": bpc, "avg_launch_us": avg * 1e6, "achieved_GBs": bpc * n / avg / 1e9, "frac_of_peak": bpc * n / avg / 1e9 / HBM_PEAK_GBS,
                          "corr_res_per_s": n / avg, "statistic": "median of five 20-launch averages"}
        H = 512
        q7 = api.pose7_from_Rt(R, t, L.F64)
        poses = np.tile(q7, (H, 1)); poses[:, 4:] += 0.01 * np.random.default_rng(1).standard_normal((H, 3))
        # warm by TIME: after the light launches above the GPU sits in a low power state and takes tens of milliseconds of load to leave it
        # (seen: the first 20 ms of passes 3.4x slower than the rest), then the median of nine single passes
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            ctx.score(L.VOTE_33, poses, THRE_3D, mode=L.SCORE_EXACT)
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            ctx.score(L.VOTE_33, poses, THRE_3D, mode=L.SCORE_EXACT)
            ts.append(time.perf_counter() - t0)
        dt = sorted(ts)[len(ts) // 2]
        rows["K4_score_33_exact"] = {"hypotheses": H, "us_per_pass": dt * 1e6, "corr_hyp_per_s": n * H / dt, "us_per_pass_min_max": [min(ts) * 1e6, max(ts) * 1e6],
                                     "statistic": "median of nine passes after 0.2 s of passes"}
        out[str(n)] = rows
        ctx.close()
    return out


# ------------------------------------------------------------------------------------------------ one rank
def worker(args, affinity):
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get("RPE_BENCH_DRY_RUN") == "1":
        # launcher test on a CPU box: the rank reports the environment it was started with and leaves BEFORE anything touches a GPU
        if rank == 0:
            print(json.dumps({"dry_run": True, "rank": rank, "local_rank": local_rank, "world": world, "gpus": args.gpus, "steps": args.steps,
                              "master": os.environ.get("MASTER_ADDR", "") + ":" + os.environ.get("MASTER_PORT", ""),
                              "collective_plan": collective_plan(world, os.environ.get("RPE_BENCH_COLLECTIVE", "auto"),
                                                                 os.environ.get("RPE_BENCH_SHARE_GPU") == "1", args.full)}), flush=True)
        sys.exit(int(os.environ.get("RPE_BENCH_DRY_EXIT", "0")) if rank == int(os.environ.get("RPE_BENCH_DRY_EXIT_RANK", "-1")) else 0)
    import ctypes as C
    import numpy as np
    force_dist = os.environ.get("RPE_BENCH_FORCE_DIST") == "1"   # exercise the collective path with one rank
    args.gpus = world

    # Load librgbdpose_hip.so (and let it register its gfx950 code objects) BEFORE torch initialises HIP: measured on
    # MI355X / ROCm 7.x, a library whose fat binary is registered after hipInit() pays 2-3x the launch latency per
    # kernel.  torch's bundled libamdhip64 is the one runtime of the process (_lib.py).
    from rgbd_pose_estimation_amd import _lib as L, api
    L.lib()
    n_dev = L.device_count()
    import torch
    import torch.distributed as dist
    from rgbd_pose_estimation_amd.distributed import HipShard, ShardedGaussNewton, init_host_exchange, init_native_comm, init_p2p, shard_range

    if n_dev < 1 or not torch.cuda.is_available():
        sys.exit("bench.py: no MI355X visible (the HIP path has no CPU fallback)")
    if local_rank >= n_dev and os.environ.get("RPE_BENCH_SHARE_GPU") == "1":
        local_rank = 0   # test rig: several ranks on the one GPU of the box
    torch.cuda.set_device(local_rank)
    backend = os.environ.get("RPE_BENCH_BACKEND", "nccl")
    cdev = f"cuda:{local_rank}" if backend == "nccl" else "cpu"   # where tensors handed to torch.distributed live
    dist_path = world > 1 or force_dist
    if dist_path:
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", RANK="0", WORLD_SIZE="1")
        # plumbing backend: "nccl" (= RCCL) in production; "gloo" lets the tests run two ranks on ONE GPU (RCCL refuses that)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    # ---- workload
    if world > 1:
        total_n = args.n_total if args.n_total > 0 else N_SHARDED
        lo, hi = shard_range(total_n, rank, world)
        n = hi - lo
        workload = (f"configs[4]: {total_n} 3D-3D correspondences sharded over {world} GPUs (contiguous ranges, {n} on rank 0), point-to-point "
                    "Gauss-Newton step over the RANSAC inlier mask, ONE all-reduce(sum) of the 32-double record per iteration")
        workload_short = f"configs[4]: {total_n} 3D-3D corr sharded over {world} GPUs, p2p GN step over inlier mask, one all-reduce of the 32-double record per iteration"
        scaling = "strong"
    else:
        n = args.n_per_gpu
        total_n = n
        workload = (f"configs[1]: 640x480 dense depth, {n} 3D-3D correspondences, point-to-point absolute orientation, Gauss-Newton "
                    "step (K1 normal equations + host 6x6 solve + SE3 exp-map update) over the RANSAC inlier mask")
        workload_short = f"configs[1]: 640x480 dense depth, {n} 3D-3D corr, point-to-point GN step (K1 normal eq + host 6x6 solve + SE3 exp) over inlier mask"
        scaling = "weak"
    sc = make_shard(rank, n)
    # the collective needs the kernel on the stream torch orders the all-reduce after; one GPU uses the library's own stream
    stream = torch.cuda.Stream(device=local_rank) if dist_path else None
    import contextlib
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        shard = HipShard(local_rank, stream)
        ctx = shard.ctx
        ctx.load(L.F32, xw=sc.Q, xc=sc.P)
        R0, t0 = initial_pose(sc)
        from rgbd_pose_estimation_amd.api import pose12, pose7_from_Rt
        # untimed prologue: one scoring pass at the initial pose writes the 3D-3D inlier mask (K4b), as RANSAC would
        q0 = pose7_from_Rt(R0, t0, L.F32)
        inl = int(ctx.inlier_mask(L.VOTE_33, q0, thre_3d=THRE_3D))
        shard.kind, shard.flags = L.RES_P2P, L.USE_MASK
        gn = ShardedGaussNewton(shard.normal_eq)
        pose = pose12(R0, t0)

        # ---- N > 1: how the shards' 32-double records meet every iteration (collective_plan above).  The north star's collective --
        # ONE RCCL all-reduce per Gauss-Newton iteration, on a communicator the library owns -- carries the measurement whenever RCCL
        # can be set up; the host-side exchange (and, on request, the in-kernel peer-to-peer mailboxes) are timed in the same run and
        # reported beside it in config.collective_step_us.
        want = os.environ.get("RPE_BENCH_COLLECTIVE", "auto")
        plan = collective_plan(world if world > 1 else (2 if force_dist else 1), want, os.environ.get("RPE_BENCH_SHARE_GPU") == "1", args.full)
        if world == 1 and force_dist:   # the collective path exercised with one rank (tests)
            plan.update(rccl_ranks_expected=1 if plan["rccl_init"] else 0, distinct_gpu_check=False)
        p2p = native = rccl_ok = hostex = False
        rccl_ranks, rccl_verified, bus_ids = 0, False, []
        coll_times = {}
        if dist_path:
            for _ in range(200):   # first launches of a process on a cold box can take seconds: ranks enter the first collective together
                ctx.normal_eq(L.RES_P2P, pose12(R0, t0), L.USE_MASK)
            dist.barrier()
            # one process per GPU: every rank must sit on a GPU of its own (the test rig with several ranks on one GPU says so explicitly)
            bus_ids = [None] * world
            dist.all_gather_object(bus_ids, ctx.bus_id())
            if plan["distinct_gpu_check"] and len(set(bus_ids)) != world:
                sys.exit(f"bench.py: rank {rank}: the {world} ranks do not sit on {world} different GPUs (PCI bus ids {bus_ids}); "
                         "one process per GPU is required (RPE_BENCH_SHARE_GPU=1 is the test rig's override)")

        def verify_step(label):
            """one sharded step's record against the all-reduced local records (every rank takes part; all ranks get the same answer)"""
            chk, rec = pose12(R0, t0), np.zeros(32)
            try:
                L.check(L.lib().rpe_gn_step_dist(ctx._h, L.RES_P2P, L.USE_MASK, chk.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), None))
                delivered = 1
            except L.RpeError as e:
                delivered = 0
                print(f"[bench] rank {rank}: {label} step failed: {e}", file=sys.stderr, flush=True)
            ref = shard.normal_eq(pose12(R0, t0)).clone().to(cdev)
            dist.all_reduce(ref)
            ref = ref.cpu().numpy()
            # (the two records come from different kernels -- resident / one launch per step -- whose fp32 pair sums are widened at
            # different points: they agree to the rounding of fp32 products, a missing or doubled shard is off by O(1))
            good = int(delivered and record_close(rec, ref, 2e-6))
            flag = torch.tensor([good], dtype=torch.int32, device=cdev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return int(flag.item()) == 1

        def timed(k, refine=False, device=False):
            q = pose12(R0, t0)
            run = (lambda kk: ctx.gn_refine([L.RES_P2P], q, None, L.USE_MASK, kk, 0.0)) if refine else (
                  (lambda kk: ctx.gn_steps_dist_device(L.RES_P2P, q, kk, L.USE_MASK)) if device else (lambda kk: ctx.gn_steps_dist(L.RES_P2P, q, kk, L.USE_MASK)))
            run(200)
            dist.barrier()
            t0_ = time.perf_counter()
            run(k)
            tt = torch.tensor([time.perf_counter() - t0_], dtype=torch.float64, device=cdev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            return float(tt.item()) / k

        def all_ok(ok):
            f = torch.tensor([int(ok)], dtype=torch.int32, device=cdev)
            dist.all_reduce(f, op=dist.ReduceOp.MIN)
            return int(f.item()) == 1

        # (1) RCCL on the library's communicator
        if dist_path and plan["rccl_init"]:
            rccl_ok = init_native_comm(ctx)
            if rccl_ok:
                rccl_verified = verify_step("RCCL")
                rccl_ranks = ctx.comm_count() if rccl_verified else 0   # from the communicator (ncclCommCount), not from which path wins
                if not rccl_verified:
                    if rank == 0:
                        print("[bench] the RCCL step's record differs from the all-reduced local records: communicator dropped", file=sys.stderr, flush=True)
                    ctx.comm_destroy()
                    rccl_ok = False
            if rccl_ok and args.full:
                coll_times["rccl_us"] = timed(400) * 1e6   # rpe_gn_steps_dist = kernel + ncclAllReduce of its run records + publish kernel per step
                # ... and the same steps chained on the device (rpe_gn_steps_dist_device: solve + exp-map in the kernels, the host enqueues
                # 400 x {kernel, ncclAllReduce} and waits once) -- timed beside: the headline keeps the exp-map on the host (north star)
                try:
                    coll_times["rccl_device_us"] = timed(400, device=True) * 1e6
                except L.RpeError as e:
                    print(f"[bench] rank {rank}: chained sharded steps failed: {e}", file=sys.stderr, flush=True)
        # (2) the in-kernel peer-to-peer exchange (only on request: it has never run on real xGMI)
        if dist_path and ("p2p" in plan["timed_beside"] or plan["headline"] == "p2p"):
            p2p = init_p2p(ctx)
            if p2p:
                dist.barrier()
                if not verify_step("peer-to-peer"):
                    if rank == 0:
                        print("[bench] peer-to-peer record differs from the all-reduced one: dropped", file=sys.stderr, flush=True)
                    ctx.p2p_destroy()
                    p2p = False
            if p2p:
                if args.full:
                    coll_times["p2p_us"] = timed(400) * 1e6
                if plan["headline"] != "p2p":
                    dist.barrier()
                    ctx.p2p_destroy()   # timed beside; the headline runs on RCCL
                    p2p = False
            if not p2p and plan["headline"] == "p2p" and os.environ.get("RPE_BENCH_STRICT_COLLECTIVE") == "1":
                sys.exit("bench.py: the peer-to-peer collective was requested strictly and is not available")
        # (3) the host-side exchange (every rank keeps its resident kernel; the hosts add the records through shared memory)
        if dist_path and ("host" in plan["timed_beside"] or plan["headline"] == "host" or not (rccl_ok or p2p)):
            hostex = init_host_exchange(ctx)
            if hostex and not verify_step("host-exchange"):
                if rank == 0:
                    print("[bench] host-exchange record differs from the all-reduced one: dropped", file=sys.stderr, flush=True)
                ctx.hostex_destroy()
                hostex = False
            if hostex:
                # rpe_gn_refine: resident kernel per rank + exchange between the hosts.  Every wait in it is bounded, so a rank that fails
                # takes the others out with it after the exchange's timeout: all ranks arrive at the flag below and fall back together.
                def refine_ok(k):
                    if os.environ.get("RPE_BENCH_INJECT_HOSTEX_FAIL") == str(rank):   # tests: this rank drops out, the peers run into the exchange's timeout
                        print(f"[bench] rank {rank}: injected host-exchange failure", file=sys.stderr, flush=True)
                        return False
                    try:
                        ctx.gn_refine([L.RES_P2P], pose12(R0, t0), None, L.USE_MASK, k, 0.0)
                        return True
                    except (L.RpeError, AssertionError) as e:
                        print(f"[bench] rank {rank}: refinement over the host-side exchange failed: {e}", file=sys.stderr, flush=True)
                        return False
                good = all_ok(refine_ok(200))   # the ranks agree after every phase, so they always enter the same torch collective next
                host_us = None
                if good and args.full:
                    dist.barrier()
                    t0_ = time.perf_counter()
                    ran = refine_ok(400)
                    tt = torch.tensor([time.perf_counter() - t0_], dtype=torch.float64, device=cdev)
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    host_us = float(tt.item()) / 400 * 1e6
                    good = all_ok(ran)
                if not good:
                    if rank == 0:
                        print("[bench] host-side exchange dropped", file=sys.stderr, flush=True)
                    ctx.hostex_destroy()
                    hostex = False
                else:
                    coll_times["host_us"] = host_us
            if hostex and (rccl_ok or p2p) and plan["headline"] != "host":
                dist.barrier()
                ctx.hostex_destroy()   # timed beside; the headline runs on the RCCL communicator (north star)
                hostex = False
            if not hostex and plan["headline"] == "host" and not (rccl_ok or p2p):
                sys.exit("bench.py: the host-side exchange was requested and neither it nor RCCL is available")
        native = rccl_ok or p2p
        collective = "none" if not dist_path else (
            "host-side exchange: every rank's host thread adds the peers' 32 fp64 records (shared memory, rank order) each iteration" if hostex else
            "peer-to-peer exchange of 32 fp64 per step inside the kernel (xGMI, HIP IPC mailboxes)" if p2p else
            ("rccl: one all-reduce(sum) per step of the launch's run records (8 x 32 fp64: the 17 / 29 sums per run), " if native else "rccl: all-reduce(sum) of 32 fp64 per step over RCCL, ") + ("library-owned communicator" if native else "torch.distributed"))

        # The host side of the loop (wait for the record, 6x6 solve, SE(3) exp-map update, next pose out) is C++ inside the library:
        # rpe_gn_refine / rpe_gn_steps_dist with tol = 0 run exactly k iterations, so the timed region contains no Python per step.
        # sharded + host exchange: rpe_gn_refine on every rank (resident kernel when every rank has its own GPU)
        shared_gpu = os.environ.get("RPE_BENCH_SHARE_GPU") == "1"
        resident = ((not dist_path) or (hostex and not shared_gpu)) and os.environ.get("RPE_RESIDENT", "1") != "0"
        # ... and the context must actually be able to run them (large BAR, co-residency cap >= 1, fewer than two lost grids); the state
        # is read again after the timed region: a grid lost in it (another process on the GPU) means the labels below would describe a
        # path that did not run
        res_state0 = ctx.resident_state()
        resident = resident and res_state0["enabled"] and res_state0.get("host_driven", True)

        # rpe_gn_refine called straight through ctypes with arguments prepared once: the timed region should hold the library's loop, not
        # numpy conversions (about 5 us per call, a quarter of a microsecond per step at --steps 20)
        _kinds = np.array([L.RES_P2P], np.int32)
        _pose = np.zeros(12)
        _its, _stepn, _cost = C.c_int(0), C.c_double(0), C.c_double(0)
        _refine = L.lib().rpe_gn_refine
        _args = (ctx._h, 1, _kinds.ctypes.data_as(C.c_void_p), None, L.USE_MASK, _pose.ctypes.data_as(C.c_void_p))
        _tail = (C.c_double(0.0), C.byref(_its), C.byref(_stepn), C.byref(_cost))

        last = {}   # what the path returned besides the pose in its last call (--dump-outputs)

        def run_steps(p, k):
            if k <= 0:
                return p
            if not dist_path or hostex:
                _pose[:] = p
                L.check(_refine(*_args, k, *_tail))
                assert _its.value == k
                last.update(step_norm=_stepn.value, cost=_cost.value)
                return _pose.copy()
            if native:
                last.update(step_norm=ctx.gn_steps_dist(L.RES_P2P, p, k, L.USE_MASK))
                return p
            for _ in range(k):
                p, step_norm, _ = gn.step(p)
            last.update(step_norm=step_norm)
            return p

        # untimed pre-warm, independent of --warmup: the first process on a freshly booted box runs its kernels slower for about a
        # second, and the runtime's lazy initialisation stalls once -- neither may land in the timed region
        if dist_path:
            pose = run_steps(pose, int(os.environ.get("RPE_BENCH_PREWARM_STEPS", "20000")))   # a FIXED count: every rank issues the same number of collective steps
        else:
            # launches of the TIMED length, so that every launch of the resident kernel in this process serves args.steps iterations
            # and a rocprofv3 --kernel-trace --stats average over the run is the average timed launch (only the --warmup launch differs);
            # at most PREWARM_MAX_STEPS per launch, so that a long timed region does not stretch the pre-warm past its time
            t_pre = time.perf_counter()
            while time.perf_counter() - t_pre < float(os.environ.get("RPE_BENCH_PREWARM_S", "1.5")):
                pose = run_steps(pose12(R0, t0), min(args.steps, PREWARM_MAX_STEPS))
        # which host CPU polls fastest differs from box to box (GPU-local cores usually, the other socket's on some boxes, by 5-10 %).
        # The choice is the LIBRARY's (rpe_tune_host_thread: a few candidates of both kinds, a short refinement each, the calling
        # thread left pinned to the fastest) -- any C++ caller of rpe_gn_refine gets the same with one call or RPE_HOST_CPU=auto.
        if not dist_path and resident and not args.no_extras and os.environ.get("RPE_BENCH_NO_CALIBRATE") != "1":   # (--no-extras: profiled runs hold the timed launches only)
            try:
                if ORIG_AFFINITY:
                    os.sched_setaffinity(0, ORIG_AFFINITY)   # every CPU the process may use is a candidate again
                tune_steps = min(args.steps, PREWARM_MAX_STEPS)   # every candidate CPU runs reps x tune_steps: bounded like the pre-warm
                tune = ctx.tune_host_thread(L.RES_P2P, pose12(R0, t0), flags=L.USE_MASK, steps=tune_steps, reps=max(3, min(12, 6000 // tune_steps)))
                affinity = dict(affinity, pinned=True, cpu=tune["cpu"], tuned_by="rpe_tune_host_thread (library call; RPE_HOST_CPU=auto does the same for any caller)",
                                calibration_us_per_step={str(k): round(v, 3) for k, v in tune["trials"].items()})
            except Exception as e:  # noqa: BLE001
                affinity = dict(affinity, calibration_error=repr(e))
        run_steps(pose12(R0, t0), args.warmup)
        if not args.full:
            # the first region after the warm-up runs slower than the ones after it (on one box: 7.0-8.6 us per 20-step region
            # against a median of 6.5-6.8 over 50): a plain run times ONE region, so untimed regions of the same form go first, as
            # many as stood before the median of --full's 50 (a fixed count: every rank runs the same collectives)
            for _ in range(SETTLE_REGIONS):
                if world > 1:
                    dist.barrier()
                torch.cuda.synchronize()
                run_steps(pose12(R0, t0), min(args.steps, PREWARM_MAX_STEPS))
                torch.cuda.synchronize()
        if os.environ.get("RPE_BENCH_INJECT_LOST_GRID"):   # tests: a workgroup withholds its sums in the timed region's refinements
            ctx.inject_resident_fault(int(os.environ["RPE_BENCH_INJECT_LOST_GRID"]), 0.0)

        # ---- timed: `repeats` repetitions of EXACTLY `steps` steps, each bracketed by barrier + synchronize, MAX over ranks
        launches_per_rep = 1 if resident else args.steps
        time_every = 1 if (resident or args.steps < 256) else 16
        per_rep_records = (launches_per_rep + time_every - 1) // time_every
        budget = 4096
        # HIP events on a launch are instrumentation with a cost of their own (about 8 us per launch: 0.4 us per step of a 20-step
        # region): with --full, --event-reps of the repetitions carry them (for roofline.avg_launch_us), interleaved with the plain ones;
        # a plain run times its steps without them
        timed_reps = max(1, min(args.repeats, args.event_reps, budget // max(per_rep_records, 1))) if args.full else 0
        event_every = max(1, args.repeats // max(timed_reps, 1))
        samples, k_cnt, k_total_ms, k_min_ms = [], 0, 0.0, 1e30
        for rep in range(args.repeats):
            timing = rep % event_every == 0 and rep // event_every < timed_reps
            if timing:
                ctx.timing_enable(per_rep_records + 1, time_every)
            p_start = pose12(R0, t0)
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t_start = time.perf_counter()
            pose = run_steps(p_start, args.steps)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            el = time.perf_counter() - t_start
            if world > 1:
                tmax = torch.tensor([el], dtype=torch.float64, device=cdev)
                dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                el = float(tmax.item())
            samples.append(el)
            if timing:
                cnt, tot_ms, mn_ms = ctx.timing_collect()
                k_cnt += cnt; k_total_ms += tot_ms
                if cnt:
                    k_min_ms = min(k_min_ms, mn_ms)
                ctx.timing_enable(0, 1)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, pose, last)
        ev_avg_ms, ev_min_ms = ctx.timing_calibrate(200) if args.full else (None, None)
        elapsed = percentile(samples, 0.5)
        res_state1 = ctx.resident_state()
        resident_lost_in_run = res_state1["lost"] - res_state0["lost"]
        resident_ran = resident and resident_lost_in_run == 0 and res_state1["enabled"]

        # where a step's time goes, seen from the host thread (resident loop only): waiting for the GPU vs its own work
        loop_prof = None
        if args.full and not dist_path and hasattr(L.lib(), "rpe_debug_loop_profile"):
            try:
                gpu_us, host_us, cnt = C.c_double(0), C.c_double(0), C.c_longlong(0)
                L.lib().rpe_debug_loop_profile(ctx._h, 1, None, None, None)
                run_steps(pose12(R0, t0), args.steps)
                L.lib().rpe_debug_loop_profile(ctx._h, 0, C.byref(gpu_us), C.byref(host_us), C.byref(cnt))
                if cnt.value:
                    loop_prof = {"steps": cnt.value, "host_waits_for_record_us": gpu_us.value / cnt.value, "host_solve_update_handover_us": host_us.value / cnt.value,
                                 "note": "per step, host clock inside rpe_gn_refine: waiting = pose hand-over in flight + kernel iteration + record in flight; "
                                         "host = 6x6 LDL^T solve + SE(3) exp-map update + 13 stores into the control block"}
            except Exception as e:  # noqa: BLE001
                loop_prof = {"error": repr(e)}

    # extra on the collective path (every rank takes part): the sharded device-resident loop
    sharded_loop = None
    if world > 1 and p2p and args.full and not args.no_extras:
        try:
            K = 500
            ctx.gn_refine_device([(L.RES_P2P, 1.0)], pose12(R0, t0), L.USE_MASK, 50, 0.0)
            dist.barrier()
            t0d = time.perf_counter()
            pd, itd, _, _ = ctx.gn_refine_device([(L.RES_P2P, 1.0)], pose12(R0, t0), L.USE_MASK, K, 0.0)
            td = torch.tensor([time.perf_counter() - t0d], dtype=torch.float64, device=cdev)
            dist.all_reduce(td, op=dist.ReduceOp.MAX)
            dtd = float(td.item())
            sharded_loop = {"value": float(total_n) * K / dtd, "unit": "correspondence-residuals/s", "us_per_iteration": dtd / K * 1e6, "iterations": itd,
                            "note": "rpe_gn_refine_device after rpe_p2p_init: one launch per iteration on every GPU; beside, not instead of, the headline"}
        except Exception as e:  # noqa: BLE001
            sharded_loop = {"error": repr(e)}

    # weak-scaling figure beside the strong-scaling headline (every rank takes part): a frame-sized shard (configs[1]: 307 200) on every
    # rank, the same way of adding the records as the headline
    weak = None
    if world > 1 and args.full and not args.no_extras and (hostex or (rccl_ok and not p2p)):
        try:
            wn = 307200
            wsc = make_shard(1000 + rank, wn)
            wctx = api.Context(local_rank)
            wctx.load(L.F32, xw=wsc.Q, xc=wsc.P)
            Rw0, tw0 = initial_pose(wsc)
            winl = int(wctx.inlier_mask(L.VOTE_33, pose7_from_Rt(Rw0, tw0, L.F32), thre_3d=THRE_3D))
            ok = init_host_exchange(wctx) if hostex else init_native_comm(wctx)
            if ok:
                Kw = 400
                def wrun(k):
                    q = pose12(Rw0, tw0)
                    if hostex:
                        wctx.gn_refine([L.RES_P2P], q, None, L.USE_MASK, k, 0.0)
                    else:
                        wctx.gn_steps_dist(L.RES_P2P, q, k, L.USE_MASK)
                wrun(200)
                dist.barrier()
                t0w = time.perf_counter()
                wrun(Kw)
                tw = torch.tensor([time.perf_counter() - t0w], dtype=torch.float64, device=cdev)
                dist.all_reduce(tw, op=dist.ReduceOp.MAX)
                tiw = torch.tensor([winl], dtype=torch.int64, device=cdev)
                dist.all_reduce(tiw)
                weak = {"corr_per_rank": wn, "global_corr": wn * world, "valid_corr_per_step": int(tiw.item()), "us_per_step": float(tw.item()) / Kw * 1e6,
                        "value": float(tiw.item()) * Kw / float(tw.item()), "unit": "correspondence-residuals/s",
                        "note": "weak scaling: a configs[1]-sized shard (307 200) on every rank, records added as in the headline; beside, not instead of, it"}
                dist.barrier()
                if hostex:
                    wctx.hostex_destroy()
                else:
                    wctx.comm_destroy()
            wctx.close()
        except Exception as e:  # noqa: BLE001
            weak = {"error": repr(e)}

    # global inlier count (valid correspondences) for the headline value
    inl_total = inl
    if world > 1:
        ti = torch.tensor([inl], dtype=torch.int64, device=cdev)
        dist.all_reduce(ti)
        inl_total = int(ti.item())

    out = None
    invalid = None
    if rank == 0:
        if resident and not resident_ran:
            # a resident grid was lost during this process (the library finished those refinements with one launch per iteration and
            # returned RPE_OK): repetitions of BOTH paths are in the samples, so neither set of labels describes the run
            invalid = ("%d resident grid(s) lost during the run (another process on this GPU?): the timed repetitions mix the resident loop with "
                       "one launch per iteration; rerun on an idle GPU" % resident_lost_in_run)
            resident = False
        steps_per_launch = args.steps if resident else 1
        k_avg_s = (k_total_ms / max(k_cnt, 1)) * 1e-3
        bytes_per_launch = BYTES_PER_CORR * n * steps_per_launch
        achieved = bytes_per_launch / k_avg_s / 1e9 if k_avg_s > 0 else None
        kernel_name = "rpe::normal_eq_resident_kernel<float, 0, 256, true, false, 2, 0, true>" if resident else "rpe::normal_eq_kernel<float, 0, 512, true, false, true>"
        # profiles/ evidence of this command (rocprofv3 --kernel-trace --stats; two --pmc passes), recorded per steps-per-launch.  A
        # per-launch value from a file stands in the line ONLY if the file's launches served the same number of steps as this run's;
        # otherwise the line carries the file's per-step values with the file's own steps_per_launch beside them.
        traffic, profile_same, profile_other = None, None, []
        traffic_source = "none: PMC traffic is recorded for the single-GPU resident kernel only"
        if world == 1 and resident:
            for e in profile_entries().get("normal_eq_resident_p2p_f32", []):
                if e.get("steps_per_launch") == steps_per_launch and profile_same is None:
                    profile_same = e
                else:
                    profile_other.append({k: e.get(k) for k in ("steps_per_launch", "rocprofv3_us_per_step", "traffic_bytes_per_step", "source")})
            # file-derived, so it goes stale the moment the kernel changes: it stands in the line only while the sources the kernel is
            # compiled from hash to what the profile was taken on (traffic_source says which file, which hash, and whether it held)
            prof_hash, now_hash = profile_entries().get("kernel_src_sha256"), kernel_source_hash()
            if profile_same and prof_hash and prof_hash == now_hash:
                traffic = profile_same.get("traffic_bytes_per_launch")
                traffic_source = "%s (PMC passes of this command; kernel sources %s = this build)" % (PROFILE_INDEX, prof_hash)
            elif profile_same:
                traffic_source = "none: %s was taken on kernel sources %s, this build is %s" % (PROFILE_INDEX, prof_hash, now_hash)
            else:
                traffic_source = "none: %s holds no profile with %d steps per launch" % (PROFILE_INDEX, steps_per_launch)
        ms_med = elapsed / args.steps * 1e3
        out = {
            "metric": "correspondence-residuals/sec", "value": float(inl_total) * args.steps / elapsed, "unit": "correspondence-residuals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_med,
            "ms_per_step_untuned": (UNTUNED or {}).get("ms_per_step"), "untuned": UNTUNED,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload, "workload_short": workload_short, "corr_rank0": n, "global_corr": total_n, "valid_corr_per_step": inl_total,
                       "value_counts": "valid correspondences = rows that pass the RANSAC inlier mask (SURVEY 8d); every row is streamed",
                       "streamed_corr_per_s": float(total_n) * args.steps / elapsed, "accumulate": "fp64", "collective": collective,
                       "collective_step_us": ({"rccl_us": coll_times.get("rccl_us"), "rccl_device_us": coll_times.get("rccl_device_us"), "host_us": coll_times.get("host_us"), "p2p_us": coll_times.get("p2p_us")} if dist_path else None),
                       "collective_step_us_note": "same run, same shards, 400 steps each: rccl = kernel (run records left on the device) + ncclAllReduce of the run records + one-workgroup kernel that sends them to the host as tagged pairs, per step; rccl_device = the same steps chained on the device (rpe_gn_steps_dist_device: every launch solves for its own pose, the host enqueues all of them and waits once); host = resident kernel per rank + records added by the host threads; p2p = in-kernel mailboxes (timed on request only: RPE_BENCH_COLLECTIVE=auto_p2p)" if dist_path else None,
                       "rccl_ranks": rccl_ranks, "rccl_ranks_source": "ncclCommCount on the library's communicator after one verified all-reduce" if rccl_ranks else None,
                       "resident_state": {"before": res_state0, "after": res_state1, "lost_in_run": resident_lost_in_run, "resident_loop_ran": resident_ran},
                       "rccl_verified": rccl_verified, "pci_bus_ids": bus_ids or None, "collective_plan": plan if dist_path else None,
                       "host_loop": "rpe_gn_refine: ONE resident launch per refinement, poses handed over through device memory" if resident else
                                    ("rpe_gn_refine on every rank: one launch per step + exchange between the host threads (ranks share a GPU)" if hostex else
                                     "rpe_gn_steps_dist: one launch + one collective per step" if dist_path else "rpe_gn_refine: one launch per step")},
            "timing": {"repeats": args.repeats, "statistic": "median over repetitions of the whole K-step region (MAX over ranks each)",
                       "event_timed_repetitions": timed_reps, "event_timed_note": "every %d-th repetition also carries HIP events on its launches (instrumentation for roofline.avg_launch_us, about 8 us per launch); all repetitions enter the median" % event_every,
                       "ms_per_step_p10": percentile(samples, 0.1) / args.steps * 1e3, "ms_per_step_p90": percentile(samples, 0.9) / args.steps * 1e3,
                       "ms_per_step_min": min(samples) / args.steps * 1e3, "hsa_enable_interrupt": os.environ.get("HSA_ENABLE_INTERRUPT"), "host_thread": {k: v for k, v in affinity.items() if k != "gpu_local_cpu_ids"}, "loop_profile": loop_prof},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic, "traffic_source": traffic_source,
                         "library_sha256": library_hash(), "kernel_src_sha256": kernel_source_hash(),
                         "traffic_per_step": (traffic / steps_per_launch) if traffic else None,
                         "traffic_over_algorithmic": (traffic / bytes_per_launch) if traffic else None,
                         "kernel": kernel_name, "algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_bytes_per_step": BYTES_PER_CORR * n,
                         "steps_per_launch": steps_per_launch,
                         "avg_launch_us": (k_avg_s * 1e6) if k_cnt else None, "avg_launch_us_per_step": (k_avg_s * 1e6 / steps_per_launch) if k_cnt else None,
                         "min_launch_us": (k_min_ms * 1e3) if k_cnt else None,
                         "launches_timed": k_cnt, "empty_event_pair_us": (ev_avg_ms * 1e3) if ev_avg_ms is not None else None,
                         "profile_same_steps_per_launch": profile_same, "profiles_other_steps_per_launch": profile_other or None,
                         "note": "HIP events on the kernel's own stream (hipExtLaunchKernelGGL start / stop = the dispatch's begin / end timestamps, what "
                                 "rocprofv3 reports); one launch per step, 26 B x correspondences of this rank per launch" if not resident else
                                 "HIP events on the kernel's own stream (hipExtLaunchKernelGGL start / stop = the dispatch's begin / end timestamps, what "
                                 "rocprofv3 reports).  One launch of the resident kernel serves steps_per_launch iterations; its duration INCLUDES the host's "
                                 "turn of every iteration (record over PCIe, 6x6 solve, exp-map, next pose over PCIe): algorithmic bytes = 26 B x "
                                 "correspondences x iterations.  The correspondences of a frame-sized problem stay in registers between iterations, so "
                                 "this is not an HBM-streaming figure (DESIGN.md section 5; the bandwidth-bound figures are in roofline_hbm).  traffic = PMC "
                                 "bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, separate passes) from profile_same_steps_per_launch, i.e. from a "
                                 "profile of this command whose launches served the same number of steps as this run's; null when no such profile is "
                                 "committed (the per-step values of the other profiles are listed with their own steps_per_launch)"},
        }
        if world == 1 and not args.full:
            out["cpu_baseline"] = None
        elif world == 1:
            try:   # pose parity: converged GN pose vs the CPU oracle's closed form (shinji, fp64, same fp32 inputs, same inlier set)
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import oracle_lib as O
                m = ctx.download_mask(L.MOD_33)
                Ro, to, _ = O.shinji_f32in_f64(sc.Q[m == 1], sc.P[m == 1])
                out["pose_error_vs_cpu"] = {"rot_rad": rot_err(pose[:9].reshape(3, 3), Ro),
                                            "trans_rel": float(np.linalg.norm(pose[9:] - to) / np.linalg.norm(to)),
                                            "tolerance": {"rot_rad": 1e-5, "trans_rel": 1e-4},
                                            "reference": "oracle shinji() fp64 on the same fp32 inputs and inlier set"}
            except Exception as e:  # noqa: BLE001
                out["pose_error_vs_cpu"] = {"error": repr(e)}
            try:   # iterations until |delta| < 1e-9 from the initial pose, over all points and over the inliers
                if args.no_extras:   # (--no-extras keeps the profiled runs to launches of the timed length only)
                    raise StopIteration
                conv = {}
                for name, flags, sel in (("all_points", 0, slice(None)), ("inliers_only", L.USE_MASK, m == 1)):
                    pc, itc, stepc, _ = ctx.gn_refine([L.RES_P2P], pose12(R0, t0), None, flags, 50, 1e-9)
                    Rk, tk, _ = O.shinji_f32in_f64(sc.Q[sel], sc.P[sel])
                    conv[name] = {"iterations": itc, "last_step": stepc, "rot_rad_vs_cpu_closed_form": rot_err(pc[:9].reshape(3, 3), Rk),
                                  "trans_rel_vs_cpu_closed_form": float(np.linalg.norm(pc[9:] - tk) / np.linalg.norm(tk))}
                out["convergence"] = conv
            except StopIteration:
                pass
            except Exception as e:  # noqa: BLE001
                out["convergence"] = {"error": repr(e)}
            out["cpu_baseline"] = None if args.no_cpu_baseline else cpu_baseline(sc, args.cpu_seconds)
            if not args.no_hbm:
                try:
                    out["roofline_hbm"] = hbm_roofline(local_rank)
                except Exception as e:  # noqa: BLE001
                    out["roofline_hbm"] = {"error": repr(e)}
                try:   # the kernels behind the reference's own API (moments, nl_round, winner's mask) on the same roofline
                    out["roofline_hbm"]["reference_api_kernels"] = reference_api_roofline(local_rank)
                except Exception as e:  # noqa: BLE001
                    out["roofline_hbm"]["reference_api_kernels"] = {"error": repr(e)}
            if not args.no_extras:
                extras(out, args, ctx, sc, n, R0, t0, pose, local_rank)
                try:
                    out["fp64"] = fp64_lines(local_rank)
                except Exception as e:  # noqa: BLE001
                    out["fp64"] = {"error": repr(e)}
        else:
            if sharded_loop is not None:
                out["device_resident_loop"] = sharded_loop
            out["pose_error_vs_truth"] = {"rot_rad": rot_err(pose[:9].reshape(3, 3), sc.R), "trans_abs_m": float(np.linalg.norm(pose[9:] - sc.t))}
            out["cpu_baseline"] = None
            # the weak-scaling figure beside the strong-scaling headline: every rank's own frame-sized shard at the same step rate
            out["weak_scaling"] = weak
            out["weak_scaling_note"] = "strong scaling (fixed 10 M total) is the headline for N > 1; per-GPU work at N = 1 is configs[1] (307 200)"
    # tear everything down first: RCCL prints its version banner on stdout around communicator life-cycle events, and
    # the JSON line must be the LAST line rank 0 prints
    if world > 1:
        dist.barrier()   # no rank may unmap its mailbox / destroy its communicator while a peer can still reach it
    ctx.close()
    if dist_path:
        dist.destroy_process_group()
    sys.stdout.flush()
    try:  # RCCL's banner sits in the C stdio buffer until exit: push it out before the JSON line
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if rank == 0:
        if invalid:
            out["valid"] = False
            out["invalid_reason"] = invalid
            print("bench.py: INVALID RUN: " + invalid, file=sys.stderr, flush=True)
        write_extras(out)
        print(contract_line(out), flush=True)
        if invalid:
            sys.exit(3)


LINE_LIMIT = 4096            # the driver keeps the last 8 KB of stdout; the round-4 line (21.9 KB) could not be parsed
EXTRAS_FILE = "bench_extras.json"


def _num(x, digits=6):
    """floats rounded to `digits` significant digits (the line is for reading and parsing, the full values are in the extras file)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    try:
        x = float(x)
    except (TypeError, ValueError):
        return None
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{digits}g}")


def _get(d, *path):
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def contract_line(full: dict, strict: bool = False) -> str:
    """The ONE line the driver parses: the contract's keys and nothing else (each object flat, strings short), at most LINE_LIMIT bytes.
    Everything else this run measured is in EXTRAS_FILE (write_extras) -- never in the line."""
    cfg, roof, cpu, tim = (full.get(k) or {} for k in ("config", "roofline", "cpu_baseline", "timing"))
    resident = (roof.get("steps_per_launch") or 1) > 1
    line = {
        "metric": full.get("metric"), "value": _num(full.get("value"), 9), "unit": full.get("unit"), "n_gpus": full.get("n_gpus"),
        "steps": full.get("steps"), "warmup": full.get("warmup"), "ms_per_step": _num(full.get("ms_per_step"), 9),
        "higher_is_better": True, "scaling": full.get("scaling"), "vs_baseline": None, "dtype": full.get("dtype"), "data": full.get("data"),
        "config": {"workload": cfg.get("workload_short") or (cfg.get("workload") or "")[:200], "corr_rank0": cfg.get("corr_rank0"),
                   "global_corr": cfg.get("global_corr"), "valid_corr_per_step": cfg.get("valid_corr_per_step"),
                   "collective": (cfg.get("collective") or "none")[:40], "rccl_ranks": cfg.get("rccl_ranks"), "rccl_verified": cfg.get("rccl_verified"),
                   "host_loop": "resident kernel, host exp-map" if resident else "launch per step, host exp-map",
                   # N > 1: the same sharded step by the ways of adding the records, microseconds per iteration (400 steps each; flat keys)
                   **({("step_" + k): _num(v) for k, v in cfg.get("collective_step_us").items() if v is not None} if isinstance(cfg.get("collective_step_us"), dict) else {}),
                   "repeats": tim.get("repeats"), "ms_per_step_p10": _num(tim.get("ms_per_step_p10")), "ms_per_step_p90": _num(tim.get("ms_per_step_p90"))},
        "roofline": {"bound": roof.get("bound"), "achieved": _num(roof.get("achieved")), "peak": roof.get("peak"), "unit": roof.get("unit"),
                     "frac": _num(roof.get("frac")), "traffic": _num(roof.get("traffic"), 9), "traffic_source": (roof.get("traffic_source") or "none")[:150],
                     "traffic_over_algorithmic": _num(roof.get("traffic_over_algorithmic")), "kernel": (roof.get("kernel") or "")[:96],
                     "avg_launch_us": _num(roof.get("avg_launch_us")), "steps_per_launch": roof.get("steps_per_launch"),
                     "bytes_per_launch": roof.get("algorithmic_bytes_per_launch"), "launches_timed": roof.get("launches_timed")},
        "cpu_baseline": None if not cpu else {
            "value": _num(cpu.get("value")), "unit": cpu.get("unit"), "cores": cpu.get("cores"), "kind": cpu.get("kind"),
            "sample": (cpu.get("sample_short") or cpu.get("sample") or "")[:160], "cpu_model": (cpu.get("cpu_model") or "")[:48],
            "host_cpus": cpu.get("host_cpus"), "all_cores_value": _num(_get(cpu, "all_cores", "value")), "all_cores_threads": _get(cpu, "all_cores", "threads")},
    }
    pe = full.get("pose_error_vs_cpu") or {}
    if "rot_rad" in pe:
        line["pose_error_vs_cpu"] = {"rot_rad": _num(pe.get("rot_rad"), 3), "trans_rel": _num(pe.get("trans_rel"), 3), "tol_rot_rad": 1e-5, "tol_trans_rel": 1e-4}
    # at most three scalar extras: configs[3] (the HBM-bound run) steady / cold, and K4 scoring against the fp32 vector peak
    for key, val in (("config3_frac_steady", _get(full, "roofline_hbm", "config3_p2plane_1M_steady", "frac_of_peak")),
                     ("config3_frac_cold", _get(full, "roofline_hbm", "config3_p2plane_1M_cold", "frac_of_peak")),
                     ("k4_exact_33_valu_frac", _get(full, "ransac_scoring", "roofline", "exact_33", "valu_frac"))):
        if val is not None:
            line[key] = _num(val, 4)
    if full.get("valid") is False:
        line["valid"] = False
        line["invalid_reason"] = (full.get("invalid_reason") or "")[:160]
    line["extras_file"] = EXTRAS_FILE
    return fit_line(line, strict)


def fit_line(line: dict, strict: bool = False) -> str:
    """Serialise the line; should it reach LINE_LIMIT (a long CPU model string, a future key ...), degrade it instead of failing after
    the whole measurement: drop the optional scalars first, then shorten every string, then drop the optional objects -- the contract's
    own keys always go out.  strict (the contract test): a line that needs any of this is an error."""
    dumps = lambda d: json.dumps(d, separators=(",", ":")).replace("\n", " ")
    text = dumps(line)
    if len(text) < LINE_LIMIT:
        return text
    if strict:
        raise RuntimeError(f"bench.py: the contract line is {len(text)} bytes (limit {LINE_LIMIT}): something long was added to it")
    line = json.loads(text)
    for key in ("config3_frac_steady", "config3_frac_cold", "k4_exact_33_valu_frac", "pose_error_vs_cpu", "extras_file"):
        line.pop(key, None)
        if len(dumps(line)) < LINE_LIMIT:
            break
    def shorten(o, cap):
        if isinstance(o, dict):
            return {k: shorten(v, cap) for k, v in o.items()}
        return o[:cap] if isinstance(o, str) else o
    for cap in (96, 48, 24):
        if len(dumps(line)) < LINE_LIMIT:
            break
        line = shorten(line, cap)
    if len(dumps(line)) >= LINE_LIMIT:   # last resort: the contract's scalar keys and the three objects' required members
        keep = {"config": ("workload",), "roofline": ("bound", "achieved", "peak", "unit", "frac", "traffic"), "cpu_baseline": ("value", "unit", "cores", "kind", "sample")}
        line = {k: ({m: v.get(m) for m in keep[k]} if k in keep and isinstance(v, dict) else v) for k, v in line.items()
                if k in keep or not isinstance(v, (dict, list))}
    line["truncated"] = True
    return dumps(line)


def write_extras(full: dict):
    """Everything beside the headline (bandwidth-bound figures, the reference-API kernels, fp64, untuned, configs[2] pipeline, notes) goes to
    bench_extras.json next to bench.py -- and to gpurun_out/ when that directory exists, so that it comes back from the GPU box."""
    text = json.dumps(full, indent=1, default=repr)
    paths = [os.path.join(d, EXTRAS_FILE) for d in (ROOT, os.path.join(ROOT, "gpurun_out")) if os.path.isdir(d)]
    if os.environ.get("RPE_BENCH_EXTRAS"):   # tests: a path of their own
        paths = [os.environ["RPE_BENCH_EXTRAS"]]
    for path in paths:
        try:
            with open(path, "w") as f:
                f.write(text + "\n")
        except OSError as e:
            print(f"bench.py: could not write {path}: {e}", file=sys.stderr)


def extras(out, args, ctx, sc, n, R0, t0, pose, local_rank):
    """Legs reported BESIDE the headline (never part of `value`)."""
    import ctypes as C
    import numpy as np
    from rgbd_pose_estimation_amd import _lib as L, api
    from rgbd_pose_estimation_amd.api import pose12, pose7_from_Rt
    # (1) the same iterations with one launch per step (RPE_RESIDENT=0 behaviour), for the step-time budget
    try:
        K = 2000
        p0 = pose12(R0, t0)
        best = 1e9
        for _ in range(3):
            t0s = time.perf_counter()
            for _k in range(K // 500):
                api_steps = 500
                q = p0.copy()
                for _s in range(api_steps):   # rpe_gn_step: one launch + wait + host solve per call (ctypes per step: ~2 us of it)
                    ctx.gn_step(L.RES_P2P, q, L.USE_MASK)
            best = min(best, (time.perf_counter() - t0s) / K)
        out["launch_per_step_loop"] = {"us_per_step": best * 1e6, "note": "rpe_gn_step per iteration (kernel launch + record + host solve each step), Python-driven"}
    except Exception as e:  # noqa: BLE001
        out["launch_per_step_loop"] = {"error": repr(e)}
    # (2) solve + exp-map on the GPU too (not the headline: the north star keeps the exp-map on the host)
    try:
        K = 500
        p0d = pose12(R0, t0)
        ctx.gn_refine_device([(L.RES_P2P, 1.0)], p0d, L.USE_MASK, 50, 0.0)
        t0d = time.perf_counter()
        pd, itd, _, _ = ctx.gn_refine_device([(L.RES_P2P, 1.0)], p0d, L.USE_MASK, K, 0.0)
        dtd = time.perf_counter() - t0d
        out["device_resident_loop"] = {"value": out["config"]["valid_corr_per_step"] * K / dtd, "unit": "correspondence-residuals/s", "us_per_iteration": dtd / K * 1e6,
                                       "iterations": itd, "rot_rad_vs_host_loop": rot_err(pd[:9].reshape(3, 3), pose[:9].reshape(3, 3)),
                                       "note": "rpe_gn_refine_device: solve + exp-map on the GPU, one launch for the whole loop (the resident grid iterates by itself); reported beside, not instead of, the host-update headline"}
    except Exception as e:  # noqa: BLE001
        out["device_resident_loop"] = {"error": repr(e)}
    # (3) the step BEFORE the path: dense projective ICP on two rendered 640x480 depth frames
    try:
        from rgbd_pose_estimation_amd import simulator as S
        Ra, ta = S._rot_zyx(0.05, -0.1, 0.02), np.array([0.1, -0.05, 0.2])
        dR = S._rot_zyx(0.02, -0.015, 0.01)
        Rb, tb = dR @ Ra, dR @ ta + np.array([0.03, -0.02, 0.025])
        fctx = api.Context(local_rank)
        fctx.frame_set_depth(S.render_depth(Ra, ta, as_u16=True), S.DEFAULT_CAMERA, 0.001, 0.1, 10.0, 0.1)
        fctx.model_from_frame(pose12(Ra, ta))
        fctx.frame_set_depth(S.render_depth(Rb, tb, as_u16=True), S.DEFAULT_CAMERA, 0.001, 0.1, 10.0, 0.1)
        K, reps = 20, 25
        modes = {}
        for name, dev_res in (("host_update_resident_kernel", False), ("device_resident_one_launch", True)):
            fctx.icp(pose12(Ra, ta), L.RES_P2PLANE, K, 0.0, 0.15, 0.8, device_resident=dev_res, fused=True)
            t0i = time.perf_counter()
            for _ in range(reps):
                pi, iti, _, _, pairs = fctx.icp(pose12(Ra, ta), L.RES_P2PLANE, K, 0.0, 0.15, 0.8, device_resident=dev_res, fused=True)
            dti = (time.perf_counter() - t0i) / reps
            modes[name] = {"us_per_round": dti / K * 1e6, "pixel_residuals_per_s": pairs * K / dti, "rot_err_rad_vs_truth": rot_err(pi[:9].reshape(3, 3), Rb),
                           "trans_err_m_vs_truth": float(np.linalg.norm(pi[9:] - tb))}
        best = modes["host_update_resident_kernel"]
        out["icp_frame_loop"] = {"value": best["pixel_residuals_per_s"], "unit": "pixel-residuals/s", "us_per_round": best["us_per_round"], "rounds": K,
                                 "pairs": pairs, "pixels": 307200, "rot_err_rad_vs_truth": best["rot_err_rad_vs_truth"],
                                 "trans_err_m_vs_truth": best["trans_err_m_vs_truth"], "modes": modes,
                                 "note": "rpe_icp, fused projective association + point-to-plane normal equations; value = host-update form (ONE resident launch "
                                         "per call: the frame's pixels stay in registers, the host hands over a pose per round); per call incl. the launch and "
                                         "the closing association pass"}
        fctx.close()
    except Exception as e:  # noqa: BLE001
        out["icp_frame_loop"] = {"error": repr(e)}
    # (4) the other half of the hot path: batched RANSAC hypothesis scoring (vote loops V1/V2/V4, kernel K4), 512 hypotheses per pass,
    # against BOTH ceilings SURVEY 8(d) names: the fp32 vector rate (157.3 TFLOP/s; flops per correspondence x hypothesis counted from
    # the predicates, stated below) and HBM amortised over the hypotheses of a pass (the arrays are read once per pass)
    try:
        rng_s = np.random.default_rng(3)
        H = 512
        dq = 0.002 * rng_s.standard_normal((H, 7))
        base7 = pose7_from_Rt(sc.R, sc.t, L.F32)
        poses = base7[None, :] + dq
        poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
        poses = np.ascontiguousarray(poses.astype(np.float32).astype(np.float64))
        # a bearing for every correspondence (camera point direction + ~4.5 px of noise at f = 585): the 2D test at full load
        bv = sc.P / np.linalg.norm(sc.P, axis=1, keepdims=True) + (0.3 * 15.0 / 585.0) * rng_s.standard_normal(sc.P.shape)
        bv = (bv / np.linalg.norm(bv, axis=1, keepdims=True)).astype(np.float32)
        sctx = api.Context(local_rank).load(L.F32, xw=sc.Q, xc=sc.P, bv=bv)
        cthr = math.cos(math.atan(8.0 / 585.0))
        FLOPS = {"33": {"fast": 32, "exact": 41}, "33_23": {"fast": 46, "exact": 58}}   # per correspondence x hypothesis: transform / quaternion
        # rotation 18 / 30, 3D test 11-14, 2D test (dot, |p|^2, compare form; exact: + reciprocal square root estimate) 14-17
        BYTES = {"33": 24, "33_23": 36}
        res, roof, v_exact = {}, {}, None
        for kname, kind in (("33", L.VOTE_33), ("33_23", L.VOTE_33_23)):
            for mode, name in ((L.SCORE_FAST, "fast"), (L.SCORE_EXACT, "exact")):
                t_w = time.perf_counter()
                while time.perf_counter() - t_w < 0.15:
                    sctx.score(kind, poses, THRE_3D, cthr, mode=mode)
                per_call = []
                for _ in range(30):   # every call timed by itself: the median is not moved by one stalled call
                    t0s = time.perf_counter()
                    v = sctx.score(kind, poses, THRE_3D, cthr, mode=mode)
                    per_call.append(time.perf_counter() - t0s)
                per_call.sort()
                dts = per_call[len(per_call) // 2]
                res[kname + "_" + name] = {"corr_hyp_per_s": n * H / dts, "us_per_pass": dts * 1e6, "us_per_pass_min": per_call[0] * 1e6}
                roof[name + "_" + kname] = {"valu_frac": n * H * FLOPS[kname][name] / dts / 157.3e12, "flops_per_corr_hyp": FLOPS[kname][name],
                                            "hbm_amortised_frac": BYTES[kname] * n / dts / 1e9 / HBM_PEAK_GBS, "bytes_per_pass": BYTES[kname] * n}
                if mode == L.SCORE_EXACT and kname == "33":
                    v_exact = v
        # (4b) a RANSAC-shaped sequence on the resident arrays -- one batch of 8 hypotheses, then the winner's masks -- served by ONE
        # resident launch (scoring session, kernel K4r) against a launch each; wall time of the whole sequence, median of 200
        sess = {}
        try:
            p8s = np.ascontiguousarray(poses[:8])

            def run_seq(session):
                if session and not sctx.score_session_begin(L.VOTE_33, thre_3d=THRE_3D):
                    return None
                vs = sctx.score(L.VOTE_33, p8s, THRE_3D)
                sctx.inlier_mask(L.VOTE_33, p8s[int(np.argmax(vs))], thre_3d=THRE_3D)
                if session:
                    sctx.score_session_end()
                return vs
            for label, flag in (("launch_each", False), ("session", True)):
                ref = run_seq(flag)
                if ref is None:
                    sess[label] = None
                    continue
                tsq = []
                for _ in range(200):
                    t0s = time.perf_counter(); run_seq(flag); tsq.append(time.perf_counter() - t0s)
                tsq.sort()
                sess[label] = {"us_per_run": tsq[len(tsq) // 2] * 1e6, "us_min": tsq[0] * 1e6, "votes_of_first": int(ref[0])}
            sess["what"] = "score 8 hypotheses (exact 3D vote) + winner's masks over 307 200 resident correspondences, through the Python binding"
        except Exception as e:  # noqa: BLE001
            sess = {"error": repr(e)}
        sctx.close()
        cpu = None
        if not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib as O
            votes_cpu = np.zeros(8, np.int32)
            xw32, xc32 = np.ascontiguousarray(sc.Q, np.float32), np.ascontiguousarray(sc.P, np.float32)
            p8 = np.ascontiguousarray(poses[:8])
            O.lib().orc_time_votes33.restype = C.c_double
            dtc = O.lib().orc_time_votes33(xw32.ctypes.data_as(C.c_void_p), xc32.ctypes.data_as(C.c_void_p), n, p8.ctypes.data_as(C.c_void_p), 8,
                                            C.c_float(THRE_3D), votes_cpu.ctypes.data_as(C.c_void_p))
            cpu = {"corr_hyp_per_s": n * 8 / dtc, "cores": 1, "sample": "8 hypotheses through the oracle's vote loop",
                   "votes_equal_exact_mode": bool(np.array_equal(votes_cpu, v_exact[:8]))}
        out["ransac_scoring"] = {"hypotheses": H, "kinds": "3D-3D (V1/V2) and 3D-3D + 2D-3D (V4), a bearing for every correspondence", "passes": res, "roofline": roof,
                                 "ransac_run": sess, "cpu_port": cpu, "peaks": {"fp32_vector_TFLOPs": 157.3, "hbm_GBs": HBM_PEAK_GBS},
                                 "note": "wall time per rpe_score call incl. pose upload and vote read-out (median of 30); beside, not instead of, the headline"}
    except Exception as e:  # noqa: BLE001
        out["ransac_scoring"] = {"error": repr(e)}
    # (5) configs[2] exactly as SURVEY 8d states it: 307 200 3D-3D + 2 000 bearings, 300 RANSAC iterations of shinji + kneip from a
    # fixed seeded sample list, scored in batches, best-so-far / adaptive-Iter replay, joint GN refine -- GPU pipeline and CPU oracle
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import config3_case
        out["config3_pipeline"] = config3_case.run(with_cpu=not args.no_cpu_baseline)
    except Exception as e:  # noqa: BLE001
        out["config3_pipeline"] = {"error": repr(e)}


def untuned_probe(args):
    """What a caller gets WITHOUT any host-side tuning: default CPU placement (no pinning, no calibration), default environment
    (HSA_ENABLE_INTERRUPT untouched), the same K-step regions bracketed by synchronisations.  Runs in a process of its own -- the
    runtime knobs are read when it initialises -- before the parent touches the GPU; prints one JSON object."""
    import ctypes as C
    import numpy as np
    import torch
    from rgbd_pose_estimation_amd import _lib as L, api
    from rgbd_pose_estimation_amd.api import pose12, pose7_from_Rt
    n = args.n_per_gpu
    sc = make_shard(0, n)
    ctx = api.Context(0)
    ctx.load(L.F32, xw=sc.Q, xc=sc.P)
    R0, t0 = initial_pose(sc)
    ctx.inlier_mask(L.VOTE_33, pose7_from_Rt(R0, t0, L.F32), thre_3d=THRE_3D)

    def run(k):
        return ctx.gn_refine([L.RES_P2P], pose12(R0, t0), None, L.USE_MASK, k, 0.0)
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 1.0:
        run(args.steps)
    ts = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0_ = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0_) / args.steps)
    ctx.close()
    print(json.dumps({"ms_per_step": percentile(ts, 0.5) * 1e3, "ms_per_step_p10": percentile(ts, 0.1) * 1e3, "ms_per_step_p90": percentile(ts, 0.9) * 1e3,
                      "steps": args.steps, "repeats": args.repeats, "cpu": sorted(os.sched_getaffinity(0))[:4], "cpus_allowed": len(os.sched_getaffinity(0)),
                      "hsa_enable_interrupt": os.environ.get("HSA_ENABLE_INTERRUPT"),
                      "note": "no pinning, no CPU calibration, default environment: what a C++ caller of rpe_gn_refine sees before rpe_tune_host_thread / RPE_HOST_CPU"}))


UNTUNED = None


def main():
    global UNTUNED
    # Completion signals polled by the waiting thread instead of interrupt-driven (ROCm runtime knob, this process only, must be in the
    # environment before the runtime initialises): the closing synchronisation of a 20-step region returns ~5 us sooner (A/B:
    # profiles/r03_hsa_interrupt_ab.txt).  Left alone if the caller set it; reported in timing.hsa_enable_interrupt.
    caller_set_interrupt = "HSA_ENABLE_INTERRUPT" in os.environ
    if "--untuned-probe" not in sys.argv:
        os.environ.setdefault("HSA_ENABLE_INTERRUPT", "0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--full", action="store_true", help="also measure everything reported beside the headline (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy (float64)")
    ap.add_argument("--repeats", type=int, default=None, help="repetitions of the timed K-step region; the median is reported (default 1, 50 with --full)")
    ap.add_argument("--event-reps", type=int, default=16, help="how many of the repetitions also time their launches with HIP events (roofline.avg_launch_us)")
    ap.add_argument("--n-per-gpu", type=int, default=N_FRAME, help="correspondences at N = 1 (configs[1])")
    ap.add_argument("--n-total", type=int, default=0, help="total correspondences at N > 1 (default configs[4]: 10 000 000)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the legs reported beside the headline (profiling runs: only the headline's launches)")
    ap.add_argument("--untuned-probe", action="store_true", help="internal: print the K-step figure of a process with NO host-side tuning (no pinning, default environment) and exit")
    ap.add_argument("--no-hbm", action="store_true", help="skip the live bandwidth-bound block (roofline_hbm: 1 M point-to-plane steady / cold, 10 M / 20 M point-to-point)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 50 if args.full else 1
    if args.gpus < 1 or args.steps < 1 or args.repeats < 1:
        sys.exit("bench.py: --gpus, --steps and --repeats must be positive")
    if args.untuned_probe:
        untuned_probe(args)
        return
    if args.full and args.gpus == 1 and "WORLD_SIZE" not in os.environ and not args.no_extras and os.environ.get("RPE_BENCH_NO_UNTUNED") != "1":
        # the untuned figure beside the headline: a child process with the caller's own environment and no pinning, run BEFORE this
        # process initialises the GPU (the two never use it at the same time)
        try:
            env = dict(os.environ)
            if not caller_set_interrupt:
                env.pop("HSA_ENABLE_INTERRUPT", None)
            env.pop("RPE_HOST_CPU", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--untuned-probe", "--steps", str(args.steps), "--repeats", str(min(args.repeats, 30)),
                                "--n-per-gpu", str(args.n_per_gpu)], env=env, capture_output=True, text=True, timeout=600)
            UNTUNED = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": (r.stderr or r.stdout)[-400:]}
        except Exception as e:  # noqa: BLE001
            UNTUNED = {"error": repr(e)}
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_children(sys.argv[1:], args.gpus))   # this process never initialises HIP
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and "WORLD_SIZE" in os.environ:
        args.gpus = world
    affinity = pin_to_gpu_numa_node(int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))) if os.environ.get("RPE_BENCH_NO_PIN") != "1" else {"pinned": False, "reason": "RPE_BENCH_NO_PIN=1"}
    worker(args, affinity)


if __name__ == "__main__":
    main()
