"""Compile the HIP backend for gfx950 in-tree: rgbd_pose_estimation_amd/lib/librgbdpose_hip.so.

hipcc cross-compiles without a GPU.  UNITS below is the manifest of the library: every compiled unit once, in link order, with its
kind and what it holds.  Kernel units share device code in csrc/rpe_reduce.hpp and csrc/rpe_residuals.hpp and the front end's
bit-exact rules in csrc/rpe_volume_field.hpp, csrc/rpe_sdf_rule.hpp, csrc/rpe_sdf_robust_rule.hpp, csrc/rpe_mc_rules.hpp and csrc/rpe_feature_rules.hpp; each names one of its kernels
with RPE_PRELOAD (csrc/rpe_kernels.h), through which rpe_create loads its code object.  Host units are the C-ABI side behind
include/rgbd_pose_hip.h Part 2 / 3 (csrc/rpe_host.hpp lists them; csrc/rpe_devbuf.hpp owns their device memory,
csrc/rpe_gn_host.hpp holds the Gauss-Newton step, round loop, level driver and coarse-to-fine walk of their host loops,
csrc/rpe_frontend_host.hpp what the Part 3 units share).  What each unit must satisfy is the gate table of tests/unit_gates.py.

{units}

The units compile in parallel (RPE_BUILD_JOBS, default 6)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "librgbdpose_hip.so")
# (source under csrc/, kind, what it holds).  kind: "kernel" = hipcc, must hold device code; "host" = hipcc, must hold none; "cpp" = g++
UNITS = [
    ("rpe_normal_eq.hip", "kernel", "K1-K3 Gauss-Newton normal equations + the resident form"),
    ("rpe_icp.hip", "kernel", "fused ICP rounds"),
    ("rpe_joint.hip", "kernel", "joint normal equations"),
    ("rpe_score.hip", "kernel", "K4 scoring, K4b masks"),
    ("rpe_nl.hip", "kernel", "K1' moments, K5, publish kernels"),
    ("rpe_frontend.hip", "kernel", "depth-frame front end; the model maps raycast from the map; the volume term's rows and round, on the window and on the map; "
                                   "the keyframe list fused into the map's bricks (csrc/rpe_mapfuse.hpp); the volume colour term's rows and round (csrc/rpe_sdf_photo.hpp), "
                                   "on the window and on the map (csrc/rpe_map_sdf_photo.hpp); the robust rounds of the four volume terms and their weight hook "
                                   "(csrc/rpe_sdf_robust.hpp)"),
    ("rpe_filter.hip", "kernel", "the bilateral depth filter in front of it"),
    ("rpe_volume.hip", "kernel", "TSDF volume: integrate, raycast"),
    ("rpe_mesh.hip", "kernel", "marching cubes over the volume"),
    ("rpe_color.hip", "kernel", "colour of the volume: frame colour, colour integrate, colour sampling"),
    ("rpe_photo.hip", "kernel", "photometric term beside ICP: intensity maps, the RGB-D round"),
    ("rpe_feature.hip", "kernel", "keypoints, descriptors and matches for relocalisation"),
    ("rpe_feature_oriented.hip", "kernel", "the oriented descriptor: moments, angle bin, steered tests"),
    ("rpe_feature_scale.hip", "kernel", "the scale levels: the detector and both descriptors over a ladder of resampled images in one index space"),
    ("rpe_keyframe.hip", "kernel", "the keyframe store: snapshot, the batched match of a frame against every keyframe, count and rank, gather"),
    ("rpe_graph.hip", "kernel", "the keyframe graph: pair lists of keyframe-to-keyframe matches, the joint Gauss-Newton round over every edge, "
                                "the store rewritten at the corrected poses"),
    ("rpe_rebuild.hip", "kernel", "the volume rebuilt from the keyframes: the depth packed beside a keyframe, a list of keyframes fused in one "
                                  "pass over the voxels"),
    ("rpe_register.hip", "kernel", "colour registration: a separate colour camera reprojected onto the depth frame through a z-buffer"),
    ("rpe_shift.hip", "kernel", "the moving volume: the TSDF and colour volume shifted by whole voxels into a spare"),
    ("rpe_archive.hip", "kernel", "the volume archive: which leaving bricks are non-zero, bricks gathered into a pool of slots and scattered back"),
    ("rpe_mapmesh.hip", "kernel", "the map mesh: marching cubes over the listed bricks of the window and the archive, a workgroup per brick"),
    ("rpe_hypotheses.hip", "kernel", "batched hypothesis generation"),
    ("rpe_prosac.hip", "kernel", "PROSAC order: top-k select + sort"),
    ("rpe_context.hip", "host", "context life cycle, resident arrays, the preload walk"),
    ("rpe_receive.hip", "host", "where a launch leaves its result and how the host receives it"),
    ("rpe_capi.hip", "host", "the thin C-ABI shim"),
    ("rpe_refine.hip", "host", "the Gauss-Newton loops"),
    ("rpe_session.hip", "host", "resident scoring sessions"),
    ("rpe_dist.hip", "host", "sharded contexts"),
    ("rpe_frontend_api.hip", "host", "Part 3: depth-frame front end and ICP"),
    ("rpe_volume_api.hip", "host", "Part 3: TSDF volume"),
    ("rpe_mesh_api.hip", "host", "Part 3: mesh extraction"),
    ("rpe_color_api.hip", "host", "Part 3: colour of frame, volume, model and mesh"),
    ("rpe_photo_api.hip", "host", "Part 3: photometric term beside ICP"),
    ("rpe_sdf_api.hip", "host", "Part 3: the volume term, a frame tracked against the TSDF volume itself, and the volume colour term, a photometric term "
                                "against the colour volume beside it; each on the window or on the whole map's volumes"),
    ("rpe_feature_api.hip", "host", "Part 3: features and relocalisation"),
    ("rpe_keyframe_api.hip", "host", "Part 3: keyframes"),
    ("rpe_graph_api.hip", "host", "Part 3: the keyframe graph"),
    ("rpe_rebuild_api.hip", "host", "Part 3: the volume rebuilt from the keyframes"),
    ("rpe_register_api.hip", "host", "Part 3: colour registration"),
    ("rpe_shift_api.hip", "host", "Part 3: the moving volume"),
    ("rpe_archive_api.hip", "host", "Part 3: the volume archive"),
    ("rpe_mapmesh_api.hip", "host", "Part 3: the map: mesh and raycast; the brick grid and the map's field for the calls that track against it"),
    ("rpe_mapfuse_api.hip", "host", "Part 3: the map rebuilt from the keyframes"),
    ("library.cpp", "cpp", "reference-compatible ao / ao_ransac / py2c and the adapter-level pipelines"),
    ("rpe_hostex.cpp", "cpp", "host-side all-reduce between the rank processes of one node"),
]
SOURCES = [src for src, _, _ in UNITS]
__doc__ = (__doc__ or "{units}").format(units="\n".join(f"  csrc/{src} ({kind}): {what}" for src, kind, what in UNITS))
ARCH = "gfx950"
LINK_RT = "--rtlib=libgcc"
# what every kernel unit (and anything that must see the device rules as the kernels do: tests/test_gpu_volume_rules.py) is compiled
# with; FMA contraction is switched off in the sources themselves (#pragma clang fp contract(off)), not here
HIP_FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "--offload-compress"]


def _deps():
    out = []
    for root in (CSRC, os.path.join(PKG, "include"), os.path.join(os.path.dirname(PKG), "include")):
        for d, _, fs in os.walk(root):
            out += [os.path.join(d, f) for f in fs if f.endswith((".hip", ".cpp", ".h", ".hpp"))]
    return out


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > t for p in _deps())


def _run_parallel(cmds, verbose):
    jobs = max(1, int(os.environ.get("RPE_BUILD_JOBS", "6")))
    running = []
    def reap(block):
        for p, c in list(running):
            rc = p.wait() if block else p.poll()
            if rc is None:
                continue
            running.remove((p, c))
            if rc != 0:
                for q, _ in running:
                    q.kill()
                raise subprocess.CalledProcessError(rc, c)
    for cmd in cmds:
        while len(running) >= jobs:
            reap(False)
            if len(running) >= jobs:
                import time
                time.sleep(0.05)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        running.append((subprocess.Popen(cmd), cmd))
    while running:
        reap(True)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: the HIP backend cannot be built (there is no CPU fallback)")
    os.makedirs(LIBDIR, exist_ok=True)
    objs, cmds = [], []
    for src in SOURCES:
        obj = os.path.join(LIBDIR, os.path.splitext(src)[0] + ".o")
        if src.endswith(".cpp"):
            # pure host code over the C ABI (the drop-in headers, ao / ao_ransac / rpe_run): the host C++ compiler, IEEE arithmetic
            # without contraction -- the minimal solvers in pose/*.hpp evaluate the reference's expressions operation by operation
            cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-c", os.path.join(CSRC, src), "-o", obj]
        else:
            # --offload-compress: the gfx950 code objects are stored compressed in the fat binary (a third of the size; the runtime
            # unpacks a unit once, when its first kernel is looked up -- rpe_create touches every unit)
            cmd = [hipcc, *HIP_FLAGS,
                   "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        if not force and os.path.exists(obj) and all(os.path.getmtime(p) <= os.path.getmtime(obj) for p in _deps()):
            objs.append(obj)   # this unit is newer than every source and header: keep it
            continue
        cmds.append(cmd)
        objs.append(obj)
    _run_parallel(cmds, verbose)
    # --rtlib=libgcc: the complex multiply / divide helpers (__divdc3 ...) that std::complex code in the P3P solver calls must be the
    # host toolchain's (libgcc), as in any g++-built caller of the headers; clang's compiler-rt copies round differently
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", LINK_RT, "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return LIB


def build_stamps(level: int = 1, verbose: bool = False) -> str:
    """DIAGNOSTIC build (never loaded by the product): the same library with -DRPE_STAMPS=<level>, whose reduction kernels stamp the
    100 MHz clock at their phase boundaries (scripts/tail_timeline.py).  Only rpe_normal_eq.hip is recompiled.  The outputs are
    The stamps libraries are scratch: build them right before the diagnostic run and delete them after (they are never loaded by
    the product and should not ride along with every push to the GPU box)."""
    build()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(LIBDIR, f"librgbdpose_hip_stamps{level}.so")
    obj = os.path.join(LIBDIR, f"rpe_normal_eq_stamps{level}.o")
    if os.path.exists(out) and all(os.path.getmtime(p) <= os.path.getmtime(out) for p in _deps()):
        return out
    cmd = [hipcc, *HIP_FLAGS, f"-DRPE_STAMPS={level}",
           "-x", "hip", "-c", os.path.join(CSRC, "rpe_normal_eq.hip"), "-o", obj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    objs = [obj] + [os.path.join(LIBDIR, os.path.splitext(src)[0] + ".o") for src in SOURCES if src != "rpe_normal_eq.hip"]
    subprocess.check_call([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", LINK_RT, "-o", out] + objs)
    return out


def build_score_stats(verbose: bool = False) -> str:
    """DIAGNOSTIC build (never loaded by the product): the library with -DRPE_SCORE_STATS, whose exact 2D vote counts how often a wave
    falls through its band filter (scripts/score_filter_stats.py).  Only rpe_score.hip is recompiled; scratch, like the stamps builds."""
    build()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out, obj = os.path.join(LIBDIR, "librgbdpose_hip_scorestats.so"), os.path.join(LIBDIR, "rpe_score_stats.o")
    cmd = [hipcc, *HIP_FLAGS, "-DRPE_SCORE_STATS",
           "-x", "hip", "-c", os.path.join(CSRC, "rpe_score.hip"), "-o", obj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    objs = [obj] + [os.path.join(LIBDIR, os.path.splitext(src)[0] + ".o") for src in SOURCES if src != "rpe_score.hip"]
    subprocess.check_call([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", LINK_RT, "-o", out] + objs)
    return out


EXAMPLES = ["simple_main", "test_main", "icp_main", "engine_profile", "gn_refine_main"]


def build_examples(verbose: bool = False) -> list[str]:
    """The reference's two demo drivers rebuilt on the drop-in headers: plain g++, linking only the C ABI."""
    root = os.path.dirname(PKG)
    outs = []
    for ex in EXAMPLES:
        src, out = os.path.join(root, "examples", ex + ".cpp"), os.path.join(root, "examples", ex)
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(PKG, "include", "pose"), "-I", os.path.join(PKG, "include"),
               src, "-L", LIBDIR, "-lrgbdpose_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,$ORIGIN/../rgbd_pose_estimation_amd/lib", "-o", out]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
        outs.append(out)
    return outs


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    if "--examples" in sys.argv:
        print(build_examples(verbose=True))
