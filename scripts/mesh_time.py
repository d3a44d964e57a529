"""Mesh extraction at 640 x 480: host wall time of rpe_volume_mesh (extraction, ending in a device synchronise)
and of rpe_volume_mesh_download in volumes of 256^3 and 512^3 over the room of simulator.default_room() fused from three frames, and a
worst case: an uploaded 256^3 noise volume with every cube active.  Prints one JSON line (and writes it to argv[1] when given).  Kernel
times: run it under `rocprofv3 --kernel-trace --stats` with RPE_MESH_KERNELS_ONLY=1 (a short pass of each call)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
# a cube over the room [-2.5, 2.7] x [-1.6, 1.5] x [-1.0, 5.0]: 6.4 m on a side (as scripts/volume_time.py)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4
HBM_PEAK = 8.0e12   # bytes/s, MI355X spec


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def measure(ctx, n, reps, min_weight=1.0):
    lib = L.lib()
    nv, nt = C.c_int64(0), C.c_int64(0)

    def extract():
        L.check(lib.rpe_volume_mesh(ctx._h, float(min_weight), C.byref(nv), C.byref(nt))); ctx.synchronize()
    extract()
    V = np.empty((nv.value, 3), np.float32); N = np.empty_like(V); T = np.empty((nt.value, 3), np.int32)

    def download():
        L.check(lib.rpe_volume_mesh_download(ctx._h, V.ctypes.data_as(C.c_void_p), N.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)))
    download()
    vox = n ** 3
    # classify must read every voxel once (8 bytes); the rest of the workspace is <= 6 bytes per voxel written and read
    out = {"voxels": vox, "vertices": nv.value, "triangles": nt.value, "mesh_us": timed(extract, reps), "download_us": timed(download, reps),
           "mesh_bytes": int(V.nbytes + N.nbytes + T.nbytes), "classify_read_bytes": 8 * vox,
           "classify_hbm_floor_us": 8 * vox / HBM_PEAK * 1e6}
    return out


def main():
    short = os.environ.get("RPE_MESH_KERNELS_ONLY") == "1"
    reps = 3 if short else 20
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    for n in (256, 512):
        s = SIDE / n
        ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
        for k in (0, 1, 2):
            ctx.frame_set_depth(VC.depth_at(VC.view(k), CAM), CAM, 1.0, *RANGE)
            ctx.volume_integrate(VC.view(k))
        ctx.synchronize()
        out[f"room{n}"] = dict(voxel_m=s, **measure(ctx, n, reps))
    # worst case: every cube active, tsdf signs at random (about half of all edges crossed)
    n = 256
    rng = np.random.default_rng(1)
    vol = np.empty((n, n, n, 2), np.float32)
    vol[..., 0] = rng.uniform(-1, 1, (n, n, n)).astype(np.float32)
    vol[..., 1] = 1.0
    ctx.volume_init((n, n, n), SIDE / n, ORIGIN, 3 * SIDE / n, 64)
    ctx.volume_upload(vol)
    del vol
    out[f"noise{n}"] = measure(ctx, n, max(3, reps // 4))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
