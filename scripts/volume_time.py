"""TSDF volume at 640 x 480: host wall time of rpe_volume_integrate and rpe_volume_raycast in volumes of 256^3 and
512^3 over the room of simulator.default_room(), and of one frame of the tracking loop split by stage (set_depth_pyramid, raycast +
model pyramid, icp_pyramid, integrate).  Prints one JSON line (and writes it to argv[1] when given).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` with RPE_VOL_KERNELS_ONLY=1 (a short pass of each call)."""
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
RAY = (0.1, 7.0)
# a cube over the room [-2.5, 2.7] x [-1.6, 1.5] x [-1.0, 5.0]: 6.4 m on a side
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def main():
    short = os.environ.get("RPE_VOL_KERNELS_ONLY") == "1"
    reps = 5 if short else 30
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    p0 = VC.view(0)
    depth = VC.depth_at(p0, CAM)
    ctx.frame_set_depth(depth, CAM, 1.0, *RANGE)
    for n in (256, 512):
        s = SIDE / n
        ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
        ctx.synchronize()

        def integrate():
            ctx.volume_integrate(p0); ctx.synchronize()

        def raycast():
            ctx.volume_raycast(p0, CAM, *RAY); ctx.synchronize()
        integrate()
        vol = ctx.volume_download()
        updated = int((vol[..., 1] > 0).sum())
        raycast()
        hits = float((~np.isnan(ctx.frame_download(L.MAP_MODEL_VERTEX)).any(1)).mean())
        out[f"vol{n}"] = {"voxel_m": s, "bytes": n ** 3 * 8, "updated_voxels": updated, "integrate_us": timed(integrate, reps),
                          "raycast_us": timed(raycast, reps), "raycast_hit_fraction": hits,
                          "samples_per_ray_max": int((RAY[1] - RAY[0]) / s)}
        del vol
    # the tracking loop at 640 x 480, 256^3, host wall per stage (medians over the frames)
    n = 256
    s = SIDE / n
    depths = VC.track_depths(CAM)
    levels = len(VC.TRACK_ITERS)
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
    est = VC.track_pose(0)
    ctx.frame_set_depth(depths[0], CAM, 1.0, *RANGE, levels=levels)
    ctx.volume_integrate(est)
    ctx.synchronize()
    st = {"set_depth_pyramid": [], "raycast_and_model_pyramid": [], "icp_pyramid": [], "integrate": []}
    for f in range(1, VC.TRACK_FRAMES):
        t = [time.perf_counter_ns()]
        ctx.frame_set_depth(depths[f], CAM, 1.0, *RANGE, levels=levels); ctx.synchronize(); t.append(time.perf_counter_ns())
        ctx.volume_raycast(est, CAM, *RAY, levels=levels); ctx.synchronize(); t.append(time.perf_counter_ns())
        est = ctx.icp_pyramid(est, VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)[0]; t.append(time.perf_counter_ns())
        ctx.volume_integrate(est); ctx.synchronize(); t.append(time.perf_counter_ns())
        for k, a, b in zip(st, t, t[1:]):
            st[k].append((b - a) / 1e3)
    out["track640_vol256_us"] = {k: statistics.median(v) for k, v in st.items()}
    out["track640_vol256_us"]["frame"] = sum(out["track640_vol256_us"].values())
    out["track640_final_error"] = VC.pose_error(est, VC.track_pose(VC.TRACK_FRAMES - 1))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
