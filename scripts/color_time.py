"""Colour of the TSDF volume at 640 x 480: host wall medians of rpe_volume_integrate_color against
rpe_volume_integrate in volumes of 256^3 and 512^3 over the textured room (the sizes of scripts/volume_time.py), the colour bytes moved,
rpe_frame_set_color, rpe_model_sample_color on the 640 x 480 raycast model, rpe_volume_mesh_colors on the room's meshes against
rpe_volume_mesh, and one frame of the tracking loop with and without the colour upload + colour integrate.  Prints one JSON line (and
writes it to argv[1] when given).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` with RPE_COLOR_KERNELS_ONLY=1 (a
short pass of each call)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import color_cases as CC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
RAY = (0.1, 7.0)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def main():
    short = os.environ.get("RPE_COLOR_KERNELS_ONLY") == "1"
    reps = 5 if short else 30
    ctx = api.Context(0)
    lib, h = L.lib(), ctx._h
    out = {"cam": list(CAM)}
    p0 = VC.view(0)
    depth, rgb = VC.depth_at(p0, CAM), CC.rgb_at(p0, CAM)
    ctx.frame_set_depth(depth, CAM, 1.0, *RANGE)
    ctx.frame_set_color(rgb)
    ctx.synchronize()

    def set_color():
        ctx.frame_set_color(rgb); ctx.synchronize()
    out["set_color_us"] = timed(set_color, reps)
    for n in (256, 512):
        s = SIDE / n
        ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
        ctx.volume_integrate_color(p0)
        ctx.synchronize()
        vol = ctx.volume_download()
        cvol = ctx.volume_color_download()
        updated, band = int((vol[..., 1] > 0).sum()), int((cvol[..., 3] > 0).sum())
        del vol, cvol

        def integrate():
            ctx.volume_integrate(p0); ctx.synchronize()

        def integrate_color():
            ctx.volume_integrate_color(p0); ctx.synchronize()

        def raycast():
            ctx.volume_raycast(p0, CAM, *RAY); ctx.synchronize()

        def sample():
            L.check(lib.rpe_model_sample_color(h)); ctx.synchronize()
        a, b = [], []
        for _ in range(reps):                      # alternated, so that both see the same state of the machine
            a.append(timed(integrate, 1)); b.append(timed(integrate_color, 1))
        raycast()
        r = {"voxel_m": s, "updated_voxels": updated, "band_voxels": band,
             "colour_bytes": {"band_pairs": band * 16, "frame_colour": band * 4, "total": band * 20},
             "integrate_us": statistics.median(a), "integrate_color_us": statistics.median(b),
             "raycast_us": timed(raycast, reps), "model_color_us": timed(sample, reps)}
        r["integrate_color_ratio"] = r["integrate_color_us"] / r["integrate_us"]
        nv = [0]

        def mesh():
            nv[0] = len(ctx.volume_mesh()[0])

        def mesh_colors():
            ctx.volume_mesh_colors()
        r["mesh_us"] = timed(mesh, max(3, reps // 3))
        r["mesh_vertices"] = nv[0]
        r["mesh_colors_us"] = timed(mesh_colors, reps)
        r["mesh_colors_share"] = r["mesh_colors_us"] / r["mesh_us"]
        out[f"vol{n}"] = r
    # the tracking loop at 640 x 480, 256^3, host wall per stage (medians over the frames), without and with colour
    n = 256
    s = SIDE / n
    depths = VC.track_depths(CAM)
    rgbs = [CC.rgb_at(VC.track_pose(f), CAM) for f in range(VC.TRACK_FRAMES)]
    levels = len(VC.TRACK_ITERS)
    for colour in (False, True):
        ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
        est = VC.track_pose(0)
        ctx.frame_set_depth(depths[0], CAM, 1.0, *RANGE, levels=levels)
        if colour:
            ctx.frame_set_color(rgbs[0]); ctx.volume_integrate_color(est)
        else:
            ctx.volume_integrate(est)
        ctx.synchronize()
        st = {"set_depth_pyramid": [], "set_color": [], "raycast_and_model_pyramid": [], "icp_pyramid": [], "integrate": []}
        for f in range(1, VC.TRACK_FRAMES):
            t = [time.perf_counter_ns()]
            ctx.frame_set_depth(depths[f], CAM, 1.0, *RANGE, levels=levels); ctx.synchronize(); t.append(time.perf_counter_ns())
            if colour:
                ctx.frame_set_color(rgbs[f]); ctx.synchronize()
            t.append(time.perf_counter_ns())
            ctx.volume_raycast(est, CAM, *RAY, levels=levels); ctx.synchronize(); t.append(time.perf_counter_ns())
            est = ctx.icp_pyramid(est, VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)[0]; t.append(time.perf_counter_ns())
            if colour:
                ctx.volume_integrate_color(est)
            else:
                ctx.volume_integrate(est)
            ctx.synchronize(); t.append(time.perf_counter_ns())
            for k, a, b in zip(st, t, t[1:]):
                st[k].append((b - a) / 1e3)
        key = "track640_vol256_color_us" if colour else "track640_vol256_us"
        out[key] = {k: statistics.median(v) for k, v in st.items()}
        out[key]["frame"] = sum(out[key].values())
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
