"""The map volume term on one GPU beside the routes the parent has, one run: host wall around a synchronise,
medians of interleaved rounds AFTER the routes' poses have been compared.
  (a) windows of N^3 over the room fused from four views, N = 256 and 512, a 640 x 480 frame tracked over three levels, nothing
      archived, box = the window: "window" icp_pyramid_sdf against "map" icp_pyramid_map_sdf -- the price of the sparse route where it
      buys nothing (the rows are bit-equal, the poses agree to rounding)
  (b) the final map of the walk of tests/archive_cases.py (64^3 window, 507 bricks held, bounds 136 x 64 x 64), the last frame of the
      walk at 160 x 120 and at 640 x 480 tracked from an offset pose: "map" icp_pyramid_map_sdf against "raycast" volume_map_raycast(levels=3)
      + icp_pyramid, the only route to the same surfaces before; "window" icp_pyramid_sdf for scale (it sees fewer rows)
  (c) the brick grid's build and upload alone: one-round calls on a 16 x 12 frame, whose kernel time is nothing -- map form minus
      window form, for the three maps above (32^3, 64^3 and 17 x 8 x 8 bricks)
  (d) the two kernels' own times: a separate `rocprofv3 --kernel-trace --stats -- python scripts/mapsdf_time.py --kernels` run, merged
      with `python scripts/mapsdf_time.py --kernel-stats kernel_stats.csv out.json`
Prints one JSON line and writes it to argv[1] (default profiles/mapsdf_time_640.json)."""
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)
TINY = (14.625, 14.625, 8.0, 6.0, 16, 12)
RANGE = (0.1, 10.0, 0.1)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
LEVELS, ITERS, GATES, COS = 3, (6, 4, 3), (0.1, 0.15, 0.2), 0.8
DEFAULT_OUT = os.path.join(ROOT, "profiles", "mapsdf_time_640.json")


def timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter_ns()
    f()
    ctx.synchronize()
    return (time.perf_counter_ns() - t0) / 1e3


def interleaved(ctx, routes, reps, warm=3):
    """{name: median and quartiles}: the calls alternated, so that all see the same state of the machine"""
    for _ in range(warm):
        for f in routes.values():
            f()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t[k].append(timed(ctx, f))
    return {k: {"median_us": round(statistics.median(v), 2), "quartiles_us": [round(x, 2) for x in statistics.quantiles(v, n=4)]}
            for k, v in t.items()}


def grid_alone(ctx, pose, reps):
    """(c): the caller has set the tiny frame"""
    r = interleaved(ctx, {"window_one_round": lambda: ctx.sdf_normal_eq(pose, 0, 0.1, COS),
                          "map_one_round": lambda: ctx.map_sdf_normal_eq(pose, 0, 0.1, COS)}, reps)
    lo, hi = ctx.volume_map_bounds()
    r["bricks"] = int(((hi - lo) // 8).prod())
    r["grid_us"] = round(r["map_one_round"]["median_us"] - r["window_one_round"]["median_us"], 2)
    return r


def merge_kernel_stats(stats_csv, out_json):
    out = json.load(open(out_json))
    want = {"icp_map_sdf_kernel", "map_sdf_rows_kernel", "icp_sdf_kernel", "sdf_rows_kernel", "map_raycast_kernel", "icp_fused_kernel"}
    for row in csv.DictReader(open(stats_csv)):
        m = re.search(r"(\w+_kernel)(<[^>]*>)?", row["Name"])
        if m and m.group(1) in want:
            out.setdefault("kernels_us", {})[m.group(0)] = {
                "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    line = json.dumps(out)
    print(line)
    open(out_json, "w").write(line + "\n")


def main():
    import numpy as np
    import archive_cases as AC
    import sdf_cases as SDC
    import shift_cases as SC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import _lib as L, api
    kernels = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
    reps = 4 if kernels else 20
    out = {"cam": list(CAM), "levels": LEVELS, "iters": list(ITERS), "gates": list(GATES), "cos_thr": COS, "reps": reps}
    ctx = api.Context(0)
    truth = VC.held_out_pose()
    start = SDC.moved(truth, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)    # a frame-to-frame step: 2 cm, 5 mrad
    views = [(VC.view(k), VC.depth_at(VC.view(k), CAM)) for k in VC.ACC_VIEWS]
    frame = VC.depth_at(truth, CAM)
    tiny = VC.depth_at(truth, TINY)
    # ---- (a) and (c) on full room windows
    for nv in (256,) if kernels else (256, 512):
        s = SIDE / nv
        ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
        for p, d in views:
            ctx.frame_set_depth(d, CAM, 1.0, *RANGE, levels=LEVELS)
            ctx.volume_integrate(p)
        ctx.frame_set_depth(frame, CAM, 1.0, *RANGE, levels=LEVELS)
        box = ctx.volume_map_bounds()
        window = lambda: ctx.icp_pyramid_sdf(start, ITERS, GATES, 1e-6, COS)            # noqa: E731
        sparse = lambda: ctx.icp_pyramid_map_sdf(start, ITERS, GATES, 1e-6, COS, box=box)   # noqa: E731
        pw, pm = window(), sparse()
        res = {"voxel_m": s, "start_error": list(VC.pose_error(start, truth)), "window_error": list(VC.pose_error(pw[0], truth)),
               "map_error": list(VC.pose_error(pm[0], truth)), "pose_difference": float(np.abs(pw[0] - pm[0]).max()),
               "rounds": [list(pw[1]), list(pm[1])], "rows": [int(pw[4]), int(pm[4])]}
        assert np.abs(pw[0] - pm[0]).max() < 1e-6 and abs(pw[4] - pm[4]) <= 2 + 1e-4 * pw[4], (pw, pm)
        assert np.array_equal(np.isnan(ctx.sdf_rows(truth)), np.isnan(ctx.map_sdf_rows(truth, box=box)))
        res["frame"] = interleaved(ctx, {"window": window, "map": sparse}, reps)
        res["map_over_window"] = round(res["frame"]["map"]["median_us"] / res["frame"]["window"]["median_us"], 3)
        res["one_round"] = interleaved(ctx, {"window": lambda: ctx.icp_sdf(start, 1, 0.0, GATES[0], COS),
                                             "map": lambda: ctx.icp_map_sdf(start, 1, 0.0, GATES[0], COS, box=box)}, reps)
        ctx.frame_set_depth(tiny, TINY, 1.0, *RANGE)
        res["grid"] = grid_alone(ctx, truth, reps)
        out["vol%d" % nv] = res
    # ---- (b) and (c) on the walk's map
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(AC.CAPACITY)
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = ctx.volume_follow(p, SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(p)
    last = AC.pose(len(AC.PATH) - 1)
    off = SDC.moved(last, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)
    lo, hi = ctx.volume_map_bounds()
    out["walk"] = {"held": ctx.volume_archive_info()["held"], "box": [int(x) for x in hi - lo]}
    for cam, tag in ((AC.CAM, "160"), (CAM, "640")):
        ctx.frame_set_depth(VC.depth_at(last, cam), cam, 1.0, *SC.RANGE, levels=LEVELS)

        def raycast_route():
            ctx.volume_map_raycast(off, cam, *SC.RAY, levels=LEVELS)
            return ctx.icp_pyramid(off, ITERS, GATES, L.RES_P2PLANE, 1e-6, COS, fused=True)
        map_route = lambda: ctx.icp_pyramid_map_sdf(off, ITERS, GATES, 1e-6, COS)        # noqa: E731
        window_route = lambda: ctx.icp_pyramid_sdf(off, ITERS, GATES, 1e-6, COS)         # noqa: E731
        pr, pm, pw = raycast_route(), map_route(), window_route()
        res = {"start_error": list(VC.pose_error(off, last)), "raycast_error": list(VC.pose_error(pr[0], last)),
               "map_error": list(VC.pose_error(pm[0], last)), "window_error": list(VC.pose_error(pw[0], last)),
               "pairs_or_rows": {"raycast": int(pr[4]), "map": int(pm[4]), "window": int(pw[4])},
               "rounds": {"raycast": list(pr[1]), "map": list(pm[1]), "window": list(pw[1])}}
        res["frame"] = interleaved(ctx, {"map": map_route, "raycast": raycast_route, "window": window_route}, reps)
        res["map_over_raycast"] = round(res["frame"]["map"]["median_us"] / res["frame"]["raycast"]["median_us"], 3)
        if kernels:
            ctx.map_sdf_rows(last)
        out["walk"][tag] = res
    ctx.frame_set_depth(VC.depth_at(last, TINY), TINY, 1.0, *SC.RANGE)
    out["walk"]["grid"] = grid_alone(ctx, last, reps)
    ctx.close()
    if kernels:
        return 0
    line = json.dumps(out)
    print(line)
    with open(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel-stats":
        merge_kernel_stats(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT)
    else:
        sys.exit(main())
