"""The map volume colour term on one GPU beside the routes the parent has, one run: host wall around a
synchronise, medians of interleaved calls AFTER the routes' poses have been compared.
  (a) where the sparse route buys nothing: windows of N^3 over the room fused WITH colour from four views, N = 256 and 512, a 640 x 480
      frame tracked over three levels, nothing archived, box = the window: "window" icp_pyramid_sdf_rgbd against "map"
      icp_pyramid_map_sdf_rgbd (the rows are bit-equal, the poses agree to rounding)
  (b) on a walked map with colour -- the wall walk of tests/mapsdf_photo_cases.py (64^3 window, 470 bricks held), the frame of its
      middle evaluated position at 160 x 120 and at 640 x 480 from an offset pose: "map_rgbd" icp_pyramid_map_sdf_rgbd against "raycast_rgbd"
      volume_map_raycast(levels=3, color=True) + photo_prepare + icp_pyramid_rgbd, the only route to the same result before, and
      against "map_sdf" icp_pyramid_map_sdf without colour
  (c) one round per call at level 0 for the forms above; the kernels' own times come from a separate
      `rocprofv3 --kernel-trace --stats -- python scripts/mapsdf_photo_time.py --kernels` run, merged with
      `python scripts/mapsdf_photo_time.py --kernel-stats kernel_stats.csv out.json`
What is slower is reported as SLOWER.  Prints one JSON line and writes it to argv[1] (default profiles/mapsdf_photo_time_640.json)."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from mapsdf_time import CAM, COS, GATES, ITERS, LEVELS, ORIGIN, RANGE, SIDE, interleaved  # noqa: E402

WEIGHT = 0.01
RAY = (0.1, 7.0)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "mapsdf_photo_time_640.json")
WANT = {"icp_map_sdf_photo_kernel", "map_sdf_photo_rows_kernel", "icp_sdf_photo_kernel", "icp_map_sdf_kernel", "map_raycast_kernel",
        "icp_photo_kernel", "frame_intensity_kernel"}


def verdict(new_us, old_us):
    """"1.23x faster" / "SLOWER x1.23": the new route against the other"""
    return "%.2fx faster" % (old_us / new_us) if new_us <= old_us else "SLOWER x%.2f" % (new_us / old_us)


def merge_kernel_stats(stats_csv, out_json):
    out = json.load(open(out_json))
    for row in csv.DictReader(open(stats_csv)):
        m = re.search(r"(\w+_kernel)(<[^>]*>)?", row["Name"])
        if m and m.group(1) in WANT:
            out.setdefault("kernels_us", {})[m.group(0)] = {
                "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    line = json.dumps(out)
    print(line)
    open(out_json, "w").write(line + "\n")


def main():
    import numpy as np
    import mapsdf_photo_cases as MPC
    import photo_cases as PC
    import sdf_cases as SDC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import api
    kernels = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
    reps = 4 if kernels else 20
    out = {"cam": list(CAM), "levels": LEVELS, "iters": list(ITERS), "gates": list(GATES), "cos_thr": COS, "weight": WEIGHT, "reps": reps}
    ctx = api.Context(0)
    truth = VC.held_out_pose()
    start = SDC.moved(truth, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)    # a frame-to-frame step: 2 cm, 5 mrad
    views = [(VC.view(k), VC.depth_at(VC.view(k), CAM), PC.rgb_at(VC.view(k), CAM, None)) for k in VC.ACC_VIEWS]
    frame, rgb = VC.depth_at(truth, CAM), PC.rgb_at(truth, CAM, None)
    # ---- (a) full room windows, nothing archived
    for nv in (256,) if kernels else (256, 512):
        s = SIDE / nv
        ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
        for p, d, c in views:
            ctx.frame_set_depth(d, CAM, 1.0, *RANGE, levels=LEVELS)
            ctx.frame_set_color(c)
            ctx.volume_integrate_color(p)
        ctx.frame_set_depth(frame, CAM, 1.0, *RANGE, levels=LEVELS)
        ctx.frame_set_color(rgb)
        box = ctx.volume_map_bounds()
        window = lambda: ctx.icp_pyramid_sdf_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS)                 # noqa: E731
        sparse = lambda: ctx.icp_pyramid_map_sdf_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS, box=box)    # noqa: E731
        pw, pm = window(), sparse()
        res = {"voxel_m": s, "start_error": list(VC.pose_error(start, truth)), "window_error": list(VC.pose_error(pw[0], truth)),
               "map_error": list(VC.pose_error(pm[0], truth)), "pose_difference": float(np.abs(pw[0] - pm[0]).max()),
               "rounds": [list(pw[1]), list(pm[1])], "rows": [[int(pw[4]), int(pw[6])], [int(pm[4]), int(pm[6])]]}
        assert np.abs(pw[0] - pm[0]).max() < 1e-5 and abs(pw[6] - pm[6]) <= 2 + 1e-4 * pw[6], (pw, pm)
        a, b = ctx.sdf_photo_rows(truth), ctx.map_sdf_photo_rows(truth, box=box)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
        res["frame"] = interleaved(ctx, {"window": window, "map": sparse}, reps)
        res["map_against_window"] = verdict(res["frame"]["map"]["median_us"], res["frame"]["window"]["median_us"])
        res["one_round"] = interleaved(ctx, {"window": lambda: ctx.icp_sdf_rgbd(start, WEIGHT, 1, 0.0, GATES[0], COS),
                                             "map": lambda: ctx.icp_map_sdf_rgbd(start, WEIGHT, 1, 0.0, GATES[0], COS, box=box)}, reps)
        res["one_round_map_against_window"] = verdict(res["one_round"]["map"]["median_us"], res["one_round"]["window"]["median_us"])
        out["vol%d" % nv] = res
    # ---- (b) the wall walk's map, with colour
    ctx.volume_init(MPC.WALK_DIMS, **MPC.WALK_KW)
    ctx.volume_archive(1024)
    for n in range(MPC.WALK_FRAMES):
        if n:
            ctx.volume_shift((MPC.WALK_STEP, 0, 0))
        d, c = MPC.walk_frame(MPC.walk_pose(n), n)
        ctx.frame_set_depth(d, MPC.WALK_CAM, 1.0, *RANGE)
        ctx.frame_set_color(c)
        ctx.volume_integrate_color(MPC.walk_pose(n))
    at = MPC.walk_eval_pose(1)
    off = MPC.walk_start(1)
    lo, hi = ctx.volume_map_bounds()
    out["walk"] = {"held": ctx.volume_archive_info()["held"], "box": [int(x) for x in hi - lo]}
    for cam, tag in ((MPC.WALK_CAM, "160"), (CAM, "640")):
        ctx.frame_set_depth(PC.depth_at(at, cam, PC.WALL), cam, 1.0, *RANGE, levels=LEVELS)
        ctx.frame_set_color(PC.rgb_at(at, cam, PC.WALL))

        def raycast_rgbd():
            ctx.volume_map_raycast(off, cam, *RAY, levels=LEVELS, color=True)
            ctx.photo_prepare(LEVELS)
            return ctx.icp_pyramid_rgbd(off, WEIGHT, ITERS, GATES, 1e-6, COS)
        map_rgbd = lambda: ctx.icp_pyramid_map_sdf_rgbd(off, WEIGHT, ITERS, GATES, 1e-6, COS)    # noqa: E731
        map_sdf = lambda: ctx.icp_pyramid_map_sdf(off, ITERS, GATES, 1e-6, COS)                  # noqa: E731
        pr, pm, pg = raycast_rgbd(), map_rgbd(), map_sdf()
        res = {"start_error": list(VC.pose_error(off, at)), "raycast_rgbd_error": list(VC.pose_error(pr[0], at)),
               "map_rgbd_error": list(VC.pose_error(pm[0], at)), "map_sdf_error": list(VC.pose_error(pg[0], at)),
               "pairs_or_rows": {"raycast_rgbd": [int(pr[4]), int(pr[6])], "map_rgbd": [int(pm[4]), int(pm[6])], "map_sdf": int(pg[4])},
               "rounds": {"raycast_rgbd": list(pr[1]), "map_rgbd": list(pm[1]), "map_sdf": list(pg[1])}}
        res["frame"] = interleaved(ctx, {"map_rgbd": map_rgbd, "raycast_rgbd": raycast_rgbd, "map_sdf": map_sdf}, reps)
        f = res["frame"]
        res["map_rgbd_against_raycast_rgbd"] = verdict(f["map_rgbd"]["median_us"], f["raycast_rgbd"]["median_us"])
        res["map_rgbd_against_map_sdf"] = verdict(f["map_rgbd"]["median_us"], f["map_sdf"]["median_us"])
        res["one_round"] = interleaved(ctx, {"map_rgbd": lambda: ctx.icp_map_sdf_rgbd(off, WEIGHT, 1, 0.0, GATES[0], COS),
                                             "map_sdf": lambda: ctx.icp_map_sdf(off, 1, 0.0, GATES[0], COS),
                                             "window_rgbd": lambda: ctx.icp_sdf_rgbd(off, WEIGHT, 1, 0.0, GATES[0], COS)}, reps)
        if kernels:
            ctx.map_sdf_photo_rows(at)
            ctx.map_sdf_photo_normal_eq(at)
        out["walk"][tag] = res
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
