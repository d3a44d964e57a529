"""The robust volume terms on one GPU beside the unweighted routes, one run: host wall around a synchronise,
medians of interleaved calls AFTER the routes' poses have been compared.  A 256^3 window over the room fused WITH colour from four
views, a 640 x 480 frame tracked over three levels from a frame-to-frame step, nothing archived (the map forms read the window through
the brick grid).  For each of the four forms -- window, map, window with colour, map with colour -- the weight off / Huber / Tukey:
  frame      the coarse-to-fine loop of the form
  one_round  one round per call at level 0
Each robust figure is measured against the SAME run's off route of its form; what is slower is reported as SLOWER.  The kernels' own
times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/sdf_robust_time.py --kernels` run, merged with
`python scripts/sdf_robust_time.py --kernel-stats kernel_stats.csv out.json`.  Prints one JSON line and writes it to argv[1]
(default profiles/sdf_robust_time_640.json)."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from mapsdf_time import CAM, COS, GATES, ITERS, LEVELS, ORIGIN, RANGE, SIDE, interleaved  # noqa: E402

WEIGHT = 0.01
NV = 256
SETTINGS = {"off": (0, 0.0, 0.0), "huber": (1, 0.01, 5.0), "tukey": (3, 0.05, 25.0)}       # (kind, k [m], photo_k [levels])
DEFAULT_OUT = os.path.join(ROOT, "profiles", "sdf_robust_time_640.json")
WANT = {"icp_sdf_kernel", "icp_map_sdf_kernel", "icp_sdf_photo_kernel", "icp_map_sdf_photo_kernel", "icp_sdf_robust_kernel",
        "icp_map_sdf_robust_kernel", "icp_sdf_photo_robust_kernel", "icp_map_sdf_photo_robust_kernel", "sdf_robust_weights_kernel"}


def verdict(new_us, old_us):
    """"1.23x faster" / "SLOWER x1.23": the robust route against the off route"""
    return "%.3fx faster" % (old_us / new_us) if new_us <= old_us else "SLOWER x%.3f" % (new_us / old_us)


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
    import photo_cases as PC
    import sdf_cases as SDC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import api
    kernels = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
    reps = 4 if kernels else 20
    s = SIDE / NV
    out = {"cam": list(CAM), "levels": LEVELS, "iters": list(ITERS), "gates": list(GATES), "cos_thr": COS, "weight": WEIGHT, "reps": reps,
           "volume": NV, "voxel_m": s, "settings": {k: list(v) for k, v in SETTINGS.items()}}
    ctx = api.Context(0)
    truth = VC.held_out_pose()
    start = SDC.moved(truth, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)    # a frame-to-frame step: 2 cm, 5 mrad
    ctx.volume_init((NV, NV, NV), s, ORIGIN, 3 * s, 64)
    for k in VC.ACC_VIEWS:
        ctx.frame_set_depth(VC.depth_at(VC.view(k), CAM), CAM, 1.0, *RANGE, levels=LEVELS)
        ctx.frame_set_color(PC.rgb_at(VC.view(k), CAM, None))
        ctx.volume_integrate_color(VC.view(k))
    ctx.frame_set_depth(VC.depth_at(truth, CAM), CAM, 1.0, *RANGE, levels=LEVELS)
    ctx.frame_set_color(PC.rgb_at(truth, CAM, None))
    box = ctx.volume_map_bounds()
    forms = {
        "window": (lambda: ctx.icp_pyramid_sdf(start, ITERS, GATES, 1e-6, COS), lambda: ctx.icp_sdf(start, 1, 0.0, GATES[0], COS)),
        "map": (lambda: ctx.icp_pyramid_map_sdf(start, ITERS, GATES, 1e-6, COS, box=box),
                lambda: ctx.icp_map_sdf(start, 1, 0.0, GATES[0], COS, box=box)),
        "window_colour": (lambda: ctx.icp_pyramid_sdf_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS),
                          lambda: ctx.icp_sdf_rgbd(start, WEIGHT, 1, 0.0, GATES[0], COS)),
        "map_colour": (lambda: ctx.icp_pyramid_map_sdf_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS, box=box),
                       lambda: ctx.icp_map_sdf_rgbd(start, WEIGHT, 1, 0.0, GATES[0], COS, box=box)),
    }

    def under(setting, call):
        def run():
            ctx.sdf_set_robust(*SETTINGS[setting])      # (a host-side store: no launch, no wait)
            return call()
        return run
    out["start_error"] = list(VC.pose_error(start, truth))
    for form, (frame, one) in forms.items():
        res = {"end_error": {}, "rounds": {}, "rows": {}}
        for setting in SETTINGS:                        # the routes' poses first
            p = under(setting, frame)()
            res["end_error"][setting] = list(VC.pose_error(p[0], truth))
            res["rounds"][setting], res["rows"][setting] = list(p[1]), int(p[4])
        res["frame"] = interleaved(ctx, {k: under(k, frame) for k in SETTINGS}, reps)
        res["one_round"] = interleaved(ctx, {k: under(k, one) for k in SETTINGS}, reps)
        for what in ("frame", "one_round"):
            off = res[what]["off"]
            spread = off["quartiles_us"][2] - off["quartiles_us"][0]
            res[what]["off_spread_us"] = round(spread, 2)
            for k in ("huber", "tukey"):
                res[what][k + "_against_off"] = verdict(res[what][k]["median_us"], off["median_us"])
                res[what][k + "_minus_off_us"] = round(res[what][k]["median_us"] - off["median_us"], 2)
        out[form] = res
    if kernels:
        ctx.sdf_set_robust(*SETTINGS["tukey"])
        ctx.sdf_robust_weights(truth)
        ctx.sdf_robust_weights(truth, photo=True)
        ctx.map_sdf_robust_weights(truth, box=box)
        ctx.map_sdf_robust_weights(truth, photo=True, box=box)
    ctx.sdf_set_robust(0)
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
