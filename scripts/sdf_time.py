"""The volume term at 640 x 480 beside the raycast route, the room fused in 256^3 and 512^3 volumes, one run:
after both routes' poses have been compared, host wall medians, the routes interleaved, of (a) one round of rpe_icp_sdf against one
fused ICP round (one-round calls, one launch per round both), and (b) a whole tracked frame both ways:
volume_raycast(levels=3) + icp_pyramid + integrate against icp_pyramid_sdf + integrate.  Prints one JSON line and writes it to argv[1]
(default profiles/sdf_time_640.json).

    python scripts/sdf_time.py [out.json]
    RPE_SDF_KERNELS_ONLY=1 rocprofv3 --kernel-trace --stats ... -- python scripts/sdf_time.py /dev/null     (a short pass of each call)
    python scripts/sdf_time.py --kernel-stats kernel_stats.csv out.json [kernel_trace.csv]     (the kernel's own time and achieved
                                                                              bytes/s into out.json; with the trace, per level)

Bytes of a round, from the shapes: per pixel 12 B of vertex and 12 B of normal streamed and eight 8-byte corner voxels gathered."""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)
RANGE = (0.1, 10.0, 0.1)
RAY = (0.1, 7.0)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
LEVELS, ITERS, GATES, COS = 3, (6, 4, 3), (0.1, 0.15, 0.2), 0.8
BYTES_PER_PIXEL = 12 + 12 + 8 * 8
DEFAULT_OUT = os.path.join(ROOT, "profiles", "sdf_time_640.json")


def wall(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def interleaved(a, b, reps, warm=3):
    """medians (and quartiles) of two calls alternated, so that both see the same state of the machine"""
    for _ in range(warm):
        a(); b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall(a)); tb.append(wall(b))
    q = lambda t: [round(x, 2) for x in statistics.quantiles(t, n=4)]   # noqa: E731
    return {"median_us": [round(statistics.median(ta), 2), round(statistics.median(tb), 2)], "quartiles_us": [q(ta), q(tb)], "reps": reps}


def merge_kernel_stats(stats_csv, out_json, trace_csv=None):
    out = json.load(open(out_json))
    n = CAM[4] * CAM[5]
    for row in csv.DictReader(open(stats_csv)):
        if "icp_sdf_kernel" in row["Name"]:
            us = float(row["AverageNs"]) / 1e3
            # (the pass runs the three levels: the average is over rounds of 307 200, 76 800 and 19 200 pixels; MaxNs is a level-0 round)
            top = float(row["MaxNs"]) / 1e3
            out["icp_sdf_kernel"] = {"calls": int(row["Calls"]), "average_us": round(us, 2), "min_us": float(row["MinNs"]) / 1e3, "max_us": top,
                                     "bytes_level0": n * BYTES_PER_PIXEL, "achieved_GBps_at_max_us": round(n * BYTES_PER_PIXEL / top / 1e3, 1)}
        for k in ("icp_fused_kernel", "volume_raycast_kernel", "sdf_rows_kernel"):
            if k in row["Name"]:
                out.setdefault("other_kernels_us", {})[k + ("<%s>" % row["Name"].split("<")[1].split(">")[0] if "<" in row["Name"] else "")] = \
                    {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    if trace_csv:   # per level (the launch's threads tell the levels apart): the median of the round kernel's launches
        per = {}
        for row in csv.DictReader(open(trace_csv)):
            if "icp_sdf_kernel" in row["Kernel_Name"]:
                per.setdefault(int(row["Grid_Size_X"]), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        top = max(per)
        out["icp_sdf_kernel"]["by_threads_median_us"] = {str(k): round(statistics.median(v), 2) for k, v in sorted(per.items())}
        out["icp_sdf_kernel"]["achieved_GBps_level0_median"] = round(n * BYTES_PER_PIXEL / statistics.median(per[top]) / 1e3, 1)
    line = json.dumps(out)
    print(line)
    open(out_json, "w").write(line + "\n")


def main():
    import numpy as np
    import volume_cases as VC
    from rgbd_pose_estimation_amd import _lib as L, api
    short = os.environ.get("RPE_SDF_KERNELS_ONLY") == "1"
    reps = 5 if short else 40
    out = {"cam": list(CAM), "levels": LEVELS, "iters": list(ITERS), "gates": list(GATES), "cos_thr": COS, "bytes_per_pixel": BYTES_PER_PIXEL}
    ctx = api.Context(0)
    import sdf_cases as SC
    truth = VC.held_out_pose()
    start = SC.moved(truth, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)     # a frame-to-frame step: 2 cm, 5 mrad
    far = SC.poses()[1]                                                     # 5.4 cm, 11 mrad: beyond the band of the 512^3 volume
    views = [(VC.view(k), VC.depth_at(VC.view(k), CAM)) for k in VC.ACC_VIEWS]
    frame = VC.depth_at(truth, CAM)
    for nv in (256, 512):
        s = SIDE / nv
        ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
        for p, d in views:
            ctx.frame_set_depth(d, CAM, 1.0, *RANGE, levels=LEVELS)
            ctx.volume_integrate(p)
        ctx.frame_set_depth(frame, CAM, 1.0, *RANGE, levels=LEVELS)
        ctx.synchronize()
        res = {"voxel_m": s, "trunc_m": 3 * s}

        def raycast_route():
            ctx.volume_raycast(start, CAM, *RAY, levels=LEVELS)
            p = ctx.icp_pyramid(start, ITERS, GATES, L.RES_P2PLANE, 1e-6, COS, fused=True)[0]
            ctx.volume_integrate(truth); ctx.synchronize()
            return p

        def sdf_route():
            p = ctx.icp_pyramid_sdf(start, ITERS, GATES, 1e-6, COS)[0]
            ctx.volume_integrate(truth); ctx.synchronize()
            return p
        # the poses first: both routes from the same start against the same volume
        pr, ps = raycast_route(), sdf_route()
        res["start_error"] = list(VC.pose_error(start, truth))
        res["raycast_route_error"] = list(VC.pose_error(pr, truth))
        res["sdf_route_error"] = list(VC.pose_error(ps, truth))
        res["sdf_rows_at_truth"] = int(ctx.sdf_normal_eq(truth, 0, GATES[0], COS)[28])
        # ... and from the far start: where the term's basin, the truncation band, ends
        ctx.volume_raycast(far, CAM, *RAY, levels=LEVELS)
        res["far_start_error"] = list(VC.pose_error(far, truth))
        res["far_raycast_route_error"] = list(VC.pose_error(ctx.icp_pyramid(far, ITERS, GATES, L.RES_P2PLANE, 1e-6, COS, fused=True)[0], truth))
        try:
            res["far_sdf_route_error"] = list(VC.pose_error(ctx.icp_pyramid_sdf(far, ITERS, GATES, 1e-6, COS)[0], truth))
        except L.RpeError as e:
            res["far_sdf_route_error"] = "status %d" % e.code
        # (a) one round per call at level 0; the fused ICP round needs its model: the raycast of the start pose
        ctx.volume_raycast(start, CAM, *RAY, levels=LEVELS)
        res["one_round_sdf_vs_fused_icp"] = interleaved(lambda: ctx.icp_sdf(start, 1, 0.0, GATES[0], COS),
                                                        lambda: ctx.icp(start, L.RES_P2PLANE, 1, 0.0, GATES[0], COS, fused=True), reps)
        # (b) a whole tracked frame both ways
        res["frame_sdf_vs_raycast"] = interleaved(sdf_route, raycast_route, reps)
        res["raycast_levels3"] = interleaved(lambda: (ctx.volume_raycast(start, CAM, *RAY, levels=LEVELS), ctx.synchronize()),
                                             lambda: ctx.synchronize(), reps)["median_us"][0]
        if short:
            ctx.sdf_rows(truth, 0, GATES[0], COS)
        out["vol%d" % nv] = res
    ctx.close()
    line = json.dumps(out)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel-stats":
        merge_kernel_stats(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT, sys.argv[4] if len(sys.argv) > 4 else None)
    else:
        main()
