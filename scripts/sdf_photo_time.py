"""The volume colour term at 640 x 480, the room fused WITH colour in 256^3 and 512^3 volumes, three levels, one run:
after the routes' poses have been compared, host wall (with a synchronise) medians, the routes interleaved call by call, of
  (a) icp_pyramid_sdf against icp_pyramid_sdf_rgbd: what the colour costs on the direct route;
  (b) volume_raycast(levels=3) + model_color + photo_prepare + icp_pyramid_rgbd against icp_pyramid_sdf_rgbd: the only route to colour
      tracking before, against the direct one;
  (c) the round kernel per level against icp_sdf_kernel: from a kernel trace of a short pass of the same script.
Prints one JSON line and writes it to argv[1] (default profiles/sdf_photo_time_640.json).

    python scripts/sdf_photo_time.py [out.json]
    RPE_SDF_PHOTO_KERNELS_ONLY=1 rocprofv3 --kernel-trace ... -- python scripts/sdf_photo_time.py /dev/null   (a short pass of each call)
    python scripts/sdf_photo_time.py --kernel-trace kernel_trace.csv [out.json]     ((c): the kernels' own times per level into out.json)

Bytes of a combined round, from the shapes: per pixel 12 B of vertex, 12 B of normal and 4 B of intensity streamed, eight 8-byte TSDF
corners and eight 8-byte colour corners gathered."""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from sdf_time import CAM, COS, GATES, ITERS, LEVELS, ORIGIN, RANGE, RAY, SIDE, interleaved  # noqa: E402

WEIGHT = 0.01
BYTES_PER_PIXEL = 12 + 12 + 4 + 8 * 8 + 8 * 8
DEFAULT_OUT = os.path.join(ROOT, "profiles", "sdf_photo_time_640.json")
KERNELS = ("icp_sdf_photo_kernel", "icp_sdf_kernel", "sdf_photo_rows_kernel", "frame_intensity_kernel", "icp_photo_kernel")


def merge_kernel_trace(trace_csv, out_json):
    """(c): per kernel and per launch size (the launch's threads tell the levels apart) the median of its launches in the trace"""
    out = json.load(open(out_json))
    per = {}
    for row in csv.DictReader(open(trace_csv)):
        for k in KERNELS:
            if k + "<" in row["Kernel_Name"] or row["Kernel_Name"].endswith(k) or k + "(" in row["Kernel_Name"]:
                name = k + ("<%s>" % row["Kernel_Name"].split(k + "<")[1].split(">")[0] if k + "<" in row["Kernel_Name"] else "")
                per.setdefault(name, {}).setdefault(int(row["Grid_Size_X"]), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out["kernels_by_threads_median_us"] = {k: {str(g): [round(statistics.median(v), 2), len(v)] for g, v in sorted(per[k].items())} for k in sorted(per)}
    n = CAM[4] * CAM[5]
    top = [statistics.median(v[max(v)]) for k, v in per.items() if k.startswith("icp_sdf_photo_kernel<true")]
    if top:
        out["combined_round_level0"] = {"bytes": n * BYTES_PER_PIXEL, "achieved_GBps": round(n * BYTES_PER_PIXEL / top[0] / 1e3, 1)}
    line = json.dumps(out)
    print(line)
    open(out_json, "w").write(line + "\n")


def main():
    import color_oracle  # noqa: F401  (tests/ on the path: the scenes' modules import it)
    import photo_cases as PC
    import sdf_cases as SC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import _lib as L, api
    short = os.environ.get("RPE_SDF_PHOTO_KERNELS_ONLY") == "1"
    reps = 5 if short else 40
    out = {"cam": list(CAM), "levels": LEVELS, "iters": list(ITERS), "gates": list(GATES), "cos_thr": COS, "weight": WEIGHT,
           "bytes_per_pixel": BYTES_PER_PIXEL}
    ctx = api.Context(0)
    truth = VC.held_out_pose()
    start = SC.moved(truth, 0.004, -0.003, 0.002, 0.012, -0.008, 0.015)     # a frame-to-frame step: 2 cm, 5 mrad
    views = [(VC.view(k), VC.depth_at(VC.view(k), CAM), PC.rgb_at(VC.view(k), CAM, None)) for k in VC.ACC_VIEWS]
    frame, rgb = VC.depth_at(truth, CAM), PC.rgb_at(truth, CAM, None)
    for nv in (256, 512):
        s = SIDE / nv
        ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
        for p, d, c in views:
            ctx.frame_set_depth(d, CAM, 1.0, *RANGE, levels=LEVELS)
            ctx.frame_set_color(c)
            ctx.volume_integrate_color(p)
        ctx.frame_set_depth(frame, CAM, 1.0, *RANGE, levels=LEVELS)
        ctx.frame_set_color(rgb)
        ctx.synchronize()
        res = {"voxel_m": s, "trunc_m": 3 * s}

        def sdf_route():
            p = ctx.icp_pyramid_sdf(start, ITERS, GATES, 1e-6, COS)[0]
            ctx.synchronize()
            return p

        def sdf_rgbd_route():
            r = ctx.icp_pyramid_sdf_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS)
            ctx.synchronize()
            return r

        def raycast_rgbd_route():
            ctx.volume_raycast(start, CAM, *RAY, levels=LEVELS)
            ctx.model_color()
            ctx.photo_prepare(LEVELS)
            p = ctx.icp_pyramid_rgbd(start, WEIGHT, ITERS, GATES, 1e-6, COS)[0]
            ctx.synchronize()
            return p
        # the poses first: the three routes from the same start against the same volumes
        ps, rr, pr = sdf_route(), sdf_rgbd_route(), raycast_rgbd_route()
        res["start_error"] = list(VC.pose_error(start, truth))
        res["sdf_route_error"] = list(VC.pose_error(ps, truth))
        res["sdf_rgbd_route_error"] = list(VC.pose_error(rr[0], truth))
        res["raycast_rgbd_route_error"] = list(VC.pose_error(pr, truth))
        res["rows_of_the_last_round"] = {"geometric": int(rr[4]), "photometric": int(rr[6]), "rounds": list(rr[1])}
        # (a) what the colour costs on the direct route; (b) the route to colour tracking before, against the direct one
        res["frame_sdf_vs_sdf_rgbd"] = interleaved(sdf_route, sdf_rgbd_route, reps)
        res["frame_raycast_rgbd_vs_sdf_rgbd"] = interleaved(raycast_rgbd_route, sdf_rgbd_route, reps)
        # one round per call at level 0, both kernels
        res["one_round_sdf_vs_sdf_rgbd"] = interleaved(lambda: ctx.icp_sdf(start, 1, 0.0, GATES[0], COS),
                                                       lambda: ctx.icp_sdf_rgbd(start, WEIGHT, 1, 0.0, GATES[0], COS), reps)
        if short:
            ctx.sdf_photo_rows(truth, 0, GATES[0])
            ctx.sdf_photo_normal_eq(truth, 0, GATES[0], WEIGHT)
        out["vol%d" % nv] = res
    ctx.close()
    line = json.dumps(out)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel-trace":
        merge_kernel_trace(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT)
    else:
        main()
