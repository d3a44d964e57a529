"""Colour registration at 640 x 480 depth: host wall medians of rpe_frame_register_color -- upload of the colour
camera's image to completion, with a host wait -- for a 1280 x 720 and a 640 x 480 distorted colour camera 50 mm beside the depth
camera, with z-buffer cells of 0 (no occlusion test), 2 and 3 colour pixels, interleaved in ONE run with rpe_frame_set_color of a
registered 640 x 480 image (the call it stands in for) and with the count (one more host wait).  Prints one JSON line (and writes it
to argv[1] when given).  Kernel times of R1 (splat) and R2 (gather): run the script under `rocprofv3 --kernel-trace --stats
--output-format csv` with RPE_REGISTER_KERNELS_ONLY=1 (a short pass of each configuration) and give that run's kernel trace csv as
argv[2] of the plain invocation: the dispatches come in the order of the configurations, equally many each."""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


import color_cases as CC  # noqa: E402
import register_cases as RC  # noqa: E402
import register_oracle as RO  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
COLOR_CAMS = {"1280x720": (1170.0, 1170.0, 640.0, 360.0, 1280, 720), "640x480": (585.0, 585.0, 320.0, 240.0, 640, 480)}
CELLS = (0, 2, 3)
CONFIGS = [(name, cell) for name in COLOR_CAMS for cell in CELLS]


def timed(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def kernel_times(path):
    """median duration (us) of R1 and R2 per configuration from the kernel trace csv of a RPE_REGISTER_KERNELS_ONLY=1 pass"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "register_" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kind in ("splat", "gather"):
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "register_%s_kernel" % kind in r["Kernel_Name"]]
        cfgs = [c for c in CONFIGS if kind == "gather" or c[1] > 0]          # cell 0 has no splat
        per = len(ns) // len(cfgs)
        for k, (name, cell) in enumerate(cfgs):
            out.setdefault("%s_cell%d" % (name, cell), {})["%s_kernel_us" % kind] = statistics.median(ns[k * per:(k + 1) * per]) / 1e3
    out["dispatches"] = len(rows)
    return out


def main():
    short = os.environ.get("RPE_REGISTER_KERNELS_ONLY") == "1"
    reps = 5 if short else 200
    p = VC.view(0)
    depth, rgb = VC.depth_at(p, CAM), CC.rgb_at(p, CAM)
    ctx = api.Context(0)
    ctx.frame_set_depth(depth, CAM, 1.0, *RANGE)
    out = {"cam": list(CAM), "reps": reps, "dist": list(RC.DIST), "occl_tol": [0.02, 0.01]}

    def set_color():
        ctx.frame_set_color(rgb); ctx.synchronize()
    set_color()
    images = {}
    for name, cell in CONFIGS:
        ccam = COLOR_CAMS[name]
        rig = RO.Rig(ccam, RC.DIST, tuple(RC.RIG_POSE), 0.0, cell, 0.02, 0.01)
        if name not in images:
            images[name] = RC.color_image(p, rig)
        img = images[name]
        r = ctx.color_rig(rig.cam, rig.dist, rig.pose12, rig.r2_max, rig.cell, rig.occl_tol, rig.occl_tol_z2)

        def register():
            ctx.frame_register_color(img, r); ctx.synchronize()

        def register_count():
            return ctx.frame_register_color(img, r, want_known=True)
        known = register_count()
        register(); set_color()                                          # warm-up of every shape the timed window uses
        a, b, c = [], [], []
        for _ in range(reps):                                            # alternated, so that all see the same state of the machine
            a.append(timed(register)); b.append(timed(set_color))
            if not short:
                c.append(timed(register_count))
        row = {"register_us": statistics.median(a), "set_color_us": statistics.median(b), "known": known,
               "known_share": known / (CAM[4] * CAM[5]), "z_buffer_words": (rig.grid()[0] + 1) * (rig.grid()[1] + 1) if cell else 0}
        if c:
            row["register_count_us"] = statistics.median(c)
        row["register_over_set_color"] = row["register_us"] / row["set_color_us"]
        out["%s_cell%d" % (name, cell)] = row
    ctx.close()
    if len(sys.argv) > 2:
        for k, v in kernel_times(sys.argv[2]).items():
            if isinstance(v, dict):
                out[k].update(v)
            else:
                out["kernel_trace_" + k] = v
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
