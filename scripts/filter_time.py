"""The depth filter at 640 x 480 ("Depth filter"): host wall time of the frame build -- rpe_frame_set_depth and
rpe_frame_set_depth_pyramid(levels = 3), upload to completion -- with the filter off and on at radii 1 / 3 / 4, in ONE run, so that
the off column (the path without the filter) is the figure the on columns are read against.  The frame is the sensor's: uint16
millimetres with simulator.sensor_depth's noise.  Prints one JSON line (and writes it to argv[1] when given).  Kernel time of the
filter itself: run the script under `rocprofv3 --kernel-trace --stats --output-format csv` with RPE_FILTER_KERNELS_ONLY=1 (a short
pass of each call) and give that run's kernel trace csv as argv[2] of the plain invocation: the filter's dispatches come in the order
of the radii, equally many each, and their median duration per radius goes into the JSON line."""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from frontend_util import rot  # noqa: E402
from rgbd_pose_estimation_amd import api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
RADII = (1, 3, 4)


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def kernel_times(path):
    """median duration of depth_filter_kernel per radius from the kernel trace csv of a RPE_FILTER_KERNELS_ONLY=1 pass"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "depth_filter_kernel" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    per = len(ns) // len(RADII)
    return {"dispatches": len(ns), **{f"r{r}_kernel_us": statistics.median(ns[i * per:(i + 1) * per]) / 1e3 for i, r in enumerate(RADII)}}


def main():
    short = os.environ.get("RPE_FILTER_KERNELS_ONLY") == "1"
    reps = 5 if short else 200
    depth = S.sensor_depth(rot(0.05, -0.1, 0.02), np.array([0.1, -0.05, 0.2]), CAM, np.random.default_rng(5))
    ctx = api.Context(0)
    out = {"cam": list(CAM), "levels": 3, "reps": reps, "sigma_space": 2.0, "depth_cut": 0.01, "depth_cut_z2": 0.02}

    def single():
        ctx.frame_set_depth(depth, CAM, 0.001, *RANGE); ctx.synchronize()

    def pyramid():
        ctx.frame_set_depth(depth, CAM, 0.001, *RANGE, levels=3); ctx.synchronize()

    rounds = 1 if short else 3             # off and on interleaved, so that a drift of the machine shows in both
    cols = {"off": 0, **{f"r{r}": r for r in RADII}}
    times = {c: {"single": [], "pyramid": []} for c in cols}
    for _ in range(rounds):
        for c, r in cols.items():
            ctx.frame_set_filter(r)
            single(); pyramid()
            times[c]["single"].append(timed(single, reps))
            times[c]["pyramid"].append(timed(pyramid, reps))
    for c in cols:
        out[c] = {"frame_set_depth_us": min(times[c]["single"]), "frame_set_depth_pyramid_us": min(times[c]["pyramid"])}
    for c in cols:
        if c != "off":
            out[c]["single_over_off"] = out[c]["frame_set_depth_us"] / out["off"]["frame_set_depth_us"]
            out[c]["pyramid_over_off"] = out[c]["frame_set_depth_pyramid_us"] / out["off"]["frame_set_depth_pyramid_us"]
    ctx.close()
    if len(sys.argv) > 2:
        out["kernel_trace"] = kernel_times(sys.argv[2])
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
