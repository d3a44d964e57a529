"""The keyframe graph at 640 x 480.  Stores of 8, 64 and 256 keyframes as scripts/keyframe_time.py builds them
(the model view of tests/feature_cases.py's wide pair, added K times): host wall of rpe_keyframes_link(first = 0) and of linking the
last keyframe alone, and ONE round of the optimisation split into rpe_graph_normal_eq (corrections up, the launch over every edge, the
records down -- one host wait --, the records' turn into tangent blocks on the host) and the dense solve, rpe_graph_solve.  Then the whole optimisation
of the eight-keyframe room of tests/graph_cases.py at 160 x 120 and 320 x 240, beside one tracked RGB-D frame (725 us,
profiles/feature_time_640.json).  Prints one JSON line (and writes it to argv[1] when given).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` with RPE_GRAPH_KERNELS_ONLY=1 (one link and one round at every K, nothing else)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import feature_cases as FC  # noqa: E402
import graph_cases as GC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
KS = (8, 64, 256)


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def main():
    short = os.environ.get("RPE_GRAPH_KERNELS_ONLY") == "1"
    p = FC.pair("full", "wide2")
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    p.upload(ctx)
    out["keypoints"] = ctx.features_detect(L.FEAT_MODEL)
    for K in KS:
        reps = 1 if short else max(2, 24 // K)
        while ctx.keyframes_len() < K:
            ctx.keyframe_add()
        edges, pairs = ctx.keyframes_link()
        row = {"edges": edges, "pairs": pairs}
        if not short:
            row["link_all_us"] = timed(lambda: ctx.keyframes_link(), reps)
            row["link_last_us"] = timed(lambda: ctx.keyframes_link(first=K - 1), max(3, reps))
        rec = ctx.graph_normal_eq(None, 0.1)
        ji = ctx.graph_edges()[:, :2]
        if not short:
            # one round = rpe_graph_normal_eq (corrections up, the launch over every edge, the raw records down -- one host wait --
            # and the records' turn into tangent blocks on the host) + rpe_graph_solve.  The kernel's own time comes from the
            # rocprofv3 pass; what is left of the first call is the copy and the host's part
            row["round_normal_eq_us"] = timed(lambda: ctx.graph_normal_eq(None, 0.1), max(3, reps))
            fixed = np.zeros(K, bool)
            fixed[0] = True
            row["round_solve_us"] = timed(lambda: api.graph_solve(K, ji, rec, fixed), max(3, reps))
            row["record_bytes_down"] = int(edges * 40 * 8)
        out["K%d" % K] = row
    ctx.close()
    if not short:
        for cam in ("small", "half"):
            c = GC.case(cam)
            ctx = api.Context(0)
            c.fill(ctx)
            ctx.keyframes_link()

            def whole():
                return ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=False)
            poses, st = whole()
            end = c.errors(poses)
            out["room_" + cam] = {"edges": ctx.graph_info()[0], "pairs": ctx.graph_info()[1], "rounds": len(st),
                                  "link_us": timed(lambda: ctx.keyframes_link(), 10), "optimize_us": timed(whole, 10),
                                  "worst_end_error": [max(e[0] for e in end), max(e[1] for e in end)], "tracked_frame_us": 725}
            ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
