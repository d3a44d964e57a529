"""Coarse-to-fine ICP at 640 x 480, L = 3: host wall time of the frame build (rpe_frame_set_depth against
rpe_frame_set_depth_pyramid) and of one frame's ICP on the x6 scene of tests/test_gpu_pyramid.py -- icp_pyramid((3, 3, 10)) against
icp(max_iter=17) -- in the host-round, fused (host-driven resident grid) and device-resident forms.  Prints one JSON line (and writes it
to argv[1] when given).  Kernel times and launch counts: run it under `rocprofv3 --kernel-trace --stats` with RPE_PYR_KERNELS_ONLY=1
(a short pass of each call)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from frontend_util import pose12, two_views  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
FORMS = {"host": dict(device_resident=False, fused=False), "fused": dict(device_resident=False, fused=True),
         "resident": dict(device_resident=True, fused=True)}


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def main():
    short = os.environ.get("RPE_PYR_KERNELS_ONLY") == "1"
    reps = 5 if short else 50
    motion = tuple(6 * m for m in (0.02, -0.015, 0.01, 0.03, -0.02, 0.025))
    (RA, tA, dA), (RB, tB, dB) = two_views(CAM, motion, noise=0.002, seed=1)
    pA, pB = pose12(RA, tA), pose12(RB, tB)
    ctx = api.Context(0)
    out = {"cam": list(CAM), "levels": 3}

    def single():
        ctx.frame_set_depth(dB, CAM, 1.0, *RANGE); ctx.synchronize()

    def pyramid():
        ctx.frame_set_depth(dB, CAM, 1.0, *RANGE, levels=3); ctx.synchronize()
    for f in (single, pyramid):
        f()
    out["frame_set_depth_us"] = timed(single, reps)
    out["frame_set_depth_pyramid_us"] = timed(pyramid, reps)

    ctx.frame_set_depth(dA, CAM, 1.0, *RANGE, levels=3)
    ctx.model_from_frame(pA)
    ctx.frame_set_depth(dB, CAM, 1.0, *RANGE, levels=3)
    for name, form in FORMS.items():
        one = lambda: ctx.icp(pA, L.RES_P2PLANE, 17, 1e-6, 0.15, 0.8, **form)     # noqa: E731
        pyr = lambda: ctx.icp_pyramid(pA, (3, 3, 10), (0.15, 0.2, 0.3), L.RES_P2PLANE, 1e-6, 0.8, **form)  # noqa: E731
        r1, r2 = one(), pyr()
        err = lambda p: (float(np.linalg.norm(p[:9] - pB[:9])), float(np.linalg.norm(p[9:] - pB[9:])))  # noqa: E731
        out[name] = {"icp17_us": timed(one, reps), "icp17_rounds": r1[1], "icp17_err": err(r1[0]),
                     "pyramid_us": timed(pyr, reps), "pyramid_rounds": r2[1], "pyramid_err": err(r2[0])}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
