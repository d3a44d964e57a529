"""The oriented descriptor at 640 x 480 beside the upright one, both kinds in ONE process on the pairs of
tests/oriented_cases.py's motions at the full camera: host wall medians of rpe_features_detect per side (the call ends in its own host
wait for the count) and of rpe_relocalize -- with both detections, and with the features already there; the keypoints, matches and the
relocalised pose's error of each kind on a rolled pair (roll 0.6) and on the unrolled wide pair scripts/feature_time.py times.  Prints
one JSON line (and writes it to argv[1] when given).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` with
RPE_ORIENTED_KERNELS_ONLY=1 (a short pass of each call): feat_describe_kernel and feat_describe_oriented_kernel are the two rows to
compare, the five detector kernels before them are shared."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import feature_cases as FC  # noqa: E402
import oriented_cases as OC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
KINDS = (("upright", L.DESC_UPRIGHT), ("oriented", L.DESC_ORIENTED))


def timed(f, reps, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def stage(ctx, p, reps):
    """host wall of detection and relocalisation on one pair, with the context's current descriptor kind"""
    p.upload(ctx)
    out = {"keypoints": [ctx.features_detect(L.FEAT_FRAME), ctx.features_detect(L.FEAT_MODEL)]}
    out["detect_frame_us"] = timed(lambda: ctx.features_detect(L.FEAT_FRAME), reps)
    out["detect_model_us"] = timed(lambda: ctx.features_detect(L.FEAT_MODEL), reps)
    out["matches"] = ctx.features_match()
    kw = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, ls=api.LS_SHINJI_INLIERS, **FC.RELOC_THRE)
    try:
        r = ctx.relocalize(api.M_SK_PROSAC, **kw)
        out["relocalize"] = {"matches": r["matches"], "votes": r["max_votes"], "iters": r["iters"], "error": list(VC.pose_error(r["pose12"], p.pb))}
    except L.RpeError as e:
        if e.code != L.RPE_ERR_DEGENERATE:
            raise
        out["relocalize"] = None                     # too few matches: no pose, nothing to time
        return out
    out["relocalize_features_present_us"] = timed(lambda: ctx.relocalize(api.M_SK_PROSAC, **kw), reps)

    def drop():                                      # a new colour on both sides: relocalize detects again (outside the timed window)
        ctx.frame_set_color(p.cb); ctx.model_color_upload(p.model_rgba); ctx.synchronize()
    out["relocalize_us"] = timed(lambda: ctx.relocalize(api.M_SK_PROSAC, **kw), reps, before=drop)
    return out


def main():
    reps = 5 if os.environ.get("RPE_ORIENTED_KERNELS_ONLY") == "1" else 30
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    pairs = {"wide2": FC.Pair(CAM, FC.WIDE2), "roll0.6": FC.Pair(CAM, OC.MOTIONS["roll0.6"])}
    for rnd in (0, 1):                               # every kind twice, interleaved: the second round shows the run-to-run spread
        for name, kind in KINDS:
            ctx.features_set_descriptor(kind)
            for pname, p in pairs.items():
                out[f"{pname}_{name}_{rnd}"] = stage(ctx, p, reps)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
