"""The scale levels at 640 x 480 beside the one-level stage, 1 / 2 / 3 / 4 levels in ONE process, interleaved,
after the bits of every number of levels were compared with tests/scale_oracle.py on the pair: host wall medians of rpe_features_detect
per side (the call ends in its own host wait for the count), and rpe_relocalize -- with both detections, and with the features already
there -- at 1 and 4 levels on the pair whose frame was taken 1.6 m closer and on the narrow pair, with matches, votes, iterations and the
pose's error beside the time.  The yardstick is levels = 1 in the same run.  Prints one JSON line (and writes it to argv[1] when given).
Kernel times: run it under `rocprofv3 --kernel-trace` with RPE_SCALE_KERNELS_ONLY=1 (nothing but REPS detections of the frame per number
of levels, in order), then give the trace as argv[2]: the sum of a detection's kernels, median per number of levels, goes into the
JSON as `detect_kernel_us`."""
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import feature_cases as FC  # noqa: E402
import scale_cases as SC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
LEVELS = (1, 2, 3, 4)
KERNEL_REPS = 5
FIRST = ("feat_score_kernel", "feat_resample_kernel")          # the first kernel of a detection with one / with more levels


def timed(f, reps, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def compare_bits(ctx, p, levels):
    """both sides against the oracle: xy, score, descriptor, level, level pixel"""
    for which, view in ((L.FEAT_FRAME, p.frame), (L.FEAT_MODEL, p.model)):
        o = SC.detect(view, levels)
        assert ctx.features_detect(which) == len(o[0]), (which, levels)
        got = ctx.features(which) + ctx.features_scale(which)
        assert all(np.array_equal(a, b) for a, b in zip(got, o[:5])), (which, levels)


def stage(ctx, p, reps, reloc):
    """host wall of detection (and relocalisation) on one pair, with the context's current number of levels"""
    p.upload(ctx)
    out = {"keypoints": [ctx.features_detect(L.FEAT_FRAME), ctx.features_detect(L.FEAT_MODEL)]}
    out["detect_frame_us"] = timed(lambda: ctx.features_detect(L.FEAT_FRAME), reps)
    out["detect_model_us"] = timed(lambda: ctx.features_detect(L.FEAT_MODEL), reps)
    out["matches"] = ctx.features_match()
    if not reloc:
        return out
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


def kernels_only(ctx, p):
    p.upload(ctx)
    for n in LEVELS:
        ctx.features_set_levels(n)
        for _ in range(KERNEL_REPS):
            ctx.features_detect(L.FEAT_FRAME)


def kernel_times(trace):
    """per number of levels the median over its detections of the summed kernel time (us), from the trace of a kernels-only pass"""
    groups = []
    for row in csv.DictReader(open(trace)):
        name = row["Kernel_Name"]
        if "feat_" not in name:
            continue
        if any(f in name for f in FIRST):
            groups.append(0.0)
        if groups:
            groups[-1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
    assert len(groups) == KERNEL_REPS * len(LEVELS), len(groups)
    return {str(n): statistics.median(groups[i * KERNEL_REPS:(i + 1) * KERNEL_REPS]) for i, n in enumerate(LEVELS)}


def main():
    closer, narrow = FC.Pair(CAM, SC.MOTIONS["tz-1.6"]), FC.Pair(CAM, SC.MOTIONS["narrow"])
    ctx = api.Context(0)
    if os.environ.get("RPE_SCALE_KERNELS_ONLY") == "1":
        kernels_only(ctx, closer)
        ctx.close()
        return
    out = {"cam": list(CAM), "pixel_ratio": {str(n): float(sum(np.prod(SC.SO.level_size(CAM[4], CAM[5], l)) for l in range(n)) / (CAM[4] * CAM[5]))
                                             for n in LEVELS}}
    closer.upload(ctx)
    for n in LEVELS:
        ctx.features_set_levels(n)
        compare_bits(ctx, closer, n)
    out["bits_compared"] = True
    for rnd in (0, 1):                               # every number twice, interleaved: the second round shows the run-to-run spread
        for n in LEVELS:
            ctx.features_set_levels(n)
            out[f"closer_{n}_{rnd}"] = stage(ctx, closer, 30, n in (1, 4))
            if n in (1, 4):
                out[f"narrow_{n}_{rnd}"] = stage(ctx, narrow, 30, True)
    ctx.close()
    if len(sys.argv) > 2:
        out["detect_kernel_us"] = kernel_times(sys.argv[2])
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
