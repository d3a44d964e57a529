"""The feature stage at 640 x 480: host wall medians (every call ends in its own host wait for a count) of
rpe_features_detect per side, rpe_features_match without and with the cross-check, and rpe_relocalize -- with both detections and with
the features already there -- on the wide pair of tests/feature_cases.py; the same on the worst case the stage admits, 4096 x 4096
keypoints (a noise image), with the match's popcount count beside it; and, in the same run on the same box, one frame of the tracking
loop of scripts/photo_time.py (640 x 480, 256^3, with the photometric term).  Prints one JSON line (and writes it to argv[1] when
given).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` with RPE_FEATURE_KERNELS_ONLY=1 (a short pass of each call,
without the tracking loop)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import feature_cases as FC  # noqa: E402
import photo_cases as PC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
RAY = (0.1, 7.0)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
# VALU instructions per descriptor pair and lane in feat_best_kernel: 8 v_xor, 8 v_bcnt (each adds into the running sum) and the
# compare / select of (d1, index, d2); a wave64 VALU instruction issues in 2 cycles on one of 4 SIMDs of 256 compute units
VALU_PER_PAIR = 8 + 8 + 6
WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2


def timed(f, reps, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def stage(ctx, p, reps, reloc):
    """host wall of every call on one pair"""
    p.upload(ctx)
    out = {"keypoints": [ctx.features_detect(L.FEAT_FRAME), ctx.features_detect(L.FEAT_MODEL)]}
    out["detect_frame_us"] = timed(lambda: ctx.features_detect(L.FEAT_FRAME), reps)
    out["detect_model_us"] = timed(lambda: ctx.features_detect(L.FEAT_MODEL), reps)
    out["matches"] = ctx.features_match()
    out["match_us"] = timed(lambda: ctx.features_match(), reps)
    out["matches_cross_check"] = ctx.features_match(cross_check=True)
    out["match_cross_check_us"] = timed(lambda: ctx.features_match(cross_check=True), reps)
    nf, nm = out["keypoints"]
    out["match_popcounts"] = nf * nm * 8
    out["match_valu_issue_bound_us"] = nf * nm * VALU_PER_PAIR / 64 / WAVE_INSTR_PER_S * 1e6
    if reloc:
        kw = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, ls=api.LS_SHINJI_INLIERS, **FC.RELOC_THRE)
        r = ctx.relocalize(api.M_SK_PROSAC, **kw)
        out["relocalize"] = {"matches": r["matches"], "votes": r["max_votes"], "iters": r["iters"], "error": list(VC.pose_error(r["pose12"], p.pb))}
        out["relocalize_features_present_us"] = timed(lambda: ctx.relocalize(api.M_SK_PROSAC, **kw), reps)

        def drop():                              # a new colour on both sides: relocalize detects again (outside the timed window)
            ctx.frame_set_color(p.cb); ctx.model_color_upload(p.model_rgba); ctx.synchronize()
        out["relocalize_us"] = timed(lambda: ctx.relocalize(api.M_SK_PROSAC, **kw), reps, before=drop)
    return out


def track_frame(ctx):
    """scripts/photo_time.py's tracking loop with the term: the median host wall of one frame"""
    levels, nv = 3, 256
    s = SIDE / nv
    poses = [PC.room_pose(f) for f in range(VC.TRACK_FRAMES)]
    frames = PC.loop_frames(poses, None, CAM)
    ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
    est = poses[0]
    ctx.frame_set_depth(frames[0][0], CAM, 1.0, *RANGE, levels=levels)
    ctx.frame_set_color(frames[0][1])
    ctx.volume_integrate_color(est)
    ctx.synchronize()
    ts = []
    for f in range(1, VC.TRACK_FRAMES):
        t0 = time.perf_counter_ns()
        ctx.frame_set_depth(frames[f][0], CAM, 1.0, *RANGE, levels=levels); ctx.frame_set_color(frames[f][1])
        ctx.volume_raycast(est, CAM, *RAY, levels=levels)
        L.check(L.lib().rpe_model_sample_color(ctx._h)); ctx.photo_prepare(levels)
        est = ctx.icp_pyramid_rgbd(est, PC.WEIGHT, VC.TRACK_ITERS, VC.TRACK_GATES, 1e-6, PC.COS_THR)[0]
        ctx.volume_integrate_color(est); ctx.synchronize()
        ts.append((time.perf_counter_ns() - t0) / 1e3)
    return {"frame_us": statistics.median(ts), "last_frame_error": list(VC.pose_error(est, poses[-1]))}


def main():
    short = os.environ.get("RPE_FEATURE_KERNELS_ONLY") == "1"
    reps = 5 if short else 30
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    out["wide2"] = stage(ctx, FC.pair("full", "wide2"), reps, True)
    out["noise_4096"] = stage(ctx, FC.overcap_pair(CAM), reps, False)
    if not short:
        out["track640_vol256_rgbd"] = track_frame(ctx)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
