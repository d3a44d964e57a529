"""The photometric term at 640 x 480 and its three pyramid levels: host wall medians of (a) one round of
rpe_icp_rgbd against one round of the fused rpe_icp, alternated in the same process, per level; (b) the time per round of a 10-round
rpe_icp_rgbd against rpe_icp in its one-launch-per-round host form (one-round calls) and in its resident form (a different execution
form, reported beside it); (c) rpe_photo_prepare per frame; (d) one frame of the tracking loop with and without the term.  Prints one
JSON line (and writes it to argv[1] when given).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` with
RPE_PHOTO_KERNELS_ONLY=1 (a short pass of each call)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import photo_cases as PC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
RANGE = (0.1, 10.0, 0.1)
RAY = (0.1, 7.0)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def main():
    short = os.environ.get("RPE_PHOTO_KERNELS_ONLY") == "1"
    reps = 5 if short else 30
    ctx = api.Context(0)
    out = {"cam": list(CAM), "weight": PC.WEIGHT}
    pa, da, ca, pb, db, cb = PC.pair(None, CAM)
    levels = 3
    ctx.frame_set_depth(da, CAM, 1.0, *RANGE, levels=levels)
    ctx.frame_set_color(ca)
    ctx.model_from_frame(pa)
    ctx.model_color_from_frame()
    ctx.frame_set_depth(db, CAM, 1.0, *RANGE, levels=levels)
    ctx.frame_set_color(cb)

    def prepare():
        ctx.photo_prepare(levels); ctx.synchronize()
    out["photo_prepare_us"] = timed(prepare, reps)
    # (a) one round per call, per level: a pyramid call with rounds at that level only (level 0 needs one: subtracted for l > 0)
    per_level = {}
    for l in range(levels):
        iters = tuple(1 if k in (0, l) else 0 for k in range(levels))

        def rgbd():
            ctx.icp_pyramid_rgbd(pa, PC.WEIGHT, iters, VC.TRACK_GATES, 0.0, PC.COS_THR)

        def fused():
            ctx.icp_pyramid(pa, iters, VC.TRACK_GATES, L.RES_P2PLANE, 0.0, PC.COS_THR, fused=True)
        a, b = [], []
        for _ in range(reps):                      # alternated, so that both see the same state of the machine
            a.append(timed(rgbd, 1)); b.append(timed(fused, 1))
        per_level[l] = {"pixels": (CAM[4] >> l) * (CAM[5] >> l), "rgbd_call_us": statistics.median(a), "fused_call_us": statistics.median(b)}
    for l in range(1, levels):
        for k in ("rgbd_call_us", "fused_call_us"):
            per_level[l][k.replace("call", "round")] = per_level[l][k] - per_level[0][k]
    out["one_round_calls"] = per_level
    # (b) time per round of a 10-round loop at level 0
    n = 10
    out["rgbd_round_us"] = timed(lambda: ctx.icp_rgbd(pa, PC.WEIGHT, n, 0.0, 0.1, PC.COS_THR), reps) / n
    out["icp_one_launch_per_round_us"] = timed(lambda: ctx.icp(pa, L.RES_P2PLANE, 1, 0.0, 0.1, PC.COS_THR, fused=True), reps)
    out["rgbd_one_round_call_us"] = timed(lambda: ctx.icp_rgbd(pa, PC.WEIGHT, 1, 0.0, 0.1, PC.COS_THR), reps)
    out["icp_resident_round_us"] = timed(lambda: ctx.icp(pa, L.RES_P2PLANE, n, 0.0, 0.1, PC.COS_THR, fused=True), reps) / n
    # (d) the tracking loop at 640 x 480, 256^3, host wall per stage (medians over the frames), without and with the term
    nv = 256
    s = SIDE / nv
    poses = [PC.room_pose(f) for f in range(VC.TRACK_FRAMES)]
    frames = PC.loop_frames(poses, None, CAM)
    for term in (False, True):
        ctx.volume_init((nv, nv, nv), s, ORIGIN, 3 * s, 64)
        est = poses[0]
        ctx.frame_set_depth(frames[0][0], CAM, 1.0, *RANGE, levels=levels)
        ctx.frame_set_color(frames[0][1])
        ctx.volume_integrate_color(est)
        ctx.synchronize()
        st = {"set_depth_pyramid_and_color": [], "raycast_and_model_pyramid": [], "model_color_and_prepare": [], "icp": [], "integrate_color": []}
        for f in range(1, VC.TRACK_FRAMES):
            t = [time.perf_counter_ns()]
            ctx.frame_set_depth(frames[f][0], CAM, 1.0, *RANGE, levels=levels); ctx.frame_set_color(frames[f][1]); ctx.synchronize()
            t.append(time.perf_counter_ns())
            ctx.volume_raycast(est, CAM, *RAY, levels=levels); ctx.synchronize(); t.append(time.perf_counter_ns())
            if term:
                L.check(L.lib().rpe_model_sample_color(ctx._h)); ctx.photo_prepare(levels); ctx.synchronize()
            t.append(time.perf_counter_ns())
            if term:
                est = ctx.icp_pyramid_rgbd(est, PC.WEIGHT, VC.TRACK_ITERS, VC.TRACK_GATES, 1e-6, PC.COS_THR)[0]
            else:
                est = ctx.icp_pyramid(est, VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, PC.COS_THR)[0]
            t.append(time.perf_counter_ns())
            ctx.volume_integrate_color(est); ctx.synchronize(); t.append(time.perf_counter_ns())
            for k, a, b in zip(st, t, t[1:]):
                st[k].append((b - a) / 1e3)
        key = "track640_vol256_rgbd_us" if term else "track640_vol256_us"
        out[key] = {k: statistics.median(v) for k, v in st.items()}
        out[key]["frame"] = sum(out[key].values())
        out[key]["last_frame_error"] = list(VC.pose_error(est, poses[-1]))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
