"""The keyframe store at 640 x 480: keyframes of the size of tests/feature_cases.py's wide pair (its model view,
added K times) and its frame as the query.  Host wall medians (each call ends in its own host wait) of rpe_keyframes_query at K = 1, 8,
64 and 256, without and with the cross-check; on the same tree, K consecutive rpe_keyframe_match calls; rpe_relocalize_keyframes over
three candidates; and, for ONE keyframe, the route a caller had before the store -- rpe_model_upload + rpe_model_color_upload +
rpe_features_detect(MODEL) + rpe_features_match, the existing API only, so RPE_KEYFRAME_PARENT_ROUTE=1 times that part alone on a tree
without the store (the parent commit).  Prints one JSON line (and writes it to argv[1] when given).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` with RPE_KEYFRAME_KERNELS_ONLY=1 (a short pass of the query at every K, nothing else)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import feature_cases as FC  # noqa: E402
import volume_cases as VC  # noqa: E402
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S  # noqa: E402

CAM = S.DEFAULT_CAMERA
KS = (1, 8, 64, 256)
# VALU instructions per descriptor pair and lane, counted as scripts/feature_time.py counts them for feat_best_kernel: 8 v_xor, 8 v_bcnt
# and the compare / select of (d1, index, d2); a wave64 VALU instruction issues in 2 cycles on one of 4 SIMDs of 256 compute units
VALU_PER_PAIR = 8 + 8 + 6
WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); f(); ts.append((time.perf_counter_ns() - t0) / 1e3)
    return statistics.median(ts)


def parent_route(ctx, p, reps):
    """one keyframe put back as the model and matched, through the API that was there before the store"""
    p.upload(ctx)
    ctx.features_detect(L.FEAT_FRAME)

    def route():
        ctx.model_upload(p.model.V, p.model.N, p.cam, p.pa)
        ctx.model_color_upload(p.model_rgba)
        ctx.features_detect(L.FEAT_MODEL)
        return ctx.features_match()
    return {"matches": route(), "us": timed(route, reps)}


def main():
    short = os.environ.get("RPE_KEYFRAME_KERNELS_ONLY") == "1"
    reps = 3 if short else 30
    p = FC.pair("full", "wide2")
    ctx = api.Context(0)
    out = {"cam": list(CAM)}
    if not short:
        out["parent_route_one_keyframe"] = parent_route(ctx, p, reps)
    if os.environ.get("RPE_KEYFRAME_PARENT_ROUTE") != "1":
        p.upload(ctx)
        nf, nm = ctx.features_detect(L.FEAT_FRAME), ctx.features_detect(L.FEAT_MODEL)
        out["keypoints"] = [nf, nm]
        for K in KS:
            while ctx.keyframes_len() < K:
                ctx.keyframe_add()
            counts, order = ctx.keyframes_query()
            row = {"count": int(counts[0]), "query_us": timed(lambda: ctx.keyframes_query(), reps),
                   "query_cross_check_us": timed(lambda: ctx.keyframes_query(cross_check=True), reps),
                   "pairs": nf * nm * K, "best_valu_issue_bound_us": nf * nm * K * VALU_PER_PAIR / 64 / WAVE_INSTR_PER_S * 1e6}
            if not short:
                def singles():
                    for k in range(K):
                        ctx.keyframe_match(k)
                row["single_matches_us"] = timed(singles, max(3, reps // (1 + K // 8)))
                row["single_matches_cross_check_us"] = timed(lambda: [ctx.keyframe_match(k, cross_check=True) for k in range(K)],
                                                             max(3, reps // (1 + K // 8)))
            out["K%d" % K] = row
        if not short:
            kw = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, ls=api.LS_SHINJI_INLIERS, **FC.RELOC_THRE)
            r = ctx.relocalize_keyframes(api.M_SK_PROSAC, candidates=3, **kw)
            out["relocalize_keyframes_K256_3_candidates"] = {"keyframe": r["keyframe"], "matches": r["matches"], "votes": r["max_votes"],
                "error": list(VC.pose_error(r["pose12"], p.pb)), "us": timed(lambda: ctx.relocalize_keyframes(api.M_SK_PROSAC, candidates=3, **kw), reps)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
