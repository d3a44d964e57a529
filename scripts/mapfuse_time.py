"""The map fuse on one GPU beside the routes the parent has, one run: host wall around a synchronise, medians of
interleaved rounds AFTER the routes' bits have been compared.
  (a) where the sparse route buys nothing: a 256^3 window over the room, nothing archived, box = the window, 8 and 64 keyframes at
      640 x 480 (the eight views, repeated): "window" rpe_volume_fuse_keyframes against "map" rpe_volume_map_fuse_keyframes, both with
      RPE_FUSE_CLEAR.  The map route runs two passes and builds the grid: how much slower it is
  (b) the drifted walk of tests/mapfuse_cases.py (64^3 window, 512 bricks held, bounds 136 x 64 x 64, 13 keyframes at 160 x 120): "map"
      against "park", the only earlier route to the same content (up to the rounding of each stop's origin) -- the window parked over the box in window-sized stops,
      rpe_volume_fuse_keyframes at each stop, shifted onward so that the archive catches what leaves, and back
  (c) the kernels' own times, one case per run: `rocprofv3 --kernel-trace --output-format csv -- python scripts/mapfuse_time.py --kernels
      CASE` (CASE = vol256_8, vol256_64 or walk), merged with `python scripts/mapfuse_time.py --kernel-trace kernel_trace.csv out.json
      CASE`: per kernel the median over the run's dispatches, and for (a) the map route split into pass 1, pass 2 and the host's part
      (the route's median minus the two kernels' medians)
Prints one JSON line and writes it to argv[1] (default profiles/mapfuse_time.json)."""
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)
RANGE = (0.1, 10.0, 0.1)
ORIGIN, SIDE, NV = (-2.9, -3.2, -1.2), 6.4, 256     # scripts/volume_time.py's cube over the room
DEFAULT_OUT = os.path.join(ROOT, "profiles", "mapfuse_time.json")


def timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter_ns()
    f()
    ctx.synchronize()
    return (time.perf_counter_ns() - t0) / 1e3


def interleaved(ctx, routes, reps, warm=2):
    """{name: median and quartiles}: the calls alternated, so that all see the same state of the machine"""
    for _ in range(warm):
        for f in routes.values():
            f()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t[k].append(timed(ctx, f))
    return {k: {"median_us": round(statistics.median(v), 2), "quartiles_us": [round(x, 2) for x in statistics.quantiles(v, n=4)]}
            for k, v in t.items()}


def merge_kernel_trace(trace_csv, out_json, case):
    out = json.load(open(out_json))
    t = {}
    for row in csv.DictReader(open(trace_csv)):
        m = re.search(r"(map_fuse_kernel|volume_fuse_kernel)(<[^>]*>)?", row["Kernel_Name"])
        if m:
            t.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    k = {n: {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for n, v in t.items()}
    out.setdefault("kernels_us", {})[case] = k
    mark = [v["median_us"] for n, v in k.items() if n.startswith("map_fuse_kernel") and n.endswith("true>")]
    write = [v["median_us"] for n, v in k.items() if n.startswith("map_fuse_kernel") and n.endswith("false>")]
    if len(mark) == 1 and len(write) == 1:
        total = out[case]["frame"]["map"]["median_us"]
        out[case]["map_split_us"] = {"pass1": mark[0], "pass2": write[0], "host": round(total - mark[0] - write[0], 2)}
    line = json.dumps(out)
    print(line)
    open(out_json, "w").write(line + "\n")


def add_keyframe(ctx, rng, pose, cam):
    """a keyframe of four arbitrary keypoints that carries the current frame's depth"""
    import numpy as np
    i = ctx.keyframe_add_host(rng.integers(4, 60, (4, 2)), rng.integers(0, 99, (4, 8)), rng.normal(0, 1, (4, 3)), np.tile([0, 0, 1.0], (4, 1)),
                              pose, cam[4], cam[5])
    ctx.keyframe_attach_frame(i)
    return i


def in_box(ctx, lo, hi):
    """the map's content inside the box: the window's words and the held bricks of the box, for a comparison of two routes"""
    import numpy as np
    coords, tsdf, _ = ctx.volume_archive_download()
    keep = ((8 * coords >= lo) & (8 * coords < hi)).all(1) if len(coords) else np.zeros(0, bool)
    return ctx.volume_download().view(np.uint32), coords[keep], tsdf[keep].view(np.uint32)


def main():
    import numpy as np
    import archive_cases as AC
    import mapfuse_cases as MFC
    import shift_cases as SC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import api
    kernels = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
    only = sys.argv[2] if kernels and len(sys.argv) > 2 else None
    reps = 5 if kernels else 11
    out = {"cam": list(CAM), "reps": reps}
    rng = np.random.default_rng(5)
    # ---- (a) a full 256^3 window, box = the window
    ctx = api.Context(0)
    s = SIDE / NV
    ctx.volume_init((NV, NV, NV), s, ORIGIN, 3 * s, 64)
    ids = []
    for k in range(8):
        ctx.frame_set_depth(VC.depth_at(VC.view(k), CAM), CAM, 1.0, *RANGE)
        ids.append(add_keyframe(ctx, rng, VC.view(k), CAM))
    box = ctx.volume_map_bounds()
    for count in (8, 64):
        if only not in (None, "vol256_%d" % count):
            continue
        lst = (ids * 8)[:count]
        window = lambda: ctx.volume_fuse_keyframes(lst, clear=True)                       # noqa: E731
        sparse = lambda: ctx.volume_map_fuse_keyframes(lst, clear=True, box=box)          # noqa: E731
        window()
        want = ctx.volume_download().view(np.uint32)
        stats = sparse()
        assert np.array_equal(want, ctx.volume_download().view(np.uint32)) and (want != 0).any()
        res = {"stats": stats, "frame": interleaved(ctx, {"window": window, "map": sparse}, reps)}
        res["map_over_window"] = round(res["frame"]["map"]["median_us"] / res["frame"]["window"]["median_us"], 3)
        out["vol256_%d" % count] = res
    ctx.close()
    if only not in (None, "walk"):
        return 0
    # ---- (b) the drifted walk's map
    ctx = api.Context(0)
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(4096)
    P, at, ids = MFC.walk_poses("drifted"), MFC.keyframe_positions(), []
    for n in range(len(AC.PATH)):
        if n:
            sh = ctx.volume_follow(P[n], SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(P[n])
        if n in at:
            ids.append(add_keyframe(ctx, rng, P[n], AC.CAM))
    Q = MFC.walk_poses("corrected")
    poses = [Q[n] for n in at]
    lo, hi = ctx.volume_map_bounds()
    total = ctx.volume_geometry()["total_shift"]
    stops = [np.array([x, int(lo[1]), int(lo[2])], np.int64) for x in range(int(lo[0]), int(hi[0]), AC.DIMS[0])]
    assert all(int(hi[a] - lo[a]) == AC.DIMS[a] for a in (1, 2)) and np.array_equal(total[1:], lo[1:])   # the box is one window high and deep

    def sparse():
        return ctx.volume_map_fuse_keyframes(ids, poses, clear=True, box=(lo, hi))

    def park():
        at_now = total.copy()
        for stop in stops + [total]:
            ctx.volume_shift(stop - at_now)
            at_now = stop
            if stop is not total:
                ctx.volume_fuse_keyframes(ids, poses, clear=True)
    stats = sparse()
    a = in_box(ctx, lo, hi)
    park()
    b = in_box(ctx, lo, hi)
    # the same content up to the origin's rounding: a stop's window has its own fp32 origin, the box one for all of it, so voxel centres
    # differ by an ulp beyond the first stop: the tsdf's last bits, and a voxel at the edge of the band may fall the other way
    fa, fb = a[0].view(np.float32), b[0].view(np.float32)
    differ = float(((np.abs(fa[..., 0] - fb[..., 0]) > 1e-3) | (fa[..., 1] != fb[..., 1])).mean())   # beyond rounding: the voxel was updated otherwise
    assert differ < 0.01 and len(a[1]) > 100 and abs(len(a[1]) - len(b[1])) <= 0.02 * len(a[1]), (differ, len(a[1]), len(b[1]))
    res = {"window_voxels_that_differ": differ, "held_park": int(len(b[1])), "held": int(len(a[1])), "box": [int(x) for x in hi - lo], "keyframes": len(ids), "stops": len(stops), "stats": stats,
           "frame": interleaved(ctx, {"map": sparse, "park": park}, reps)}
    res["map_over_park"] = round(res["frame"]["map"]["median_us"] / res["frame"]["park"]["median_us"], 3)
    out["walk"] = res
    ctx.close()
    if kernels:
        return 0
    line = json.dumps(out)
    print(line)
    with open(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel-trace":
        merge_kernel_trace(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        sys.exit(main())
