"""The map raycast on one GPU.  Host wall around a synchronise ("us") and the time the C call itself takes to
return ("call_us": the checks, the host's brick grid, its upload and the launches), medians of interleaved rounds AFTER the bits were
compared (vertex and normal maps as words):
  windows of N^3 over the room fused from four views, N = 256 and 512, raycast at 640 x 480, nothing archived, box = the window:
    "window"        rpe_volume_raycast: the parent's route, the yardstick
    "map"           rpe_volume_map_raycast with the occupancy pre-pass
    "map_noskip"    ... with RPE_MAPRAY_NO_SKIP
  the final map of the walk of tests/archive_cases.py (64^3 window, 507 bricks held, bounds 136 x 64 x 64) from the walk's last
  pose, at 160 x 120 and at 640 x 480: "walk_window", "walk_map", "walk_map_noskip" (the window shows less: hits are listed)
  a tracking frame of the walk at 160 x 120 -- depth pyramid of 3 levels, raycast with its model pyramid, ICP pyramid; the integrate
  is left out so that every round sees the same map -- with either raycast: "frame_window", "frame_map" (the wrapper's default: no
  pre-pass)
The device's kernel times (grid upload apart, pre-pass, raycast kernel) come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/mapray_time.py --kernels` run.  Prints one JSON line and writes it to argv[1]
when given (profiles/mapray_time.json)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
RAY = (0.1, 7.0)
REPS = 9


def room(n):
    import volume_cases as VC
    from rgbd_pose_estimation_amd import api, simulator as S
    ctx, cam, s = api.Context(0), S.DEFAULT_CAMERA, SIDE / n
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
    for k in range(4):
        ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, 0.1, 10.0, 0.1)
        ctx.volume_integrate(VC.view(k))
    return ctx


def walk():
    import archive_cases as AC
    import shift_cases as SC
    from rgbd_pose_estimation_amd import api
    ctx = api.Context(0)
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(AC.CAPACITY)
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = ctx.volume_follow(p, SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(p)
    return ctx


def maps(ctx):
    from rgbd_pose_estimation_amd import _lib as L
    return [ctx.frame_download(m).view("uint32") for m in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL)]


def timed(ctx, f):
    """(wall with the synchronise, wall of the call alone), microseconds"""
    ctx.synchronize()
    t0 = time.perf_counter_ns()
    f()
    t1 = time.perf_counter_ns()
    ctx.synchronize()
    return (time.perf_counter_ns() - t0) / 1e3, (t1 - t0) / 1e3


def routes_of(ctx, pose, cam, ray, prefix=""):
    return {prefix + "window": (ctx, lambda: ctx.volume_raycast(pose, cam, *ray)),
            prefix + "map": (ctx, lambda: ctx.volume_map_raycast(pose, cam, *ray, skip_empty=True)),
            prefix + "map_noskip": (ctx, lambda: ctx.volume_map_raycast(pose, cam, *ray, skip_empty=False))}


def main():
    import numpy as np
    import archive_cases as AC
    import shift_cases as SC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import _lib as L, simulator as S
    kernels = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
    big, pose = S.DEFAULT_CAMERA, VC.held_out_pose()
    routes, hits = {}, {}
    for n in (256,) if kernels else (256, 512):
        ctx = room(n)
        ctx.volume_raycast(pose, big, *RAY)                          # the bits first
        a = maps(ctx)
        for skip in (True, False):
            ctx.volume_map_raycast(pose, big, *RAY, skip_empty=skip)
            assert all((x == y).all() for x, y in zip(a, maps(ctx))), "the map raycast of the window's extent is not the window's raycast"
        routes.update(routes_of(ctx, pose, big, RAY, "%d_" % n))
    w, last = walk(), AC.pose(len(AC.PATH) - 1)
    for cam, tag in ((AC.CAM, "160"), (big, "640")):
        r = routes_of(w, last, cam, SC.RAY, "walk%s_" % tag)
        for name, (c, f) in r.items():
            f()
            hits[name] = int((~np.isnan(c.frame_download(L.MAP_MODEL_VERTEX)).any(1)).sum())
        routes.update(r)
    depth = AC.depth(len(AC.PATH) - 1)

    def frame(raycast):
        w.frame_set_depth(depth, AC.CAM, 1.0, *SC.RANGE, levels=3)
        raycast(last, AC.CAM, *SC.RAY, levels=3)
        w.icp_pyramid(last, VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)
    routes["frame_window"] = (w, lambda: frame(w.volume_raycast))
    routes["frame_map"] = (w, lambda: frame(w.volume_map_raycast))
    t = {r: [] for r in routes}
    for r, (c, f) in routes.items():                                 # warm-up: buffers exist now
        f()
    for _ in range(5 if kernels else REPS):
        for r, (c, f) in routes.items():
            t[r].append(timed(c, f))
    if kernels:
        return 0
    out = {"reps": REPS, "ray": list(RAY), "walk_ray": list(SC.RAY), "walk_held": w.volume_archive_info()["held"],
           "walk_box": [int(x) for x in np.subtract(*w.volume_map_bounds()[::-1])], "hits": hits, "routes": {}}
    for r in routes:
        us, call = [x[0] for x in t[r]], [x[1] for x in t[r]]
        out["routes"][r] = {"us": statistics.median(us), "min_max_us": [min(us), max(us)], "call_us": statistics.median(call)}
    for n in (256, 512):
        base = out["routes"]["%d_window" % n]["us"]
        out["map_over_window_%d" % n] = out["routes"]["%d_map" % n]["us"] / base
        out["map_noskip_over_window_%d" % n] = out["routes"]["%d_map_noskip" % n]["us"] / base
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
