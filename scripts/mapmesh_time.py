"""The map mesh on one GPU.  A 256^3 window over the room fused from four views; the extraction alone (the C
call: list, upload, launches, the one wait; no download), host wall around a synchronise, medians of interleaved rounds AFTER the
bits were compared (the two meshes as sorted triangles of position and normal words):
  "dense"      rpe_volume_mesh of the window: the parent's route, the baseline
  "map"        rpe_volume_map_mesh of the window's extent, nothing archived: the same triangles, brick by brick
  "map+512"    the same window after 512 bricks of a slab have left into the archive, the whole map
  "map+4096"   ... after 4 096 bricks (four slabs) have left
The archived bricks hold a plane across the slab: every one of them is known (no early exit), one layer of them has triangles.
"list_us" is the host's list and neighbour table on their own: the same call on an EMPTY window of the same size (every workgroup
takes the early exit, no vertex, no second pair of launches) minus the same call over a single brick.  The use case of
tests/mapmesh_cases.py (the walk out and back, 64^3 window, 507 bricks held) is timed whole-map against window-only.  The device's
kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/mapmesh_time.py --kernels` run.  Prints one
JSON line and writes it to argv[1] when given (profiles/mapmesh_time.json)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N = 256
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
REPS = 9


def timed(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def room(ctx):
    import volume_cases as VC
    from rgbd_pose_estimation_amd import simulator as S
    cam = S.DEFAULT_CAMERA
    for k in range(4):
        ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, 0.1, 10.0, 0.1)
        ctx.volume_integrate(VC.view(k))


def window(n=N):
    from rgbd_pose_estimation_amd import api
    ctx = api.Context(0)
    s = SIDE / n
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
    return ctx


def with_archive(slabs, rows):
    """the room's window after `slabs` x-slabs of bricks, `rows` brick rows high, have left into the archive"""
    import numpy as np
    ctx = window()
    ctx.volume_archive(8192)
    vol = np.zeros((N, N, N, 2), np.float32)
    z = np.arange(N, dtype=np.float32)[:, None, None]
    vol[:, : 8 * rows, : 8 * slabs, 0] = np.clip((z - (N / 2 + 0.3)) / 3, -1, 1)
    vol[:, : 8 * rows, : 8 * slabs, 1] = 2
    ctx.volume_upload(vol)
    ctx.volume_shift((8 * slabs, 0, 0))
    assert ctx.volume_archive_info()["held"] == slabs * rows * (N // 8)
    room(ctx)
    return ctx


def extract_dense(ctx):
    from rgbd_pose_estimation_amd import _lib as L
    nv, nt = C.c_int64(0), C.c_int64(0)
    L.check(L.lib().rpe_volume_mesh(ctx._h, 1.0, C.byref(nv), C.byref(nt)))
    ctx.synchronize()
    return nt.value


def extract_map(ctx, box=None):
    import numpy as np
    from rgbd_pose_estimation_amd import _lib as L
    nv, nt = C.c_int64(0), C.c_int64(0)
    lo, hi = (None, None) if box is None else (np.ascontiguousarray(b, np.int64) for b in box)
    L.check(L.lib().rpe_volume_map_mesh(ctx._h, 1.0, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                        C.byref(nv), C.byref(nt)))
    ctx.synchronize()
    return nt.value


def use_case():
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


def kernels_only():
    ctx = window()
    room(ctx)
    for _ in range(5):
        extract_dense(ctx)
        extract_map(ctx)
    ctx = with_archive(4, N // 8)
    for _ in range(5):
        extract_map(ctx)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        return kernels_only()
    import mapmesh_cases as MC
    plain = window()
    room(plain)
    # the bits first
    Vd, Nd, Td = plain.volume_mesh(1.0)
    Vm, Nm, Tm = plain.volume_map_mesh(1.0)
    a, b = MC.triangle_words(Vd, Nd, Td), MC.triangle_words(Vm, Nm, Tm)
    assert a.shape == b.shape and (a == b).all(), "the map mesh of the window's extent is not the window's mesh"
    empty, one = window(), window(8)
    routes = {"dense": (plain, extract_dense), "map": (plain, extract_map), "map+512": (with_archive(1, 16), extract_map),
              "map+4096": (with_archive(4, N // 8), extract_map), "empty_window": (empty, extract_map), "one_brick": (one, extract_map)}
    uc = use_case()
    routes["use_case_window"] = (uc, extract_dense)
    routes["use_case_map"] = (uc, extract_map)
    out = {"n": N, "reps": REPS, "routes": {}}
    t = {r: [] for r in routes}
    tri = {r: f(c) for r, (c, f) in routes.items()}                  # warm-up: workspaces and buffers exist now
    for _ in range(REPS):
        for r, (c, f) in routes.items():
            t[r].append(timed(lambda: f(c)))
    for r in routes:
        out["routes"][r] = {"triangles": tri[r], "us": statistics.median(t[r]), "min_max_us": [min(t[r]), max(t[r])]}
    for r in ("map", "map+512", "map+4096", "use_case_map"):
        c = routes[r][0]
        lo, hi = c.volume_map_bounds()
        out["routes"][r]["held"] = c.volume_archive_info()["held"]
        out["routes"][r]["box"] = [int(x) for x in hi - lo]
    out["list_us"] = out["routes"]["empty_window"]["us"] - out["routes"]["one_brick"]["us"]
    out["map_over_dense"] = out["routes"]["map"]["us"] / out["routes"]["dense"]["us"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
