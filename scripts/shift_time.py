"""The moving volume on one GPU: volume_shift at 256^3 and 512^3, with and without a colour volume, for the
shifts (8,0,0), (0,0,8), (1,1,1), (7,0,0) and a full clear, against two yardsticks in the SAME run, interleaved round by round:
  "copy_us"   a plain device-to-device copy of the same buffers (torch tensors of the same sizes, dst.copy_(src))
  "host_us"   the route a user has without the feature: volume_download, the numpy shift of tests/shift_oracle.py, volume_upload (and
              the same for the colour volume)
Host wall around a synchronise, medians; "GBps" = bytes read + written / time.  Before anything is timed the two routes' bits are
compared.  Then, at 256^3 on the fused room: volume_mesh of a box of 8 slabs against the full volume_mesh; and the tracking loop of
tests/shift_cases.py, its frames with a shift against those without.  Every volume size runs in a child process of its own under
`timeout -k 10`; the script stops at the first non-zero status.  Prints one JSON line and writes it to argv[1] when given
(profiles/shift_time.json).  `--kernels N` only runs every shift a few times on an N^3 volume with colour: the body of a separate
`rocprofv3 --kernel-trace --stats -- python scripts/shift_time.py --kernels 512` run, whose kernel times are the device's own."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIZES = (256, 512)
SHIFTS = {"x8": (8, 0, 0), "z8": (0, 0, 8), "xyz1": (1, 1, 1), "x7": (7, 0, 0)}
STEP_LIMIT_S = 420
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
REPS, HOST_REPS = 9, 2


def timed(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def content(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((n, n, n, 2), dtype=np.float32)
    cvol = rng.integers(0, 0x5c00, (n, n, n, 4), dtype=np.uint16)
    return vol, cvol


def kernels_only(n):
    from rgbd_pose_estimation_amd import api
    ctx = api.Context(0)
    s = SIDE / n
    vol, cvol = content(n, 1)
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64).volume_upload(vol).volume_color_upload(cvol.view("float16"))
    for _ in range(5):
        for d in SHIFTS.values():
            ctx.volume_shift(d)
    ctx.synchronize()


def child(n, path):
    import numpy as np
    import torch

    import shift_oracle as SO
    from rgbd_pose_estimation_amd import api

    ctx = api.Context(0)
    s = SIDE / n
    vol, cvol = content(n, n)
    out = {"voxel_m": s}
    for colour in (False, True):
        ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64).volume_upload(vol)
        if colour:
            ctx.volume_color_upload(cvol.view(np.float16))
        nbytes = vol.nbytes + (cvol.nbytes if colour else 0)
        src = [torch.empty(vol.nbytes // 4, dtype=torch.int32, device="cuda")] + ([torch.empty(cvol.nbytes // 4, dtype=torch.int32, device="cuda")] if colour else [])
        dst = [torch.empty_like(t) for t in src]

        def copy():
            for a, b in zip(dst, src):
                a.copy_(b)
            torch.cuda.synchronize()

        def host(d):
            v = ctx.volume_download()
            c = ctx.volume_color_download().view(np.uint16) if colour else None
            v, c = SO.shift(v, c, d)
            ctx.volume_upload(v)
            if colour:
                ctx.volume_color_upload(c.view(np.float16))

        def device(d):
            ctx.volume_shift(d)
            ctx.synchronize()

        # the bits first: the device shift against the host route, from the same content
        d = SHIFTS["xyz1"]
        device(d)
        got, cgot = ctx.volume_download(), ctx.volume_color_download().view(np.uint16) if colour else None
        ctx.volume_upload(vol)
        if colour:
            ctx.volume_color_upload(cvol.view(np.float16))
        host(d)
        assert np.array_equal(got.view(np.uint32), ctx.volume_download().view(np.uint32)), "shift != host route"
        assert not colour or np.array_equal(cgot, ctx.volume_color_download().view(np.uint16)), "colour shift != host route"
        del got, cgot
        rec = {"bytes_moved": 2 * nbytes}
        copy(); device(d)                                            # warm-up (the spares exist now)
        names = list(SHIFTS) + ["clear"]
        t = {k: [] for k in names}
        tc = []
        for _ in range(REPS):                                        # interleaved: one of each per round
            tc.append(timed(copy))
            for k in names:
                dd = SHIFTS.get(k, (n, 0, 0))
                t[k].append(timed(lambda: device(dd)))
        rec["copy_us"] = statistics.median(tc)
        rec["copy_GBps"] = 2 * nbytes / rec["copy_us"] / 1e3
        for k in names:
            rec[k + "_us"] = statistics.median(t[k])
            rec[k + "_GBps"] = (nbytes if k == "clear" else 2 * nbytes) / rec[k + "_us"] / 1e3
            rec[k + "_share_of_copy"] = rec["copy_us"] / rec[k + "_us"]
        rec["host_us"] = statistics.median([timed(lambda: host(SHIFTS["x8"])) for _ in range(HOST_REPS)])
        rec["host_over_shift"] = rec["host_us"] / rec["x8_us"]
        out["colour" if colour else "tsdf"] = rec
        del src, dst
    if n == 256:
        out["mesh"] = mesh_times(ctx, n, s)
        out["track"] = track_times(ctx)
    with open(path, "w") as f:
        json.dump(out, f)


def mesh_times(ctx, n, s):
    """the room fused from four views; a box of 8 x-slabs against the full mesh (both sweep the whole volume)"""
    import volume_cases as VC
    from rgbd_pose_estimation_amd import simulator as S
    cam = S.DEFAULT_CAMERA
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
    for k in range(4):
        ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, 0.1, 10.0, 0.1)
        ctx.volume_integrate(VC.view(k))
    box = ((0, 0, 0), (8, n - 1, n - 1))
    full = ctx.volume_mesh(1.0)
    slab = ctx.volume_mesh(1.0, box=box)
    tf = statistics.median([timed(lambda: ctx.volume_mesh(1.0)) for _ in range(5)])
    tb = statistics.median([timed(lambda: ctx.volume_mesh(1.0, box=box)) for _ in range(5)])
    return {"full_us": tf, "full_triangles": len(full[2]), "box8_us": tb, "box8_triangles": len(slab[2])}


def track_times(ctx):
    """tests/shift_cases.py's walk: host wall per frame (follow, mesh of what leaves, shift, set_depth, raycast, ICP, integrate)"""
    import shift_cases as SC
    import shift_oracle as SO
    from rgbd_pose_estimation_amd import _lib as L
    ds = SC.depths()
    levels = len(SC.ITERS)
    with_shift, without = [], []
    for rep in range(3):
        ctx.volume_init(SC.DIMS, **SC.desc())
        est = SC.path_pose(0)
        ctx.frame_set_depth(ds[0], SC.CAM, 1.0, *SC.RANGE, levels=levels)
        ctx.volume_integrate(est)
        for f in range(1, SC.FRAMES):
            t0 = time.perf_counter_ns()
            sh = ctx.volume_follow(est, SC.LOOK_AHEAD, SC.GRANULE)
            if sh.any():
                for box in SO.leaving_boxes(SC.DIMS, sh):
                    ctx.volume_mesh(SC.MIN_WEIGHT, box=box)
                ctx.volume_shift(sh)
            ctx.frame_set_depth(ds[f], SC.CAM, 1.0, *SC.RANGE, levels=levels)
            ctx.volume_raycast(est, SC.CAM, *SC.RAY, levels=levels)
            est = ctx.icp_pyramid(est, SC.ITERS, SC.GATES, L.RES_P2PLANE, 1e-6, 0.8)[0]
            ctx.volume_integrate(est)
            ctx.synchronize()
            dt = (time.perf_counter_ns() - t0) / 1e3
            if rep:                                                  # the first pass warms up
                (with_shift if sh.any() else without).append(dt)
    return {"frame_with_shift_us": statistics.median(with_shift), "frames_with_shift": len(with_shift) // 2,
            "frame_without_us": statistics.median(without), "frames_without": len(without) // 2}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        return kernels_only(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), sys.argv[3])
    out = {"sizes": list(SIZES), "shifts": {k: list(v) for k, v in SHIFTS.items()}, "reps": REPS}
    for n in SIZES:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "part.json")
            rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(n), path])
            if rc != 0:
                print(f"shift_time: size {n} ended with status {rc}; stopping", file=sys.stderr)
                return rc
            out[str(n)] = json.load(open(path))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
