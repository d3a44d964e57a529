"""The volume archive on one GPU: volume_shift((8, 0, 0)) and the shift back at 256^3 and 512^3, with and without
a colour volume, over four routes in the SAME run, interleaved round by round after their bits were compared:
  "off"        the archive off: the plain shift, the baseline
  "empty"      the archive on over an empty window: the occupancy kernel, the host wait and the shift, nothing to copy
  "room"       the archive on, the room fused from four views (realistic occupancy)
  "full"       the archive on, every brick non-zero: a whole slab of bricks is gathered on the way out and scattered on the way back
Host wall around a synchronise, medians.  Per route: the bricks archived and restored, out_us / back_us, and -- by DIFFERENCES of the
medians, since the phases run behind one another on one stream -- a1_wait_us = empty - off, gather_us = out - empty's out, scatter_us =
back - empty's back, and the gather / scatter rate in TB/s over bytes read + written.  The device's own kernel times come from a
separate `rocprofv3 --kernel-trace --stats -- python scripts/archive_time.py --kernels 512` run.  Every volume size runs in a child
process under `timeout -k 10`; the script stops at the first non-zero status.  Prints one JSON line and writes it to argv[1] when
given (profiles/archive_time.json)."""
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
OUT, BACK = (8, 0, 0), (-8, 0, 0)
STEP_LIMIT_S = 420
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room
REPS = 9
ROUTES = ("off", "empty", "room", "full")


def timed(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def fill(ctx, route, n, colour):
    """the route's content in a fresh volume"""
    import numpy as np
    s = SIDE / n
    ctx.volume_init((n, n, n), s, ORIGIN, 3 * s, 64)
    if route == "room":
        import volume_cases as VC
        from rgbd_pose_estimation_amd import simulator as S
        cam = S.DEFAULT_CAMERA
        rng = np.random.default_rng(3)
        for k in range(4):
            ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, 0.1, 10.0, 0.1)
            if colour:
                ctx.frame_set_color(rng.integers(1, 256, (cam[5], cam[4], 3)).astype(np.uint8))
                ctx.volume_integrate_color(VC.view(k))
            else:
                ctx.volume_integrate(VC.view(k))
    elif route in ("off", "full"):
        rng = np.random.default_rng(n)
        ctx.volume_upload(rng.standard_normal((n, n, n, 2), dtype=np.float32))
        if colour:
            ctx.volume_color_upload(rng.integers(1, 0x5c00, (n, n, n, 4), dtype=np.uint16).view(np.float16))
    elif colour:
        ctx.volume_color_upload(np.zeros((n, n, n, 4), np.float16))
    if route != "off":
        ctx.volume_archive((n // 8) ** 2)


def step(ctx, d):
    ctx.volume_shift(d)
    ctx.synchronize()


def kernels_only(n):
    from rgbd_pose_estimation_amd import api
    ctx = api.Context(0)
    fill(ctx, "full", n, True)
    for _ in range(5):
        step(ctx, OUT)
        step(ctx, BACK)


def child(n, path):
    import numpy as np

    import shift_oracle as SO
    from rgbd_pose_estimation_amd import api

    out = {"voxel_m": SIDE / n, "slab_bricks": (n // 8) ** 2}
    for colour in (False, True):
        ctxs = {r: api.Context(0) for r in ROUTES}
        for r in ROUTES:
            fill(ctxs[r], r, n, colour)
        rec = {r: {} for r in ROUTES}
        # the bits first: out with the archive on is the plain shift of the same content; out and back is the identity
        for r in ("room", "full"):
            c = ctxs[r]
            v0 = c.volume_download()
            c0 = c.volume_color_download().view(np.uint16) if colour else None
            step(c, OUT)
            rec[r]["archived"] = c.volume_archive_info()["held"]
            want, cwant = SO.shift(v0, c0, OUT)
            assert np.array_equal(c.volume_download().view(np.uint32), want.view(np.uint32)), "archive on: out != plain shift"
            assert not colour or np.array_equal(c.volume_color_download().view(np.uint16), cwant), "archive on: colour out != plain shift"
            del want, cwant
            step(c, BACK)
            rec[r]["restored"] = rec[r]["archived"] - c.volume_archive_info()["held"]
            assert np.array_equal(c.volume_download().view(np.uint32), v0.view(np.uint32)), "out and back is not the identity"
            assert not colour or np.array_equal(c.volume_color_download().view(np.uint16), c0), "colour: out and back is not the identity"
            del v0, c0
        for r in ("off", "empty"):                                   # warm-up: the spares exist now
            step(ctxs[r], OUT); step(ctxs[r], BACK)
            rec[r]["archived"] = rec[r]["restored"] = 0
        t = {r: ([], []) for r in ROUTES}
        for _ in range(REPS):                                        # interleaved: one out and one back of each route per round
            for r in ROUTES:
                t[r][0].append(timed(lambda: step(ctxs[r], OUT)))
                t[r][1].append(timed(lambda: step(ctxs[r], BACK)))
        for r in ROUTES:
            rec[r]["out_us"], rec[r]["back_us"] = statistics.median(t[r][0]), statistics.median(t[r][1])
            rec[r]["out_min_max_us"] = [min(t[r][0]), max(t[r][0])]
            rec[r]["back_min_max_us"] = [min(t[r][1]), max(t[r][1])]
        per_brick = 2 * 4096 * (2 if colour else 1)                  # read + written
        rec["empty"]["a1_wait_us"] = rec["empty"]["out_us"] - rec["off"]["out_us"]
        for r in ("room", "full"):
            rec[r]["on_minus_off_us"] = rec[r]["out_us"] - rec["off"]["out_us"]
            rec[r]["gather_us"] = rec[r]["out_us"] - rec["empty"]["out_us"]
            rec[r]["scatter_us"] = rec[r]["back_us"] - rec["empty"]["back_us"]
            for k, cnt in (("gather", rec[r]["archived"]), ("scatter", rec[r]["restored"])):
                us = rec[r][k + "_us"]
                rec[r][k + "_TBps"] = cnt * per_brick / us / 1e6 if us > 0 else None
        nvox = n ** 3
        rec["shift_bytes"] = 2 * nvox * 8 * (2 if colour else 1)
        rec["gather_share_of_shift_bytes"] = rec["full"]["archived"] * per_brick / rec["shift_bytes"]
        out["colour" if colour else "tsdf"] = rec
        for c in ctxs.values():
            c.close()
    with open(path, "w") as f:
        json.dump(out, f)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        return kernels_only(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), sys.argv[3])
    out = {"sizes": list(SIZES), "shift": list(OUT), "reps": REPS}
    for n in SIZES:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "part.json")
            rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(n), path])
            if rc != 0:
                print(f"archive_time: size {n} ended with status {rc}; stopping", file=sys.stderr)
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
