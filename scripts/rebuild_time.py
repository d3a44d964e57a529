"""The volume rebuilt from keyframes at 640 x 480: the room cube of scripts/volume_time.py at 256^3 and 512^3,
stores of 8, 64 and 256 keyframes -- the fan of tests/keyframe_cases.py KF_MOTIONS, repeated with small offsets -- each carrying its
depth and colour.  Four routes, interleaved in one process per volume size, each with a warm-up and a host wait around the timed region
(host wall, medians):
  (a) the route that needs nothing of this feature: clear, then per keyframe the host upload + frame_set_depth + frame_set_color +
      volume_integrate_color                                                   "sequential_color_us"
  (b) volume_fuse_keyframes(clear, color)                                      "fuse_color_us"
  (c) (b) with the cull switched off                                           "fuse_color_nocull_us"
  (d) (b) without colour, against the depth-only variant of (a)                "fuse_us", "sequential_us"
Before timing, (a) and (b) are checked once per volume size to leave the same bits.  Every volume size runs in a child process of its
own under `timeout -k 10`; the script stops at the first non-zero status.  Prints one JSON line and writes it to argv[1] when given
(profiles/rebuild_time_640.json)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

KS = (8, 64, 256)
SIZES = (256, 512)
STEP_LIMIT_S = 420
RANGE = (0.1, 10.0, 0.1)
ORIGIN, SIDE = (-2.9, -3.2, -1.2), 6.4          # scripts/volume_time.py's cube over the room


def timed(f):
    t0 = time.perf_counter_ns(); f(); return (time.perf_counter_ns() - t0) / 1e3


def child(n, path):
    import numpy as np

    import color_cases as CC
    import keyframe_cases as KC
    import photo_cases as PC
    import volume_cases as VC
    from rgbd_pose_estimation_amd import api, simulator as S

    cam = S.DEFAULT_CAMERA
    base = [PC.moved(PC.START, *m) for m in KC.KF_MOTIONS]
    depth = [VC.depth_at(p, cam) for p in base]
    rgb = [CC.rgb_at(p, cam) for p in base]

    def pose(k):
        """keyframe k: the fan's pose k % 8, nudged a little more with every turn round the fan"""
        r = k // len(base)
        return PC.moved(base[k % len(base)], 0.002 * r, -0.003 * r, 0.001 * r, 0.004 * r, -0.002 * r, 0.003 * r)

    ctx = api.Context(0)
    s = SIDE / n
    desc = ((n, n, n), s, ORIGIN, 3 * s, 64)
    out = {"voxel_m": s}
    for K in KS:
        poses = [pose(k) for k in range(K)]
        ctx.keyframes_clear()
        for k in range(K):
            t = KC.tiny_keyframe(k)
            kid = ctx.keyframe_add_host(t["xy"], t["desc"], t["xw"], t["nw"], poses[k], cam[4], cam[5])
            ctx.frame_set_depth(depth[k % 8], cam, 1.0, *RANGE)
            ctx.frame_set_color(rgb[k % 8])
            ctx.keyframe_attach_frame(kid)
        ctx.volume_init(*desc)

        def sequential(color):
            ctx.volume_init(*desc)
            for k in range(K):
                ctx.frame_set_depth(depth[k % 8], cam, 1.0, *RANGE)
                if color:
                    ctx.frame_set_color(rgb[k % 8])
                    ctx.volume_integrate_color(poses[k])
                else:
                    ctx.volume_integrate(poses[k])
            ctx.synchronize()

        def fuse(color, cull=True):
            ctx.volume_fuse_keyframes(clear=True, color=color, cull=cull)
            ctx.synchronize()

        if K == KS[0]:                             # once per volume size: (a) and (b) leave the same bits
            sequential(True)
            a, ac = ctx.volume_download().view(np.uint32), ctx.volume_color_download().view(np.uint16)
            fuse(True)
            same = bool(np.array_equal(a, ctx.volume_download().view(np.uint32)))
            del a
            same = same and bool(np.array_equal(ac, ctx.volume_color_download().view(np.uint16)))
            del ac
            out["same_bits"] = same
            if not same:
                raise SystemExit("the fuse and the sequential route differ")
        routes = {"sequential_color_us": lambda: sequential(True), "fuse_color_us": lambda: fuse(True),
                  "fuse_color_nocull_us": lambda: fuse(True, False), "fuse_us": lambda: fuse(False),
                  "fuse_nocull_us": lambda: fuse(False, False), "sequential_us": lambda: sequential(False)}
        for f in routes.values():                  # warm-up
            f()
        reps = 3 if K == 256 else 5
        ts = {k: [] for k in routes}
        for _ in range(reps):                      # interleaved, so that all see the same state of the machine
            for k, f in routes.items():
                ts[k].append(timed(f))
        row = {k: statistics.median(v) for k, v in ts.items()}
        row["speedup_color"] = row["sequential_color_us"] / row["fuse_color_us"]
        row["speedup_depth"] = row["sequential_us"] / row["fuse_us"]
        row["cull_gain_color"] = row["fuse_color_nocull_us"] / row["fuse_color_us"]
        out["K%d" % K] = row
        print(n, K, row, flush=True)
    ctx.close()
    with open(path, "w") as f:
        json.dump(out, f)


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--volume":
        return child(int(sys.argv[2]), sys.argv[3])
    out = {"cam": [585.0, 585.0, 320.0, 240.0, 640, 480], "keyframes": list(KS)}
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            part = os.path.join(tmp, "vol%d.json" % n)
            rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--volume", str(n), part])
            if rc != 0:
                print("volume %d: status %d, stopping" % (n, rc))
                sys.exit(rc)
            out["vol%d" % n] = json.load(open(part))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
