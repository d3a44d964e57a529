"""Host wall time of the first `api.Context(0)` of a process: library load, HIP start-up, the workspace and the walk over every kernel
unit's RPE_PRELOAD node (rpe_create loads each unit's code object there).  One figure per process by nature, so every run is a fresh one.

    python scripts/create_time.py                         one run of the built library (or of RPE_LIBRARY): prints milliseconds
    python scripts/create_time.py --ab OLD.so NEW.so [N]  N (default 9) pairs, OLD first, alternating, each run a fresh child process with
                                                          RPE_LIBRARY set, behind one unrecorded run of each; prints one JSON line with the raw times.  ok = NEW's median
                                                          does not exceed OLD's slowest run (the yardstick of profiles/rules_ab.json)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one():
    from rgbd_pose_estimation_amd import api
    t = time.perf_counter()
    ctx = api.Context(0)
    ms = (time.perf_counter() - t) * 1e3
    ctx.close()
    return ms


def child(lib):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, RPE_LIBRARY=os.path.abspath(lib)), check=True,
                         capture_output=True, text=True, timeout=120).stdout
    return float(out.split()[-1])


def main(argv):
    if not argv:
        print(f"{one():.3f}")
        return 0
    old, new, n = argv[1], argv[2], int(argv[3]) if len(argv) > 3 else 9
    times = {"parent": [], "new": []}
    child(old), child(new)   # not recorded: the first process on a machine also pays for the file cache and the driver's start
    for _ in range(n):
        times["parent"].append(child(old))
        times["new"].append(child(new))
    res = dict(what="first api.Context(0) of a fresh process, host wall ms, behind one unrecorded run of each library", pairs=n, **times, parent_median=statistics.median(times["parent"]),
               parent_slowest=max(times["parent"]), new_median=statistics.median(times["new"]))
    res["ok"] = res["new_median"] <= res["parent_slowest"]
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
