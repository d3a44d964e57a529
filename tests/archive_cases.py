"""The use case of the volume archive, shared by the CPU oracle test and the GPU test: the camera of tests/shift_cases.py walks out
along its path (every 6th frame) and comes back over the same poses.  The 64 x 64 x 64 window at 4 cm follows it in steps of a brick
(granule 8).  Every frame is fused at its TRUE pose, so integrate and raycast are bit-exact on the GPU and the figures need no margin.
Without the archive every slab that re-enters on the way back starts empty; with it the slab returns as it left.  Before a frame is
fused the window is raycast from the frame's pose: the hits say what the map already knows there.  The figures below were measured
with the oracle (oracle_walk; tests/test_archive_oracle.py recomputes them)."""
import hashlib

import numpy as np

import archive_oracle as AO
import shift_cases as SC
import shift_oracle as SO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO

CAM = SC.CAM
DIMS, VOXEL = SC.DIMS, SC.VOXEL                  # 64^3 at 4 cm
GRANULE = 8
STRIDE = 6
OUT = list(range(0, SC.FRAMES, STRIDE))          # frames 0, 6 .. 72 of shift_cases.path_pose
PATH = OUT + OUT[-2::-1]                         # ... and back over the same poses: 25 frames, the last one the start pose
RETURN = range(len(OUT), len(PATH))              # the return leg, as positions in PATH


def pose(n):
    return SC.path_pose(PATH[n])


def depth(n):
    """the depth image of position n of the walk: a fixed seed per position"""
    return VC.depth_at(pose(n), CAM, SC.NOISE, np.random.default_rng(100 + n))


def hits(MV, n):
    """(pixels of position n with a true depth that have a raycast hit, pixels with a true depth): shift_cases.hit_share as two counts"""
    has = VC.depth_at(pose(n), CAM).reshape(-1) > 0
    return int((has & ~np.isnan(MV).any(1)).sum()), int(has.sum())


def digest(vol):
    """sha256 of the volume's bits, every NaN taken as the same NaN"""
    a = np.ascontiguousarray(vol, np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return hashlib.sha256(a.view(np.uint32).tobytes()).hexdigest()


def oracle_walk(archive):
    """per position: follow -> shift (through the store model, or shift_oracle.shift without the archive) -> raycast -> integrate.
    Returns dict(hits = per position of the return leg, pixels likewise, peak = most bricks held after any shift, in_flight = most
    slots in use DURING a shift (the leaving bricks are gathered before the entering ones give their slots back: what a pool must
    hold), mean_weight of the final window, window = the final window, total)"""
    total = (0, 0, 0)
    G = SC.geometry(total)
    vol = G.empty()
    store, peak, in_flight, got, pix = {}, 0, 0, [], []
    for n in range(len(PATH)):
        p = pose(n)
        if n:
            sh = SO.follow(p, SC.LOOK_AHEAD, GRANULE, SO.origin_after(SC.first_origin(), VOXEL, total), DIMS, VOXEL)
            if sh.any():
                if archive:
                    before = set(store)
                    vol, _, total = AO.shift(vol, None, total, sh, store)
                    peak = max(peak, len(store))
                    in_flight = max(in_flight, len(before | set(store)))   # what left is in the pool before what returns is out of it
                else:
                    vol, total = SO.shift(vol, None, sh)[0], tuple(int(t) + int(s) for t, s in zip(total, sh))
                G = SC.geometry(total)
            if n in RETURN:
                MV, _ = VO.raycast(vol, G, CAM, p, *SC.RAY)
                h, m = hits(MV, n)
                got.append(h)
                pix.append(m)
        vol = VO.integrate(vol, G, FO.frame_maps(depth(n), CAM, 1.0, *SC.RANGE)[0], CAM, p)
    return dict(hits=got, pixels=pix, peak=peak, in_flight=in_flight, mean_weight=float(vol[..., 1].mean()), window=vol, total=total, digest=digest(vol))


# ---- the figures (oracle_walk, measured on the CPU; tests/test_archive_oracle.py recomputes them)
# Every pixel of the 160 x 120 camera has a true depth in the room: 19 200 per frame.  Raycast hits per position of the return leg
# (frames 66, 60 .. 0), before the frame is fused:
PIXELS = 19200
HITS_ARCHIVE = [13148, 13073, 12283, 11561, 11990, 12822, 12490, 12408, 11194, 10765, 10187, 9584]
HITS_PLAIN = [13148, 13073, 10853, 9908, 9870, 10483, 11260, 10118, 8937, 7695, 5956, 5263]
# At the last return frame -- the start pose -- the archive shows 49.9 % of the view against 27.4 %: 1.82 x (the condition on the case
# is 1.5 x); over the return leg the mean is 61 % against 51 %.  The first two positions agree: nothing has re-entered yet.
GAIN_LIMIT = 1.5
# The archive peaks at 507 bricks held after a shift (the condition on the case is <= 512).  DURING a shift the bricks that leave are in
# the pool before the ones that return have given their slots back: at most 565 slots are in use at once, and that is the capacity
# the GPU test gives the pool -- exactly enough.  The final window's mean weight is 3.25 with the archive, 1.47 without; and the final
# windows differ, bit for bit these (digest: sha256 over the bits, every NaN the same NaN):
PEAK_HELD, PEAK_LIMIT = 507, 512
PEAK_IN_FLIGHT = 565
CAPACITY = PEAK_IN_FLIGHT
MEAN_WEIGHT_ARCHIVE, MEAN_WEIGHT_PLAIN = 3.2548, 1.4688
DIGEST_ARCHIVE = "3a2026f965fae8a82c1e5749e452409c963f51bda0ab7816e6fb78c0e93fe13d"
DIGEST_PLAIN = "4d5eabf27e534184a41eb214a70bb4073b517ffebfc3d6ffcdc489d94c6d6023"
