"""Scenes shared by the keyframe tests (CPU oracle and GPU): eight keyframes around the default room and one query frame near each,
at two camera sizes; a store of both cameras; the repeated texture whose descriptors tie; a flat query frame.  The figures next to
each case are the ORACLE's (tests/test_keyframe_oracle.py recomputes them)."""
import numpy as np

import color_oracle as CO
import feature_cases as FC
import feature_oracle as FE
import keyframe_oracle as KO
import photo_cases as PC
import volume_cases as VC
from frontend_util import FO, SMALL_CAM

HALF_CAM = FC.HALF_CAM
CAMS = {"small": SMALL_CAM, "half": HALF_CAM}
NOISE = 0.002
# the keyframes' poses: feature_cases.START moved by these (photo_cases.moved: rx ry rz x y z), a fan across the room
KF_MOTIONS = ((0, 0, 0, 0, 0, 0), (0, -.35, 0, .5, 0, .1), (0, -.7, 0, .9, 0, .2), (0, .35, 0, -.5, 0, .1), (0, .7, 0, -.9, 0, .2),
              (.1, -1.05, 0, 1, .1, .3), (.05, 1.05, 0, -1, .1, .3), (.2, 0, 0, 0, .3, .4))
QUERY_MOTION = FC.WIDE1          # query i = keyframe i's pose moved by this
KF_SEED, QUERY_SEED = 100, 200   # depth noise: seeds KF_SEED + i, QUERY_SEED + i
CANDIDATES, MIN_MATCHES = 3, 12


class Shot:
    """one camera position: pose, what the GPU is given (depth, rgb) and the oracle's maps -- as a frame (V N B, camera frame) and as a
    model view in the world at its true pose (MV MN, rgba)"""
    def __init__(self, pose, cam, seed, rgb=None):
        self.pose, self.cam = pose, cam
        self.w, self.h = cam[4], cam[5]
        self.depth = PC.depth_at(pose, cam, None, NOISE, np.random.default_rng(seed))
        self.rgb = FC.rgb_at(pose, cam) if rgb is None else rgb
        self.rgba = CO.frame_rgba(self.rgb).reshape(self.h, self.w, 4).copy()
        self.V, self.N, self.B = FO.frame_maps(self.depth, cam, 1.0, *VC.RANGE)
        self.MV, self.MN = FO.to_world(self.V, self.N, pose)

    def keyframe(self, *fopt):
        return KO.keyframe(self.rgba, self.MV, self.MN, *fopt)

    def features(self, *fopt):
        """(xy, desc) of the shot as a frame"""
        xy, _, desc = FE.detect(self.rgba, self.V, self.N, *fopt)
        return xy, desc

    def as_frame(self, ctx):
        ctx.frame_set_depth(self.depth, self.cam, dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])
        ctx.frame_set_color(self.rgb)

    def as_model(self, ctx):
        """the shot as the model of a context, through the existing upload path, and its features detected"""
        ctx.model_upload(self.MV, self.MN, self.cam, self.pose)
        ctx.model_color_upload(self.rgba)
        from rgbd_pose_estimation_amd import _lib as L
        return ctx.features_detect(L.FEAT_MODEL)

    def match(self, kf, mopt=KO.MOPT):
        xy, desc = self.features()
        return KO.match(xy, desc, self.V, self.N, self.B, self.w, kf, mopt)


_ROOMS = {}


class Room:
    """the eight keyframes and the eight queries at one camera"""
    def __init__(self, cam):
        self.cam = cam
        self.kf_poses = [PC.moved(FC.START, *m) for m in KF_MOTIONS]
        self.shots = [Shot(p, cam, KF_SEED + i) for i, p in enumerate(self.kf_poses)]
        self.keyframes = [s.keyframe() for s in self.shots]
        self.queries = [Shot(PC.moved(p, *QUERY_MOTION), cam, QUERY_SEED + i) for i, p in enumerate(self.kf_poses)]

    def fill(self, ctx):
        """the eight keyframes into the context's store through keyframe_add; returns their ids"""
        ids = []
        for s in self.shots:
            s.as_model(ctx)
            ids.append(ctx.keyframe_add())
        return ids


def room(name):
    if name not in _ROOMS:
        _ROOMS[name] = Room(CAMS[name])
    return _ROOMS[name]


def correct(q, m):
    """per match: the world distance between the matched points at the query's true pose is below feature_cases.CORRECT_DIST"""
    R, t = q.pose[:9].reshape(3, 3).astype(np.float64), q.pose[9:]
    Xw = (m["XC"].astype(np.float64) - t) @ R
    return np.linalg.norm(Xw - m["XW"], axis=1) < FC.CORRECT_DIST


def oracle_relocalise(oracle_lib, q, keyframes, candidates=CANDIDATES, min_matches=MIN_MATCHES, mopt=KO.MOPT):
    """the oracle's walk for the query shot q: dict(counts, order, keyframe, pose12, votes, iters, match) -- pose12 None when degenerate"""
    xy, desc = q.features()
    counts, order = KO.query(desc, keyframes, mopt)
    lists = {}

    def run(i):
        lists[i] = KO.match(xy, desc, q.V, q.N, q.B, q.w, keyframes[i], mopt)
        pose, r = FC.oracle_relocalise(oracle_lib, q, lists[i])
        return r["max_votes"], (pose, r)

    win, got = KO.walk(counts, order, candidates, min_matches, run)
    if got is None:
        return dict(counts=counts, order=order, keyframe=win, pose12=None)
    return dict(counts=counts, order=order, keyframe=win, pose12=got[0], votes=got[1]["max_votes"], iters=got[1]["iters"], match=lists[win])


def two_camera_store():
    """keyframes 0, 2, 4, 6 at SMALL_CAM and 1, 3, 5, 7 at HALF_CAM, in id order: [(shot, keyframe)]"""
    out = []
    for i in range(len(KF_MOTIONS)):
        r = room("small" if i % 2 == 0 else "half")
        out.append((r.shots[i], r.keyframes[i]))
    return out


def tiled_store(cam=SMALL_CAM):
    """the repeated texture of feature_cases.tiled_pair seen from three of the poses (descriptors repeat inside and across keyframes),
    and the query: the texture with one pixel in fifty replaced.  Ratio 2 / 1 lets the ties through"""
    p = FC.tiled_pair(cam)
    shots = [Shot(PC.moved(FC.START, *KF_MOTIONS[i]), cam, KF_SEED + i, rgb=p.ca) for i in (0, 1, 3)]
    q = Shot(p.pb, cam, QUERY_SEED, rgb=p.cb)
    return shots, [s.keyframe() for s in shots], q


def flat_query(cam=SMALL_CAM):
    """a frame of one colour: no keypoint"""
    return Shot(PC.moved(FC.START, *QUERY_MOTION), cam, QUERY_SEED, rgb=np.full((cam[5], cam[4], 3), 128, np.uint8))


def tiny_keyframe(i, count=3, seed=5):
    """a host keyframe of `count` random descriptors (for stores of exact shapes): dict as keyframe_oracle.keyframe's, 64 x 48 image"""
    rng = np.random.default_rng(seed * 1000 + i)
    xy = np.stack([rng.integers(0, 64, count), rng.integers(0, 48, count)], 1).astype(np.int32)
    desc = rng.integers(0, 1 << 32, (count, 8), dtype=np.uint64).astype(np.uint32)
    return dict(xy=xy, desc=desc, xw=rng.normal(size=(count, 3)).astype(np.float32), nw=rng.normal(size=(count, 3)).astype(np.float32))


# ---- the oracle's figures (tests/test_keyframe_oracle.py recomputes every one).  Per camera: the keyframes' keypoints, and per query
# i (keyframe i's pose moved by QUERY_MOTION): the query's counts (defaults: max_dist 64, ratio 8 / 10, no cross-check), the keyframe
# the walk over CANDIDATES = 3 keeps, its votes and adapted Iter (feature_cases.oracle_relocalise: M_SK_PROSAC + LS_SHINJI_INLIERS,
# RELOC_*), `reloc` = the pose's error against the truth (volume_cases.pose_error: rotation rad, camera centre m), `icp` = where oracle
# RGB-D pyramid ICP against the winning keyframe ends from that pose.  Query 6 is the one whose second-ranked keyframe is the closer
# one; the walk keeps the first on its votes.  Every query at both cameras lands within RELOC_BOUND.
# Where the ICP ends is held to two bounds, for all sixteen queries (test_keyframe_oracle.py):
#  (a) TRACK_MARGIN x the end of the SAME ICP on the SAME pair started at the true pose.  That end is the tracker's own figure for the
#      pair (its fixed point on these noisy maps), so this is the claim itself: relocalisation hands the tracker a start from which it
#      ends where tracking ends.  Both runs have the same fixed iteration budget and descend to the same minimum; 2 is the margin this
#      suite gives a loop that repeats another's arithmetic from another start.  (The two ends agree to three digits in every query.)
#  (b) TRACK_ORDER[cam] x photo_cases.PAIR_ROOM_RGBD, "the order of a tracked pair".  10 at HALF_CAM is the rule test_feature_oracle.py
#      holds its own wide pairs to at that camera.  At SMALL_CAM that rule does NOT hold -- the ICP ends at 0.4 - 1.1 mrad / 1.4 - 3.9 mm,
#      up to 21 x / 12 x the pair's figure, from the true pose just the same, so it is the tracker's floor on a 0.27 rad / 0.3 m pair at
#      160 x 120 and not the relocalisation's doing.  The bound there is the HALF_CAM one scaled by the camera: the end is a mean of
#      per-pixel errors -- depth noise (the same in metres), projective association and the colour gradient (both proportional to the
#      pixel pitch) -- over the overlapping pixels, so it scales as pitch / sqrt(pixels): twice the pitch and a quarter of the pixels
#      give 2 x 2 = 4, hence 40.
FIGURES = {
    "small": dict(keypoints=(480, 566, 519, 490, 535, 493, 459, 537), queries=[
        dict(counts=[189, 211, 102, 102, 29, 42, 20, 150], keyframe=1, votes=388, iters=3, reloc=(7.20e-04, 4.20e-03), icp=(4.05e-04, 2.31e-03)),
        dict(counts=[71, 286, 270, 45, 9, 143, 12, 69], keyframe=1, votes=522, iters=3, reloc=(1.36e-03, 5.29e-03), icp=(4.38e-04, 1.42e-03)),
        dict(counts=[37, 153, 317, 23, 12, 253, 13, 25], keyframe=2, votes=590, iters=3, reloc=(2.13e-03, 3.78e-03), icp=(1.05e-03, 3.93e-03)),
        dict(counts=[197, 82, 27, 198, 59, 12, 29, 135], keyframe=3, votes=371, iters=3, reloc=(2.46e-03, 8.33e-03), icp=(4.25e-04, 2.28e-03)),
        dict(counts=[79, 29, 19, 185, 232, 10, 110, 62], keyframe=4, votes=430, iters=3, reloc=(3.55e-03, 9.57e-03), icp=(8.05e-04, 2.65e-03)),
        dict(counts=[13, 57, 165, 7, 13, 287, 18, 14], keyframe=5, votes=537, iters=3, reloc=(2.12e-03, 9.91e-04), icp=(4.04e-04, 1.43e-03)),
        dict(counts=[32, 15, 25, 66, 250, 13, 235, 29], keyframe=4, votes=461, iters=3, reloc=(3.62e-03, 1.00e-02), icp=(1.04e-03, 3.29e-03)),
        dict(counts=[121, 130, 59, 74, 18, 15, 18, 220], keyframe=7, votes=407, iters=3, reloc=(2.64e-03, 9.61e-03), icp=(6.97e-04, 2.50e-03)),
    ]),
    "half": dict(keypoints=(1210, 1328, 1076, 1104, 1051, 891, 797, 1309), queries=[
        dict(counts=[588, 636, 303, 232, 110, 184, 64, 537], keyframe=1, votes=1180, iters=3, reloc=(1.23e-03, 4.04e-03), icp=(1.03e-04, 8.74e-04)),
        dict(counts=[232, 715, 615, 126, 79, 319, 69, 246], keyframe=1, votes=1351, iters=2, reloc=(3.10e-04, 5.32e-04), icp=(7.27e-05, 2.99e-04)),
        dict(counts=[154, 401, 610, 97, 79, 479, 62, 155], keyframe=2, votes=1146, iters=3, reloc=(2.15e-04, 1.14e-03), icp=(1.20e-04, 6.41e-04)),
        dict(counts=[502, 193, 117, 549, 261, 63, 98, 397], keyframe=3, votes=1029, iters=3, reloc=(2.47e-04, 8.41e-04), icp=(1.92e-04, 6.93e-04)),
        dict(counts=[231, 142, 80, 567, 576, 59, 297, 196], keyframe=4, votes=1084, iters=3, reloc=(3.79e-04, 1.37e-03), icp=(1.77e-04, 9.50e-04)),
        dict(counts=[88, 196, 280, 131, 113, 486, 71, 102], keyframe=5, votes=851, iters=4, reloc=(8.65e-04, 2.12e-03), icp=(1.12e-04, 3.44e-04)),
        dict(counts=[126, 86, 75, 301, 560, 63, 464, 132], keyframe=4, votes=1015, iters=3, reloc=(9.25e-04, 3.05e-03), icp=(2.37e-04, 9.86e-04)),
        dict(counts=[424, 436, 219, 210, 101, 129, 55, 712], keyframe=7, votes=1355, iters=2, reloc=(5.44e-04, 3.11e-03), icp=(3.21e-04, 7.47e-04)),
    ]),
}
RELOC_BOUND = (5e-3, 15e-3)
TRACK_MARGIN = 2
TRACK_ORDER = {"half": 10, "small": 40}
# other cases.  two_camera_store: counts of SMALL_CAM query 0 and HALF_CAM query 1 -- a keyframe of the other camera still collects a
# few matches; the tiled store at ratio 2 / 1: 459 query keypoints, 392 / 380 / 389 per keyframe, EQUAL counts (the ranking falls back
# on the ids), 361 of keyframe 0's 453 matches are ties d1 = d2; with the cross-check on top the counts differ again
TWO_CAMERA = {("small", 0): dict(counts=[189, 15, 102, 9, 29, 13, 20, 12], keyframe=0, votes=346, iters=3),
              ("half", 1): dict(counts=[75, 715, 85, 126, 50, 319, 66, 246], keyframe=1, votes=1351, iters=2)}
TILED = dict(keypoints=(459, (392, 380, 389)), counts=[453, 453, 453], order=[0, 1, 2], ties=361, cross_counts=[57, 52, 54], cross_order=[0, 2, 1])
CROSS_SMALL_0 = [183, 196, 92, 93, 28, 38, 18, 139]        # room "small", query 0, cross-check on
