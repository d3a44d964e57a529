"""Scenes shared by the keyframe-graph tests (CPU oracle and GPU): the eight keyframes of keyframe_cases.room with a drift accumulated
along the ids, linked all-pairs by their own matches and refined by the gated Gauss-Newton loop with keyframe 0 as the anchor.  The
figures below are the ORACLE's (tests/test_graph_oracle.py recomputes every one)."""
import numpy as np

import graph_oracle as GO
import keyframe_cases as KC
import photo_cases as PC
import volume_cases as VC

DRIFT_SEED = 7
DRIFT_ROT, DRIFT_TRANS = 0.01, 0.02          # per step: N(0, .) rad about each axis, N(0, .) m along each axis
GATES = (0.1, 0.1, 0.05, 0.05, 0.03, 0.03, 0.03)
ANCHOR = 0
MIN_MATCHES = GO.MIN_MATCHES
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


def compose(d, p):
    """the pose p followed by d: Xc = Rd (R Xw + t) + td"""
    Rd, R = d[:9].reshape(3, 3), p[:9].reshape(3, 3)
    return np.concatenate([(Rd @ R).reshape(9), Rd @ p[9:] + d[9:]])


def drifts(count, seed=DRIFT_SEED):
    """per keyframe the accumulated drift: identity for keyframe 0, then one step more per id, composed on the left"""
    rng = np.random.default_rng(seed)
    out = [IDENTITY.copy()]
    for _ in range(1, count):
        step = PC.moved(IDENTITY, *rng.normal(0, DRIFT_ROT, 3), *rng.normal(0, DRIFT_TRANS, 3))
        out.append(compose(step, out[-1]))
    return out


def reexpress(k, true_pose, pose):
    """the keyframe's world points and normals as a tracker at `pose` would have stored them: the same camera-frame points"""
    R0, t0 = true_pose[:9].reshape(3, 3), true_pose[9:]
    R, t = pose[:9].reshape(3, 3), pose[9:]
    xc = k["xw"].astype(np.float64) @ R0.T + t0
    return dict(k, xw=((xc - t) @ R).astype(np.float32), nw=(k["nw"].astype(np.float64) @ R0.T @ R).astype(np.float32))


_CASES = {}


class Case:
    """the drifted store of one camera: true poses, drifted poses, the keyframes as stored, the oracle's edges"""
    def __init__(self, cam):
        self.cam = cam
        self.room = KC.room(cam)
        self.truth = [np.asarray(p, np.float64) for p in self.room.kf_poses]
        self.poses0 = [compose(d, p) for d, p in zip(drifts(len(self.truth)), self.truth)]
        self.keyframes = [reexpress(k, p, q) for k, p, q in zip(self.room.keyframes, self.truth, self.poses0)]
        self.true_keyframes = self.room.keyframes
        self._edges = self._loop = None

    @property
    def edges(self):
        if self._edges is None:
            self._edges = GO.link(self.keyframes)
        return self._edges

    @property
    def loop(self):
        """(poses, stats) of the oracle loop, computed once and left unchanged"""
        if self._loop is None:
            self._loop = GO.optimize(self.keyframes, self.edges, self.poses0, GATES, ANCHOR)
        return self._loop

    def errors(self, poses):
        return [VC.pose_error(p, t) for p, t in zip(poses, self.truth)]

    def fill(self, ctx, keyframes=None, poses=None, upto=None):
        kfs = self.keyframes if keyframes is None else keyframes
        ps = self.poses0 if poses is None else poses
        w, h = self.room.shots[0].w, self.room.shots[0].h
        return [ctx.keyframe_add_host(k["xy"], k["desc"], k["xw"], k["nw"], p, w, h) for k, p in list(zip(kfs, ps))[:upto]]


def case(cam):
    if cam not in _CASES:
        _CASES[cam] = Case(cam)
    return _CASES[cam]


def correct_fraction(c, edge):
    """the part of an edge's pairs whose true world points are less than feature_cases.CORRECT_DIST apart"""
    import feature_cases as FC
    j, i, a, b = edge
    d = np.linalg.norm(c.true_keyframes[j]["xw"][a].astype(np.float64) - c.true_keyframes[i]["xw"][b], axis=1)
    return float((d < FC.CORRECT_DIST).mean())


# ---- the oracle's figures (tests/test_graph_oracle.py recomputes every one).  Per camera: the edges of the all-pairs link at the
# default match options with >= 12 pairs (of 28 pairs of keyframes) and their pairs; the worst keyframe's error before (rotation rad,
# camera centre m: volume_cases.pose_error); the counted pairs per round; the error of every keyframe at the end.  At SMALL_CAM seven of
# the 26 edges are almost entirely wrong matches (12 - 17 pairs, at most 14 % correct; the good edges are 50 - 91 % correct): the gate
# alone deals with both.  Every keyframe ends within keyframe_cases.RELOC_BOUND at both cameras; the drifted start is far outside it.
FIGURES = {
    "small": dict(edges=26, pairs=1968, start=(0.0744, 0.0659), round_pairs=[1046, 1711, 1583, 1580, 1280, 1275, 1276],
                  end=[(0, 0), (0.00231, 0.00342), (0.00266, 0.00605), (0.00206, 0.00322), (0.00153, 0.00403), (0.00224, 0.003),
                       (0.00186, 0.00434), (0.0031, 0.00842)]),
    "half": dict(edges=28, pairs=5901, start=(0.0744, 0.0659), round_pairs=[2616, 4130, 4083, 4083, 3837, 3839, 3839],
                 end=[(0, 0), (0.000477, 0.00199), (0.00059, 0.00193), (0.000581, 0.00213), (0.000593, 0.00175), (0.000534, 0.00166),
                      (0.00113, 0.00352), (0.00057, 0.00221)]),
}
