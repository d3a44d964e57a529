"""Scenes shared by the oriented-descriptor tests (CPU oracle and GPU): the room of tests/feature_cases.py seen by a camera that has
ROLLED between the keyframe and the frame, the three existing motions in oriented mode, and the synthetic views of the GPU edge cases
(keypoints 16 px from every image edge in bins whose steered offsets leave the image, isolated dots whose moments vanish).  The figures
next to each case are the ORACLE's (tests/test_oriented_oracle.py recomputes them)."""
import numpy as np

import feature_cases as FC
import feature_oracle as FE
import oriented_oracle as OO
from frontend_util import SMALL_CAM


def roll(r):
    """feature_cases.NARROW with the rotation about the optical axis replaced"""
    return (0.02, -0.015, r, 0.03, -0.02, 0.025)


MOTIONS = {"roll0.3": roll(0.3), "roll0.6": roll(0.6), "roll1.2": roll(1.2), "roll3.0": roll(3.0),
           "wide1_rz0.8": FC.WIDE1[:2] + (0.8,) + FC.WIDE1[3:], "wide2_rz-0.7": FC.WIDE2[:2] + (-0.7,) + FC.WIDE2[3:],
           "narrow": FC.NARROW, "wide1": FC.WIDE1, "wide2": FC.WIDE2}
ROLLED = ["roll0.3", "roll0.6", "roll1.2", "roll3.0", "wide1_rz0.8", "wide2_rz-0.7"]
CAMS = {"small": FC.CAMS["small"], "half": FC.CAMS["half"]}
MOPT = (FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, False)
_PAIRS = {}


def pair(cam_name, motion_name):
    """the pair, made once (nothing changes it)"""
    key = (cam_name, motion_name)
    if key not in _PAIRS:
        _PAIRS[key] = FC.Pair(CAMS[cam_name], MOTIONS[motion_name])
    return _PAIRS[key]


def oracle(p, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS), mopt=MOPT):
    """feature_cases.Pair.oracle with the oriented descriptor: its dict, and the angle bins fb / mb of frame / model"""
    fxy, fs, fd, fb = OO.detect(p.frame.rgba, p.frame.V, p.frame.N, *fopt)
    mxy, ms, md, mb = OO.detect(p.model.rgba, p.model.V, p.model.N, *fopt)
    fi, mi, d1, d2 = FE.match(fd, md, *mopt)
    XW, XC, BV, NW, NC, wq = FE.slots(fxy, mxy, fi, mi, d1, p.frame.V, p.frame.N, p.frame.B, p.model.V, p.model.N, p.cam[4], p.cam[4])
    return dict(fxy=fxy, fs=fs, fd=fd, fb=fb, mxy=mxy, ms=ms, md=md, mb=mb, fi=fi, mi=mi, d1=d1, d2=d2, XW=XW, XC=XC, BV=BV, NW=NW, NC=NC,
                w=wq)


# ---- synthetic views (SMALL_CAM, the same image on both sides of a NARROW pair: only the depths differ)
BACKGROUND, BRIGHT = 60, 255


def reach_bins():
    """per image edge the bins in which some steered offset is 17 px towards that edge: {"left": [bins], "right", "top", "bottom"}"""
    P = OO.steer(np.arange(OO.BINS))
    x, y = P[..., (0, 2)].reshape(OO.BINS, -1), P[..., (1, 3)].reshape(OO.BINS, -1)
    return {"left": np.flatnonzero(x.min(1) <= -17).tolist(), "right": np.flatnonzero(x.max(1) >= 17).tolist(),
            "top": np.flatnonzero(y.min(1) <= -17).tolist(), "bottom": np.flatnonzero(y.max(1) >= 17).tolist()}


def blob_for_bin(b):
    """the centre (cx, cy) of a 3 x 3 blob inside the disc whose moments fall in bin b (m10 = 9 Y cx, m01 = 9 Y cy): the one closest
    to the bin's own direction"""
    best = None
    for cy in range(-8, 9):
        for cx in range(-8, 9):
            if 36 <= cx * cx + cy * cy <= 100 and OO.angle_bin(cx, cy) == b:
                off = abs(np.angle(complex(cx, cy) * np.exp(-2j * np.pi * b / OO.BINS)))
                if best is None or off < best[0]:
                    best = (off, cx, cy)
    return best[1], best[2]


def edge_rgb(cam=SMALL_CAM):
    """isolated bright dots on a flat background, each a corner: along every edge at exactly 16 px from it, with a blob beside the dot
    that turns its patch into a bin whose steered offsets leave the image on that side; and dots alone in the interior, whose moments
    are zero (a 32-way tie: bin 0).  Returns (rgb, {edge: [(u, v, bin)]}, [(u, v)] of the lone dots)"""
    h, w = cam[5], cam[4]
    img = np.full((h, w, 3), BACKGROUND, np.uint8)
    placed, R = {}, reach_bins()
    for edge, bins in R.items():
        placed[edge] = []
        for i, b in enumerate(bins[:3]):
            along = 32 + 30 * i
            u, v = {"left": (16, along), "right": (w - 17, along), "top": (along + 15, 16), "bottom": (along + 15, h - 17)}[edge]
            cx, cy = blob_for_bin(b)
            img[v, u] = BRIGHT
            img[v + cy - 1: v + cy + 2, u + cx - 1: u + cx + 2] = BRIGHT
            placed[edge].append((u, v, b))
    lone = [(w // 2 + 20 * i, h // 2 + 12 * j) for i in (-2, -1, 0, 1, 2) for j in (-1, 1)]      # some fall where a side has no normal
    for u, v in lone:
        img[v, u] = BRIGHT
    return img, placed, lone


def edge_pair():
    img, placed, lone = edge_rgb()
    return FC.Pair(SMALL_CAM, FC.NARROW, rgb_a=img, rgb_b=img), placed, lone


def holes_pair():
    """a rolled pair whose model colour has A = 0 holes: every disc holds some (they read as luma 0 in the moments)"""
    return FC.Pair(FC.HALF_CAM, MOTIONS["roll0.6"], holes=True)


# ---- keyframes: keyframe_cases' room with an oriented store, and queries that have rolled
QUERY_MOTION = FC.WIDE1[:2] + (0.8,) + FC.WIDE1[3:]       # keyframe_cases.QUERY_MOTION with rz replaced by 0.8


def keyframe(shot):
    """keyframe_oracle.keyframe of a keyframe_cases.Shot, with oriented descriptors"""
    xy, _, desc, _ = OO.detect(shot.rgba, shot.MV, shot.MN)
    pix = xy[:, 1].astype(np.int64) * shot.w + xy[:, 0]
    return dict(xy=xy, desc=desc, xw=shot.MV[pix].astype(np.float32), nw=shot.MN[pix].astype(np.float32))


def rolled_queries(room):
    """per keyframe of the room the frame at its pose moved by QUERY_MOTION (keyframe_cases' seeds)"""
    import keyframe_cases as KC
    import photo_cases as PC
    return [KC.Shot(PC.moved(p, *QUERY_MOTION), room.cam, KC.QUERY_SEED + i) for i, p in enumerate(room.kf_poses)]


# ---- the oracle's figures, in the convention of feature_cases.FIGURES (defaults: threshold 12, cap 4096, max_dist 64, ratio 8 / 10,
# no cross-check).  Per pair: keypoints of frame / model (the detector's: the same in both modes), `upright` = (matches, share
# correct) of feature_oracle's descriptor, `oriented` = the same of oriented_oracle's.  At "half", end to end (errors are
# volume_cases.pose_error's: rotation rad, camera centre m): `start` = the stale pose A against the truth, `reloc` =
# feature_cases.oracle_relocalise on the oriented matches, `reloc_upright` = the same on the upright matches (None: no pose).
FIGURES = {
    ("half", "roll0.3"): dict(keypoints=(1331, 1210), upright=(182, 0.791), oriented=(605, 0.944), start=(3.01e-01, 4.39e-02),
        reloc=(7.05e-04, 2.22e-03), votes=1145, iters=2, reloc_upright=(3.93e-03, 1.10e-02)),
    ("half", "roll0.6"): dict(keypoints=(1211, 1210), upright=(42, 0.024), oriented=(508, 0.933), start=(6.01e-01, 4.39e-02),
        reloc=(2.19e-04, 8.39e-04), votes=953, iters=3, reloc_upright=(6.36e-01, 8.31e-01)),
    ("half", "roll1.2"): dict(keypoints=(1249, 1210), upright=(52, 0.0), oriented=(485, 0.944), start=(1.20e+00, 4.39e-02),
        reloc=(4.00e-04, 1.84e-03), votes=923, iters=2, reloc_upright=(2.71e+00, 5.25e+00)),
    ("half", "roll3.0"): dict(keypoints=(1330, 1210), upright=(69, 0.0), oriented=(644, 0.949), start=(3.00e+00, 4.39e-02),
        reloc=(9.01e-04, 3.70e-03), votes=1224, iters=2, reloc_upright=(3.12e+00, 1.88e+00)),
    ("half", "wide1_rz0.8"): dict(keypoints=(1253, 1210), upright=(50, 0.0), oriented=(230, 0.861), start=(8.16e-01, 2.74e-01),
        reloc=(7.50e-04, 2.83e-03), votes=401, iters=4, reloc_upright=None),
    ("half", "wide2_rz-0.7"): dict(keypoints=(1379, 1210), upright=(46, 0.0), oriented=(209, 0.804), start=(7.54e-01, 5.48e-01),
        reloc=(9.14e-04, 3.87e-03), votes=337, iters=6, reloc_upright=(7.77e-01, 2.38e+00)),
    ("half", "narrow"): dict(keypoints=(1180, 1210), upright=(919, 0.973), oriented=(638, 0.964), start=(2.70e-02, 4.39e-02),
        reloc=(1.59e-03, 3.42e-03), votes=1104, iters=4, reloc_upright=(1.26e-03, 4.69e-03)),
    ("half", "wide1"): dict(keypoints=(1311, 1210), upright=(588, 0.901), oriented=(337, 0.852), start=(1.55e-01, 2.74e-01),
        reloc=(8.19e-04, 2.98e-03), votes=579, iters=5, reloc_upright=(7.25e-04, 2.04e-03)),
    ("half", "wide2"): dict(keypoints=(1385, 1210), upright=(333, 0.868), oriented=(190, 0.768), start=(3.09e-01, 5.48e-01),
        reloc=(7.42e-04, 3.79e-03), votes=291, iters=8, reloc_upright=(7.32e-04, 2.16e-03)),
    ("small", "roll0.3"): dict(keypoints=(515, 483), upright=(63, 0.905), oriented=(223, 0.906), start=(3.01e-01, 4.39e-02),
        reloc=(1.96e-03, 4.15e-03), votes=421, iters=3, reloc_upright=(3.27e-03, 9.46e-03)),
    ("small", "roll0.6"): dict(keypoints=(510, 483), upright=(9, 0.0), oriented=(190, 0.895), start=(6.01e-01, 4.39e-02),
        reloc=(3.96e-03, 9.82e-03), votes=343, iters=3, reloc_upright=None),
    ("small", "roll1.2"): dict(keypoints=(539, 483), upright=(13, 0.0), oriented=(189, 0.91), start=(1.20e+00, 4.39e-02),
        reloc=(1.05e-02, 1.83e-02), votes=302, iters=6, reloc_upright=None),
    ("small", "roll3.0"): dict(keypoints=(503, 483), upright=(13, 0.0), oriented=(231, 0.905), start=(3.00e+00, 4.39e-02),
        reloc=(8.39e-04, 3.03e-03), votes=438, iters=2, reloc_upright=None),
    ("small", "wide1_rz0.8"): dict(keypoints=(526, 483), upright=(9, 0.0), oriented=(78, 0.795), start=(8.16e-01, 2.74e-01),
        reloc=(4.91e-03, 2.10e-02), votes=134, iters=5, reloc_upright=None),
    ("small", "wide2_rz-0.7"): dict(keypoints=(574, 483), upright=(18, 0.0), oriented=(48, 0.75), start=(7.54e-01, 5.48e-01),
        reloc=(1.16e-02, 3.68e-02), votes=69, iters=10, reloc_upright=None),
    ("small", "narrow"): dict(keypoints=(515, 483), upright=(374, 0.869), oriented=(232, 0.905), start=(2.70e-02, 4.39e-02),
        reloc=(6.10e-03, 1.52e-02), votes=363, iters=7, reloc_upright=(2.01e-03, 1.61e-03)),
    ("small", "wide1"): dict(keypoints=(539, 483), upright=(188, 0.936), oriented=(91, 0.824), start=(1.55e-01, 2.74e-01),
        reloc=(7.62e-03, 1.73e-02), votes=135, iters=9, reloc_upright=(2.79e-03, 7.05e-03)),
    ("small", "wide2"): dict(keypoints=(552, 483), upright=(114, 0.912), oriented=(52, 0.75), start=(3.09e-01, 5.48e-01),
        reloc=(4.54e-03, 1.21e-02), votes=84, iters=6, reloc_upright=(1.94e-03, 3.87e-03)),
}
RELOC_BOUND = (5e-3, 15e-3)      # keyframe_cases.RELOC_BOUND: the margin the keyframe tests hold a relocalised pose to
