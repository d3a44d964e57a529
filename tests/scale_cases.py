"""Scenes shared by the scale-level tests (CPU oracle and GPU): the room of tests/feature_cases.py seen by a camera that has moved
CLOSER to (or away from) what the keyframe saw, with and without a roll, and the synthetic views of the GPU edge cases (odd and small
cameras, a keypoint 16 level pixels from every edge of every level, a depth hole at a level keypoint's level-0 centre, more survivors
than the cap with the tie score on several levels).  The figures next to each case are the ORACLE's (tests/test_scale_oracle.py
recomputes them)."""
import numpy as np

import feature_cases as FC
import feature_edge_cases as FEC
import feature_oracle as FE
import oriented_cases as OC
import oriented_oracle as OO
import scale_oracle as SO
from frontend_util import SMALL_CAM


def along(tz, base=FC.NARROW):
    """`base` with the translation along the optical axis replaced: negative = the frame's camera has moved towards the scene"""
    return base[:5] + (tz,)


MOTIONS = {"narrow": FC.NARROW, "tz-1.0": along(-1.0), "tz-1.6": along(-1.6), "tz-2.1": along(-2.1), "tz+0.6": along(0.6),
           "wide1_tz-1.6": along(-1.6, FC.WIDE1), "roll0.6_tz-1.6": along(-1.6, OC.roll(0.6)),
           "wide1_rz0.8_tz-1.6": along(-1.6, OC.MOTIONS["wide1_rz0.8"])}
CAMS = {"small": FC.CAMS["small"], "half": FC.CAMS["half"]}
MOPT = OC.MOPT
_PAIRS = {}


def pair(cam_name, motion_name):
    """the pair, made once (nothing changes it)"""
    key = (cam_name, motion_name)
    if key not in _PAIRS:
        _PAIRS[key] = FC.Pair(CAMS[cam_name], MOTIONS[motion_name])
    return _PAIRS[key]


def detect(view, levels, kind=SO.UPRIGHT, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS)):
    return SO.detect(view.rgba, view.V, view.N, fopt[0], fopt[1], levels, kind)


def oracle(p, levels, kind=SO.UPRIGHT, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS), mopt=MOPT, model=None):
    """oriented_cases.oracle over `levels` scale levels: its dict, and level / level pixel of frame and model keypoints (fl, flxy, ml,
    mlxy).  model: another pair's model view in this one's place (mixed cameras)"""
    mv = p.model if model is None else model
    fxy, fs, fd, fl, flxy, fb = detect(p.frame, levels, kind, fopt)
    mxy, ms, md, ml, mlxy, mb = detect(mv, levels, kind, fopt)
    fi, mi, d1, d2 = FE.match(fd, md, *mopt)
    XW, XC, BV, NW, NC, wq = FE.slots(fxy, mxy, fi, mi, d1, p.frame.V, p.frame.N, p.frame.B, mv.V, mv.N, p.frame.w, mv.w)
    return dict(fxy=fxy, fs=fs, fd=fd, fb=fb, fl=fl, flxy=flxy, mxy=mxy, ms=ms, md=md, mb=mb, ml=ml, mlxy=mlxy, fi=fi, mi=mi, d1=d1, d2=d2,
                XW=XW, XC=XC, BV=BV, NW=NW, NC=NC, w=wq)


def keyframe(shot, levels, kind=SO.UPRIGHT):
    """keyframe_oracle.keyframe of a keyframe_cases.Shot detected over `levels` levels"""
    xy, _, desc = SO.detect(shot.rgba, shot.MV, shot.MN, levels=levels, kind=kind)[:3]
    pix = xy[:, 1].astype(np.int64) * shot.w + xy[:, 0]
    return dict(xy=xy, desc=desc, xw=shot.MV[pix].astype(np.float32), nw=shot.MN[pix].astype(np.float32))


# ---- synthetic views
# feature_cases.noise_rgb at HALF_CAM under this seed: 9 800 survivors over four levels, and the score of the 4096th has survivors on
# levels 0 AND 1 on both sides -- the frame keeps 3 of its 10 (level 0's: the level-1 tie is cut), the model 9 of its 11
NOISE_SEED = 7


def overcap_pair(cam=FC.HALF_CAM, seed=NOISE_SEED):
    img = FC.noise_rgb(cam, seed)
    return FC.Pair(cam, FC.NARROW, rgb_a=img, rgb_b=img)


def level_dots(w, h, levels=SO.MAX_LEVELS):
    """per level the four level pixels 16 from two edges of the level, [(l, u, v)], levels with an interior only"""
    out = []
    for l in range(levels):
        wl, hl = SO.level_size(w, h, l)
        if wl > 2 * FE.BORDER and hl > 2 * FE.BORDER:
            out += [(l, u, v) for u in (FE.BORDER, wl - FE.BORDER - 1) for v in (FE.BORDER, hl - FE.BORDER - 1)]
    return out


def paint_block(img, l, u, v, value):
    """the source footprint of level pixel (u, v) of level l, painted: at that level the pixel reads `value` exactly"""
    p, q = SO.P[l], SO.Q[l]
    x0, x1 = q * u // p, (q * u + q - 1) // p
    y0, y1 = q * v // p, (q * v + q - 1) // p
    img[y0:y1 + 1, x0:x1 + 1] = value


def corner_scene(cam=SMALL_CAM, oriented=False):
    """isolated bright dots on a flat background over the plane z = 1 (feature_edge_cases.Scene: every vertex and normal is finite),
    one per (level, corner of the level's interior): the source footprint of the level pixel 16 level pixels from two edges of its
    level, so that it is a keypoint OF THAT LEVEL standing on the border.  oriented: a 3 x 3 level-pixel blob beside each dot
    (oriented_cases.blob_for_bin) that turns its patch into a bin whose steered offsets reach 17 towards the near side edge.
    Returns (scene, [(l, u, v)])"""
    h, w = cam[5], cam[4]
    img = np.full((h, w, 3), OC.BACKGROUND, np.uint8)
    dots, reach = level_dots(w, h), OC.reach_bins()
    for l, u, v in dots:
        paint_block(img, l, u, v, OC.BRIGHT)
        if oriented:
            cx, cy = OC.blob_for_bin(reach["left" if u == FE.BORDER else "right"][0])
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    paint_block(img, l, u + cx + dx, v + cy + dy, OC.BRIGHT)
    return FEC.Scene(img, cam), dots


def outside_samples(level, lxy, bins, w, h):
    """per level the number of steered sample positions of its keypoints that lie outside the level's image"""
    out = [0] * SO.MAX_LEVELS
    for l, (u, v), b in zip(level, lxy, bins):
        wl, hl = SO.level_size(w, h, l)
        P = OO.steer(np.array([b]))[0]
        X, Y = u + P[:, (0, 2)], v + P[:, (1, 3)]
        out[l] += int(((X < 0) | (X >= wl) | (Y < 0) | (Y >= hl)).sum())
    return out


def centre_hole_pair(cam=SMALL_CAM):
    """the tz-1.6 scene, and per level >= 1 one strong frame keypoint whose level-0 centre pixel gets a depth hole ONE pixel wide: the
    level pixel's colour is untouched, the vertex at (c(u), c(v)) is not finite.  Returns (pair with the holes, pair without,
    [(l, u, v)] of the chosen keypoints)"""
    clean = FC.Pair(cam, MOTIONS["tz-1.6"])
    xy, sc, _, lev, lxy, _ = detect(clean.frame, SO.MAX_LEVELS)
    chosen, db = [], clean.db.copy()
    for l in range(1, SO.MAX_LEVELS):
        m = np.flatnonzero(lev == l)
        k = m[np.argmax(sc[m])]
        chosen.append((l, int(lxy[k, 0]), int(lxy[k, 1])))
        db[xy[k, 1], xy[k, 0]] = 0.0
    holed = FC.Pair(cam, MOTIONS["tz-1.6"])
    holed.db = db
    V, N, B = FC.FO.frame_maps(db, cam, 1.0, *FC.VC.RANGE)
    holed.frame = FC.View(holed.frame.rgba, V, N, B, cam)
    return holed, clean, chosen


# ---- the oracle's figures, in the convention of oriented_cases.FIGURES (defaults: threshold 12, cap 4096, max_dist 64, ratio 8 / 10,
# no cross-check).  Per (camera, motion, descriptor kind): `one` = (matches, correct matches) at 1 level, `four` = the same at 4 levels,
# `reloc_one` / `reloc_four` = feature_cases.oracle_relocalise on those matches, as volume_cases.pose_error (rotation rad, camera
# centre m; None: no pose), `votes_four` / `iters_four` its consensus and adapted Iter at 4 levels.  "tz-1.6" at 2 and 3 levels: LADDER.
UP, OR = SO.UPRIGHT, SO.ORIENTED
FIGURES = {
    ("half", "narrow", UP): dict(one=(919, 894), four=(2105, 1977), reloc_one=(1.26e-03, 4.69e-03), reloc_four=(1.53e-03, 2.87e-03),
        votes_four=3837, iters_four=3),
    ("half", "tz-1.0", UP): dict(one=(163, 123), four=(680, 597), reloc_one=(1.41e-03, 2.12e-03), reloc_four=(1.50e-03, 3.74e-03),
        votes_four=1136, iters_four=5),
    ("half", "tz-1.6", UP): dict(one=(89, 21), four=(449, 364), reloc_one=(5.09e-02, 4.12e-02), reloc_four=(2.04e-03, 1.65e-03),
        votes_four=701, iters_four=7),
    ("half", "tz-2.1", UP): dict(one=(81, 2), four=(339, 223), reloc_one=(9.06e-01, 2.62e+00), reloc_four=(1.94e-03, 8.97e-03),
        votes_four=385, iters_four=23),
    ("half", "wide1_tz-1.6", UP): dict(one=(98, 20), four=(491, 399), reloc_one=(5.81e-03, 1.18e-02), reloc_four=(1.54e-03, 2.47e-03),
        votes_four=727, iters_four=9),
    ("small", "tz-1.6", UP): dict(one=(18, 2), four=(121, 83), reloc_one=None, reloc_four=(9.51e-03, 1.11e-02),
        votes_four=182, iters_four=8),
    ("half", "tz+0.6", UP): dict(one=(641, 592), four=(1249, 1119), reloc_one=(1.34e-03, 5.75e-03), reloc_four=(1.60e-03, 5.12e-03),
        votes_four=2227, iters_four=4),
    ("half", "roll0.6_tz-1.6", OR): dict(one=(57, 0), four=(222, 142), reloc_one=None, reloc_four=(1.00e-03, 2.60e-03),
        votes_four=262, iters_four=20),
    ("half", "wide1_rz0.8_tz-1.6", OR): dict(one=(47, 3), four=(211, 134), reloc_one=None, reloc_four=(2.87e-03, 8.87e-03),
        votes_four=251, iters_four=19),
}
LADDER = {2: (260, 182), 3: (388, 303), 4: (449, 364)}      # ("half", "tz-1.6", UP): (matches, correct) per number of levels
WITHIN = [k for k in FIGURES if k[0] == "half" and k[1] not in ("tz+0.6",)]     # at 4 levels inside RELOC_BOUND
LOST_AT_ONE = [("half", "tz-1.6", UP), ("half", "tz-2.1", UP)]                   # at 1 level outside it
RELOC_BOUND = OC.RELOC_BOUND      # keyframe_cases.RELOC_BOUND
