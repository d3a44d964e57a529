"""Scenes and figures of the robust volume terms' tests (CPU oracle and GPU): frames in which part of the depth is NOT the map's -- an
intruder, a block of the frame moved towards the camera by a constant -- tracked against the map with the robust weight off and on.
  WINDOW  sdf_cases' room at 160 x 120 in 8 cm voxels, the held-out frame (noise-free), icp_pyramid_sdf from sdf_cases.poses()[1].
  COLOUR  sdf_photo_cases' textured wall (every frame of the wall path fused with its colour at its true pose), one of its frames with
          the intruder in depth AND colour, icp_pyramid_sdf_rgbd with photo_k off and on.
  MAP     mapsdf_photo_cases' walk along the wall, the frame of its first evaluated position with the same intruder,
          icp_pyramid_map_sdf_rgbd against the window and the archived bricks.
The figures next to each case are the ORACLE's (tests/sdf_robust_oracle.py; tests/test_sdf_robust_oracle.py recomputes them); the GPU
loops' sums round differently, so they get volume_cases' margin x2."""
import functools

import numpy as np

import color_oracle as CO
import mapsdf_photo_cases as MPC
import mapsdf_photo_oracle as MP
import photo_oracle as PH
import pyramid_oracle as PO
import sdf_cases as SC
import sdf_photo_cases as SPC
import sdf_robust_oracle as RO
import volume_cases as VC
from frontend_util import SMALL_CAM

NONE, HUBER, TUKEY = RO.NONE, RO.HUBER, RO.TUKEY
LEVELS = SC.LEVELS
COS_THR = SC.TRACK_COS                                  # the loops: 0.8
OFFSET = (0.006, -0.008, 0.004, 0.03, -0.02, 0.04)      # sdf_cases.poses()[1]'s: 10.8 mrad / 54 mm off
# the intruder's block as fractions of the frame (rows, columns): 70 x 60 of 120 x 160 pixels = 22 % of the frame; the smaller one
# 40 x 40 = 8 %
PATCH = ((0.25, 100 / 120), (0.125, 0.5))
SMALL_PATCH = ((1 / 3, 2 / 3), (0.1875, 0.4375))
FRAMES = {"clean": (0.0, None), "intruder 8 cm": (0.08, PATCH), "smaller intruder 8 cm": (0.08, SMALL_PATCH),
          "intruder 15 cm": (0.15, PATCH)}
SETTINGS = {"none": (NONE, 0.0), "huber 10 mm": (HUBER, 0.01), "huber 5 mm": (HUBER, 0.005), "tukey 50 mm": (TUKEY, 0.05),
            "tukey 30 mm": (TUKEY, 0.03)}


def patch_slices(cam, patch):
    (r0, r1), (c0, c1) = patch
    return slice(int(round(r0 * cam[5])), int(round(r1 * cam[5]))), slice(int(round(c0 * cam[4])), int(round(c1 * cam[4])))


def intrude(depth, cam, delta, patch):
    """the depth with the block `patch` moved towards the camera by delta metres (invalid pixels stay invalid)"""
    d = np.array(depth, np.float32).copy()
    if patch is not None and delta:
        rs, cs = patch_slices(cam, patch)
        block = d[rs, cs]
        d[rs, cs] = np.where(block > 0, block - np.float32(delta), block)
    return d


def limit(err):
    """what a GPU loop is held to: the oracle's end error x2"""
    return 2 * err[0], 2 * err[1]


# ---------------------------------------------------------------------------------------------- WINDOW
WINDOW_CAM = SMALL_CAM


def window_truth():
    return VC.held_out_pose()


def window_start():
    return SC.moved(window_truth(), *OFFSET)


def window_depth(frame):
    delta, patch = FRAMES[frame]
    return intrude(VC.depth_at(window_truth(), WINDOW_CAM), WINDOW_CAM, delta, patch)


def oracle_window(oracle_lib, frame, setting):
    """(rad, m) from the truth where icp_pyramid_sdf ends on `frame` under `setting`, in the oracles"""
    _, _, G, vol = SC.room_volume(WINDOW_CAM)
    pyr = PO.frame_pyramid(window_depth(frame), WINDOW_CAM, 1.0, *VC.RANGE, LEVELS)
    kind, k = SETTINGS[setting]
    p, _ = RO.icp_pyramid_sdf(oracle_lib, vol, G, pyr, window_start(), VC.TRACK_ITERS, VC.TRACK_GATES, COS_THR, kind, k)
    return VC.pose_error(p, window_truth())


# The oracle's end errors (rad, m), start 10.8 mrad / 54 mm off.  THE CONDITIONS ON THE CASE (test_sdf_robust_oracle.py): on the 8 cm / 22 %
# intruder Tukey k = 50 mm ends within 2 x the clean frame's unweighted error, and the unweighted loop ends at least 4 x further off
# than Tukey.
WINDOW_ORACLE = {
    "clean": {"none": (1.32e-3, 5.98e-3), "huber 10 mm": (1.25e-3, 5.32e-3), "huber 5 mm": (1.11e-3, 4.61e-3),
              "tukey 50 mm": (1.29e-3, 5.47e-3), "tukey 30 mm": (1.19e-3, 4.90e-3)},
    "intruder 8 cm": {"none": (1.48e-2, 6.33e-2), "huber 10 mm": (6.48e-3, 2.61e-2), "huber 5 mm": (5.53e-3, 2.16e-2),
                      "tukey 50 mm": (1.59e-3, 6.56e-3), "tukey 30 mm": (1.67e-3, 6.58e-3)},
    "smaller intruder 8 cm": {"none": (5.55e-3, 2.53e-2), "huber 10 mm": (2.21e-3, 9.29e-3), "huber 5 mm": (1.98e-3, 7.90e-3),
                              "tukey 50 mm": (1.48e-3, 6.19e-3), "tukey 30 mm": (1.46e-3, 5.90e-3)},
    "intruder 15 cm": {"none": (3.05e-2, 1.19e-1), "huber 10 mm": (1.52e-3, 6.31e-3), "huber 5 mm": (1.56e-3, 6.16e-3),
                       "tukey 50 mm": (1.55e-3, 6.45e-3), "tukey 30 mm": (1.63e-3, 6.47e-3)},
}

# ---------------------------------------------------------------------------------------------- COLOUR
COLOUR_CAM = VC.HALF_CAM
COLOUR_FRAME = SPC.JAC_FRAME
COLOUR_DELTA = 0.08
COLOUR_LEVELS = 40.0        # the intruder's colour: every channel of the block moved by this many levels (clipped to 0 .. 255)
# (kind, k, photo_k)
COLOUR_SETTINGS = {"none": (NONE, 0.0, 0.0), "tukey 50 mm": (TUKEY, 0.05, 0.0), "tukey 50 mm, 25 levels": (TUKEY, 0.05, 25.0),
                   "huber 10 mm, 5 levels": (HUBER, 0.01, 5.0)}


def colour_truth():
    return SPC.wall_fused(COLOUR_CAM)[3][COLOUR_FRAME]


def colour_start():
    return SC.moved(colour_truth(), *OFFSET)


def colour_frame(intruder):
    """(depth, rgb (h, w, 3) uint8) of the wall frame; with the intruder the block is closer by COLOUR_DELTA and brighter by COLOUR_LEVELS"""
    d, rgb = SPC.wall_fused(COLOUR_CAM)[4][COLOUR_FRAME]
    if not intruder:
        return np.array(d, np.float32), np.ascontiguousarray(rgb)
    rs, cs = patch_slices(COLOUR_CAM, PATCH)
    rgb = np.array(rgb).copy()
    rgb[rs, cs] = np.clip(rgb[rs, cs].astype(np.float32) + COLOUR_LEVELS, 0, 255).astype(np.uint8)
    return intrude(d, COLOUR_CAM, COLOUR_DELTA, PATCH), np.ascontiguousarray(rgb)


def oracle_colour(oracle_lib, intruder, setting):
    G, vol, cvol, _, _ = SPC.wall_fused(COLOUR_CAM)
    d, rgb = colour_frame(intruder)
    h, w = COLOUR_CAM[5], COLOUR_CAM[4]
    pyr = PO.frame_pyramid(d, COLOUR_CAM, 1.0, *VC.RANGE, LEVELS)
    fint = PH.intensity_pyramid(PH.intensity(CO.frame_rgba(rgb).reshape(h, w, 4)), LEVELS)
    kind, k, photo_k = COLOUR_SETTINGS[setting]
    p, _ = RO.icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, pyr, fint, colour_start(), VC.TRACK_ITERS, VC.TRACK_GATES, COS_THR, SPC.WEIGHT,
                                   kind, k, photo_k)
    return VC.pose_error(p, colour_truth())


# The oracle's end errors (rad, m) without and with the intruder (22 % of the frame closer by 8 cm and brighter by 40 levels), start
# 10.8 mrad / 54 mm off.  The wall is a plane: its geometry holds three of the six degrees of freedom, the colour the rest.  With the
# intruder the unweighted loop ends 150 mm off.  A weight on the GEOMETRIC rows alone (photo_k = 0) DOES NOT PAY HERE: the intruder's
# photometric rows keep their full weight, nothing is left to hold against them, and the loop ends further off than the unweighted one.
# With photo_k as well the loop ends within 1.4 x the clean frame's error.  Huber gets a seventh of the way.
COLOUR_ORACLE = {
    False: {"none": (8.80e-5, 4.55e-5), "tukey 50 mm": (8.80e-5, 4.64e-5), "tukey 50 mm, 25 levels": (8.80e-5, 4.62e-5),
            "huber 10 mm, 5 levels": (8.80e-5, 4.56e-5)},
    True: {"none": (1.25e-2, 1.50e-1), "tukey 50 mm": (6.25e-1, 2.24), "tukey 50 mm, 25 levels": (1.24e-4, 6.12e-5),
           "huber 10 mm, 5 levels": (2.18e-3, 2.10e-2)},
}

# ---------------------------------------------------------------------------------------------- MAP
MAP_CAM = MPC.WALK_CAM
MAP_POSITION = 0


def map_truth():
    return MPC.walk_eval_pose(MAP_POSITION)


def map_frame(intruder):
    d, rgb = MPC.walk_frame(map_truth(), 50 + MAP_POSITION)
    if not intruder:
        return np.array(d, np.float32), np.ascontiguousarray(rgb)
    rs, cs = patch_slices(MAP_CAM, PATCH)
    rgb = np.array(rgb).copy()
    rgb[rs, cs] = np.clip(rgb[rs, cs].astype(np.float32) + COLOUR_LEVELS, 0, 255).astype(np.uint8)
    return intrude(d, MAP_CAM, COLOUR_DELTA, PATCH), np.ascontiguousarray(rgb)


@functools.lru_cache(maxsize=None)
def map_virtual():
    vol, cvol, total, store = MPC.oracle_walk_map()
    return MP.virtual(vol, cvol, total, store, MPC.WALK_KW)


def oracle_map(oracle_lib, intruder, setting):
    mvol, mcvol, mG, _ = map_virtual()
    d, rgb = map_frame(intruder)
    _, pyr, fint = MPC.frame_levels(MAP_CAM, d, CO.frame_rgba(rgb), VC.RANGE)
    kind, k, photo_k = COLOUR_SETTINGS[setting]
    p, _ = RO.icp_pyramid_sdf_rgbd(oracle_lib, mvol, mcvol, mG, pyr, fint, MPC.walk_start(MAP_POSITION), MPC.WALK_ITERS, MPC.WALK_GATES,
                                   MPC.COS_THR, MPC.WEIGHT, kind, k, photo_k)
    return VC.pose_error(p, map_truth())


# The same on the map (the walk's first evaluated position: most of the wall in view lies in archived bricks), start 7.8 mrad / 32 mm
# off: the unweighted loop ends 112 mm off, the weight on the geometric rows alone DOES NOT PAY (173 mm), both weights end at 1.0 mm --
# 110 x closer than the unweighted loop, 5.8 x the clean frame's 0.18 mm.
MAP_ORACLE = {
    False: {"none": (2.05e-4, 1.77e-4), "tukey 50 mm": (2.05e-4, 1.77e-4), "tukey 50 mm, 25 levels": (2.05e-4, 1.77e-4),
            "huber 10 mm, 5 levels": (2.05e-4, 1.77e-4)},
    True: {"none": (1.32e-2, 1.12e-1), "tukey 50 mm": (5.52e-2, 1.73e-1), "tukey 50 mm, 25 levels": (6.09e-4, 1.02e-3),
           "huber 10 mm, 5 levels": (2.17e-3, 1.96e-2)},
}
