"""Scenes and figures of the volume colour term's tests (CPU oracle and GPU): sdf_cases' room volume fused WITH colour, its spoiled and
cropped forms, the frames (holes in the depth, A = 0 in 1 % of the colour pixels), and the two tracking loops of photo_cases -- the
textured wall, where the volume term alone is lost, and volume_cases' room path with colour -- on the direct route: no raycast, no
model, the frame tracked against the TSDF and the colour volume themselves.  The figures next to each case are the ORACLE's
(tests/test_sdf_photo_oracle.py recomputes them); the GPU loops' sums round differently, so they get volume_cases' margin x2."""
import functools

import numpy as np

import color_oracle as CO
import photo_cases as PC
import photo_oracle as PH
import pyramid_oracle as PO
import sdf_cases as SC
import sdf_photo_oracle as SP
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM

WEIGHT = PC.WEIGHT          # 0.01 m per intensity level
LEVELS = SC.LEVELS
COS_THR = SC.TRACK_COS      # the loops: 0.8
ROOM = None               # simulator.default_room()


def rgb_at(p, cam, room=None):
    return PC.rgb_at(p, cam, ROOM if room is None else room)


@functools.lru_cache(maxsize=None)
def room_volume(cam=SMALL_CAM, voxel=SC.VOXEL):
    """(dims, desc, G, vol, cvol): sdf_cases.room_volume's frames fused with their colour; vol is bit for bit sdf_cases' volume"""
    dims, desc, G = SC.geometry(voxel)
    vol, cvol = G.empty(), CO.empty(G)
    for k in VC.ACC_VIEWS:
        p = VC.view(k)
        V = FO.frame_maps(VC.depth_at(p, cam), cam, 1.0, *VC.RANGE)[0]
        vol, cvol = CO.integrate(vol, cvol, G, V, CO.frame_rgba(rgb_at(p, cam)), cam, p)
    vol.setflags(write=False)
    cvol.setflags(write=False)
    return dims, desc, G, vol, cvol


def spoiled_color(cvol, step=211):
    """every step-th coloured voxel loses its weight (from half a step in: sdf_cases.spoiled takes every step-th of nearly the same
    voxels for its NaN tsdf, and a cell lost to that shows nothing here); of the others every (step + 2)-th gets a NaN red, every
    (step + 6)-th an Inf green and every (step + 12)-th a -Inf blue bit pattern under its weight"""
    out = cvol.copy()
    flat = out.reshape(-1, 4)
    idx = np.nonzero(CO.f32(flat[:, 3]) > 0)[0]
    flat[idx[step // 2::step], 3] = 0
    flat[idx[5::step + 2], 0] = 0x7E01
    flat[idx[9::step + 6], 1] = 0x7C00
    flat[idx[13::step + 12], 2] = 0xFC00
    return out


def cropped_color(cvol, crop=SC.CROP):
    return np.ascontiguousarray(cvol[:, :, crop[0]:crop[1]])


def frame(cam, pose=None, holes=SC.HOLES, seed=11):
    """(depth, rgba (h*w, 4) uint8) of the room from `pose` (the held-out pose): sdf_cases.frame_depth's holes, and A = 0 in 1 % of the
    colour pixels"""
    pose = VC.held_out_pose() if pose is None else pose
    rgba = CO.frame_rgba(rgb_at(pose, cam)).copy()
    if holes:
        rng = np.random.default_rng(seed + 1)
        rgba[rng.integers(0, len(rgba), int(holes * len(rgba))), 3] = 0
    return SC.frame_depth(cam, pose, holes, seed), rgba


def frame_levels(cam, depth, rgba):
    """[(V, N, If)] per level of the frame"""
    pyr = PO.frame_pyramid(depth, cam, 1.0, *VC.RANGE, LEVELS)
    fint = PH.intensity_pyramid(PH.intensity(rgba.reshape(cam[5], cam[4], 4)), LEVELS)
    return [(pyr[l][1], pyr[l][2], fint[l].reshape(-1)) for l in range(LEVELS)]


# ---- coverage, so that no test passes on an empty answer: the share of a level's pixels with a photometric row at the held-out pose on
# the uncropped room with TRACK_GATES[l].  The oracle gives 0.86 / 0.83 / 0.72 at 160 x 120 and at 161 x 119
# (test_sdf_photo_oracle.py::test_coverage_figures recomputes them)
COVER_ORACLE = (0.86, 0.83, 0.72)
COVER = 0.6

# ---- the row against central differences of the oracle's own residual (test_sdf_photo_oracle.py::test_the_row_against_central_
# differences): the WALL volume with every frame of the wall path fused with its colour at its true pose (wall_fused), frame JAC_FRAME
# at its true pose, steps of one voxel at the wall (JAC_STEP_T metres, JAC_STEP_T / 3 radians).  Per column the largest |J - dr| over
# the largest |dr| among the pixels with a row at all three poses.  A central difference over +-1 voxel of a trilinear interpolant is
# not the cell's own gradient, so the ratio is no rounding figure; a sign or order error shows as ~1 or as a negative correlation.
# The oracle gives, per column, ratios 0.18 0.16 0.21 0.19 0.12 0.14 and correlations 0.9985 0.9978 0.9935 0.9980 0.9985 0.9984;
# JAC_SEEN is the worst column's ratio, the bound 3 x that.
JAC_STEP_T, JAC_STEP_R = PC.WALL_VOXEL, PC.WALL_VOXEL / 3
JAC_FRAME = 2
JAC_SEEN = 0.21
JAC_BOUND = 3 * JAC_SEEN


def loop_scene(which):
    """(poses, frames, (dims, desc)) of a loop: "wall" = photo_cases' wall path in its 4-cm slab, "room" = volume_cases' path with colour"""
    if which == "wall":
        poses = [PC.wall_pose(k) for k in range(PC.WALL_FRAMES)]
        return poses, PC.loop_frames(poses, PC.WALL), PC.wall_geometry()
    poses = [PC.room_pose(f) for f in range(VC.TRACK_FRAMES)]
    return poses, PC.loop_frames(poses, ROOM), VC.room_geometry(VC.TRACK_VOXEL)


@functools.lru_cache(maxsize=None)
def wall_fused(cam=VC.HALF_CAM):
    """(G, vol, cvol, poses, frames): every frame of the wall path fused with its colour at its TRUE pose"""
    poses, frames, (dims, desc) = loop_scene("wall")
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    vol, cvol = G.empty(), CO.empty(G)
    for p, (d, rgb) in zip(poses, frames):
        vol, cvol = CO.integrate(vol, cvol, G, FO.frame_maps(d, cam, 1.0, *VC.RANGE)[0], CO.frame_rgba(rgb), cam, p)
    return G, vol, cvol, poses, frames


def oracle_loop(oracle_lib, poses, frames, geometry, weight, cam=VC.HALF_CAM):
    """set_depth_pyramid; set_color; the frame tracked against the volume from the previous estimate (weight = None: the volume term
    alone); integrate_color at its own -- all in the oracles.  Frame 0 is fused at its true pose.  Returns the worst (rotation, camera
    centre) error over the frames and the last round's (geometric, photometric) rows per frame."""
    dims, desc = geometry
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    h, w = cam[5], cam[4]
    est = [poses[0]]
    V0 = FO.frame_maps(frames[0][0], cam, 1.0, *VC.RANGE)[0]
    vol, cvol = CO.integrate(G.empty(), CO.empty(G), G, V0, CO.frame_rgba(frames[0][1]), cam, est[0])
    worst, rows = [0.0, 0.0], []
    for f in range(1, len(poses)):
        pyr = PO.frame_pyramid(frames[f][0], cam, 1.0, *VC.RANGE, LEVELS)
        rgba = CO.frame_rgba(frames[f][1])
        fint = PH.intensity_pyramid(PH.intensity(rgba.reshape(h, w, 4)), LEVELS)
        p, hist = SP.icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, pyr, fint, est[-1], VC.TRACK_ITERS, VC.TRACK_GATES, COS_THR, weight)
        est.append(p)
        rows.append(hist[-1][:2])
        vol, cvol = CO.integrate(vol, cvol, G, pyr[0][1], rgba, cam, p)
        e = VC.pose_error(p, poses[f])
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    return tuple(worst), rows


# The oracle loops (worst frame, rotation rad / camera centre m).  WALL: the volume term alone loses the path, as ICP alone does; with
# the colour term it holds it.  ROOM: with the term against the volume term alone (sdf_cases.TRACK_ORACLE) -- the same order.
WALL_LOOP_SDF = (1.61e-2, 1.59e-1)
WALL_LOOP_RGBD = (2.53e-4, 1.65e-4)
ROOM_LOOP_RGBD = (7.01e-4, 4.99e-3)
ROOM_LOOP_SDF = (8.45e-4, 4.71e-3)     # = sdf_cases.TRACK_ORACLE, on this loop's frames
# rows of the last round per tracked frame, of 76 800 pixels: (geometric, photometric) between
WALL_ROWS = ((72000, 75000), (72500, 75500))
ROOM_ROWS = ((62000, 67000), (62500, 68000))


def wall_limit():
    return 2 * WALL_LOOP_RGBD[0], 2 * WALL_LOOP_RGBD[1]


def room_limit():
    return 2 * ROOM_LOOP_RGBD[0], 2 * ROOM_LOOP_RGBD[1]
