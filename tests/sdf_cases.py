"""Scenes and figures of the volume-term tests (CPU oracle and GPU), on volume_cases' room: the 8 cm volume fused from ACC_VIEWS, its
cropped and spoiled variants that exercise every gate of the rule, the frames and poses the rows are compared at, the convergence
case and the 10-frame tracking loop with the volume term in place of raycast + model pyramid + ICP.  Thresholds are the oracle's own
figures (tests/test_sdf_oracle.py recomputes them on the CPU) times the margin stated next to each."""
import functools

import numpy as np

import pyramid_oracle as PO
import sdf_oracle as SO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12, rot

RAGGED_CAM = (146.25, 146.25, 80.5, 59.5, 161, 119)   # n = 19 159 is no multiple of 4; levels 1 (80 x 59) and 2 (40 x 29) drop a row and a column
FULL_CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)     # one group per thread over 150 workgroups
VOXEL = 0.08                                          # the room in 72 x 44 x 84 voxels, trunc 3 voxels
LEVELS = 3
COS_THR = 0.9                                         # the rows and records (the interface's default); the loops use volume_cases' 0.8
TRACK_COS = 0.8
CROP = (20, 56)                                       # the cropped volume keeps voxels CROP[0] <= i < CROP[1] along x
HOLES = 0.01


def moved(p, rx, ry, rz, x, y, z):
    dR = rot(rx, ry, rz)
    return pose12(dR @ p[:9].reshape(3, 3), dR @ p[9:] + np.array([x, y, z]))


def poses():
    """the held-out pose, an offset pose (inside the band, part of it outside the distance gate), and a pose far enough off that part of
    the frame leaves the volume and the rest lands in free or unobserved space"""
    held = VC.held_out_pose()
    return [held, moved(held, 0.006, -0.008, 0.004, 0.03, -0.02, 0.04), moved(held, 0.05, 0.3, -0.02, 1.2, 0.3, -0.9)]


def geometry(voxel=VOXEL):
    dims, desc = VC.room_geometry(voxel)
    return dims, desc, VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])


@functools.lru_cache(maxsize=None)
def room_volume(cam=SMALL_CAM, voxel=VOXEL):
    """(dims, desc, G, vol): noise-free frames of ACC_VIEWS fused by the volume oracle"""
    dims, desc, G = geometry(voxel)
    vol = G.empty()
    for k in VC.ACC_VIEWS:
        p = VC.view(k)
        vol = VO.integrate(vol, G, FO.frame_maps(VC.depth_at(p, cam), cam, 1.0, *VC.RANGE)[0], cam, p)
    vol.setflags(write=False)
    return dims, desc, G, vol


def spoiled(vol, step=211):
    """a NaN tsdf in every step-th voxel that is observed and inside the band (uploaded with volume_upload)"""
    out = vol.copy()
    flat = out.reshape(-1, 2)
    idx = np.nonzero((flat[:, 1] > 0) & (np.abs(flat[:, 0]) < 1))[0][::step]
    flat[idx, 0] = np.nan
    return out


def cropped(dims, desc, vol, crop=CROP):
    """the slab crop[0] <= i < crop[1] of the volume as a volume of its own: (dims, desc, G, vol).  It covers part of the view."""
    lo, hi = crop
    d = (hi - lo, dims[1], dims[2])
    o = (desc["origin"][0] + lo * desc["voxel_size"],) + tuple(desc["origin"][1:])
    kw = dict(desc, origin=o)
    return d, kw, VO.Geometry(d, kw["voxel_size"], o, kw["trunc"], kw["max_weight"]), np.ascontiguousarray(vol[:, :, lo:hi])


def frame_depth(cam, pose=None, holes=HOLES, seed=11):
    """depth of the room from `pose` (the held-out pose), with holes: NaN vertices, and NaN normals around them"""
    d = VC.depth_at(VC.held_out_pose() if pose is None else pose, cam).copy()
    if holes:
        rng = np.random.default_rng(seed)
        d.reshape(-1)[rng.integers(0, d.size, int(holes * d.size))] = 0
    return d


def frame_pyramid(cam, depth=None):
    return PO.frame_pyramid(frame_depth(cam) if depth is None else depth, cam, 1.0, *VC.RANGE, LEVELS)


# ---- coverage, so that no test passes on an empty answer: shares of n with a row at the held-out pose on the uncropped room, gates
# TRACK_GATES[l], cos COS_THR.  The oracle gives, at levels 0 / 1 / 2 (test_sdf_oracle.py::test_coverage_figures recomputes them):
#   160 x 120   with normals 0.77 / 0.53 / 0.32    without 0.87 / 0.86 / 0.85
#   161 x 119   with normals 0.77 / 0.54 / 0.33    without 0.87 / 0.87 / 0.85
# (the frame has holes in 1 % of its pixels, which cost a normal five; without holes 0.81 / 0.56 / 0.34 and 0.87 / 0.87 / 0.86)
COVER_NORMALS_L0, COVER_NORMALS, COVER_PLAIN = 0.5, 0.25, 0.75


def oracle_shares(cam, use_normals):
    _, _, G, vol = room_volume(SMALL_CAM)
    out = []
    for l, (_, V, N, _) in enumerate(frame_pyramid(cam)):
        ok = SO.rows(vol, G, V, N, VC.held_out_pose(), VC.TRACK_GATES[l], COS_THR, use_normals)[2]
        out.append(float(ok.sum()) / len(V))
    return out


# ---- convergence from an offset: the held-out frame (noise-free, no holes) against the volume, from view(2) -- 77 mrad / 42 mm off --
# with TRACK_ITERS rounds and TRACK_GATES.  The oracle ends (rad, m) from the truth (test_sdf_oracle.py::test_convergence_figures
# recomputes them); the GPU's sums round differently from the oracle's, so the loop is not bit-exact: margin x2, as volume_cases'.
CONVERGE = {"160": (SMALL_CAM, VOXEL), "320": (VC.HALF_CAM, 0.05)}
CONVERGE_ORACLE = {"160": (1.32e-3, 5.98e-3), "320": (3.2e-4, 1.95e-3)}
CONVERGE_START = VC.view(2)


def converge_limit(key):
    return 2 * CONVERGE_ORACLE[key][0], 2 * CONVERGE_ORACLE[key][1]


def oracle_converge(oracle_lib, key):
    cam, voxel = CONVERGE[key]
    _, _, G, vol = room_volume(cam, voxel)
    pyr = PO.frame_pyramid(VC.depth_at(VC.held_out_pose(), cam), cam, 1.0, *VC.RANGE, LEVELS)
    p, _ = SO.icp_pyramid_sdf(oracle_lib, vol, G, pyr, CONVERGE_START, VC.TRACK_ITERS, VC.TRACK_GATES, TRACK_COS)
    return VC.pose_error(p, VC.held_out_pose())


# ---- the tracking loop of volume_cases with the volume term in place of raycast, model pyramid and ICP: frame 0 fused at the truth,
# each frame tracked from the previous estimate and integrated at its own.  The oracle loop at HALF_CAM stays within (rad, m) of the
# truth and ends each frame with TRACK_ROWS rows of 76 800 pixels (test_sdf_oracle.py::test_tracking_loop_figures recomputes them;
# the raycast loop's oracle figures are 5.6e-4 rad / 3.4e-3 m).  Margin x2 on the errors, as volume_cases'.
TRACK_ORACLE = (8.5e-4, 4.7e-3)
TRACK_ROWS = (63000, 66000)


def track_limit():
    return 2 * TRACK_ORACLE[0], 2 * TRACK_ORACLE[1]


def oracle_tracking(oracle_lib, cam=VC.HALF_CAM):
    """returns the estimated poses and the rows of the last round of every tracked frame"""
    _, _, G = geometry(VC.TRACK_VOXEL)
    depths = VC.track_depths(cam)
    est, rows = [VC.track_pose(0)], []
    vol = VO.integrate(G.empty(), G, FO.frame_maps(depths[0], cam, 1.0, *VC.RANGE)[0], cam, est[0])
    for f in range(1, VC.TRACK_FRAMES):
        pyr = PO.frame_pyramid(depths[f], cam, 1.0, *VC.RANGE, LEVELS)
        p, hist = SO.icp_pyramid_sdf(oracle_lib, vol, G, pyr, est[-1], VC.TRACK_ITERS, VC.TRACK_GATES, TRACK_COS)
        est.append(p)
        rows.append(hist[-1][0])
        vol = VO.integrate(vol, G, pyr[0][1], cam, p)
    return est, rows
