"""Scenes shared by the volume-rebuild tests (CPU oracle and GPU): the eight drifted keyframes of graph_cases.case("small") with their
shots as attachments, the small and deliberately awkward volumes they are fused into, the wide volume of the cull tests, and the
figures of the statement that the feature repairs the map (tests/test_rebuild_oracle.py recomputes every one)."""
import numpy as np

import graph_cases as GC
import photo_cases as PC
import rebuild_oracle as RO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import SMALL_CAM

CAM = SMALL_CAM


def case():
    return GC.case("small")


def shots():
    return case().room.shots


def entry(shot, pose):
    """a shot as a list entry of the fuse: the z of its frame vertex map, its RGBA8 colour, its camera, the pose it is fused at"""
    return dict(z=shot.V[:, 2].copy(), rgba=shot.rgba.reshape(-1, 4), cam=shot.cam, pose=np.asarray(pose, np.float64))


def entries(poses, ids=None):
    s = shots()
    ids = range(len(s)) if ids is None else ids
    return [entry(s[i], poses[n]) for n, i in enumerate(ids)]


def geometry(dims, voxel_size, origin, max_weight=64):
    """(oracle geometry, volume_init keywords): trunc = 3 voxels"""
    kw = dict(voxel_size=voxel_size, origin=tuple(origin), trunc=3 * voxel_size, max_weight=max_weight)
    return VO.Geometry(dims, kw["voxel_size"], kw["origin"], kw["trunc"], kw["max_weight"]), kw


# the volumes of the core test, all across the room's back wall (z = 5) or its floor and ceiling: (dims, voxel size, origin).
# odd: 24 679 voxels with an odd row length -- no row but the first starts on a 16-byte boundary, the last lane of a brick row owns
# one voxel; flat: an even row length of two bricks, one brick high, the last brick layer a single voxel thick; two: the smallest
# volume there is
VOLUMES = {"odd": ((37, 29, 23), 0.11, (-2.0, -1.6, 2.7)), "flat": ((64, 8, 5), 0.08, (-2.56, -0.3, 4.7)), "two": ((2, 2, 2), 0.3, (-0.3, -0.3, 4.7))}
LISTS = {"one": (0,), "two": (3, 1), "three": (2, 5, 7), "all": tuple(range(8))}


def room():
    dims, kw = VC.room_geometry()
    return VO.Geometry(dims, kw["voxel_size"], kw["origin"], kw["trunc"], kw["max_weight"]), dims, kw


# ---- the cull tests: a volume several views wide whose front half (z < -1) lies behind every camera of the fan; an even row
# length of two bricks; and a keyframe posed ten metres behind everything, looking away
WIDE = ((64, 36, 68), 0.1, (-3.2, -1.9, -4.6))
BLIND = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -20.0])      # camera centre at z = 20, looking along +z: the volume is behind it
# the fan rolled and pitched by the extremes of keyframe_cases.KF_MOTIONS (and a roll none of them has), so that brick boxes
# straddle the image corners
ROLLED = ((0.2, -1.05, 0.6, 1, 0.1, 0.3), (0.2, 1.05, -0.6, -1, 0.1, 0.3), (-0.2, 0.7, 0.8, -0.9, 0.3, 0.4), (0.2, -0.35, -0.8, 0.5, 0.3, 0.1))


def rolled_poses():
    return [PC.moved(PC.START, *m) for m in ROLLED]


def brick_update_share(G, mask, brick=(32, 8, 4)):
    """the share of the kernel's bricks (32 x 8 x 4 voxels) in which the update mask (d2, d1, d0) has no voxel"""
    d0, d1, d2 = G.dim
    empty = total = 0
    for k in range(0, d2, brick[2]):
        for j in range(0, d1, brick[1]):
            for i in range(0, d0, brick[0]):
                total += 1
                empty += not mask[k:k + brick[2], j:j + brick[1], i:i + brick[0]].any()
    return empty / total


# ---- the figures: the eight shots fused into volume_cases.room_geometry() at three sets of poses, raycast from the held-out pose
_FUSED = {}


def poses_of(name):
    c = case()
    return {"truth": c.truth, "drifted": c.poses0, "optimised": c.loop[0]}[name]


def fused(name):
    """the tsdf volume of the eight shots fused (CLEAR, depth only) at the poses `name`; computed once and left unchanged"""
    if name not in _FUSED:
        G, _, _ = room()
        _FUSED[name] = RO.fuse(None, None, G, entries(poses_of(name)), RO.CLEAR)[0]
    return _FUSED[name]


def held_out_figures(MV):
    """(hits, median, 90th percentile) of |camera z of a hit - rendered depth| from volume_cases.held_out_pose(), over the pixels with
    a true depth and a hit: volume_cases.hit_depth_errors' errors"""
    pose = VC.held_out_pose()
    R, t = pose[:9].reshape(3, 3), pose[9:]
    truth = VC.depth_at(pose, CAM).reshape(-1).astype(np.float64)
    both = (truth > 0) & ~np.isnan(MV).any(1)
    err = np.abs(MV[both].astype(np.float64) @ R[2] + t[2] - truth[both])
    return int(both.sum()), float(np.median(err)), float(np.percentile(err, 90))


def oracle_figures(name):
    G, _, _ = room()
    MV, _ = VO.raycast(fused(name), G, CAM, VC.held_out_pose(), *VC.RAY)
    return held_out_figures(MV)


# (hits, median m, 90th percentile m) per set of poses, measured with the oracle on the CPU (test_rebuild_oracle.py recomputes them)
# of the 19 200 pixels of the held-out view.  The map fused at the drifted poses is off by 2.2 cm in the median and 5.9 cm at the 90th
# percentile; fused again at the optimised poses it is within 0.6 mm / 2.9 mm of the map fused at the true poses.
FIGURES = {
    "truth": (18868, 1.75e-3, 9.42e-3),
    "drifted": (18447, 2.19e-2, 5.86e-2),
    "optimised": (18884, 2.37e-3, 1.23e-2),
}
