"""Cases of the map raycast, shared by tests/test_mapray_oracle.py (CPU) and tests/test_gpu_mapray.py: cameras and views around the maps
of tests/mapmesh_cases.py (Map, sphere, slab, OCTANTS), the oracle call on a Map, and the use case: the walk of tests/archive_cases.py
with the model raycast from the window alone and from the whole map at every position of the return leg."""
import numpy as np

import archive_cases as AC
import archive_oracle as AO
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapray_oracle as MR
import shift_cases as SC
import shift_oracle as SO
import volume_oracle as VO
from frontend_util import FO

F32 = np.float32
ODD_CAM = (30.0, 30.0, 19.5, 13.5, 40, 28)           # no multiple of the 16 x 16 tile: partial tiles on both edges
TILE_CAM = (14.0, 14.0, 8.0, 8.0, 16, 16)            # one tile; pixel (8, 8) looks along the optical axis


def point(kw, v):
    """the world point at world-voxel coordinates v (voxel w has its centre at v = w), in metres"""
    return np.asarray(kw["origin"], np.float64) + (np.asarray(v, np.float64) + 0.5) * kw["voxel_size"]


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """pose12 (Xc = R Xw + t) of a camera at `eye` looking at `target`"""
    eye, z = np.asarray(eye, np.float64), np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R.reshape(9), -R @ eye])


def along(kw, axis, sign, start, others=8):
    """pose12 of a camera on the centre of the world voxel that has `start` on `axis` and `others` elsewhere, looking along sign * axis
    with its image axes on the other two: the ray of pixel (cx, cy) runs through voxel centres"""
    z = np.zeros(3)
    z[axis] = sign
    x = np.zeros(3)
    x[(axis + 1) % 3] = 1.0
    R = np.stack([x, np.cross(z, x), z])
    v = np.full(3, float(others))
    v[axis] = start
    return np.concatenate([R.reshape(9), -R @ point(kw, v)])


def oracle(m, cam, pose, dmin, dmax, box=None, colour=None):
    """mapray_oracle.raycast on a mapmesh_cases.Map: (MV, MN, MC or None)"""
    return MR.raycast(m.window, m.cwindow, m.total, m.store, m.bounds() if box is None else box, m.kw, cam, pose, dmin, dmax,
                      m.has_colour() if colour is None else colour)


def grown(box, lo=8, hi=8):
    return np.asarray(box[0], np.int64) - lo, np.asarray(box[1], np.int64) + hi


# ---- the sphere map (Map((16, 16, 16)).fill(sphere(*SPHERE), OCTANTS): the box [-16, 16)^3 all present, the window at (0, -16, -16))
SPHERE_RAY = (0.05, 1.6)
SMALLER = (np.array([-16, -8, -16]), np.array([16, 16, 8]))     # the sphere leaves it through the faces y = -8 and z = 8


def sphere_views(m):
    """[(name, camera, pose, box or None)]: from outside the map along the diagonal that meets the corner of eight bricks at world
    voxel (8, 8, 8); from inside the window; from inside an absent brick of a box one brick larger than the map; a smaller box, whose
    cut faces leave normals unknown; and the one-tile camera"""
    c = point(m.kw, MC.SPHERE[0])
    lo, hi = m.bounds()
    return [("outside", ODD_CAM, look_at(point(m.kw, (24, 24, 24)), c), None),
            ("window", ODD_CAM, look_at(point(m.kw, (13, -13, -13)), c), None),
            ("absent", ODD_CAM, look_at(point(m.kw, (20, 3, 3)), c), grown((lo, hi))),
            ("smaller", ODD_CAM, look_at(point(m.kw, (28, -2, 2)), c), SMALLER),
            ("tile", TILE_CAM, look_at(point(m.kw, (-26, 20, -22)), c, up=(0.0, 0.0, 1.0)), None)]


# ---- the use case: the archive walk, raycast before each fuse of the return leg from the window alone and from the whole map
def oracle_walk():
    """archive_cases.oracle_walk(True) with a second raycast, of the map over its bounds, beside the window's: dict(window = hits per
    return position, map = likewise, subset = every window hit is a map hit, at every position, held, box = the final bounds)"""
    total, store = (0, 0, 0), {}
    G = SC.geometry(total)
    vol = G.empty()
    kw = SC.desc()
    hw, hm, subset = [], [], True
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = SO.follow(p, SC.LOOK_AHEAD, AC.GRANULE, SO.origin_after(SC.first_origin(), AC.VOXEL, total), AC.DIMS, AC.VOXEL)
            if sh.any():
                vol, _, total = AO.shift(vol, None, total, sh, store)
                G = SC.geometry(total)
            if n in AC.RETURN:
                MVw, _ = VO.raycast(vol, G, AC.CAM, p, *SC.RAY)
                MVm, _, _ = MR.raycast(vol, None, total, store, MM.bounds(total, AC.DIMS, store), kw, AC.CAM, p, *SC.RAY)
                hw.append(AC.hits(MVw, n)[0])
                hm.append(AC.hits(MVm, n)[0])
                subset = subset and bool((~np.isnan(MVm).any(1))[~np.isnan(MVw).any(1)].all())
        vol = VO.integrate(vol, G, FO.frame_maps(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)[0], AC.CAM, p)
    return dict(window=hw, map=hm, subset=subset, held=len(store), box=MM.bounds(total, AC.DIMS, store))


# ---- the figures (oracle_walk, measured on the CPU; tests/test_mapray_oracle.py recomputes them).  Hits per position of the return
# leg among the 19 200 pixels: the window's are archive_cases.HITS_ARCHIVE (61 % of the view over the leg), the whole map's are
HITS_MAP = [15497, 16674, 17667, 17154, 16441, 15859, 15665, 15339, 15449, 14884, 13839, 12562]
# 81 %.  Every pixel the window hits, the map hits too; the smallest ratio over the twelve positions is 1.179 and the condition on the
# case is
GAIN_LIMIT = 1.15
