"""Cases of the map volume term, shared by tests/test_mapsdf_oracle.py (CPU) and tests/test_gpu_mapsdf.py: small maps of
tests/mapmesh_cases.py (Map, sphere) with frames whose vertices land where the corner fetch takes another path, the classes of a
pixel's cell, and the use case: the walk of tests/archive_cases.py, tracked on its return leg against the window alone and against
the whole map."""
import numpy as np

import archive_cases as AC
import archive_oracle as AO
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapray_cases as RC
import mapray_oracle as MR
import mapsdf_oracle as MO
import pyramid_oracle as PO
import sdf_cases as SDC
import sdf_oracle as SO
import shift_cases as SC
import shift_oracle as SH
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO

F32 = np.float32
CAM_A = (30.0, 30.0, 19.5, 14.5, 40, 30)     # 1 200 pixels: several workgroups; three levels end at 10 x 7
CAM_B = (16.0, 16.0, 10.0, 6.0, 21, 13)      # 273 pixels: no multiple of 4, just over one 256-thread workgroup
CAMS = {"40x30": CAM_A, "21x13": CAM_B}
LEVELS = 3
RANGE = (0.01, 10.0, 0.1)                     # dmin, dmax, the normals' largest depth step
COS_THR = 0.9


def level_pyramid(depth, cam, rng=RANGE):
    return PO.frame_pyramid(depth, cam, 1.0, *rng, LEVELS)


def sphere_depth(kw, centre, radius, cam, pose):
    """the z-depth image of the sphere (centre and radius in voxels of the world grid) from pose12, 0 where the ray misses; from inside
    the sphere it is the far wall"""
    fx, fy, cx, cy, w, h = cam
    R, t = np.asarray(pose[:9], np.float64).reshape(3, 3), np.asarray(pose[9:], np.float64)
    eye = -R.T @ t
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, np.float64)], -1) @ R       # rows: R^T d
    oc = eye - RC.point(kw, centre)
    a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - (radius * kw["voxel_size"]) ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        root = np.sqrt(disc)
        near, far = (-b - root) / (2 * a), (-b + root) / (2 * a)
    s = np.where(near > 0, near, far)
    return np.where((disc >= 0) & (s > 0), s, 0.0).astype(F32)


# ---------------------------------------------------------------------------------------------- the classes of a pixel's cell
CLASSES = ("window", "last x", "last y", "last z", "window/held face", "held/held face", "edge", "corner", "held, a corner absent",
           "absent, a corner held", "out of the box")


def brick_status(m, box):
    """per brick of the box, (nb2, nb1, nb0): 0 absent, 1 the window's, 2 held"""
    lo, hi = (np.asarray(b, np.int64) for b in box)
    nb = (hi - lo) // 8
    st = np.zeros((nb[2], nb[1], nb[0]), np.int8)
    for key in m.store:
        b = np.asarray(key, np.int64) - lo // 8
        if ((b >= 0) & (b < nb)).all():
            st[b[2], b[1], b[0]] = 2
    w0 = np.asarray(m.total, np.int64) // 8 - lo // 8
    wn = np.asarray(m.dims, np.int64) // 8
    a, b = np.maximum(w0, 0), np.minimum(w0 + wn, nb)
    if (a < b).all():
        st[a[2]:b[2], a[1]:b[1], a[0]:b[0]] = 1
    return st


def classes(m, box, V, pose):
    """(pixels, len(CLASSES)) bool: where the cell of each frame vertex (mapray_oracle.cells of its world point) falls.  A pixel
    without a finite vertex is in no class"""
    lo, hi = (np.asarray(b, np.int64) for b in box)
    G = MM.geometry(m.kw, box)
    W = FO.to_world(V, V, pose)[0]
    i0 = MR.cells(G, W)
    fin = np.isfinite(V).all(1)
    dim = hi - lo
    inside = fin & ((i0 >= 0) & (i0 <= dim - 2)).all(1)
    st = brick_status(m, box)
    c0 = np.where(inside[:, None], i0, 0)
    corner = np.stack([st[(c0[:, 2] + dk) // 8, (c0[:, 1] + dj) // 8, (c0[:, 0] + di) // 8]
                       for dk in (0, 1) for dj in (0, 1) for di in (0, 1)], -1)            # (pixels, 8), corner 0 first
    l = c0 - (np.asarray(m.total, np.int64) - lo)                                        # the cell in the window's own index
    wd = np.asarray(m.dims, np.int64)
    in_window = ((l >= 0) & (l <= wd - 1)).all(1)
    crossing = (c0 % 8 == 7).sum(1)
    out = np.zeros((len(V), len(CLASSES)), bool)
    out[:, 0] = inside & ((l >= 0) & (l <= wd - 2)).all(1)
    for a in range(3):
        out[:, 1 + a] = inside & in_window & (l[:, a] == wd[a] - 1)
    out[:, 4] = inside & (corner == 1).any(1) & (corner == 2).any(1)
    out[:, 5] = inside & (crossing == 1) & (corner == 2).all(1)
    out[:, 6] = inside & (crossing == 2)
    out[:, 7] = inside & (crossing == 3)
    out[:, 8] = inside & (corner[:, 0] == 2) & (corner == 0).any(1)
    out[:, 9] = inside & (corner[:, 0] == 0) & (corner == 2).any(1)
    out[:, 10] = fin & ~inside
    return out


def class_depth(m, box, cam, pose, seed=3, per_class=3, steps=240, reach=2.4):
    """a depth image chosen on the CPU so that the frame has pixels in every class: a pixel's vertex depends on its own depth alone, so
    every pixel is tried at `steps` depths up to `reach` metres, per class a few pixels are given a depth that puts their cell there,
    and the rest get one of the depths at random (one pixel in 16 none).  Returns the image and the classes it was built for"""
    fx, fy, cx, cy, w, h = cam
    rng = np.random.default_rng(seed)
    cand = np.linspace(0.05, reach, steps).astype(F32)
    where = np.zeros((steps, w * h, len(CLASSES)), bool)
    for k, d in enumerate(cand):
        V = FO.frame_maps(np.full((h, w), d, F32), cam, 1.0, *RANGE)[0]
        where[k] = classes(m, box, V, pose)
    depth = cand[rng.integers(0, steps, w * h)]
    depth[rng.integers(0, 16, w * h) == 0] = 0
    taken = np.zeros(w * h, bool)
    for c in range(len(CLASSES)):
        pix = np.nonzero(where[:, :, c].any(0) & ~taken)[0]
        assert len(pix), (CLASSES[c], "no pixel of this view reaches the class")
        for p in pix[np.linspace(0, len(pix) - 1, min(per_class, len(pix))).astype(int)]:
            ks = np.nonzero(where[:, p, c])[0]
            depth[p] = cand[ks[len(ks) // 2]]
            taken[p] = True
    return depth.reshape(h, w)


# ---------------------------------------------------------------------------------------------- the maps
# the sphere of mapmesh_cases over a 16^3 window that visits five of the eight octants of [-16, 16)^3 and ends at total (0, 0, -16):
# inside the box [-16, 16)^3 the surface runs through the window, through held bricks and through the three octants never visited
SPHERE_PATH = MC.OCTANTS[:4]
SPHERE_BOX = (np.array([-16, -16, -16]), np.array([16, 16, 16]))
GROWN_BOX = (np.array([-16, -24, -16]), np.array([24, 16, 16]))        # 40 x 40 x 32: absent bricks around the map, another origin


def sphere_map(ctx=None, kw=MC.KW):
    return MC.Map(ctx, (16, 16, 16), kw).fill(MC.sphere(*MC.SPHERE), SPHERE_PATH, colour=False)


def sphere_views(m):
    """[(name, pose12)]: the sphere seen from outside along four diagonals -- towards the window's octant, a held one, one never
    visited, and one more -- and from its centre region looking at the seam"""
    c = RC.point(m.kw, MC.SPHERE[0])
    eye = lambda *v: RC.look_at(RC.point(m.kw, v), c)                      # noqa: E731
    return [("window", eye(22, 23, -24)), ("held", eye(23, 24, 22)), ("absent", eye(-23, -24, -22)), ("seam", eye(-2, 30, 3)),
            ("inside", RC.look_at(RC.point(m.kw, (1, 2, -1)), RC.point(m.kw, (-9, 9, -2))))]


def sphere_frames(m, cam):
    return [(name, pose, sphere_depth(m.kw, *MC.SPHERE, cam, pose)) for name, pose in sphere_views(m)]


# arbitrary content: a 16^3 window walks over [0, 32) x [0, 32) x [0, 24) with a third of its bricks zeroed at every stop (absent)
RANDOM_PATH = [(16, 0, 0), (0, 16, 0), (-16, 0, 8), (8, -8, -8)]
RANDOM_GATE = 0.09                                                       # = trunc: every |tsdf| < 1 passes the distance gate


def random_volume(dims, seed):
    """tsdf in (-1, 1) with a few |tsdf| >= 1, NaN and Inf; weights 0, 1, 2 with a few negative, NaN and Inf"""
    rng = np.random.default_rng(seed)
    d0, d1, d2 = dims
    vol = np.empty((d2, d1, d0, 2), F32)
    vol[..., 0] = rng.uniform(-1, 1, (d2, d1, d0))
    vol[..., 1] = rng.choice([0.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0], (d2, d1, d0))
    t, wt = vol[..., 0].reshape(-1), vol[..., 1].reshape(-1)
    pick = lambda n: rng.integers(0, t.size, n)                            # noqa: E731
    t[pick(40)] = [1.0, -1.0, 1.5, -3.0] * 10
    t[pick(20)] = np.nan
    t[pick(10)] = [np.inf, -np.inf] * 5
    wt[pick(20)] = -1.5
    wt[pick(20)] = np.nan
    wt[pick(20)] = np.inf
    return vol.reshape(d2, d1, d0, 2)


def random_map(ctx=None, seed=7):
    dims = (16, 16, 16)
    m = MC.Map(ctx, dims)
    rng = np.random.default_rng(seed)
    for n, d in enumerate([None] + RANDOM_PATH):
        if d is not None:
            m.shift(d)
        vol = random_volume(dims, seed + n)
        bricks = AO.bricks_in([((0, 0, 0), AO.bricks_of(dims))])
        for b in [bricks[i] for i in rng.permutation(len(bricks))[:len(bricks) // 3]]:
            AO._cut(vol, b)[...] = 0
        m.upload(vol)
    return m


def random_views(m, box):
    """two poses from outside the box, looking through it"""
    lo, hi = (np.asarray(b, np.float64) for b in box)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    return [RC.look_at(RC.point(m.kw, mid + d * (half + 6)), RC.point(m.kw, mid + 0.2 * half)) for d in
            np.array([(1, 0.8, -1), (-0.9, -1, 0.7)], np.float64)]


# a scene that holds all six degrees of freedom, for the record and the loops: a back wall and two spheres in front of it, in a 24^3
# window that walks over [0, 40) x [0, 40) x [0, 24) and ends at total (0, 16, 0)
SCENE_PATH = [(16, 0, 0), (0, 16, 0), (-16, 0, 0)]
SCENE_WALL = 18.0
SCENE_SPHERES = (((12.0, 14.0, 12.0), 6.0), ((28.0, 26.0, 13.0), 5.0))
SCENE_OFFSET = (0.006, -0.008, 0.004, 0.015, -0.01, 0.02)               # the loops' start: 11 mrad and 27 mm from the frame's pose


def scene_world():
    def f(X, Y, Z):
        d = SCENE_WALL - Z
        for c, r in SCENE_SPHERES:
            d = np.minimum(d, np.sqrt((X - c[0]) ** 2.0 + (Y - c[1]) ** 2.0 + (Z - c[2]) ** 2.0) - r)
        return np.clip(d / 3.0, -1.0, 1.0), 2.0
    return MC.world_of(f)


def scene_map(ctx=None, archive=True):
    m = MC.Map(ctx, (24, 24, 24), capacity=256 if archive else 0)
    return m.fill(scene_world(), SCENE_PATH, colour=False) if archive else m.fill(scene_world(), [], colour=False)


def grown(m):
    """the map's bounds with a layer of bricks below and above along z: 40^3 for the scene, absent bricks, another fp32 origin"""
    lo, hi = m.bounds()
    return lo - [0, 0, 8], hi + [0, 0, 8]


def scene_pose():
    return RC.look_at(RC.point(MC.KW, (19, 21, -22)), RC.point(MC.KW, (20, 20, 12)))


def scene_depth(cam, pose=None, kw=MC.KW):
    """the scene's z-depth from pose12: the nearest of the wall and the spheres along every pixel's ray"""
    pose = scene_pose() if pose is None else pose
    fx, fy, cx, cy, w, h = cam
    R, t = np.asarray(pose[:9], np.float64).reshape(3, 3), np.asarray(pose[9:], np.float64)
    eye = -R.T @ t
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, np.float64)], -1) @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (RC.point(kw, (0, 0, SCENE_WALL))[2] - eye[2]) / d[..., 2]
    best = np.where(s > 0, s, np.inf)
    for c, r in SCENE_SPHERES:
        z = sphere_depth(kw, c, r, cam, pose).astype(np.float64)
        best = np.where(z > 0, np.minimum(best, z), best)
    return np.where(np.isfinite(best), best, 0.0).astype(F32)


def scene_start():
    return SDC.moved(scene_pose(), *SCENE_OFFSET)


FAR_KW = dict(voxel_size=0.001, origin=(4096.0, -4096.0, 2048.0), trunc=0.003, max_weight=16.0)   # |o| / s = 2^22
FAR_SPHERE = ((8.3, 7.7, 8.2), 9.1)
FAR_RANGE = (0.001, 1.0, 0.01)


def far_map(ctx=None):
    return MC.Map(ctx, (16, 16, 16), FAR_KW).fill(MC.sphere(*FAR_SPHERE), [(16, 0, 0), (-8, 8, 0)], colour=False)


def far_frames(m, cam):
    c = RC.point(m.kw, FAR_SPHERE[0])
    return [(n, p, sphere_depth(m.kw, *FAR_SPHERE, cam, p)) for n, p in
            (("a", RC.look_at(RC.point(m.kw, (30, 24, -8)), c)), ("b", RC.look_at(RC.point(m.kw, (20, 22, 20)), c)))]


def oracle_rows(m, box, V, N, pose, gate, cos_thr=COS_THR, use_normals=True, stages=None):
    return MO.rows(m.window, m.total, m.store, m.kw, box, V, N, pose, gate, cos_thr, use_normals, stages)


def reference_context(ref, m, box):
    """a second context holding the dense virtual volume of the box: what the contract names"""
    vol, _ = m.dense(box)
    G = MM.geometry(m.kw, box)
    ref.volume_init(G.dim, **dict(m.kw, origin=tuple(SH.origin_after(m.kw["origin"], m.kw["voxel_size"], box[0]))))
    ref.volume_upload(vol)
    return vol, G


# ---------------------------------------------------------------------------------------------- the use case
# The walk of tests/archive_cases.py out and back (a 64^3 window at 4 cm, every frame fused at its true pose, the archive on).  At
# every position of the return leg, before the frame is fused, the frame is held against the window's field and against the map's
# over its bounds: the rows each term has at the TRUE pose (level 0, icp_pyramid_sdf's defaults: gate 0.1 m, cos 0.9, normals), and
# the pose each ends at from the true pose moved by WALK_OFFSET, with icp_pyramid_sdf's defaults (10, 5, 4 rounds).
WALK_OFFSET = (0.004, -0.006, 0.003, 0.02, -0.015, 0.02)
WALK_ITERS, WALK_GATES = (10, 5, 4), (0.1, 0.1, 0.1)


def walk_start(n):
    return SDC.moved(AC.pose(n), *WALK_OFFSET)


def oracle_walk(oracle_lib=None):
    """dict(window = rows per return position, map = likewise, window_err / map_err = (rad, m) from the truth where each term's loop
    ends (only with the C oracle's solver), held, box = the final bounds)"""
    total, store = (0, 0, 0), {}
    G = SC.geometry(total)
    vol = G.empty()
    kw = SC.desc()
    out = dict(window=[], map=[], window_err=[], map_err=[])
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = SH.follow(p, SC.LOOK_AHEAD, AC.GRANULE, SH.origin_after(SC.first_origin(), AC.VOXEL, total), AC.DIMS, AC.VOXEL)
            if sh.any():
                vol, _, total = AO.shift(vol, None, total, sh, store)
                G = SC.geometry(total)
            if n in AC.RETURN:
                pyr = PO.frame_pyramid(AC.depth(n), AC.CAM, 1.0, *SC.RANGE, LEVELS)
                _, V, N, _ = pyr[0]
                mvol, mG, _ = MO.virtual(vol, total, store, kw)
                out["window"].append(int(SO.rows(vol, G, V, N, p, WALK_GATES[0], COS_THR)[2].sum()))
                out["map"].append(int(SO.rows(mvol, mG, V, N, p, WALK_GATES[0], COS_THR)[2].sum()))
                if oracle_lib is not None:
                    for key, (v, g) in (("window_err", (vol, G)), ("map_err", (mvol, mG))):
                        try:
                            q, _ = SO.icp_pyramid_sdf(oracle_lib, v, g, pyr, walk_start(n), WALK_ITERS, WALK_GATES, COS_THR)
                            out[key].append(VC.pose_error(q, p))
                        except Exception as e:                             # a round without a solution: the term lost the frame
                            out[key].append((float("nan"), float("nan"), type(e).__name__))
        vol = VO.integrate(vol, G, FO.frame_maps(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)[0], AC.CAM, p)
    out.update(held=len(store), box=MM.bounds(total, AC.DIMS, store))
    return out


# ---- the figures (oracle_walk, measured on the CPU; tests/test_mapsdf_oracle.py recomputes them).  Rows at the true pose per position
# of the return leg, of the 19 200 pixels:
ROWS_WINDOW = [11755, 12050, 11571, 10876, 11160, 11022, 9778, 9312, 6949, 3356, 2272, 4669]
ROWS_MAP = [13714, 14868, 16058, 16228, 14864, 12892, 11442, 9606, 7812, 5416, 4018, 4794]
# 104 770 rows over the leg against 131 712: the map term has 26 % more, and more at every position (1.03 x to 1.77 x; the last
# position is the start pose, where the window is back over what it fused first).  From WALK_OFFSET (7.8 mrad, 32 mm off) both loops
# end within 3.2 mrad and 7.7 mm of the truth at every position; the worst rotation error is the window term's (3.1 mrad where it is
# down to 3 356 rows, the map term 1.3 mrad there), the worst translation error the map term's (7.7 mm, the window term 4.9 mm there).
ERR_LIMIT = (3.2e-3, 7.7e-3)
