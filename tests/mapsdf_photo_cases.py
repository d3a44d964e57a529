"""Cases of the map volume colour term, shared by tests/test_mapsdf_photo_oracle.py (CPU) and tests/test_gpu_mapsdf_photo.py: the maps of
tests/mapsdf_cases.py GIVEN A COLOUR VOLUME (the sphere over window / held / absent bricks, the random map, the scene, the far origin),
a random map with random colour content, a map archived in two stages -- some bricks before there was a colour volume, some after --
and the use case: the textured wall of tests/photo_cases.py seen from a moving window, tracked where most of the wall in view lies in
archived bricks."""
import functools

import numpy as np

import archive_oracle as AO
import color_oracle as CO
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapsdf_cases as MSC
import mapray_oracle as MR
import mapsdf_photo_oracle as MP
import photo_cases as PC
import photo_oracle as PH
import pyramid_oracle as PO
import sdf_cases as SDC
import sdf_oracle as SO
import sdf_photo_oracle as SP
import shift_oracle as SH
import volume_cases as VC
from frontend_util import FO, SMALL_CAM, pose12, rot

F32 = np.float32
CAM_A, CAM_B, CAMS = MSC.CAM_A, MSC.CAM_B, MSC.CAMS
LEVELS, RANGE, COS_THR = MSC.LEVELS, MSC.RANGE, MSC.COS_THR
WEIGHT = PC.WEIGHT                                  # 0.01 m per intensity level
CLASSES = MSC.CLASSES
# a row needs eight TSDF weights > 0, and a voxel of an absent brick has none: in these classes no row can stand, in the others one must
NO_ROW_CLASSES = ("held, a corner absent", "absent, a corner held", "out of the box")
ROW_CLASSES = tuple(c for c in CLASSES if c not in NO_ROW_CLASSES)


# ---------------------------------------------------------------------------------------------- mapsdf_cases' maps with a colour volume
def sphere_map(ctx=None, kw=MC.KW):
    return MC.Map(ctx, (16, 16, 16), kw).fill(MC.sphere(*MC.SPHERE), MSC.SPHERE_PATH, colour=True)


def scene_map(ctx=None, archive=True):
    m = MC.Map(ctx, (24, 24, 24), capacity=256 if archive else 0)
    return m.fill(MSC.scene_world(), MSC.SCENE_PATH if archive else [], colour=True)


def far_map(ctx=None):
    return MC.Map(ctx, (16, 16, 16), MSC.FAR_KW).fill(MC.sphere(*MSC.FAR_SPHERE), [(16, 0, 0), (-8, 8, 0)], colour=True)


def frame_rgba(cam, seed=0):
    """a frame colour (h * w, 4) uint8 with A = 255: smooth ramps plus noise, every intensity finite"""
    fx, fy, cx, cy, w, h = cam
    rng = np.random.default_rng(100 + seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    rgb = np.stack([(40 + 150 * u / w), (200 - 120 * v / h), (90 + 60 * (u + v) / (w + h))], -1) + rng.uniform(-20, 20, (h, w, 3))
    return CO.frame_rgba(np.clip(rgb, 0, 255).astype(np.uint8))


def frame_levels(cam, depth, rgba, rng=RANGE):
    """[(V, N, If)] per level of the frame, and the pyramid itself"""
    pyr = PO.frame_pyramid(depth, cam, 1.0, *rng, LEVELS)
    fint = PH.intensity_pyramid(PH.intensity(np.asarray(rgba).reshape(cam[5], cam[4], 4)), LEVELS)
    return [(pyr[l][1], pyr[l][2], fint[l].reshape(-1)) for l in range(LEVELS)], pyr, fint


def oracle_rows(m, box, V, If, pose, gate, stages=None):
    return MP.rows(m.window, m.cwindow, m.total, m.store, m.kw, box, V, If, pose, gate, stages)


def reference_context(ref, m, box):
    """a second context holding the dense virtual volume AND colour volume of the box: what the contract names"""
    vol, cvol = m.dense(box)
    G = MM.geometry(m.kw, box)
    ref.volume_init(G.dim, **dict(m.kw, origin=tuple(SH.origin_after(m.kw["origin"], m.kw["voxel_size"], box[0]))))
    ref.volume_upload(vol)
    ref.volume_color_upload(np.ascontiguousarray(cvol).view(np.float16))
    return vol, cvol, G


# ---------------------------------------------------------------------------------------------- random colour content
def random_colour(dims, seed):
    """channels 0 .. 255 as binary16; colour weights 2 with one in ten 0, and a few negative, NaN and Inf; a few channels NaN / Inf /
    -Inf, most of them under a weight > 0: those propagate, as in the window term"""
    rng = np.random.default_rng(1000 + seed)
    d0, d1, d2 = dims
    c = np.empty((d2, d1, d0, 4), np.uint16)
    for ch in range(3):
        c[..., ch] = CO.h(rng.uniform(0, 255, (d2, d1, d0)).astype(F32))
    c[..., 3] = CO.h(rng.choice([0.0] + [2.0] * 9, (d2, d1, d0)).astype(F32))
    flat = c.reshape(-1, 4)
    pick = lambda n: rng.integers(0, len(flat), n)                         # noqa: E731
    flat[pick(30), 3] = 0xBC00            # -1
    flat[pick(30), 3] = 0x7E00            # NaN
    flat[pick(30), 3] = 0x7C00            # Inf: > 0
    flat[pick(40), 0] = 0x7E01
    flat[pick(40), 1] = 0x7C00
    flat[pick(40), 2] = 0xFC00
    return c


def random_map(ctx=None, seed=7):
    """mapsdf_cases.random_map's walk and TSDF content (a third of the bricks zeroed at every stop) with random_colour beside it"""
    dims = (16, 16, 16)
    m = MC.Map(ctx, dims)
    rng = np.random.default_rng(seed)
    for n, d in enumerate([None] + MSC.RANDOM_PATH):
        if d is not None:
            m.shift(d)
        vol = MSC.random_volume(dims, seed + n)
        cvol = random_colour(dims, seed + n)
        bricks = AO.bricks_in([((0, 0, 0), AO.bricks_of(dims))])
        for b in [bricks[i] for i in rng.permutation(len(bricks))[:len(bricks) // 3]]:
            AO._cut(vol, b)[...] = 0
            AO._cut(cvol, b)[...] = 0
        m.upload(vol, cvol)
    return m


def tsdf_stands(m, box, V, pose, gate):
    """per pixel: the TSDF corners let a photometric row through (cell, eight weights > 0, no corner saturated, the distance gate): what
    the colour fetch waits for.  From the oracle alone"""
    st = {}
    vol, _, G, _ = MP.virtual(m.window, m.cwindow, m.total, m.store, m.kw, box)
    SO.rows(vol, G, V, np.zeros_like(V), pose, gate, 0.0, False, st)
    return st["finite"] & st["cell"] & st["known"] & st["band"] & st["distance"]


def class_depth(m, box, cam, pose, gate, seed=3, per_class=3, steps=240, reach=2.4, every=True):
    """mapsdf_cases.class_depth with one more condition, from the oracle alone: in every class where a row can stand (ROW_CLASSES) the
    pixels given to the class get a depth at which their TSDF corners let the row through, so the colour fetch takes the class's path
    (where this view has such a pixel; the tests ask for one in every such class over the views together).  every = False: a class this view cannot reach at all is left out.  Returns the image"""
    fx, fy, cx, cy, w, h = cam
    rng = np.random.default_rng(seed)
    cand = np.linspace(0.05, reach, steps).astype(F32)
    where = np.zeros((steps, w * h, len(CLASSES)), bool)
    stands = np.zeros((steps, w * h), bool)
    for k, d in enumerate(cand):
        V = FO.frame_maps(np.full((h, w), d, F32), cam, 1.0, *RANGE)[0]
        where[k] = MSC.classes(m, box, V, pose)
        stands[k] = tsdf_stands(m, box, V, pose, gate)
    depth = cand[rng.integers(0, steps, w * h)]
    depth[rng.integers(0, 16, w * h) == 0] = 0
    taken = np.zeros(w * h, bool)
    for c, name in enumerate(CLASSES):
        hit = where[:, :, c] & (stands if name in ROW_CLASSES else True)
        if not (hit.any(0) & ~taken).any():                                # (what lies beyond the window's last layer in this view may be absent)
            hit = where[:, :, c]
        pix = np.nonzero(hit.any(0) & ~taken)[0]
        assert len(pix) or not every, (name, "no pixel of this view reaches the class")
        for p in pix[np.linspace(0, len(pix) - 1, min(per_class, len(pix))).astype(int)]:
            ks = np.nonzero(hit[:, p])[0]
            depth[p] = cand[ks[len(ks) // 2]]
            taken[p] = True
    return depth.reshape(h, w)


def rows_per_class(m, box, V, pose, gate):
    """per class, the pixels of the class whose TSDF corners let a row through"""
    return (MSC.classes(m, box, V, pose) & tsdf_stands(m, box, V, pose, gate)[:, None]).sum(0)


# What lies beyond the window's last layer, and whether eight bricks that meet in a corner all hold weights, is the map's: no single
# map here has a row in every class of ROW_CLASSES.  The random map has them where the window meets held bricks along x and y, the
# sphere -- whose surface runs through the corner of eight held bricks and through the window's last z layer -- in the other two;
# together they cover ROW_CLASSES (tests/test_mapsdf_photo_oracle.py recomputes both sets from the oracle)
RANDOM_ROW_CLASSES = ("window", "last x", "last y", "window/held face", "held/held face", "edge")
SPHERE_ROW_CLASSES = ("window", "last z", "window/held face", "held/held face", "edge", "corner")


def sphere_class_frames(m, box, cam, gate=0.1):
    """[(name, pose, depth)]: mapsdf_cases' views of the sphere with class_depth's images in place of the sphere's own"""
    return [(name + ", classes", pose, class_depth(m, box, cam, pose, gate, every=False)) for name, pose in MSC.sphere_views(m)]


# ---------------------------------------------------------------------------------------------- a map archived in two stages
# The sphere of mapmesh_cases under mapsdf_cases' walk of the 16^3 window.  The first two stops are uploaded WITHOUT colour: the bricks
# that leave at the first two shifts are archived before there is a colour volume and are held without a colour plane (zeros).  From the
# third stop on the window has colour: what leaves then is held with its colour plane.  Two octants of each kind, the window the fifth.
TWO_STAGE_FIRST_COLOUR = 2


def two_stage_map(ctx=None, kw=MC.KW):
    m = MC.Map(ctx, (16, 16, 16), kw)
    world = MC.sphere(*MC.SPHERE)
    for n, d in enumerate([None] + list(MSC.SPHERE_PATH)):
        if d is not None:
            m.shift(d)
        vol, cvol = world(m.total, m.dims)
        m.upload(vol, cvol if n >= TWO_STAGE_FIRST_COLOUR else None)
    return m


def two_stage_frames(m, cam):
    """mapsdf_cases' views of the sphere and two more, towards the two octants held with a colour plane"""
    c = MSC.RC.point(m.kw, MC.SPHERE[0])
    more = [("plane a", MSC.RC.look_at(MSC.RC.point(m.kw, (-23, -24, 22)), c)), ("plane b", MSC.RC.look_at(MSC.RC.point(m.kw, (23, -24, 22)), c))]
    return MSC.sphere_frames(m, cam) + [(name, pose, MSC.sphere_depth(m.kw, *MC.SPHERE, cam, pose)) for name, pose in more]


def held_kinds(m, box, V, pose):
    """per pixel, from the map's model: (its cell's corner-0 brick is held WITH a colour plane, ... is held WITHOUT one)"""
    lo = np.asarray(box[0], np.int64)
    G = MM.geometry(m.kw, box)
    i0 = MR.cells(G, FO.to_world(V, V, pose)[0])
    fin = np.isfinite(V).all(1) & ((i0 >= 0) & (i0 <= np.asarray(G.dim) - 2)).all(1)
    brick = (np.where(fin[:, None], i0, 0) + lo) // 8
    plane, bare = np.zeros(len(V), bool), np.zeros(len(V), bool)
    for p in np.nonzero(fin)[0]:
        held = m.store.get(tuple(int(b) for b in brick[p]))
        if held is not None:
            (plane if np.asarray(held[1]).any() else bare)[p] = True
    return plane, bare


# ---------------------------------------------------------------------------------------------- the use case
# The textured wall of photo_cases (the plane z = 3, nothing else in view) seen from a camera that slides along it, further than its
# 64^3 window at 4 cm is wide.  Modelled on archive_cases' walk: 160 x 120 frames, every frame fused WITH ITS COLOUR at its TRUE pose,
# the archive on; the window moves a brick (8 voxels, 0.32 m) with every frame, as the camera does.  At the walk's end the window lies
# 3.84 m from where it began and the wall behind it is in archived bricks, held with their colour planes.  The frame is then held
# against the map from WALK_BACK, camera positions back along the wall, where the window covers only the rim of the view (a third to a
# sixth of its width; the rest of the wall in view lies in archived bricks), from the true pose moved by WALK_OFFSET, with three loops:
#   icp_pyramid_map_sdf         the whole map's geometry: a plane holds no in-plane motion
#   icp_pyramid_sdf_rgbd        the window's geometry and colour: a strip of rows at the view's rim
#   icp_pyramid_map_sdf_rgbd    the whole map's geometry and colour
WALK_CAM = SMALL_CAM
WALK_DIMS, WALK_VOXEL = (64, 64, 64), 0.04
WALK_KW = dict(voxel_size=WALK_VOXEL, origin=(-1.28, -1.28, 1.4), trunc=3 * WALK_VOXEL, max_weight=64.0)
WALK_FRAMES = 13
WALK_STEP = 8                                          # voxels per frame, window and camera alike
WALK_BACK = (1.7, 2.0, 2.3)                            # metres back from the last fused position
WALK_OFFSET = (0.004, -0.006, 0.003, 0.02, -0.015, 0.02)
WALK_ITERS, WALK_GATES = (10, 5, 4), (0.1, 0.1, 0.1)
WALK_NOISE = VC.TRACK_NOISE


def walk_pose_at(x):
    """the camera at (x, 0.05, 0.2) looking along +z at the wall, a little tilted"""
    R = rot(0.03, -0.02, 0.01)
    return pose12(R, -R @ np.array([x, 0.05, 0.2]))


def walk_pose(n):
    return walk_pose_at(n * WALK_STEP * WALK_VOXEL)


def walk_eval_pose(k):
    return walk_pose_at((WALK_FRAMES - 1) * WALK_STEP * WALK_VOXEL - WALK_BACK[k])


def walk_frame(pose, seed):
    """(depth, rgb) of the wall from `pose`"""
    return PC.depth_at(pose, WALK_CAM, PC.WALL, WALK_NOISE, np.random.default_rng(300 + seed)), PC.rgb_at(pose, WALK_CAM, PC.WALL)


def walk_start(k):
    return SDC.moved(walk_eval_pose(k), *WALK_OFFSET)


def walk_geometry(total):
    return SH.geometry_after(WALK_DIMS, WALK_VOXEL, WALK_KW["origin"], WALK_KW["trunc"], WALK_KW["max_weight"], [int(t) for t in total])


@functools.lru_cache(maxsize=None)
def oracle_walk_map():
    """(window, colour window, total, store) at the walk's end, in the oracles"""
    total, store = (0, 0, 0), {}
    G = walk_geometry(total)
    vol, cvol = G.empty(), CO.empty(G)
    for n in range(WALK_FRAMES):
        if n:
            vol, cvol, total = AO.shift(vol, cvol, total, (WALK_STEP, 0, 0), store)
            G = walk_geometry(total)
        d, rgb = walk_frame(walk_pose(n), n)
        vol, cvol = CO.integrate(vol, cvol, G, FO.frame_maps(d, WALK_CAM, 1.0, *VC.RANGE)[0], CO.frame_rgba(rgb), WALK_CAM, walk_pose(n))
    return vol, np.ascontiguousarray(cvol).view(np.uint16), total, store


def oracle_walk(oracle_lib):
    """per evaluated position: dict(rows_window, rows_map = photometric rows at the true pose (level 0, gate 0.1), err_map_sdf,
    err_window_rgbd, err_map_rgbd = (rad, m) from the truth where each loop ends from walk_start; NaN where a loop lost the frame)"""
    vol, cvol, total, store = oracle_walk_map()
    G = walk_geometry(total)
    mvol, mcvol, mG, box = MP.virtual(vol, cvol, total, store, WALK_KW)
    out = []
    for k in range(len(WALK_BACK)):
        p = walk_eval_pose(k)
        d, rgb = walk_frame(p, 50 + k)
        lv, pyr, fint = frame_levels(WALK_CAM, d, CO.frame_rgba(rgb), VC.RANGE)
        V, N, If = lv[0]
        res = dict(rows_window=int(SP.rows(vol, cvol, G, V, If, p, WALK_GATES[0])[2].sum()),
                   rows_map=int(SP.rows(mvol, mcvol, mG, V, If, p, WALK_GATES[0])[2].sum()))
        for key, run in (("err_map_sdf", lambda: SO.icp_pyramid_sdf(oracle_lib, mvol, mG, pyr, walk_start(k), WALK_ITERS, WALK_GATES, COS_THR)),
                         ("err_window_rgbd", lambda: SP.icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, pyr, fint, walk_start(k), WALK_ITERS,
                                                                             WALK_GATES, COS_THR, WEIGHT)),
                         ("err_map_rgbd", lambda: SP.icp_pyramid_sdf_rgbd(oracle_lib, mvol, mcvol, mG, pyr, fint, walk_start(k), WALK_ITERS,
                                                                          WALK_GATES, COS_THR, WEIGHT))):
            try:
                res[key] = tuple(float(e) for e in VC.pose_error(run()[0], p))
            except Exception as e:                                         # a round without a solution: the loop lost the frame
                res[key] = (float("nan"), float("nan"), type(e).__name__)
        out.append(res)
    return out


# ---- the figures (oracle_walk, measured on the CPU; tests/test_mapsdf_photo_oracle.py recomputes them).  The walk ends at total
# (96, 0, 0) with 470 bricks held, 192 of them with a colour in their plane (the wall's).  Photometric rows at the true pose per
# evaluated position, of the 19 200 pixels: the map has 2.7 x to 5.6 x the window's.
WALK_TOTAL, WALK_HELD = (96, 0, 0), 470
ROWS_WINDOW = [7052, 5206, 3363]
ROWS_MAP = [18957, 18942, 18922]
# Where each loop ends from WALK_OFFSET (7.8 mrad, 32 mm off), (rotation rad, camera centre m) per evaluated position.  The geometry of
# the whole map leaves the in-plane motion where it was (19 .. 36 mm); the window's colour holds it with a strip of rows (0.6 .. 2.0 mm);
# the map's colour holds it with the whole view (0.07 .. 0.19 mm).  THE CONDITION ON THE CASE: at every position the new loop's
# translation error is at most half of the smaller of the other two (here 0.30, 0.29 and 0.03 of it).
ERR_MAP_SDF = [(1.73e-2, 1.85e-2), (1.31e-3, 3.61e-2), (4.27e-4, 2.60e-2)]
ERR_WINDOW_RGBD = [(5.24e-4, 5.86e-4), (9.28e-4, 6.61e-4), (1.42e-3, 1.98e-3)]
ERR_MAP_RGBD = [(2.05e-4, 1.77e-4), (1.96e-4, 1.90e-4), (1.66e-4, 6.65e-5)]


def walk_limit(k):
    """what the GPU loop is held to at position k: the oracle's errors x2, the margin volume_cases gives such loops (the GPU's sums round
    differently from the oracle's)"""
    return 2 * ERR_MAP_RGBD[k][0], 2 * ERR_MAP_RGBD[k][1]
