"""Cases of the fuse's cull, shared by tests/test_cull_oracle.py (CPU) and tests/test_gpu_volume_rules.py: a seeded generator of small
random scenes and fixed families, one per clause of the proof in csrc/rpe_volume_field.hpp.  A SCENE is one volume, its brick shape
and a list of entries (camera, pose); a CASE is one brick of one entry, a row of the table the device probe
(tests/cpp/volume_rules_probe.hip) reads.  Every number of a scene is an fp32 value held as a Python float, so the API's casts from
double change nothing and oracle, probe and library see the same bits.

Images: the API accepts 1 x 1 (width, height >= 1), and the fixed families and the generator use sizes from 1 x 1 upwards.
Volumes through the API need dims >= 2 (and multiples of 8 for the map fuse); the probe takes any dim >= 1."""
import functools

import numpy as np

import cull_oracle as CU
import volume_oracle as VO

F = np.float32
REBUILD, MAP = (32, 8, 4), (8, 8, 8)                             # the brick of volume_fuse_kernel, of map_fuse_kernel
MAX_WEIGHT = 64
RANDOM_SCENES, SEED = 9000, 20240611

# one row per case, laid out as the probe's struct: VolumeGeometry, brick origin, brick size, Camera, PoseF (132 bytes, no padding)
BRICK = np.dtype([("dim", "<i4", 3), ("o", "<f4", 3), ("s", "<f4"), ("tr", "<f4"), ("W", "<f4"), ("i0", "<i4", 3), ("n", "<i4", 3),
                  ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("w", "<i4"), ("h", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3)])


def f32(x):
    """fp32 values as Python floats (exact)"""
    a = np.asarray(x, np.float64).astype(F)
    return float(a) if a.ndim == 0 else tuple(float(v) for v in a.reshape(-1))


def scene(name, dims, s, o, brick, entries):
    """entries: [(cam (fx, fy, cx, cy, w, h), pose12 world -> camera)]"""
    s = f32(s)
    es = [(f32(c[:4]) + (int(c[4]), int(c[5])), np.array(f32(p), np.float64)) for c, p in entries]
    o = f32(np.asarray(o, np.float64) + 0.0)                      # no -0: the map's box origin, origin + 0 * voxel_size, would be +0
    return dict(name=name, dims=tuple(int(d) for d in dims), s=s, o=o, tr=f32(3.0 * s), brick=tuple(brick), entries=es)


def geometry(sc):
    return VO.Geometry(sc["dims"], sc["s"], sc["o"], sc["tr"], MAX_WEIGHT)


def kw(sc):
    """the scene's volume as volume_init takes it"""
    return dict(voxel_size=sc["s"], origin=sc["o"], trunc=sc["tr"], max_weight=MAX_WEIGHT)


def bricks_per_axis(sc):
    return [-(-d // b) for d, b in zip(sc["dims"], sc["brick"])]


# ---------------------------------------------------------------------------------------------- rotations and poses
def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def look_at(centre, target, roll=0.0):
    """world -> camera rotation of a camera at `centre` whose +z looks at `target`, rolled about its axis"""
    z = np.asarray(target, np.float64) - np.asarray(centre, np.float64)
    z = z / np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return axis_angle([0, 0, 1], roll).T @ np.stack([x, y, z])


def pose_of(R, centre):
    """(12,) world -> camera: Xc = R Xw + t with t = -R centre"""
    R = np.asarray(R, np.float64)
    return np.concatenate([R.reshape(-1), -R @ np.asarray(centre, np.float64)])


def signed_permutation(rng):
    R = np.zeros((3, 3))
    R[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    return R


# ---------------------------------------------------------------------------------------------- the generator
def random_scene(rng, n):
    """bricks of 32 x 8 x 4 over 1 .. 3 bricks per axis with ragged ends (every dim 1 .. 3 n) or of 8 x 8 x 8 over 1 .. 3 bricks per
    axis; voxels of 5 mm .. 0.37 m; origins up to 1000 m from zero; images 1 .. 40 x 1 .. 30; fx, fy independent; the principal point
    from half an image outside to half an image beyond the other side; rotations small, arbitrary up to pi and signed axis permutations;
    the camera centre from one volume extent outside to inside the volume"""
    if rng.random() < 0.5:
        brick, dims = REBUILD, [int(rng.integers(1, 3 * b + 1)) for b in REBUILD]
    else:
        brick, dims = MAP, [8 * int(rng.integers(1, 4)) for _ in range(3)]
    s = 0.005 * (0.37 / 0.005) ** rng.random()
    o = rng.uniform(-1, 1, 3) * rng.choice([0.0, 1.0, 10.0, 100.0, 1000.0])
    w, h = int(rng.integers(1, 41)), int(rng.integers(1, 31))
    fx, fy = (w * 10 ** rng.uniform(-0.7, 0.9), h * 10 ** rng.uniform(-0.7, 0.9))
    cx, cy = rng.uniform(-0.5, 1.5) * w, rng.uniform(-0.5, 1.5) * h
    ext = np.array(dims) * s
    mid = np.asarray(o) + ext / 2
    centre = mid + rng.uniform(-1.5, 1.5, 3) * ext
    kind = rng.integers(0, 4)
    if kind == 0:
        R = axis_angle(rng.normal(0, 1, 3), rng.normal(0, 0.05))
    elif kind == 1:
        R = axis_angle(rng.normal(0, 1, 3), rng.uniform(0, np.pi))
    elif kind == 2:
        R = signed_permutation(rng)
    else:                                                          # arbitrary, but looking at a point of the volume: more bricks are seen
        R = look_at(centre, np.asarray(o) + rng.uniform(0, 1, 3) * ext + 1e-9, rng.uniform(-np.pi, np.pi))
    return scene(f"random{n}", dims, s, o, brick, [((fx, fy, cx, cy, w, h), pose_of(R, centre))])


@functools.lru_cache(None)
def random_scenes(count=RANDOM_SCENES, seed=SEED):
    rng = np.random.default_rng(seed)
    return [random_scene(rng, n) for n in range(count)]


# ---------------------------------------------------------------------------------------------- the fixed families
S0, O0 = 0.05, (-0.6, -0.4, 1.0)                                  # 5 cm voxels; the corner of the fixed families' volumes
NARROW = (60.0, 55.0, 3.5, 2.5, 8, 6)
WIDE = (6.0, 5.0, 3.5, 2.5, 8, 6)


def _both(name, dims_map, dims_rebuild, s, o, entries):
    """the family over bricks of 8 x 8 x 8 and over bricks of 32 x 8 x 4 with ragged ends"""
    return [scene(name + "/map", dims_map, s, o, MAP, entries), scene(name + "/rebuild", dims_rebuild, s, o, REBUILD, entries)]


NONFINITE_BASE = np.array(f32(pose_of(np.eye(3), np.array(O0) + np.array([0.6, 0.4, -0.6]))), np.float64)   # the pose family 7 spoils


@functools.lru_cache(None)
def families():
    """one family per clause of the proof; each a pair of scenes (8^3 bricks; 32 x 8 x 4 bricks, ragged)"""
    out = []
    dm, dr = (24, 16, 16), (70, 19, 10)
    o = np.array(O0)
    at = lambda dims, fr: o + np.array(fr) * np.array(dims) * S0

    # 1. the camera centre inside a brick: on a voxel centre, between voxels, at a brick's corner; every interval holds 0
    es = []
    for fr, R in (((0.52, 0.3, 0.4), np.eye(3)), ((0.52, 0.3, 0.4), axis_angle([1, 2, 3], 2.0)), ((1 / 3, 0.5, 0.5), axis_angle([0, 1, 0], np.pi / 2)),
                  ((0.5 + 0.5 / 24, 0.5 + 0.5 / 16, 0.5 + 0.5 / 16), axis_angle([1, 0, 0], np.pi)), ((0.1, 0.9, 0.2), signed_permutation(np.random.default_rng(1)))):
        es += [(WIDE, pose_of(R, at(dm, fr))), (NARROW, pose_of(R, at(dm, fr)))]
    out += _both("inside", dm, dr, S0, O0, es)

    # 2. bricks cut by the plane z = 0: the camera in a brick's middle plane, looking along each axis and askew
    es = []
    for R in (np.eye(3), axis_angle([0, 1, 0], np.pi / 2), axis_angle([1, 0, 0], -np.pi / 2), axis_angle([1, 1, 0], 0.7)):
        for fr in ((0.5, 0.5, 0.27), (-0.3, 0.4, 0.6), (0.7, 1.4, 0.1)):
            es.append((WIDE, pose_of(R, at(dm, fr))))
    out += _both("cut", dm, dr, S0, O0, es)

    # 3. bricks entirely at cz just above 0: the camera plane an ulp-sized to a voxel-sized step behind the first layer of centres
    es = []
    for back in (1e-7, 1e-5, 1e-3, 0.5 * S0, S0):
        c = o + np.array([0.5 * dm[0] * S0, 0.5 * dm[1] * S0, 0.5 * S0 - back])
        es += [(WIDE, pose_of(np.eye(3), c)), ((0.4, 0.3, 3.5, 2.5, 8, 6), pose_of(np.eye(3), c))]
        c = o + np.array([dm[0] * S0 - 0.5 * S0 + back, 0.3 * dm[1] * S0, 0.5 * dm[2] * S0])
        es.append((WIDE, pose_of(axis_angle([0, 1, 0], -np.pi / 2), c)))          # looking along -x from behind the last layer in x
    out += _both("grazing", dm, dr, S0, O0, es)

    # 4. seen only through column 0, only through the last column, only through one corner pixel: the volume a few pixels wide, the
    # principal point moved until all but one column (row, corner) of it falls outside; sub-pixel steps put the edge on voxel centres
    es = []
    mid, dist = at(dm, (0.5, 0.5, 0.5)), 3.0
    for k in range(6):
        c = mid + np.array([0.07 * k - 0.2, 0.05 * k - 0.1, -dist])
        R = look_at(c, mid, 0.03 * k)
        f = 10.0 + 3.0 * k                                         # the volume spans about f * 1.2 / 3 pixels
        for cx, cy, w, h in ((-0.5 * f * 0.4 + 0.1 * k, 2.5, 8, 6), (7.0 + 0.5 * f * 0.4 - 0.1 * k, 2.5, 8, 6), (-0.2 * f + 0.13 * k, -0.13 * f + 0.11 * k, 8, 6),
                             (0.2 * f - 0.17 * k, 0.13 * f - 0.07 * k, 1, 1), (7.0 + 0.2 * f - 0.1 * k, 5.0 + 0.13 * f, 8, 6)):
            es.append(((f, f * 1.1, cx, cy, w, h), pose_of(R, c)))
    # ... and close up, a voxel several pixels wide seen askew: one voxel centre of a brick's corner put on column 0, on the last column,
    # on a corner pixel and into a 1 x 1 image, so that the image holds a handful of voxels, of some bricks exactly one
    for k, vox in enumerate(((0, 0, 0), (8, 8, 8), (7, 8, 7), (23, 15, 15), (16, 7, 8), (0, 15, 8))):
        c = mid + np.array([-2.0 + 0.3 * k, -1.5 + 0.4 * k, -2.5])
        R = look_at(c, mid, 0.4 * k)
        p = R @ (o + (np.array(vox) + 0.5) * S0 - c)
        f = 150.0 + 20.0 * k
        u, v = f * p[0] / p[2], f * 1.1 * p[1] / p[2]                  # where the voxel's centre falls with the principal point at 0
        for du, dv, w, h in ((0.0, 2.6, 8, 6), (7.0, 3.3, 8, 6), (0.2, 0.1, 8, 6), (7.3, 5.2, 8, 6), (0.1, -0.2, 1, 1), (0.45, 0.45, 1, 1), (-0.3, 0.2, 2, 1)):
            es.append(((f, f * 1.1, du - u, dv - v, w, h), pose_of(R, c)))
    out += _both("edges", dm, dr, S0, O0, es)

    # 5. a 45 degree roll: |R| h is at its largest against the box's own extent
    es = []
    for k, tilt in enumerate((0.0, 0.3, -0.6)):
        c = mid + np.array([0.3 * k, -0.2 * k, -1.5])
        R = axis_angle([0, 0, 1], np.pi / 4) @ axis_angle([1, 0, 0], tilt)
        es += [(NARROW, pose_of(R, c)), (WIDE, pose_of(R, c)), ((30.0, 28.0, -3.0, 8.5, 8, 6), pose_of(R, c))]
    out += _both("roll", dm, dr, S0, O0, es)

    # 6. a far origin with 5 mm voxels: the voxel is 2^-4 .. 2^-1 ulp-widths of its own coordinate apart from its neighbour's rounding
    far = (987.3, -654.1, 321.7)
    fo = np.array(f32(far))
    es = []
    for k in range(6):
        m = fo + np.array([12, 8, 8]) * 0.005
        c = m + np.array([0.02 * k - 0.05, 0.03, -0.25 + 0.03 * k])
        R = look_at(c, m + np.array([0.01 * k, 0, 0]), 0.5 * k)
        es += [((40.0, 40.0, 3.5 - 1.5 * k, 2.5, 8, 6), pose_of(R, c)), ((300.0, 300.0, 3.5, 2.5 + k, 8, 6), pose_of(R, c))]
    out += _both("far", dm, dr, 0.005, far, es)

    # 7. a NaN and an Inf in the pose: no comparison the bad row enters may cull (the z row enters all: the entry is kept everywhere)
    es = []
    for slot, bad in ((0, np.nan), (4, np.nan), (8, np.nan), (9, np.nan), (11, np.nan), (2, np.inf), (9, np.inf), (10, -np.inf), (11, np.inf), (11, -np.inf), (8, -np.inf),
                      (6, np.nan), (7, np.inf)):
        p = NONFINITE_BASE.copy()
        p[slot] = bad
        es.append((NARROW, p))
    out += _both("nonfinite", dm, dr, S0, O0, es)

    # 8. dims smaller than one brick (the API's smallest volume is 2 voxels an axis; the probe also takes 1)
    es = []
    for k in range(5):
        c = o + np.array([0.05 + 0.02 * k, 0.04, -0.3 + 0.05 * k])
        es += [(NARROW, pose_of(look_at(c, o + 0.05, 0.2 * k), c)), ((9.0, 9.0, 0.5 + k, 0.5, 8, 6), pose_of(np.eye(3), c))]
    out += [scene("small/rebuild", (3, 2, 2), S0, O0, REBUILD, es), scene("small/rebuild5", (5, 7, 3), S0, O0, REBUILD, es),
            scene("small/probe", (1, 1, 1), S0, O0, REBUILD, es), scene("small/map", (8, 8, 8), S0, O0, MAP, es)]
    return out


# ---------------------------------------------------------------------------------------------- tables
def table(scenes):
    """(T, at): the BRICK table with one row per (scene, entry, brick), bricks x fastest, and at (n, 3) = (scene, entry, brick) per row"""
    rows, at = [], []
    for si, sc in enumerate(scenes):
        nb = bricks_per_axis(sc)
        b = np.arange(nb[0] * nb[1] * nb[2])
        i0 = np.stack([b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])], -1) * np.array(sc["brick"])
        for ei, (cam, pose) in enumerate(sc["entries"]):
            T = np.zeros(len(b), BRICK)
            T["dim"], T["o"], T["s"], T["tr"], T["W"] = sc["dims"], sc["o"], sc["s"], sc["tr"], MAX_WEIGHT
            T["i0"], T["n"] = i0, sc["brick"]
            T["fx"], T["fy"], T["cx"], T["cy"], T["w"], T["h"] = cam
            with np.errstate(invalid="ignore"):
                T["R"], T["t"] = pose[:9].astype(F), pose[9:].astype(F)
            rows.append(T)
            at.append(np.stack([np.full(len(b), si), np.full(len(b), ei), b], -1))
    return np.concatenate(rows), np.concatenate(at)


def counts(scenes):
    """per row of table(scenes): how many voxels of the brick pass volume_oracle.integrate's projection test with all depth valid"""
    out = []
    for sc in scenes:
        G = geometry(sc)
        for cam, pose in sc["entries"]:
            out.append(CU.brick_counts(CU.updated(G, cam, pose), sc["brick"]))
    return np.concatenate(out)


@functools.lru_cache(None)
def case_set():
    """(scenes, T, at, count): the fixed families and the random scenes, their table and the oracle's voxel counts.  Read-only."""
    scenes = list(families()) + list(random_scenes())
    T, at = table(scenes)
    n = counts(scenes)
    for a in (T, at, n):
        a.setflags(write=False)
    return scenes, T, at, n
