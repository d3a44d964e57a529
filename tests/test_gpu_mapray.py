"""GPU: the map raycast (map_raycast_kernel / map_occupancy_kernel of csrc/rpe_frontend.hip, rpe_mapmesh_api.hip) held BIT FOR BIT --
vertices, normals and colours as words, NaNs included -- to tests/mapray_oracle.py, and, independent of the oracle, to the existing
kernels: rpe_volume_raycast and rpe_model_sample_color of a second context that holds the dense virtual volume.  The maps are
assembled on the device by volume_upload, volume_color_upload and volume_shift with the archive on."""
import os
import subprocess

import numpy as np
import pytest

import archive_cases as AC
import archive_oracle as AO
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapray_cases as RC
import mapray_oracle as MR
import shift_cases as SC
import shift_oracle as SO
from rgbd_pose_estimation_amd import _lib as L
from test_gpu_mapmesh import random_map, snapshot, unchanged
from test_gpu_rebuild import code_of

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def model(ctx, colour):
    """(vertex map, normal map, colour map or None) as the device holds them; nothing is sampled"""
    return (ctx.frame_download(L.MAP_MODEL_VERTEX), ctx.frame_download(L.MAP_MODEL_NORMAL),
            ctx.model_color_map().reshape(-1, 4) if colour else None)


def run(ctx, m, cam, pose, ray, box=None, colour=None, skip=True):
    colour = m.has_colour() if colour is None else colour
    ctx.volume_map_raycast(pose, cam, *ray, box=box, color=colour, skip_empty=skip)
    return model(ctx, colour)


def agree(got, want, what=""):
    hit = ~np.isnan(want[0]).any(1)
    print(what, "pixels", len(hit), "hits", int(hit.sum()), "NaN normals among them", int(np.isnan(want[1][hit]).any(1).sum()),
          "coloured", None if want[2] is None else int((want[2][:, 3] == 255).sum()))
    for n, g, w in zip(("vertices", "normals", "colours"), got, want):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape)
        bad = np.nonzero((words(g) != words(w)).reshape(len(g), -1).any(1))[0]
        assert not len(bad), (what, n, len(bad), bad[:5], g[bad[:3]], w[bad[:3]])
    return hit


def check(ctx, m, cam, pose, ray, box=None, what=""):
    """the oracle, with the pre-pass and without it"""
    want = RC.oracle(m, cam, pose, *ray, box=box)
    agree(run(ctx, m, cam, pose, ray, box), want, what)
    agree(run(ctx, m, cam, pose, ray, box, skip=False), want, what + ", no skip")
    return want


# ---------------------------------------------------------------------------------------------- 1. a smooth surface over bricks and the seam
@pytest.fixture(scope="module")
def sphere_map(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    m = MC.Map(ctx, (16, 16, 16)).fill(MC.sphere(*MC.SPHERE), MC.OCTANTS)
    return ctx, m


def test_a_sphere_seen_from_outside_from_the_window_and_from_an_absent_brick(sphere_map):
    ctx, m = sphere_map
    assert len(m.store) == ctx.volume_archive_info()["held"] > 20
    before = snapshot(ctx, m)
    hits, last, seam, nan_n, a0, a255 = 0, np.zeros(4, np.int64), 0, 0, 0, 0
    for name, cam, pose, box in RC.sphere_views(m):
        MV, MN, C = check(ctx, m, cam, pose, RC.SPHERE_RAY, box, "sphere, " + name)
        b = m.bounds() if box is None else box
        hit = ~np.isnan(MV).any(1)
        i0 = MR.cells(MM.geometry(m.kw, b), MV[hit])                 # box index: the box starts on a brick, local = index % 8
        last += np.bincount((i0 % 8 == 7).sum(1), minlength=4)
        wlo = np.array(m.total) - b[0]                                # the window / archive seam: cells with one foot on each side
        seam += int((((i0 == wlo - 1) | (i0 == wlo + 15)).any(1) & ((i0 >= wlo - 1) & (i0 <= wlo + 15)).all(1)).sum())
        hits, nan_n = hits + int(hit.sum()), nan_n + int(np.isnan(MN[hit]).any(1).sum())
        a0, a255 = a0 + int((C[hit][:, 3] == 0).sum()), a255 + int((C[:, 3] == 255).sum())
        assert not (C[~hit] != 0).any()
    print("hits", hits, "cells over a face / an edge / a corner", last[1:], "seam", seam, "NaN normals", nan_n, "A = 0 / 255", a0, a255)
    assert hits > 300 and (last[1:] > 0).all() and seam > 20 and 0 < nan_n < hits and a0 > 0 and a255 > 0
    assert unchanged(before, snapshot(ctx, m))                       # nothing is written


def test_the_existing_kernels_as_the_reference(sphere_map, gpu_ctx_factory):
    """a second context holds the dense virtual volume; its volume_raycast and model_color are the map raycast"""
    ctx, m = sphere_map
    box = RC.SMALLER
    vol, cvol = m.dense(box)
    ref = gpu_ctx_factory()
    G = MM.geometry(m.kw, box)
    ref.volume_init(G.dim, **dict(m.kw, origin=tuple(SO.origin_after(m.kw["origin"], m.kw["voxel_size"], box[0]))))
    ref.volume_upload(vol)
    ref.volume_color_upload(cvol.view(np.float16))
    for name, cam, pose, _ in RC.sphere_views(m)[2:]:
        ref.volume_raycast(pose, cam, *RC.SPHERE_RAY)
        want = (ref.frame_download(L.MAP_MODEL_VERTEX), ref.frame_download(L.MAP_MODEL_NORMAL), ref.model_color().reshape(-1, 4))
        hit = agree(run(ctx, m, cam, pose, RC.SPHERE_RAY, box), want, "a smaller box against rpe_volume_raycast, " + name)
        assert ctx.frame_camera(0, model=True) == ref.frame_camera(0, model=True)
    assert hit.sum() > 20


def test_the_windows_extent_is_the_windows_own_raycast(sphere_map):
    ctx, m = sphere_map
    _, cam, pose, _ = RC.sphere_views(m)[1]
    ctx.volume_raycast(pose, cam, *RC.SPHERE_RAY)
    want = (ctx.frame_download(L.MAP_MODEL_VERTEX), ctx.frame_download(L.MAP_MODEL_NORMAL), ctx.model_color().reshape(-1, 4))
    for skip in (True, False):
        hit = agree(run(ctx, m, cam, pose, RC.SPHERE_RAY, m.extent(), skip=skip), want, "the window's extent against volume_raycast")
    assert hit.sum() > 100 and (want[2][:, 3] == 255).any()


def test_a_first_sample_behind_the_surface_gives_no_hit(sphere_map):
    ctx, m = sphere_map
    _, cam, pose, _ = RC.sphere_views(m)[4]                          # pixel (8, 8) of the one-tile camera looks at the centre
    c = RC.point(m.kw, MC.SPHERE[0])
    dist = float(np.linalg.norm(pose[:9].reshape(3, 3) @ c + pose[9:]))
    centre = 8 * 16 + 8
    near = check(ctx, m, cam, pose, RC.SPHERE_RAY, None, "dmin before the surface")
    # 11 voxels before the centre of a sphere of radius 12.9: the centre ray starts inside, rays further out still start outside
    far = check(ctx, m, cam, pose, (dist - 11 * m.kw["voxel_size"], dist + 1.0), None, "dmin behind the surface")
    assert not np.isnan(near[0][centre]).any() and np.isnan(far[0][centre]).all() and not np.isnan(far[0]).all()


# ---------------------------------------------------------------------------------------------- 2. arbitrary content, absent bricks, boxes
RANDOM_RAY = (0.02, 2.2)


def random_views(m, box):
    """the odd camera from three corners of the box's surroundings, and the one-tile camera on each of the six axis directions through
    the box's middle: rays that start outside the box and leave through each of its faces"""
    lo, hi = (np.asarray(b, np.float64) for b in box)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    views = [("corner %d" % n, RC.ODD_CAM, RC.look_at(RC.point(m.kw, mid + d * (half + 9)), RC.point(m.kw, mid + 0.3 * half)))
             for n, d in enumerate(np.array([(1, 1, 1), (-1, 1, -1), (1, -1, -0.5)], np.float64))]
    for axis in range(3):
        for sign in (1, -1):
            v = mid.copy()
            v[axis] = mid[axis] - sign * (half[axis] + 6)
            up = (0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0)
            views.append(("along %+d" % (sign * (axis + 1)), RC.TILE_CAM, RC.look_at(RC.point(m.kw, v), RC.point(m.kw, mid), up)))
    return views


@pytest.mark.parametrize("colour", (True, False), ids=("colour", "tsdf"))
def test_random_content_with_absent_bricks_low_weights_nan_and_inf(gpu_ctx_factory, colour):
    ctx = gpu_ctx_factory()
    m = random_map(ctx, colour)
    # one window brick whose weights are all 0 under a tsdf that is not, one whose weights are NaN and negative: no weight > 0 in
    # either, so the pre-pass must call both absent, though neither is all-zero bits
    vol = m.window.copy()
    AO._cut(vol, (0, 0, 0))[..., 1] = 0.0
    AO._cut(vol, (0, 0, 0))[..., 0] = 0.25
    w = AO._cut(vol, (2, 1, 0))[..., 1]
    w[...] = -1.5
    w[::2] = np.nan
    m.upload(vol, m.cwindow)
    lo, hi = m.bounds()
    assert all(np.array_equal(a, b) for a, b in zip(ctx.volume_map_bounds(), (lo, hi))) and (lo < 0).any()
    dense, _ = m.dense()
    wt, ts = dense[..., 1], dense[..., 0]
    assert ((wt > 0) & (wt < 2)).sum() > 100 and np.isnan(ts).sum() > 20 and np.isinf(ts).sum() > 10
    present = {tuple(int(x) for x in k) for k in m.store} | AO.covered(m.total, m.dims)
    assert any((k[0] + 1, k[1], k[2]) not in present for k in m.store)               # a held brick with a face neighbour absent
    before = snapshot(ctx, m)
    small = (lo + [8, 0, 0], hi - [8, 8, 0])
    assert any(not all(small[0][a] <= 8 * k[a] < small[1][a] for a in range(3)) for k in m.store)
    hits = nan_n = 0
    for box in (None, small, (lo - 16, hi + [8, 24, 16])):
        for name, cam, pose in random_views(m, m.bounds() if box is None else box):
            MV, MN, C = check(ctx, m, cam, pose, RANDOM_RAY, box, f"random, box {None if box is None else [list(b) for b in box]}, {name}")
            hit = ~np.isnan(MV).any(1)
            hits, nan_n = hits + int(hit.sum()), nan_n + int(np.isnan(MN[hit]).any(1).sum())
            assert (C is None) == (not colour)
    assert hits > 500 and 0 < nan_n < hits
    assert unchanged(before, snapshot(ctx, m))
    if not colour:
        assert code_of(ctx.volume_map_raycast, pose, cam, *RANDOM_RAY, color=True) == L.RPE_ERR_STATE   # neither colour source


# ---------------------------------------------------------------------------------------------- 3. z* on a voxel centre at local 0 and 7
@pytest.mark.parametrize("axis", (0, 1, 2), ids=("x", "y", "z"))
def test_zero_tsdf_on_a_bricks_first_and_last_layer(gpu_ctx_factory, axis):
    """tsdf exactly 0 on the layers w = 8, 16 (local 0) and w = 15 (local 7); the ray of pixel (8, 8) runs along the axis through voxel
    centres, so z* lies ON a voxel centre and the normal's samples on integer g"""
    ctx = gpu_ctx_factory()
    step = [0, 0, 0]
    step[axis] = 16
    seen, s = set(), MC.KW["voxel_size"]
    for lo, hi, sign in ((8, 16, 1.0), (8, 16, -1.0), (15, 25, 1.0), (15, 25, -1.0)):
        m = MC.Map(ctx, (16, 16, 16)).fill(MC.slab(axis, lo, hi, sign), [step])
        for direction, start in ((1, -4), (-1, 35)):
            pose = RC.along(m.kw, axis, direction, start)
            MV, MN, _ = check(ctx, m, RC.TILE_CAM, pose, (s, 45 * s), None, f"slab {lo} {hi} {sign} along {direction}")
            p = MV[8 * 16 + 8]
            assert not np.isnan(p).any()
            g = (float(p[axis]) - m.kw["origin"][axis]) / s - 0.5                  # world-voxel coordinate of the hit along the axis
            assert abs(g - round(g)) < 1e-3, g
            seen.add(int(round(g)) % 8)
    assert {0, 7} <= seen, seen


def test_a_far_origin(gpu_ctx_factory):
    """|o| / s = 2^22: an ulp of p is a quarter of a voxel and samples land where exact arithmetic would not put them"""
    ctx = gpu_ctx_factory()
    kw = dict(voxel_size=0.001, origin=(4096.0, -4096.0, 2048.0), trunc=0.003, max_weight=16.0)
    m = MC.Map(ctx, (16, 16, 16), kw).fill(MC.sphere((8.3, 7.7, 8.2), 9.1), [(16, 0, 0), (0, 16, 0)])
    c, hits = RC.point(kw, (8.3, 7.7, 8.2)), 0
    for n, eye in enumerate(((30, 24, -8), (26, -10, 20))):
        MV, _, _ = check(ctx, m, RC.ODD_CAM, RC.look_at(RC.point(kw, eye), c), (0.005, 0.075), None, f"a far origin, view {n}")
        hits += int((~np.isnan(MV).any(1)).sum())
    assert hits > 200


# ---------------------------------------------------------------------------------------------- 4. errors and lifetimes
def test_errors_and_lifetimes(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    cam, ray = RC.ODD_CAM, RC.SPHERE_RAY
    pose = RC.look_at(RC.point(MC.KW, (40, 8, 4)), RC.point(MC.KW, (16, 8, 4)))
    ray_of = lambda *a, **k: code_of(ctx.volume_map_raycast, pose, cam, *a, **k)
    assert ray_of(*ray) == L.RPE_ERR_STATE                                            # no volume
    ctx.volume_init((20, 16, 8), **MC.KW)
    assert ray_of(*ray) == L.RPE_ERR_STATE                                            # a dim
    ctx.volume_init((16, 16, 8), **MC.KW)
    ctx.volume_shift((4, 0, 0))
    assert ray_of(*ray) == L.RPE_ERR_STATE                                            # the total
    ctx.volume_shift((4, 0, 0))
    m = MC.Map(None, (16, 16, 8))
    m.total = (8, 0, 0)
    m.ctx = ctx
    m.upload(*MC.sphere((15.5, 8.2, 3.9), 5.3)(m.total, m.dims))
    want = check(ctx, m, cam, pose, ray, None, "the archive off")                     # the map is the window
    hit = ~np.isnan(want[0]).any(1)
    assert hit.sum() > 100 and ctx.frame_camera(0, model=True) == tuple(float(x) if i < 4 else int(x) for i, x in enumerate(cam))
    held = model(ctx, True)
    lo, hi = ctx.volume_map_bounds()
    bad = [(lo + [4, 0, 0], hi), (lo, hi - [0, 1, 0]), (lo, lo), (hi, lo), (lo, lo + [8, 8, (1 << 20) + 8]),
           (lo, lo + [1 << 20, 1 << 20, 8])]                                          # the last: 2^34 bricks for a grid of 2^24
    for box in bad:
        assert ray_of(*ray, box=box) == L.RPE_ERR_ARG, box
    with pytest.raises(L.RpeError) as e:
        ctx.volume_map_raycast(pose, cam, *ray, box=bad[-1])
    assert e.value.code == L.RPE_ERR_ARG and "17179869184 bricks" in str(e.value)    # the count is in the message
    for dmin, dmax in ((-0.1, 1.0), (1.0, 1.0), (2.0, 1.0), (0.1, np.inf), (np.nan, 1.0), (0.0, 0.03 * (1 << 22) * 1.01)):
        assert ray_of(dmin, dmax) == L.RPE_ERR_ARG, (dmin, dmax)
    k, p, lo64 = ctx._camera(cam), np.array(pose, np.float64), np.ascontiguousarray(lo, np.int64)
    import ctypes as C
    raw = L.lib().rpe_volume_map_raycast
    assert raw(ctx._h, None, C.byref(k), 0.1, 1.0, None, None, 0) == L.RPE_ERR_ARG                    # NULL pose
    assert raw(ctx._h, p.ctypes.data, None, 0.1, 1.0, None, None, 0) == L.RPE_ERR_ARG                 # NULL camera
    assert raw(ctx._h, p.ctypes.data, C.byref(k), 0.1, 1.0, lo64.ctypes.data, None, 0) == L.RPE_ERR_ARG   # lo without hi
    assert raw(ctx._h, p.ctypes.data, C.byref(k), 0.1, 1.0, None, None, 4) == L.RPE_ERR_ARG           # an unknown flag
    agree(model(ctx, True), held, "the model after the failed calls")                 # the model is as before
    tall = run(ctx, m, cam, pose, ray, (lo, lo + [16, 16, 1 << 20]))                  # 2^20 voxels along z: 2^21 bricks, all but two absent
    agree(tall, RC.oracle(m, cam, pose, *ray, box=(lo, lo + [16, 16, 16])), "2^20 voxels along z")
    # colour: dropped without the flag, as after any raycast; the flag without any colour source
    run(ctx, m, cam, pose, ray, colour=False)
    assert code_of(ctx.model_color_map) == L.RPE_ERR_STATE
    ctx.volume_init((16, 16, 8), **MC.KW)
    assert ray_of(*ray, color=True) == L.RPE_ERR_STATE and ray_of(*ray) == L.RPE_OK
    assert np.isnan(ctx.frame_download(L.MAP_MODEL_VERTEX)).all()                     # an empty map


def test_nothing_is_written_and_the_last_mesh_stays(sphere_map):
    ctx, m = sphere_map
    V, N, T = ctx.volume_map_mesh(1.0)
    C = ctx.volume_mesh_colors()
    before = snapshot(ctx, m)
    _, cam, pose, box = RC.sphere_views(m)[2]
    run(ctx, m, cam, pose, RC.SPHERE_RAY, box)
    assert unchanged(before, snapshot(ctx, m)) and np.array_equal(ctx.volume_mesh_colors(), C) and len(V) > 1000
    V2, N2, T2 = (np.empty_like(a) for a in (V, N, T))
    assert L.lib().rpe_volume_mesh_download(ctx._h, V2.ctypes.data, N2.ctypes.data, T2.ctypes.data) == L.RPE_OK
    assert np.array_equal(words(V2), words(V)) and np.array_equal(words(N2), words(N)) and np.array_equal(T2, T)


def test_three_levels_leave_a_model_pyramid_that_icp_accepts(gpu_ctx_factory):
    import volume_cases as VC
    ctx, cam = gpu_ctx_factory(), VC.HALF_CAM
    ctx.volume_init(AC.DIMS, **SC.desc())
    p = AC.pose(0)
    ctx.frame_set_depth(VC.depth_at(p, cam), cam, 1.0, *SC.RANGE)
    ctx.volume_integrate(p)
    ctx.volume_raycast(p, cam, *SC.RAY, levels=3)
    want = [[ctx.frame_download(mp, l) for mp in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL)] for l in range(3)]
    ctx.volume_map_raycast(p, cam, *SC.RAY, levels=3)
    for l in range(3):
        for mp, w in zip((L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL), want[l]):
            assert np.array_equal(words(ctx.frame_download(mp, l)), words(w)), (l, mp)
    ctx.frame_set_depth(VC.depth_at(p, cam, 0.002, np.random.default_rng(1)), cam, 1.0, *SC.RANGE, levels=3)
    pose, *rest = ctx.icp_pyramid(p, (5, 3, 3), (0.1, 0.15, 0.2), L.RES_P2PLANE, 0.0, 0.8)
    print("icp on the map raycast's pyramid", rest)
    ang, dist = VC.pose_error(pose, p)
    assert np.isfinite(pose).all() and ang < 0.02 and dist < 0.05, (ang, dist)


# ---------------------------------------------------------------------------------------------- 5. the C++ front end
def test_map_raycast_cpp(tmp_path):
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_map_raycast")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_raycast.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "volume_map_raycast: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- 6. the use case
def test_the_walk_out_and_back_seen_whole(gpu_ctx_factory):
    """tests/mapray_cases.py through the API: the walk of tests/archive_cases.py; before each fuse of the return leg the model is raycast
    from the window and from the whole map.  The oracle's hit counts, and the conditions: every window hit is a map hit, and the map
    shows at least GAIN_LIMIT x the window at every position"""
    ctx = gpu_ctx_factory()
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(AC.CAPACITY)
    hw, hm = [], []
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = ctx.volume_follow(p, SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
            if n in AC.RETURN:
                ctx.volume_raycast(p, AC.CAM, *SC.RAY)
                W = ctx.frame_download(L.MAP_MODEL_VERTEX)
                ctx.volume_map_raycast(p, AC.CAM, *SC.RAY)
                M = ctx.frame_download(L.MAP_MODEL_VERTEX)
                hw.append(AC.hits(W, n)[0])
                hm.append(AC.hits(M, n)[0])
                assert (~np.isnan(M).any(1))[~np.isnan(W).any(1)].all(), n             # every window hit is a map hit
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(p)
    print("window", hw, "map", hm, "smallest ratio", min(a / b for a, b in zip(hm, hw)))
    assert hw == AC.HITS_ARCHIVE and hm == RC.HITS_MAP
    assert all(a >= RC.GAIN_LIMIT * b for a, b in zip(hm, hw))
    assert AC.digest(ctx.volume_download()) == AC.DIGEST_ARCHIVE and ctx.volume_archive_info()["held"] == MC.HELD
