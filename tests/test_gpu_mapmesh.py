"""GPU: the map mesh (csrc/rpe_mapmesh.hip, rpe_mapmesh_api.hip) held BIT FOR BIT -- vertices, normals, triangles and colours as
words, order included -- to tests/mapmesh_oracle.py, and, independent of the oracle, to the existing kernels: rpe_volume_mesh of a
second context that holds the dense virtual volume, permuted.  The maps are assembled on the device by volume_upload,
volume_color_upload and volume_shift with the archive on."""
import os
import subprocess

import numpy as np
import pytest

import archive_oracle as AO
import mapmesh_cases as MC
import mapmesh_oracle as MM
import shift_oracle as SO
from rgbd_pose_estimation_amd import _lib as L
from test_gpu_rebuild import code_of, random_start

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(words(a), words(b))


def extract(ctx, m, box=None, min_weight=1.0):
    V, N, T = ctx.volume_map_mesh(min_weight, box)
    return V, N, T, ctx.volume_mesh_colors() if m.has_colour() else None


def agree(got, want, what=""):
    names = ("vertices", "normals", "triangles", "colours")
    print(what, "vertices", len(want[0]), "triangles", len(want[2]), "NaN normals", int(np.isnan(want[1]).any(1).sum()),
          "coloured", None if want[3] is None else int((want[3][:, 3] == 255).sum()))
    for n, g, w in zip(names, got, want):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape)
        bad = np.nonzero((words(g) != words(w)).reshape(len(g), -1).any(1))[0]
        assert not len(bad), (what, n, len(bad), bad[:5], g[bad[:3]], w[bad[:3]])


def check(ctx, m, box=None, min_weight=1.0, what=""):
    want = m.mesh(box, min_weight)
    agree(extract(ctx, m, box, min_weight), want, what)
    return want


def snapshot(ctx, m):
    out = [ctx.volume_download().view(np.uint32), ctx.volume_geometry()["total_shift"], ctx.volume_geometry()["origin"]]
    out += [x if x is None else np.ascontiguousarray(x).view(np.uint8) for x in ctx.volume_archive_download()]
    if m.cwindow is not None:
        out.append(ctx.volume_color_download().view(np.uint16))
    return out


def unchanged(a, b):
    return len(a) == len(b) and all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. a smooth surface over bricks and the seam
@pytest.fixture(scope="module")
def sphere_map(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    m = MC.Map(ctx, (16, 16, 16)).fill(MC.sphere(*MC.SPHERE), MC.OCTANTS)
    return ctx, m


def test_a_sphere_across_brick_faces_edges_a_corner_and_the_seam(sphere_map):
    ctx, m = sphere_map
    lo, hi = ctx.volume_map_bounds()
    assert np.array_equal(lo, [-16] * 3) and np.array_equal(hi, [16] * 3) and lo.dtype == np.int64
    assert all(np.array_equal(a, b) for a, b in zip((lo, hi), m.bounds())) and len(m.store) == ctx.volume_archive_info()["held"] > 20
    before = snapshot(ctx, m)
    want = check(ctx, m, what="sphere, the bounds")
    vol, _ = m.dense()
    cube = MC.cube_ijk(vol)                                          # box index = world + 16: local = index % 8
    last = (cube % 8 == 7).sum(1)
    assert (last == 1).any() and (last == 2).any() and (last == 3).any()              # across a face, an edge, the corner of 8 bricks
    wlo = np.array(m.total) + 16                                                      # the window / archive seam: cubes with one
    seam = ((cube == wlo - 1) | (cube == wlo + 15)).any(1) & ((cube >= wlo - 1) & (cube <= wlo + 15)).all(1)   # foot on each side
    assert seam.sum() > 20 and len(want[2]) > 2000 and not np.isnan(want[1]).all() and (want[3][:, 3] == 255).sum() > 500
    # the same call twice, and the explicit box
    again = extract(ctx, m, (lo, hi))
    agree(again, want, "sphere, again")
    assert unchanged(before, snapshot(ctx, m))                                        # nothing is written


def test_the_existing_kernels_as_the_reference(sphere_map, gpu_ctx_factory):
    """a second context holds the dense virtual volume; its volume_mesh and volume_mesh_colors, permuted, are the map mesh"""
    ctx, m = sphere_map
    box = (np.array([-16, -8, -16]), np.array([16, 16, 8]))                           # smaller than the map on three faces
    got = extract(ctx, m, box)
    vol, cvol = m.dense(box)
    ref = gpu_ctx_factory()
    G = MM.geometry(m.kw, box)
    kw = dict(m.kw, origin=tuple(SO.origin_after(m.kw["origin"], m.kw["voxel_size"], box[0])))
    ref.volume_init(G.dim, **kw)
    ref.volume_upload(vol)
    ref.volume_color_upload(cvol.view(np.float16))
    V, N, T = ref.volume_mesh(1.0)
    C = ref.volume_mesh_colors()
    agree(got, MM.permute(vol, 1.0, V, N, T, C), "sphere, a smaller box, against rpe_volume_mesh")
    agree(got, m.mesh(box), "sphere, a smaller box")
    assert len(T) > 1000


def test_the_windows_extent_is_the_windows_own_mesh(sphere_map):
    ctx, m = sphere_map
    V, N, T = ctx.volume_mesh(1.0)
    C = ctx.volume_mesh_colors()
    got = extract(ctx, m, m.extent())
    agree(got, MM.permute(m.window, 1.0, V, N, T, C), "the window's extent against volume_mesh")
    assert len(T) > 300 and same(MC.triangle_words(*got[:3]), MC.triangle_words(V, N, T))


# ---------------------------------------------------------------------------------------------- 2. the reach: t = 0 and t = 1 at local 0 and 7
@pytest.mark.parametrize("axis", (0, 1, 2), ids=("x", "y", "z"))
def test_zero_tsdf_on_a_bricks_first_and_last_layer(gpu_ctx_factory, axis):
    """tsdf exactly 0 on the layers w = 8, 16 (local 0) and w = 15 (local 7): vertices ON voxel centres, whose normal samples sit on
    integer g -- the -2 / +10 reach"""
    ctx = gpu_ctx_factory()
    step = [0, 0, 0]
    step[axis] = 16
    seen = set()
    for lo, hi, sign in ((8, 16, 1.0), (8, 16, -1.0), (15, 25, 1.0), (15, 25, -1.0)):
        m = MC.Map(ctx, (16, 16, 16)).fill(MC.slab(axis, lo, hi, sign), [step])
        check(ctx, m, what=f"slab {lo} {hi} {sign}")
        ijk, ax, t = MC.edge_t(m.dense()[0])
        seen |= {(int(i) % 8, float(x)) for i, x in zip(ijk[ax == axis][:, axis], t[ax == axis])}
    assert {(0, 0.0), (7, 0.0), (0, 1.0), (7, 1.0)} <= seen, seen


# ---------------------------------------------------------------------------------------------- 3. arbitrary content, absent bricks, boxes
def random_map(ctx, colour, seed=5):
    """random_start content uploaded at three stops of a walk, a third of the bricks zeroed at each (they are not kept: absent), a few
    Inf among the tsdf"""
    dims = (24, 16, 8)
    m = MC.Map(ctx, dims)
    G = MM.geometry(m.kw, m.extent())
    rng = np.random.default_rng(seed)
    for n, d in enumerate([None, (8, 0, 0), (-16, -8, 8), (0, 16, -16)]):
        if d is not None:
            m.shift(d)
        vol, cvol = random_start(G, seed + n)
        bricks = AO.bricks_in([((0, 0, 0), AO.bricks_of(dims))])
        for b in [bricks[i] for i in rng.permutation(len(bricks))[:len(bricks) // 3]]:
            AO._cut(vol, b)[...] = 0
            AO._cut(cvol, b)[...] = 0
        flat = vol.reshape(-1, 2)
        flat[rng.integers(0, len(flat), 12), 0] = [np.inf, -np.inf] * 6
        m.upload(vol, cvol if colour else None)
    return m


@pytest.mark.parametrize("colour", (True, False), ids=("colour", "tsdf"))
def test_random_content_with_absent_bricks_low_weights_nan_and_inf(gpu_ctx_factory, colour):
    ctx = gpu_ctx_factory()
    m = random_map(ctx, colour)
    lo, hi = m.bounds()
    assert all(np.array_equal(a, b) for a, b in zip(ctx.volume_map_bounds(), (lo, hi))) and (lo < 0).any()   # negative world bricks
    before = snapshot(ctx, m)
    vol, _ = m.dense()
    w, ts = vol[..., 1], vol[..., 0]
    assert ((w > 0) & (w < 2)).sum() > 100 and np.isnan(ts).sum() > 20 and np.isinf(ts).sum() > 10
    present = {tuple(int(x) for x in k) for k in m.store} | AO.covered(m.total, m.dims)
    assert any((k[0] + 1, k[1], k[2]) not in present for k in m.store)               # a held brick with a face neighbour absent
    for wmin in (2.0, 1.0):                                                          # 2: the weights 1 are known to the normals only
        want = check(ctx, m, None, wmin, f"random, wmin {wmin}")
        assert len(want[2]) > 500 and np.isnan(want[1]).any(1).sum() > 50 and not np.isnan(want[1]).all()
    # a box smaller than the map (held bricks outside it are absent) and one larger than it
    small = (lo + [8, 0, 0], hi - [8, 8, 0])
    assert any(not all(small[0][a] <= 8 * k[a] < small[1][a] for a in range(3)) for k in m.store)
    check(ctx, m, small, 1.0, "random, a smaller box")
    check(ctx, m, (lo - 16, hi + [8, 24, 16]), 1.0, "random, a larger box")
    assert unchanged(before, snapshot(ctx, m))
    if not colour:
        assert code_of(ctx.volume_mesh_colors) == L.RPE_ERR_STATE                    # neither colour source


def test_a_colour_plane_in_the_pool_without_a_colour_volume(gpu_ctx_factory):
    """the colour volume goes (a rebuild with RPE_FUSE_CLEAR and no colour) and the pool's colour plane stays: held bricks keep their
    colour, the window has none"""
    import rebuild_cases as RC
    ctx, c = gpu_ctx_factory(), RC.case()
    for i, s in zip(c.fill(ctx), RC.shots()):
        s.as_frame(ctx)
        ctx.keyframe_attach_frame(i)
    dims, (_, voxel, origin) = (40, 32, 24), RC.VOLUMES["odd"]
    G, kw = RC.geometry(dims, voxel, origin, max_weight=16)
    m = MC.Map(ctx, dims, kw, capacity=64)
    m.upload(*random_start(G, 51)).shift((8, 0, 0))
    assert m.colour_plane and len(m.store) == 12
    ctx.volume_fuse_keyframes(list(RC.LISTS["three"]), clear=True, color=False)
    m.window, m.cwindow = ctx.volume_download(), None
    assert code_of(ctx.volume_color_download) == L.RPE_ERR_STATE and m.has_colour()
    want = check(ctx, m, None, 1.0, "a colour plane without a colour volume")
    held = want[0][:, 0] < G.o[0] + 8 * G.s                                           # vertices inside the archived slab
    assert (want[3][held, 3] == 255).any() and not (want[3][~held & (want[0][:, 0] > G.o[0] + 10 * G.s), 3] == 255).any()


def test_a_single_brick_and_an_empty_map(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    m = MC.Map(ctx, (8, 8, 8), capacity=0)
    V, N, T = ctx.volume_map_mesh(1.0)
    assert V.shape == (0, 3) and N.shape == (0, 3) and T.shape == (0, 3)             # all zero: empty
    assert code_of(ctx.volume_mesh_colors) == L.RPE_ERR_STATE
    m.fill(MC.sphere((3.6, 4.1, 3.3), 2.7), [])
    want = check(ctx, m, None, 1.0, "a single brick")
    assert len(want[2]) > 50
    check(ctx, m, (np.array([-8, -8, -8]), np.array([16, 16, 16])), 1.0, "a single brick in a larger box")
    m2 = MC.Map(ctx, (16, 16, 16))                                                   # archive on, nothing in it, nothing in the window
    ctx.volume_shift((16, 0, 0))
    assert ctx.volume_map_mesh(1.0)[2].shape == (0, 3) and m2.store == {}


def test_a_far_origin(gpu_ctx_factory):
    """|o| / s = 2^22: an ulp of p is a quarter of a voxel and samples land where exact arithmetic would not put them"""
    ctx = gpu_ctx_factory()
    kw = dict(voxel_size=0.001, origin=(4096.0, -4096.0, 2048.0), trunc=0.003, max_weight=16.0)
    m = MC.Map(ctx, (16, 16, 16), kw).fill(MC.sphere((8.3, 7.7, 8.2), 9.1), [(16, 0, 0), (0, 16, 0)])
    want = check(ctx, m, None, 1.0, "a far origin")
    assert len(want[2]) > 500


# ---------------------------------------------------------------------------------------------- 4. errors and lifetimes
def test_errors_and_lifetimes(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    assert code_of(ctx.volume_map_mesh) == L.RPE_ERR_STATE and code_of(ctx.volume_map_bounds) == L.RPE_ERR_STATE     # no volume
    ctx.volume_init((20, 16, 8), **MC.KW)
    assert code_of(ctx.volume_map_mesh) == L.RPE_ERR_STATE and code_of(ctx.volume_map_bounds) == L.RPE_ERR_STATE     # a dim
    ctx.volume_init((16, 16, 8), **MC.KW)
    ctx.volume_shift((4, 0, 0))
    assert code_of(ctx.volume_map_mesh) == L.RPE_ERR_STATE and code_of(ctx.volume_map_bounds) == L.RPE_ERR_STATE     # the total
    ctx.volume_shift((4, 0, 0))
    m = MC.Map(None, (16, 16, 8))
    m.total = (8, 0, 0)
    m.ctx = ctx
    m.upload(*MC.sphere((15.5, 8.2, 3.9), 5.3)(m.total, m.dims))
    lo, hi = ctx.volume_map_bounds()                                                 # the archive is off: the map is the window
    assert np.array_equal(lo, [8, 0, 0]) and np.array_equal(hi, [24, 16, 8])
    bad = [(lo + [4, 0, 0], hi), (lo, hi - [0, 1, 0]), (lo, lo), (hi, lo), (lo, lo + [8, 8, (1 << 20) + 8])]
    for box in bad:
        assert code_of(ctx.volume_map_mesh, 1.0, box) == L.RPE_ERR_ARG, box
    for w in (0.0, -1.0, np.nan, np.inf, 1e-60):
        assert code_of(ctx.volume_map_mesh, w) == L.RPE_ERR_ARG, w
    assert code_of(ctx.volume_mesh_colors) == L.RPE_ERR_STATE                        # a failed extraction drops the last mesh
    want = check(ctx, m, None, 1.0, "the archive off")
    assert len(want[2]) > 100
    tall = extract(ctx, m, (lo, lo + [8, 8, 1 << 20]))                               # 2^20 voxels along z: the bricks above are absent,
    agree(tall, m.mesh((lo, lo + [8, 8, 16])), "2^20 voxels along z")                # so the mesh is that of the box two bricks high
    # the last mesh: served by the download, replaced by the next extraction of either kind, dropped by a shift and by init
    V, N, T = ctx.volume_mesh(1.0)
    C = ctx.volume_mesh_colors()
    assert same(MC.triangle_words(V, N, T), MC.triangle_words(*want[:3])) and len(C) == len(V)
    ctx.volume_map_mesh(1.0)
    ctx.volume_shift((0, 0, 0))
    assert same(ctx.volume_mesh_colors(), want[3])
    ctx.volume_shift((8, 0, 0))
    n = np.zeros(1, np.float32)
    assert code_of(ctx.volume_mesh_colors) == L.RPE_ERR_STATE
    assert L.lib().rpe_volume_mesh_download(ctx._h, n.ctypes.data, n.ctypes.data, n.ctypes.data) == L.RPE_ERR_STATE
    ctx.volume_map_mesh(1.0)
    ctx.volume_init((16, 16, 8), **MC.KW)
    assert L.lib().rpe_volume_mesh_download(ctx._h, n.ctypes.data, n.ctypes.data, n.ctypes.data) == L.RPE_ERR_STATE


# ---------------------------------------------------------------------------------------------- 5. the C++ front end
def test_map_mesh_cpp(tmp_path):
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_map_mesh")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_mesh.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "volume_map_mesh: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- 6. the use case
def test_the_walk_out_and_back_meshed_whole(gpu_ctx_factory):
    """tests/mapmesh_cases.py through the API: the walk of tests/archive_cases.py, then the whole map and the window alone; the oracle's
    mesh bits, its figures, and the one condition: the map mesh holds every triangle of the window mesh away from the window's last layer"""
    import archive_cases as AC
    import shift_cases as SC
    ctx = gpu_ctx_factory()
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(AC.CAPACITY)
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = ctx.volume_follow(p, SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(p)
    u = MC.oracle_use_case()
    assert AC.digest(ctx.volume_download()) == u["digest"] == AC.DIGEST_ARCHIVE and ctx.volume_archive_info()["held"] == MC.HELD
    lo, hi = ctx.volume_map_bounds()
    assert tuple(lo) == MC.BOX[0] and tuple(hi) == MC.BOX[1]
    Vw, Nw, Tw = ctx.volume_mesh(MC.WMIN)
    V, N, T = ctx.volume_map_mesh(MC.WMIN)
    agree((V, N, T, None), u["map"] + (None,), "the walk, the whole map")
    assert code_of(ctx.volume_mesh_colors) == L.RPE_ERR_STATE
    fm, fw = MC.figures(V, T), MC.figures(Vw, Tw)
    print("map", fm, "window", fw)
    assert fm == u["figures_map"] and fw == u["figures_window"] and fm["triangles"] == MC.TRIANGLES_MAP and fw["triangles"] == MC.TRIANGLES_WINDOW
    inner = MC.window_triangles_away_from_the_last_layer(ctx.volume_download(), Vw, Tw)
    assert len(inner) > 10000 and MC.contains(MC.triangle_words(V, None, T, normals=False), inner)
