"""CPU: the windowed oracle (integrate, field, raycast and mesh over z-slab windows of a larger volume) joins to the full oracle bit for
bit; every edge case of tests/volume_edge_cases.py really occurs and the oracle gives the value derived by hand; the checkerboard's
analytic counts; the chunk counts of the mesh scan cases."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
import volume_edge_cases as E
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12, rot

f32 = np.float32


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- windows
DIMS = (37, 29, 41)
WINDOWS = [(0, 9), (11, 24), (26, 41)]                  # separated by the unobserved slabs 9, 10, 24, 25


def windowed_scene():
    """a field of bumps over odd dims, weight 1 inside the windows (and a different third of x in each), 0 elsewhere"""
    G, desc = MC.geometry(DIMS, 0.05, (-0.9, -0.7, 0.3), max_weight=8)
    k = 2 * np.pi / 0.45
    vol = MC.sdf_volume(G, lambda x, y, z: 0.06 * np.sin(k * x) * np.cos(k * y) + 0.08 * np.sin(0.7 * k * z) - 0.02)
    vol[..., 1] = 0.0
    i = np.arange(DIMS[0])
    for n, (k0, k1) in enumerate(WINDOWS):
        cols = (i >= n * DIMS[0] // 4) if n < 2 else np.ones_like(i, bool)
        vol[k0:k1, :, cols, 1] = 1.0
    return G, vol, desc


def test_windowed_integrate_joins_to_the_full_one():
    G, vol, _ = windowed_scene()
    vol = E.awkward(G, 3, 8)
    p = pose12(rot(0.05, -0.1, 0.02), np.array([0.05, 0.02, 0.0]))
    d = np.full((SMALL_CAM[5], SMALL_CAM[4]), 1.6, f32)
    d[:, ::7] = 0
    V = FO.frame_maps(d, SMALL_CAM, 1.0, 0.1, 10.0, 0.1)[0]
    full, ok = VO.integrate(vol, G, V, SMALL_CAM, p, with_mask=True)
    assert 0.05 < ok.mean() < 0.95
    parts = [VO.integrate(vol[k0:k1], G, V, SMALL_CAM, p, k0, with_mask=True) for k0, k1 in [(0, 1), (1, 12), (12, 40), (40, 41)]]
    assert bits_equal(np.concatenate([o for o, _ in parts]), full)
    assert np.array_equal(np.concatenate([m for _, m in parts]), ok)


def test_windowed_field_raycast_and_mesh_join_to_the_full_ones():
    G, vol, _ = windowed_scene()
    windows = [(k0, vol[k0:k1].copy()) for k0, k1 in WINDOWS]
    # the field: a window answers exactly where the full volume does, and is unknown where its cell leaves the window
    rng = np.random.default_rng(1)
    X = (G.o + rng.uniform(-0.1, 1.0, (20000, 3)) * np.array(DIMS) * G.s).astype(f32)
    v, kn = VO.field(vol, G, X)
    vw, kw = VO.windows_field(windows, G, X)
    assert np.array_equal(kn, kw) and bits_equal(vw[kn], v[kn]) and 0.1 < kn.mean() < 0.9
    # the raycast: rays from in front of the volume reach every window
    p = pose12(rot(0.02, 0.03, 0.0), np.array([0.0, 0.0, 0.2]))
    MV, MN = VO.raycast(vol, G, SMALL_CAM, p, 0.1, 3.0)
    MVw, MNw = VO.raycast(windows, G, SMALL_CAM, p, 0.1, 3.0)
    assert bits_equal(MVw, MV) and bits_equal(MNw, MN)
    hit = ~np.isnan(MV).any(1)
    kz = np.floor((MV[hit, 2] - G.o[2]) / G.s).astype(int)
    assert all(((kz >= k0) & (kz < k1)).sum() > 50 for k0, k1 in WINDOWS), np.bincount(kz)
    # the mesh: windows joined with their id offsets
    for wmin in (0.5, 1.0):
        Vf, Nf, Tf = MO.mesh(vol, G, wmin)
        got, id0 = [], 0
        for k0, slab in windows:
            got.append(MO.mesh(slab, G, wmin, k0, id0))
            id0 += len(got[-1][0])
        assert all(len(g[0]) > 100 for g in got)
        assert bits_equal(np.concatenate([g[0] for g in got]), Vf) and bits_equal(np.concatenate([g[1] for g in got]), Nf)
        assert np.array_equal(np.concatenate([g[2] for g in got]), Tf)


def test_large_windows_are_separated_and_straddle_the_byte_offsets():
    G, _ = E.large_geometry()
    assert np.prod(G.dim) > 2 ** 29
    slab_bytes = 8 * G.dim[0] * G.dim[1]
    starts = sorted(k0 for k0, _ in E.LARGE_WINDOWS)
    for off in (2 ** 31, 2 ** 32):
        assert any(k0 * slab_bytes < off < k1 * slab_bytes for k0, k1 in E.LARGE_WINDOWS), off
    assert E.LARGE_WINDOWS[-1][1] == G.dim[2]
    assert all(b[0] - a[1] >= 1 for a, b in zip(E.LARGE_WINDOWS, E.LARGE_WINDOWS[1:])) and starts[0] > 0
    w = E.large_window(G, 250, 262, 0)
    ts = w[..., 0]
    assert (ts[0] > 0).all() and (ts[-1] < 0).all()                  # the surface lies inside the window


# ---------------------------------------------------------------------------------------------------------------- integrate ties
def test_integrate_ties_occur_and_give_the_hand_values():
    G, desc, depth = E.integrate_ties()
    V = FO.frame_maps(depth, E.TIE_CAM, 1.0, *E.TIE_RANGE)[0]
    assert not np.isnan(V[:, 2]).any()
    out = VO.integrate(G.empty(), G, V, E.TIE_CAM, E.IDENTITY)
    for name, ((i, j, k), want) in E.INTEGRATE_TIES.items():
        got = tuple(float(x) for x in out[k, j, i])
        assert got == ((0.0, 0.0) if want is None else want), (name, got)
    u, v = E.pixel_coord(G, 0, 3, 6)
    assert u == f32(-0.5)
    assert E.pixel_coord(G, 8, 3, 6)[0] == f32(7.5) and E.pixel_coord(G, 4, 0, 6)[1] == f32(-0.5)
    assert E.pixel_coord(G, 4, 8, 6)[1] == f32(7.5) and E.pixel_coord(G, 4, 3, 3)[1] == f32(-0.5)
    counts = E.tie_counts(G, out)
    assert all(c > 0 for c in counts.values()), counts
    # the sdf == 0 voxels hold tsdf +0 (f = +0 / tr)
    z = E.centre(G, 4, 2, 6)[2]
    assert z == 1.0 and E.bits(out[6, 2, 4, 0]) == 0


def test_integrate_ties_with_max_weight_one_and_twice():
    G, desc, depth = E.integrate_ties(max_weight=1)
    V = FO.frame_maps(depth, E.TIE_CAM, 1.0, *E.TIE_RANGE)[0]
    once = VO.integrate(G.empty(), G, V, E.TIE_CAM, E.IDENTITY)
    twice = VO.integrate(once, G, V, E.TIE_CAM, E.IDENTITY)
    up = once[..., 1] > 0
    assert np.all(twice[..., 1][up] == 1)
    # (t * 1 + f) / 2 with t = f: f again where f is exact in halves
    assert bits_equal(twice[..., 0][up], once[..., 0][up])


# ---------------------------------------------------------------------------------------------------------------- raycast ties
@pytest.mark.parametrize("name", sorted(E.raycast_ties()))
def test_raycast_ties_give_the_hand_values(name):
    G, vol, desc, cam, dmin, dmax, (zw, nw) = E.raycast_ties()[name]
    MV, MN = VO.raycast(vol, G, cam, E.IDENTITY, dmin, dmax)
    px = E.INF_PIXEL if name == "inf_makes_z_nan" else E.CENTRE_PIXEL
    if zw is None:
        assert np.isnan(MV[px]).all() and np.isnan(MN[px]).all(), (name, MV[px])
    else:
        assert tuple(MV[px]) == (0.0, 0.0, zw), (name, MV[px])
        if nw == "nan":
            assert np.isnan(MN[px]).all(), (name, MN[px])
        elif nw is not None:
            assert tuple(MN[px]) == nw, (name, MN[px])
    if name in ("f_next_plus_zero", "f_next_minus_zero"):
        F, kn = VO.field(vol, G, np.array([[0.0, 0.0, E.z_k(2)]], f32))
        assert kn[0] and E.bits(F[0]) == (0 if name == "f_next_plus_zero" else 0x80000000)
        assert (~np.isnan(MV).any(1)).sum() > 1
    if name == "first_sample_inside":
        F, kn = VO.field(vol, G, np.array([[0.0, 0.0, E.z_k(0)]], f32))
        assert kn[0] and F[0] <= 0
    if name == "one_sample":
        assert E.RAY_DMIN + E.S >= dmax > dmin
        MV2, _ = VO.raycast(vol, G, cam, E.IDENTITY, dmin, dmin + 0.3)    # a second sample: the hit appears
        assert not np.isnan(MV2[px]).any() and np.isnan(MV).all()
    if name == "last_cell_hit":
        i0 = np.floor(f32(E.z_k(4)) / G.s - f32(0.5))
        assert i0 == G.dim[2] - 2
    if name == "beyond_last_cell":
        assert np.isnan(MV).all()
    if name == "dim2_x":
        assert G.dim[0] == 2
    if name == "inf_makes_z_nan":
        ray = FO._to_world(*FO._pose_f(E.IDENTITY), np.array([[2 * z, 0.0, z] for z in (0.75, 1.0)], f32))
        F, kn = VO.field(vol, G, ray)
        assert kn.all() and F[0] == np.inf and F[1] == 0, F
        Gc, clean, _ = E._inf_nan_hit(with_inf=False)
        MVc, _ = VO.raycast(clean, Gc, cam, E.IDENTITY, dmin, dmax)
        assert tuple(MVc[px]) == (2.0, 0.0, 1.0)
        assert (~np.isnan(MV).any(1)).sum() > 0                        # other rays still hit


# ---------------------------------------------------------------------------------------------------------------- lane tails
@pytest.mark.parametrize("dims", E.TAIL_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_tail_scenes_update_skip_and_split_pairs(dims):
    G, desc, depth, p = E.tail_scene(dims)
    V = FO.frame_maps(depth, E.TAIL_CAM, 1.0, *E.TAIL_RANGE)[0]
    _, ok = VO.integrate(G.empty(), G, V, E.TAIL_CAM, p, with_mask=True)
    flat = ok.reshape(-1)
    assert flat.any() and not flat.all(), dims
    n = flat.size
    pairs = flat[: n - n % 2].reshape(-1, 2)
    if n > 8:
        assert (pairs[:, 0] != pairs[:, 1]).any(), dims                # a 16-byte pair with one half updated
    assert {n % 4 for n in (np.prod(d) for d in E.TAIL_DIMS)} == {0, 1, 2, 3}
    assert {d[0] for d in E.TAIL_DIMS} >= {2, 3, 5}


def test_awkward_fill_has_every_kind():
    G, _ = MC.geometry((9, 7, 5), 0.1, (0, 0, 0))
    vol = E.awkward(G, 0, 4)
    b = vol.view(np.uint32)
    for x in E.W_BITS:
        assert (b[..., 0] == x).any(), hex(x)
    for x in E.W_BITS[:4]:
        assert (b[..., 1] == x).any(), hex(x)
    w = vol[..., 1]
    assert (w == -1).any() and (w < -1).any() and (w == 0).any() and (w == 4).any() and (w > 4).any() and np.isinf(w).any()


def test_integrate_matches_rule():
    before = np.array([[[[1.0, 2.0], [np.nan, 3.0]]]], f32)
    want = np.array([[[[0.5, 3.0], [np.nan, 3.0]]]], f32)
    ok = np.array([[[True, False]]])
    got = want.copy()
    got.view(np.uint32)[0, 0, 1, 0] = 0x7fc00001                      # a skipped voxel's NaN payload changed
    assert E.integrate_matches(got, before, want, ok) == 1
    got = want.copy()
    got.view(np.uint32)[0, 0, 0, 0] = 0x7fc00000
    want2 = want.copy()
    want2[0, 0, 0, 0] = np.nan
    assert E.integrate_matches(got, before, want2, ok) == 0            # two NaN results compare as NaN
    assert E.integrate_matches(got, before, want, ok) == 1


# ---------------------------------------------------------------------------------------------------------------- mesh counts
@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 4, 3), (7, 2, 6)])
def test_checkerboard_counts(dims):
    G, _ = MC.geometry(dims, 0.1, (0, 0, 0))
    vol = E.checkerboard(dims)
    V, N, T = MO.mesh(vol, G, 1.0)
    nv, nt = E.checkerboard_counts(dims)
    assert len(V) == nv and len(T) == nt
    assert E.checkerboard_counts((1024, 1024, 1024))[0] == 3 * 1023 * 1024 ** 2 == 3218079744


def scan_per(nchunks):
    return -(-nchunks // 1024)


@pytest.mark.parametrize("dims, nchunks, per, last_run", [((256, 256, 64), 1024, 1, 1), ((256, 164, 100), 1025, 2, 1),
                                                          ((251, 251, 67), 1031, 2, 1), ((256, 256, 256), 4096, 4, 4),
                                                          ((228, 140, 268), 2089, 3, 1)])
def test_mesh_chunk_counts(dims, nchunks, per, last_run):
    n = int(np.prod(dims))
    assert -(-n // E.CHUNK) == nchunks and scan_per(nchunks) == per
    assert nchunks - (nchunks - 1) // per * per == last_run              # the chunks in the last busy lane's run


def test_room_at_25mm_has_the_dims_the_mesh_test_uses():
    import volume_cases as VC
    assert VC.room_geometry(0.025)[0] == (228, 140, 268)
