"""CPU: pins the numpy statement of the mesh extraction (tests/mesh_oracle.py) and the generated marching-cubes tables with analytic
cases -- the tables against their rule, a plane, a sphere and a torus (closed, consistently oriented, Euler characteristic 2 and 0, on
the surface), open boundaries at unknown voxels, min_weight, an empty volume -- and checks that the library exports the mesh entry
points, that write_ply round-trips and that the C++ driver compiles."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
import unit_gates as UG
from rgbd_pose_estimation_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_volume_upload", "rpe_volume_mesh", "rpe_volume_mesh_download"}
f32 = np.float32


def test_generated_header_is_the_generators_output():
    with open(MO.GEN.HEADER) as f:
        assert f.read() == MO.GEN.render(), "run scripts/gen_mc_tables.py"


@pytest.mark.parametrize("case", range(256))
def test_table_uses_exactly_the_crossed_edges(case):
    inside = [(case >> n) & 1 for n in range(8)]
    crossed = {e for e, (a, b) in enumerate(MO.GEN.EDGES) if inside[a] != inside[b]}
    tris = MO._TRIS[case]
    assert MO.TRI_COUNT[case] == len(tris) <= MO.MAX_TRIS
    assert {e for t in tris for e in t} == crossed
    assert all(len(set(t)) == 3 for t in tris)
    # every crossed edge is a vertex of one fan, and a loop of n edges gives n - 2 triangles: crossed = triangles + 2 x loops
    loops, odd = divmod(len(crossed) - len(tris), 2)
    assert odd == 0 and (loops == 0) == (not crossed) and 3 * loops <= len(crossed)
    # the complement case has the same crossed edges (the tables are not simply mirrored: ambiguous faces join the inside corners)
    comp = 255 - case
    assert {e for t in MO._TRIS[comp] for e in t} == crossed


def test_table_edges_and_maximum():
    assert MO.MAX_TRIS == int(MO.TRI_COUNT.max()) == 5
    assert MO.TRI_COUNT[0] == MO.TRI_COUNT[255] == 0
    for e, (a, b) in enumerate(MO.GEN.EDGES):
        assert b - a == 1 << MO.GEN.AXIS[e] and MO.GEN.OWNER[e] == a
    # the lone corner cut off: one triangle, its normal away from the corner (to the free side)
    for n in range(8):
        c = MO.GEN.corner(n).astype(float)
        (tri,) = MO._TRIS[1 << n]
        p = [MO.GEN.midpoint(e) for e in tri]
        assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), np.mean(p, 0) - c) > 0


def _check_valid(V, N, Tri):
    assert V.dtype == f32 and N.dtype == f32 and Tri.dtype == np.int32
    assert V.shape == N.shape == (len(V), 3) and Tri.shape == (len(Tri), 3)
    assert np.isfinite(V).all()
    if len(Tri):
        assert Tri.min() >= 0 and Tri.max() < len(V)
        assert np.all((Tri[:, 0] != Tri[:, 1]) & (Tri[:, 1] != Tri[:, 2]) & (Tri[:, 0] != Tri[:, 2]))
    assert np.array_equal(np.unique(Tri.reshape(-1)), np.arange(len(V)))     # every vertex is referenced
    good = ~np.isnan(N).any(1)
    assert np.allclose(np.linalg.norm(N[good].astype(np.float64), axis=1), 1, atol=1e-6)


def test_plane_vertices_lie_on_it_and_faces_point_to_the_free_side():
    G, vol, _ = MC.plane()
    V, N, Tri = MO.mesh(vol, G)
    _check_valid(V, N, Tri)
    assert len(V) > 400 and len(Tri) > 800
    # tsdf linear along every edge: t is exact up to fp32 rounding
    assert np.abs(V.astype(np.float64) @ MC.PLANE_N - MC.PLANE_D).max() < 1e-6
    fn = MC.face_normals(V, Tri)
    assert np.all(fn @ MC.PLANE_N > 0)
    good = ~np.isnan(N).any(1)
    assert good.mean() > 0.6 and np.abs(N[good].astype(np.float64) - MC.PLANE_N).max() < 1e-5
    # the plane's patch is open: its boundary edges are on the volume's faces
    _, cnt, _ = MC.mesh_edges(Tri)
    assert set(cnt) == {1, 2}


# Vertex distance to the true surface.  The oracle: sphere 6.1e-4 m, torus 1.2e-3 m at 5 / 4 cm voxels (linear interpolation of a
# curved field along an edge).  Bound: x1.5.
SURFACE_BOUND = {"sphere": 9e-4, "torus": 1.8e-3}


@pytest.mark.parametrize("name, chi", [("sphere", 2), ("torus", 0)])
def test_closed_surfaces_are_oriented_manifolds(name, chi):
    G, vol, _ = getattr(MC, name)()
    V, N, Tri = MO.mesh(vol, G)
    _check_valid(V, N, Tri)
    und, cnt, directed = MC.mesh_edges(Tri)
    assert np.all(cnt == 2)                                           # closed: every edge in exactly two triangles
    assert len(np.unique(directed, axis=0)) == len(directed)          # each directed edge once: consistent orientation
    assert MC.euler(V, Tri) == chi
    P = V.astype(np.float64)
    if name == "sphere":
        d = np.linalg.norm(P, axis=1) - MC.SPHERE_R
        grad = P / np.linalg.norm(P, axis=1)[:, None]
    else:
        q = np.sqrt(P[:, 0] ** 2 + P[:, 1] ** 2)
        d = np.sqrt((q - MC.TORUS_R) ** 2 + P[:, 2] ** 2) - MC.TORUS_r
        c = np.stack([P[:, 0] * MC.TORUS_R / q, P[:, 1] * MC.TORUS_R / q, 0 * q], 1)
        grad = (P - c) / np.linalg.norm(P - c, axis=1)[:, None]
    assert np.abs(d).max() < SURFACE_BOUND[name], np.abs(d).max()
    # faces and vertex normals point to the free side (outwards)
    fn = MC.face_normals(V, Tri)
    assert np.all(np.einsum("ij,ij->i", fn, grad[Tri].mean(1)) > 0)
    assert not np.isnan(N).any() and np.all(np.einsum("ij,ij->i", N.astype(np.float64), grad) > 0.95)


def test_unknown_voxels_leave_an_open_boundary_and_min_weight_filters():
    G, vol, _ = MC.slab()
    d0, d1, d2 = G.dim
    full = MO.mesh(MC.plane()[1] * np.array([1, 3], f32), G, 1.0)
    V, N, Tri = MO.mesh(vol, G, 1.0)
    _check_valid(V, N, Tri)
    assert 0 < len(Tri) < len(full[2])
    # no triangle of a cube with an unknown corner: the cubes of the hole's box emit nothing
    case = MO.cases(vol, 1.0)
    assert not case[4:14, 3:9, 5:12].any()
    _, cnt, _ = MC.mesh_edges(Tri)
    assert (cnt == 1).sum() > (MC.mesh_edges(full[2])[1] == 1).sum()     # the hole adds boundary edges
    # min_weight 2 drops the patch of weight 1 as well; 3 keeps the rest; above 3 nothing is known
    V2, _, T2 = MO.mesh(vol, G, 2.0)
    assert 0 < len(T2) < len(Tri)
    V3, _, T3 = MO.mesh(vol, G, 3.0)
    assert np.array_equal(V2, V3) and np.array_equal(T2, T3)
    V4, N4, T4 = MO.mesh(vol, G, 3.5)
    assert V4.shape == (0, 3) and T4.shape == (0, 3)


def test_empty_volume_and_tiny_dims():
    G, _ = MC.geometry((8, 9, 7), 0.1, (0, 0, 0))
    V, N, Tri = MO.mesh(G.empty(), G)
    assert V.shape == N.shape == (0, 3) and Tri.shape == (0, 3)
    G, _ = MC.geometry((2, 2, 2), 0.1, (0, 0, 0))
    vol = G.empty()
    vol[..., 1] = 1
    vol[..., 0] = 0.5
    vol[0, 0, 0, 0] = -0.5                    # one cube, corner 0 inside: one triangle
    V, N, Tri = MO.mesh(vol, G)
    assert len(V) == 3 and Tri.tolist() == [[0, 1, 2]] and np.isnan(N).all()   # every normal sample is outside the 2^3 field


def test_noise_volume_is_valid_at_every_min_weight():
    G, vol, _ = MC.noise()
    sizes = []
    for w in (0.5, 1.0, 2.0):
        V, N, Tri = MO.mesh(vol, G, w)
        _check_valid(V, N, Tri)
        sizes.append(len(Tri))
    assert sizes[0] > sizes[1] > sizes[2] > 0


def test_noise_volume_has_the_awkward_values():
    """the noise case really holds what the parity test claims to cover"""
    G, vol, _ = MC.noise()
    t, w = vol[..., 0], vol[..., 1]
    assert (t == 0).sum() > 100 and np.isnan(t).sum() > 100 and np.isinf(t).sum() > 50 and (w < 0).sum() > 50
    case = MO.cases(vol, 1.0)
    # ambiguous faces: a z = 0 face with its two inside corners on a diagonal
    amb = ((case & 0b1111) == 0b1001) | ((case & 0b1111) == 0b0110)
    assert amb.sum() > 20
    Vo, No, To = MO.mesh(vol, G, 1.0)
    assert len(To) > 1000 and (~np.isnan(No).any(1)).sum() > 50


def test_write_ply_round_trips(tmp_path):
    G, vol, _ = MC.torus()
    V, N, Tri = MO.mesh(vol, G)
    p = str(tmp_path / "torus.ply")
    M.write_ply(p, V, Tri, N)
    V2, T2, N2 = M.read_ply(p)
    assert np.array_equal(V, V2) and np.array_equal(Tri, T2) and np.array_equal(N, N2)
    with open(p, "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 2390\n")
    q = str(tmp_path / "bare.ply")
    M.write_ply(q, V, Tri)
    V3, T3, N3 = M.read_ply(q)
    assert np.array_equal(V, V3) and np.array_equal(Tri, T3) and N3 is None
    assert os.path.getsize(q) == len(open(q, "rb").read().split(b"end_header\n")[0]) + 11 + 12 * len(V) + 13 * len(Tri)


def test_header_and_library_export_the_mesh_entry_points():
    UG.check_entry_points(SYMS)


def test_mesh_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_mesh.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_mesh")])
