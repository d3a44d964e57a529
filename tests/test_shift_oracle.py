"""CPU: the moving volume as tests/shift_oracle.py states it.  The box mesh with the full box is the mesh; the cubes partition along a
cut, so the triangles of what leaves and of what stays are those of the whole; the mesh after a shift is the staying box's mesh at
the new geometry; follow and the origin do what the header's lines say; the figures of tests/shift_cases.py recomputed; and the
build surface: exported symbols, the header, registers of the new kernel unit."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import mesh_oracle as MO
import shift_cases as SC
import shift_oracle as SO
import unit_gates as UG
import volume_cases as VC
import volume_edge_cases as VE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_volume_shift", "rpe_volume_geometry", "rpe_volume_follow", "rpe_volume_mesh_box"}
DIMS = (23, 17, 19)                  # odd on every axis


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def triangle_bag(P, tri):
    """the multiset of triangles, each three vertex positions compared by their bits"""
    b = np.ascontiguousarray(P[tri].reshape(len(tri), 9)).view(np.uint32).tobytes()
    return Counter(b[36 * n: 36 * (n + 1)] for n in range(len(tri)))


@pytest.fixture(scope="module")
def gyroid():
    G, vol, desc = VE.gyroid(DIMS)
    return G, vol, desc, MO.mesh(vol, G, 1.0)


# ---------------------------------------------------------------------------------------------- the box mesh
def test_the_full_box_is_the_mesh(gyroid):
    G, vol, _, (P, N, tri) = gyroid
    Pb, Nb, Tb, _ = SO.mesh_box(vol, G, 1.0, *SO.full_box(G))
    assert len(tri) > 1000 and same(P, Pb) and np.array_equal(tri, Tb)
    assert np.array_equal(np.isnan(N), np.isnan(Nb)) and same(np.nan_to_num(N), np.nan_to_num(Nb))
    # an empty box gives an empty mesh
    Pe, _, Te, _ = SO.mesh_box(vol, G, 1.0, (3, 3, 3), (3, 9, 9))
    assert len(Pe) == 0 and len(Te) == 0


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_cubes_partition_along_a_cut(gyroid, axis):
    G, vol, _, (P, _, tri) = gyroid
    whole = triangle_bag(P, tri)
    lo0, hi0 = SO.full_box(G)
    for d in (1, 2, 7, G.dim[axis] - 2, G.dim[axis] - 1):
        a_hi, b_lo = list(hi0), list(lo0)
        a_hi[axis], b_lo[axis] = d, d
        Pa, _, Ta, _ = SO.mesh_box(vol, G, 1.0, lo0, a_hi)
        Pb, _, Tb, _ = SO.mesh_box(vol, G, 1.0, b_lo, hi0)
        assert len(Ta) + len(Tb) == len(tri) and triangle_bag(Pa, Ta) + triangle_bag(Pb, Tb) == whole, (axis, d)
        assert d == G.dim[axis] - 1 or (len(Ta) > 0 and len(Tb) > 0)


def test_leaving_boxes_and_the_new_window_partition_the_cubes():
    for dims, d in [((9, 7, 8), (2, 0, 0)), ((9, 7, 8), (-3, 2, 0)), ((9, 7, 8), (1, -1, 4)), ((9, 7, 8), (0, 0, -7)), ((9, 7, 8), (9, 0, 1)),
                    ((5, 5, 5), (0, 0, 0))]:
        count = np.zeros((dims[2] - 1, dims[1] - 1, dims[0] - 1), int)
        for lo, hi in SO.leaving_boxes(dims, d):
            count[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] += 1
        stays = np.ones_like(count)
        for a, sl in ((0, 2), (1, 1), (2, 0)):                  # axis a is array axis sl
            idx = np.arange(dims[a] - 1)
            ok = (idx - d[a] >= 0) & (idx + 1 - d[a] <= dims[a] - 1)                     # both corners have a place in the new window
            stays = stays * np.expand_dims(ok.astype(int), tuple(x for x in range(3) if x != sl))
        assert np.array_equal(count + stays, np.ones_like(count)), (dims, d)


@pytest.mark.parametrize("axis, d", [(0, 5), (1, 4), (2, 7), (0, -6), (2, -1)])
def test_the_mesh_after_a_shift_is_the_staying_box(gyroid, axis, d):
    """triangle count and cube order exactly; positions within 2^-20 M, M the largest |coordinate| of either window's corners: origin
    rounding from double, + t, * s, + o -- each at most half an ulp of a magnitude <= M, on both sides: 4 ulp(M) = 2^-21 M, doubled"""
    G, vol, desc, _ = gyroid
    sh = [0, 0, 0]
    sh[axis] = d
    lo, hi = list(SO.full_box(G)[0]), list(SO.full_box(G)[1])
    if d > 0:
        lo[axis] = d
    else:
        hi[axis] = G.dim[axis] - 1 + d
    Pb, _, Tb, cube_b = SO.mesh_box(vol, G, 1.0, lo, hi)
    moved, _ = SO.shift(vol, None, sh)
    G2 = SO.geometry_after(G.dim, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"], sh)
    Pa, _, Ta, cube_a = SO.mesh_box(moved, G2, 1.0, *SO.full_box(G2))
    stride = (1, G.dim[0], G.dim[0] * G.dim[1])[axis]
    assert len(Ta) == len(Tb) > 500 and np.array_equal(cube_a + d * stride, cube_b)
    corners = [np.abs(np.asarray(g.o, np.float64)) + np.array(G.dim) * float(g.s) for g in (G, G2)]
    M = max(c.max() for c in corners)
    assert np.abs(Pa[Ta].astype(np.float64) - Pb[Tb].astype(np.float64)).max() <= 2.0 ** -20 * M


def test_shift_moves_bits_and_two_shifts_are_not_their_sum():
    rng = np.random.default_rng(1)
    vol = rng.normal(size=(5, 4, 6, 2)).astype(np.float32)
    vol.view(np.uint32)[0, 0, :3, 0] = (0x7fc00001, 0xffc12345, 0x80000000)
    cvol = rng.integers(0, 65536, (5, 4, 6, 4)).astype(np.uint16)
    a, ca = SO.shift(vol, cvol, (1, -2, 3))
    assert np.array_equal(a.view(np.uint32)[:2, 2:, :5], vol.view(np.uint32)[3:, :2, 1:]) and np.array_equal(ca[:2, 2:, :5], cvol[3:, :2, 1:])
    assert not a[2:].any() and not a[:, :2].any() and not a[:, :, 5:].any() and not ca[2:].any()
    assert SO.shift(vol, None, (0, 0, 0))[0] is not vol and same(SO.shift(vol, None, (0, 0, 0))[0], vol)
    for d in ((6, 0, 0), (0, -4, 0), (0, 0, 11)):
        assert not SO.shift(vol, cvol, d)[0].any() and not SO.shift(vol, cvol, d)[1].any()
    there_and_back = SO.shift(SO.shift(vol, None, (2, 0, 0))[0], None, (-2, 0, 0))[0]
    assert same(there_and_back[:, :, 2:], vol[:, :, 2:]) and not there_and_back[:, :, :2].any()


# ---------------------------------------------------------------------------------------------- geometry and follow
def test_origin_is_one_rounding_from_the_exact_value():
    o, s = (-2.36, 0.1, 1.6), 0.04
    tot = np.zeros(3, np.int64)
    for step in ((3, -1, 0), (4, -2, 2), (-7, 3, -2)):
        tot += step
    assert np.array_equal(SO.origin_after(o, s, tot), np.array(o))
    assert SO.origin_after(o, s, (7, -3, 2))[0] == -2.36 + 7.0 * 0.04
    G = SO.geometry_after((8, 8, 8), s, o, 0.12, 8, (1 << 30, 0, -5))
    assert G.o[0] == np.float32(-2.36 + float(1 << 30) * 0.04) and G.o[2] == np.float32(1.6 + -5.0 * 0.04)


def test_follow_moves_only_by_granules():
    I = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    dims, s, o = (64, 32, 16), 0.25, (-8.0, -4.0, 0.0)            # dyadic: every double below is exact; the centre is (0, 0, 2)
    assert np.array_equal(SO.follow(I, 2.0, 4, o, dims, s), (0, 0, 0))
    pose = I.copy()
    pose[9:] = (-1.0, 0.75, 1.0)                                   # the camera centre at (1, -0.75, -1): the target at (1, -0.75, 1)
    assert np.array_equal(SO.follow(pose, 2.0, 4, o, dims, s), (4, 0, -4))       # v = (4, -3, -4): exactly +-granule moves, 3 < 4 does not
    assert np.array_equal(SO.follow(pose, 2.0, 1, o, dims, s), (4, -3, -4))
    pose[9] = -(1.0 - 2.0 ** -40)
    assert np.array_equal(SO.follow(pose, 2.0, 4, o, dims, s), (0, 0, -4))       # just below a granule
    Ry = np.array([0, 0, 1, 0, 1, 0, -1, 0, 0, 0, 0, 0], np.float64)             # R^T e_z = (-1, 0, 0): the camera looks along world -x
    assert np.array_equal(SO.follow(Ry, 2.0, 1, o, dims, s), (-8, 0, -8))        # the target at (-2, 0, 0), the centre at (0, 0, 2)


# ---------------------------------------------------------------------------------------------- the use case
def test_the_use_case_figures(oracle):
    share = SC.oracle_fixed_share()
    assert share < SC.FIXED_HITS_LIMIT and share == pytest.approx(SC.FIXED_HITS, abs=5e-4), share
    est, last_share, P, ntri, nfinal = SC.oracle_loop(oracle)
    errs = [VC.pose_error(e, SC.path_pose(f)) for f, e in enumerate(est)]
    rot_max, pos_max = max(e[0] for e in errs), max(e[1] for e in errs)
    med = float(np.median(SC.surface_distance(P)))
    print(share, rot_max, pos_max, last_share, len(P), ntri, nfinal, med)
    assert rot_max == pytest.approx(SC.ORACLE_ROT, rel=0.03) and pos_max == pytest.approx(SC.ORACLE_POS, rel=0.03), (rot_max, pos_max)
    assert med == pytest.approx(SC.ORACLE_MAP_MEDIAN, rel=0.03), med
    assert last_share > 0.5 and ntri >= nfinal + 1 and ntri > 1.5 * nfinal
    # the window is smaller than what the path sees in total: it moved by more than half its width
    assert 64 * SC.VOXEL < 3.3 + 2 * 0.5


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_shift_entry_points():
    hdr = UG.check_entry_points(SYMS)
    assert "Moving volume" in hdr


def test_shift_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_shift.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_shift")])
