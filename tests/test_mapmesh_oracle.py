"""CPU: the map mesh as tests/mapmesh_oracle.py states it.  The permutation into brick order is a bijection that keeps every triangle;
the window's extent gives the window's own mesh; a map meshed as two boxes loses exactly the cubes across the cut; the bounds with
negative world bricks; the figures of the use case of tests/mapmesh_cases.py recomputed; and the build surface: exported symbols, the
header, the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import mapmesh_cases as MC
import mapmesh_oracle as MM
import mesh_oracle as MO
import shift_cases as SC
import unit_gates as UG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_volume_map_bounds", "rpe_volume_map_mesh"}


@pytest.fixture(scope="module")
def sphere_map():
    return MC.Map(None, (16, 16, 16)).fill(MC.sphere(*MC.SPHERE), MC.OCTANTS)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------- the order
def test_the_permutation_is_a_bijection_that_keeps_every_triangle(sphere_map):
    m = sphere_map
    box = m.bounds()
    vol, cvol = m.dense(box)
    V, N, Tr = MO.mesh(vol, MM.geometry(m.kw, box), 1.0)
    pv, pt = MM.permutation(vol, 1.0)
    assert sorted(pv) == list(range(len(V))) and sorted(pt) == list(range(len(Tr))) and len(Tr) > 2000
    Vm, Nm, Tm, _ = MM.permute(vol, 1.0, V, N, Tr)
    # triangle m of the map mesh is triangle pt[m] of the dense one: the same three positions in the same rotation
    assert same(Vm[Tm.reshape(-1)], V[Tr[pt].reshape(-1)]) and same(Nm[Tm.reshape(-1)], N[Tr[pt].reshape(-1)])
    # brick order: the owner voxels' bricks ascend, inside a brick the voxels ascend in (z, y, x), then the axis
    vox, axis, cube, r = MM.owners(vol, 1.0)
    rk = MM.rank((32, 32, 32))
    key = rk[vox[pv]] * 3 + axis[pv]
    assert (np.diff(key) > 0).all() and (np.diff(rk[cube[pt]] * 8 + r[pt]) > 0).all()
    assert rk[0] == 0 and rk[7] == 7 and rk[8] == 512 and rk[32] == 8 and rk[32 * 32] == 64 and rk[8 * 32] == 4 * 512
    assert not np.array_equal(pv, np.arange(len(pv)))


def test_the_windows_extent_with_an_empty_store_is_the_windows_mesh(sphere_map):
    m = MC.Map(None, (24, 16, 8)).fill(MC.sphere((11.6, 8.3, 3.7), 5.4), [])
    V, N, Tr, C = m.mesh(m.extent())
    Vd, Nd, Td = MO.mesh(m.window, MM.geometry(m.kw, m.extent()), 1.0)
    assert len(Td) > 300 and m.store == {} and same(MC.triangle_words(V, N, Tr), MC.triangle_words(Vd, Nd, Td))
    assert C.shape == (len(V), 4) and (C[:, 3] == 255).any()
    # and in a moved window: the origin is the shifted one, rounded once
    w = sphere_map
    V, N, Tr, _ = w.mesh(w.extent())
    Vd, Nd, Td = MO.mesh(w.window, MM.SO.geometry_after(w.dims, w.kw["voxel_size"], w.kw["origin"], w.kw["trunc"], w.kw["max_weight"], w.total), 1.0)
    assert len(Td) > 300 and same(MC.triangle_words(V, N, Tr), MC.triangle_words(Vd, Nd, Td))


def test_two_boxes_lose_exactly_the_cubes_across_the_cut(sphere_map):
    m = sphere_map
    lo, hi = m.bounds()
    cut = 0                                                          # a brick plane: world x = 0, box index 16
    whole = m.mesh((lo, hi))
    left, right = m.mesh((lo, np.array([cut, hi[1], hi[2]]))), m.mesh((np.array([cut, lo[1], lo[2]]), hi))
    cube = MC.cube_ijk(m.dense()[0])
    across = cube[:, 0] == cut - 1 - lo[0]                           # cubes whose far corners lie beyond the cut
    assert across.sum() > 100 and len(left[2]) + len(right[2]) == len(whole[2]) - across.sum()
    # positions only: the right half has another fp32 origin, so it is compared through the cubes it keeps, by count, and the left
    # half, which shares the whole box's origin, word for word
    vol = m.dense()[0]
    _, pt = MM.permutation(vol, 1.0)
    keep_left = (cube[pt][:, 0] < cut - 1 - lo[0])
    Pw = np.ascontiguousarray(whole[0][whole[2].reshape(-1)]).view(np.uint32).reshape(-1, 9)
    Pl = np.ascontiguousarray(left[0][left[2].reshape(-1)]).view(np.uint32).reshape(-1, 9)
    assert np.array_equal(Pw[keep_left], Pl) and len(right[2]) == (cube[:, 0] >= cut - lo[0]).sum()   # none doubled, none lost


def test_bounds_with_negative_world_bricks():
    lo, hi = MM.bounds((8, -16, 0), (16, 16, 8), {(-3, 0, 1): None, (4, -5, -1): None})
    assert lo.dtype == np.int64 and list(lo) == [-24, -40, -8] and list(hi) == [40, 8, 16]
    lo, hi = MM.bounds((-64, 0, 8), (8, 8, 8), {})
    assert list(lo) == [-64, 0, 8] and list(hi) == [-56, 8, 16]
    m = MC.Map(None, (16, 16, 16)).fill(MC.sphere(*MC.SPHERE), MC.OCTANTS[:2])
    assert min(k[0] for k in m.store) == -2 and list(m.bounds()[0]) == [-16, -16, 0]
    # a held brick at a negative coordinate lands where floor division puts it in the dense volume
    vol, _ = m.dense()
    key = next(k for k in m.store if k[0] < 0 and m.store[k][0].any())
    at = [8 * key[a] - int(m.bounds()[0][a]) for a in range(3)]
    assert same(vol[at[2]:at[2] + 8, at[1]:at[1] + 8, at[0]:at[0] + 8], m.store[key][0])


# ---------------------------------------------------------------------------------------------- the use case
@pytest.fixture(scope="module")
def use_case():
    return MC.oracle_use_case()


def test_the_use_case_figures(use_case):
    u = use_case
    fm, fw = u["figures_map"], u["figures_window"]
    print(fm, fw, u["held"], u["box"])
    assert u["digest"] == MC.AC.DIGEST_ARCHIVE and u["total"] == (0, 0, 0) and u["held"] == MC.HELD == MC.AC.PEAK_HELD
    assert tuple(int(x) for x in u["box"][0]) == MC.BOX[0] and tuple(int(x) for x in u["box"][1]) == MC.BOX[1]
    assert fm["triangles"] == MC.TRIANGLES_MAP and fw["triangles"] == MC.TRIANGLES_WINDOW
    assert fm["share"] == pytest.approx(MC.SHARE_MAP, abs=1e-4) and fw["share"] == pytest.approx(MC.SHARE_WINDOW, abs=1e-4)
    assert fm["median"] == pytest.approx(MC.MEDIAN_MAP, abs=1e-5) and fw["median"] == pytest.approx(MC.MEDIAN_WINDOW, abs=1e-5)


def test_the_condition_on_the_case(use_case):
    """the map mesh contains every triangle of the window mesh whose cube does not touch the window's last layer"""
    u = use_case
    inner = MC.window_triangles_away_from_the_last_layer(u["window_bits"], u["window"][0], u["window"][2])
    whole = MC.triangle_words(u["map"][0], None, u["map"][2], normals=False)
    assert len(inner) > 10000 and MC.contains(whole, inner)


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_map_mesh_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert hdr.index("Map mesh: the window and the archived bricks") > hdr.index("Volume archive: what leaves")
    assert "meshing or raycasting the archive directly" not in hdr and "raycasting the archive directly" in hdr


def test_map_mesh_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_mesh.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_map_mesh")])
