"""CPU: the map raycast as tests/mapray_oracle.py states it.  The window's extent gives the window's own raycast; a box that only adds
absent bricks around the map changes no hit; the figures of the use case of tests/mapray_cases.py recomputed; and the build surface:
the exported symbol and the header, the resources of the two kernels, the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import archive_cases as AC
import isa_tools as T
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapray_cases as RC
import mapray_oracle as MR
import unit_gates as UG
import volume_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_volume_map_raycast"}


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def sphere_map():
    return MC.Map(None, (16, 16, 16)).fill(MC.sphere(*MC.SPHERE), MC.OCTANTS)


# ---------------------------------------------------------------------------------------------- the composition
def test_the_windows_extent_is_the_windows_own_raycast(sphere_map):
    m = sphere_map
    _, cam, pose, _ = RC.sphere_views(m)[1]
    MV, MN, C = RC.oracle(m, cam, pose, *RC.SPHERE_RAY, box=m.extent())
    G = MM.SO.geometry_after(m.dims, m.kw["voxel_size"], m.kw["origin"], m.kw["trunc"], m.kw["max_weight"], m.total)
    WV, WN = VO.raycast(m.window, G, cam, pose, *RC.SPHERE_RAY)
    assert same(MV, WV) and same(MN, WN) and (~np.isnan(WV).any(1)).sum() > 100
    assert np.array_equal(C, MR.CO.sample(m.cwindow, G, WV)) and (C[:, 3] == 255).any()
    # the whole map from the same pose shows more (another fp32 origin: counts, not bits)
    AV, _, _ = RC.oracle(m, cam, pose, *RC.SPHERE_RAY)
    assert (~np.isnan(AV).any(1)).sum() > (~np.isnan(WV).any(1)).sum()


def test_absent_bricks_around_the_map_change_no_hit(sphere_map):
    """a box one brick larger on the low side of every axis moves the fp32 origin; one larger on the high side only adds weight-0 voxels"""
    m = sphere_map
    _, cam, pose, _ = RC.sphere_views(m)[0]
    lo, hi = m.bounds()
    a = RC.oracle(m, cam, pose, *RC.SPHERE_RAY)
    b = RC.oracle(m, cam, pose, *RC.SPHERE_RAY, box=(lo, hi + 8))
    assert all(same(x, y) if x.dtype != np.uint8 else np.array_equal(x, y) for x, y in zip(a, b)) and (~np.isnan(a[0]).any(1)).sum() >= 300


# ---------------------------------------------------------------------------------------------- the use case
def test_the_use_case_figures():
    u = RC.oracle_walk()
    print(u)
    assert u["window"] == AC.HITS_ARCHIVE and u["map"] == RC.HITS_MAP and u["held"] == MC.HELD
    assert tuple(int(x) for x in u["box"][0]) == MC.BOX[0] and tuple(int(x) for x in u["box"][1]) == MC.BOX[1]
    # the conditions on the case: every window hit is a map hit; the map shows at least GAIN_LIMIT x the window at every position
    assert u["subset"] and all(h >= RC.GAIN_LIMIT * w for h, w in zip(u["map"], u["window"]))
    assert min(h / w for h, w in zip(u["map"], u["window"])) == pytest.approx(1.179, abs=1e-3)
    assert sum(u["window"]) / (12 * AC.PIXELS) == pytest.approx(0.61, abs=5e-3) and sum(u["map"]) / (12 * AC.PIXELS) == pytest.approx(0.81, abs=5e-3)


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_map_raycast_entry_point():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert hdr.index("Map raycast: the window and the archived bricks") > hdr.index("Map mesh: the window and the archived bricks")
    assert "RPE_MAPRAY_COLOR = 1, RPE_MAPRAY_NO_SKIP = 2" in hdr and "raycasting or tracking against the archive" not in hdr
    from rgbd_pose_estimation_amd import _lib as L
    assert (L.RPE_MAPRAY_COLOR, L.RPE_MAPRAY_NO_SKIP) == (1, 2)


def test_the_two_kernels_are_lean():
    """the gate the kernels would have in a unit of their own (rpe_mapmesh.hip and rpe_archive.hip are the precedents): no spills, no
    scratch, no LDS; a ray with its eight corners in at most 128 registers, the occupancy wave in at most 64"""
    UG.built()
    rows = {}
    for r in T.kernel_resources(UG.obj("rpe_frontend.hip")):
        rows.setdefault(r["base"], []).append(r)
    for base, regs in (("map_raycast_kernel", 128), ("map_occupancy_kernel", 64)):
        assert len(rows.get(base, [])) >= 1, (base, sorted(rows))
        for r in rows[base]:
            assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, r
            assert r["vgpr"] + r["agpr"] <= regs, r
    assert not any("filter" in b for b in rows)


def test_map_raycast_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_raycast.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_map_raycast")])
