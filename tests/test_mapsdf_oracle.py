"""CPU: the map volume term as tests/mapsdf_oracle.py states it.  The window's extent gives the window term's own rows; the frames of
tests/mapsdf_cases.py reach every path of the corner fetch; the figures of the use case recomputed; and the build surface: the four
entry points, the header's block, the resources of the two kernels, the round kernel's late arguments, the C++ driver."""
import os
import re
import subprocess

import numpy as np
import pytest

import isa_tools as T
import mapmesh_cases as MC
import mapmesh_oracle as MM
import mapsdf_cases as C
import sdf_oracle as SO
import unit_gates as UG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_map_sdf_rows", "rpe_map_sdf_normal_eq", "rpe_icp_map_sdf", "rpe_icp_pyramid_map_sdf"}


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------- the composition
def test_the_windows_extent_gives_the_window_terms_rows():
    """box = the window's extent: the virtual volume is the window and its origin the window's own, so the rows are sdf_oracle.rows on
    the window itself, bit for bit; over the sphere's box the same frames have more rows"""
    m = C.sphere_map()
    G = MM.SO.geometry_after(m.dims, m.kw["voxel_size"], m.kw["origin"], m.kw["trunc"], m.kw["max_weight"], m.total)
    rows = more = 0
    for name, pose, depth in C.sphere_frames(m, C.CAM_A):
        for _, V, N, _ in C.level_pyramid(depth, C.CAM_A):
            for use_normals in (True, False):
                r, J, ok = C.oracle_rows(m, m.extent(), V, N, pose, 0.1, C.COS_THR, use_normals)
                rw, Jw, okw = SO.rows(m.window, G, V, N, pose, 0.1, C.COS_THR, use_normals)
                assert same(r, rw) and same(J, Jw), name
                rows += int(ok.sum())
                more += int(C.oracle_rows(m, C.SPHERE_BOX, V, N, pose, 0.1, C.COS_THR, use_normals)[2].sum())
    print("rows in the window", rows, "in the map", more)
    assert rows > 300 and more > 2 * rows


def test_the_sphere_frames_see_window_held_and_absent_bricks():
    m = C.sphere_map()
    assert tuple(m.total) == (0, 0, -16) and len(m.store) == 32 and all(np.array_equal(a, b) for a, b in zip(m.bounds(), C.SPHERE_BOX))
    for cam in C.CAMS.values():
        seen = np.zeros(len(C.CLASSES), np.int64)
        for name, pose, depth in C.sphere_frames(m, cam):
            V = C.level_pyramid(depth, cam)[0][1]
            seen += C.classes(m, C.SPHERE_BOX, V, pose).sum(0)
        print(cam[4], "x", cam[5], dict(zip(C.CLASSES, seen)))
        need = ("window", "last z", "window/held face", "held/held face", "edge", "corner", "absent, a corner held")
        assert all(seen[C.CLASSES.index(k)] > 0 for k in need), seen


def test_the_random_frames_reach_every_class_of_cell():
    """the condition on the random case, from the oracle alone: every view's frame has a pixel in each class (class_depth chose the
    depths so), and the content has what the gates are for"""
    m = C.random_map()
    lo, hi = m.bounds()
    assert tuple(m.total) == (8, 8, 0) and (hi - lo <= 40).all()
    vol, _ = m.dense()
    t, w = vol[..., 0], vol[..., 1]
    assert (np.abs(t) >= 1).sum() > 20 and np.isnan(t).sum() > 10 and np.isinf(t).sum() > 5
    assert (w < 0).sum() > 10 and np.isnan(w).sum() > 10 and np.isinf(w).sum() > 10 and (w == 0).sum() > 1000
    for box in (m.bounds(), (lo - 8, hi + 8)):
        for pose in C.random_views(m, box):
            V = C.level_pyramid(C.class_depth(m, box, C.CAM_A, pose), C.CAM_A)[0][1]
            seen = C.classes(m, box, V, pose).sum(0)
            print(dict(zip(C.CLASSES, seen)))
            assert (seen > 0).all(), dict(zip(C.CLASSES, seen))


# ---------------------------------------------------------------------------------------------- the use case
def test_the_use_case_figures(oracle):
    u = C.oracle_walk(oracle)
    for n, (w, mp, ew, em) in enumerate(zip(u["window"], u["map"], u["window_err"], u["map_err"])):
        print("position", n, "rows: window", w, "map", mp, "ends (rad, m) from the truth: window", ew[:2], "map", em[:2])
    print("totals: window", sum(u["window"]), "map", sum(u["map"]))
    assert u["window"] == C.ROWS_WINDOW and u["map"] == C.ROWS_MAP and u["held"] == MC.HELD
    assert tuple(int(x) for x in u["box"][0]) == MC.BOX[0] and tuple(int(x) for x in u["box"][1]) == MC.BOX[1]
    # the condition on the case: over the return leg the map term has more rows than the window term (here at every position)
    assert sum(u["map"]) > sum(u["window"]) and all(a > b for a, b in zip(u["map"], u["window"]))
    assert (sum(u["window"]), sum(u["map"])) == (104770, 131712)
    for e in u["window_err"] + u["map_err"]:
        assert e[0] <= C.ERR_LIMIT[0] and e[1] <= C.ERR_LIMIT[1], e
    assert max(e[0] for e in u["window_err"]) == pytest.approx(3.1e-3, rel=0.02) and max(e[1] for e in u["map_err"]) == pytest.approx(7.7e-3, rel=0.02)


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert hdr.index("---- Map volume term:") > hdr.index("---- Map raycast:") > hdr.index("---- Volume term:")
    block = hdr[hdr.index("---- Map volume term:"):hdr.index("int rpe_map_sdf_rows(")]
    for what in ("VIRTUAL VOLUME", "bit for bit", "ONCE per call", "not weighted by voxel weight", "rebuilt and uploaded on every call"):
        assert what in block, what
    src = open(os.path.join(UG.CSRC, "rpe_frontend.hip")).read()
    assert "RPE_PRELOAD(map_sdf_rows_kernel)" in src and "RPE_PRELOAD(icp_map_sdf_kernel<256>)" in src


def kernels():
    UG.built()
    rows = {}
    for r in T.kernel_resources(UG.obj("rpe_frontend.hip")):
        rows.setdefault(r["base"], []).append(r)
    return rows


def test_both_kernels_meet_the_gate():
    """at most 128 registers, no vector spills, no scalar spills, no scratch, and no more LDS than icp_sdf_kernel of the same workgroup"""
    rows = kernels()
    assert len(rows.get("map_sdf_rows_kernel", [])) == 1 and len(rows.get("icp_map_sdf_kernel", [])) == 2, sorted(rows)
    blk = lambda r: int(re.search(r"ILi(\d+)E", r["mangled"]).group(1))   # noqa: E731
    lds = {blk(r): r["lds"] for r in rows["icp_sdf_kernel"]}
    for r in rows["map_sdf_rows_kernel"] + rows["icp_map_sdf_kernel"]:
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] + r["agpr"] <= 128, r
        assert r["lds"] <= (lds[blk(r)] if r["base"] == "icp_map_sdf_kernel" else min(lds.values())), (r, lds)
    assert rows["map_sdf_rows_kernel"][0]["lds"] == 0


def test_the_round_kernel_finds_its_late_arguments_in_the_kernarg_segment(tmp_path):
    """icp_map_sdf_kernel reads the pose (late_pose, inside the loop) and the reduction's argument (late_finish_at, behind it) from the
    kernarg segment at the offsets of a struct that mirrors the argument list: the metadata must hold both exactly there"""
    UG.built()
    co = T.code_object(UG.obj("rpe_frontend.hip"), str(tmp_path))
    notes = subprocess.check_output([T.READELF, "--notes", co]).decode()
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S*icp_map_sdf_kernel\S*)\n", notes):
        if m.group(1).endswith(".kd"):
            continue
        args = notes[notes.rfind(".args:", 0, m.start()):m.start()]
        layout = [(int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)", args)]
        assert layout[:8] == [(0, 8), (8, 8), (16, 8), (24, 64), (88, 36), (124, 16), (140, 48), (192, 136)], (m.group(1), layout[:9])
        seen += 1
    assert seen == 2, seen
    src = open(os.path.join(UG.CSRC, "rpe_frontend.hip")).read()
    assert "offsetof(MapSdfRoundArgs, fin) == 192 && sizeof(Finish) == 136" in src
    assert "offsetof(MapSdfRoundArgs, T) == 140 && sizeof(PoseF) == 48" in src


def test_volume_map_sdf_track_cpp_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_sdf_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_map_sdf_track")])
