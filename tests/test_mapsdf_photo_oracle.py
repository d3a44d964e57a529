"""CPU: the map volume colour term as tests/mapsdf_photo_oracle.py states it -- a composition, so what is checked is the composition: with
the window's extent for a box it IS the volume colour term on the window, bit for bit; the cases of tests/mapsdf_photo_cases.py meet
their conditions (every class of cell reached by a pixel whose TSDF corners let a row through, both kinds of held brick seen, the wall
walk's figures); and the build surface: the four entry points, the resources and kernarg layout of the new kernels, the C++ example."""
import os
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import mapmesh_oracle as MM
import mapsdf_cases as MSC
import mapsdf_photo_cases as C
import mapsdf_photo_oracle as MP
import sdf_photo_oracle as SP
import unit_gates as UG
from test_sdf_photo_oracle import frontend_kernels, kernarg_layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_map_sdf_photo_rows", "rpe_map_sdf_photo_normal_eq", "rpe_icp_map_sdf_rgbd", "rpe_icp_pyramid_map_sdf_rgbd"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the composition
@pytest.mark.parametrize("archive", (True, False), ids=("archive on", "archive off"))
def test_the_windows_extent_is_the_window_term_bit_for_bit(archive):
    m = C.scene_map(None, archive)
    assert bool(m.store) == archive
    G = MM.geometry(m.kw, m.extent())
    rows = 0
    for n, cam in enumerate(C.CAMS.values()):
        lv, _, _ = C.frame_levels(cam, MSC.scene_depth(cam), C.frame_rgba(cam, n))
        for pose in (MSC.scene_pose(), MSC.scene_start()):
            for l, (V, N, If) in enumerate(lv):
                a = C.oracle_rows(m, m.extent(), V, If, pose, 0.1)
                b = SP.rows(m.window, m.cwindow, G, V, If, pose, 0.1)
                assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
                rows += int(a[2].sum())
                if not archive:                                            # the map is the window: its bounds are the extent
                    c = C.oracle_rows(m, None, V, If, pose, 0.1)
                    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(bits(a[1]), bits(c[1]))
    assert rows > 200                                                      # (one voxel in 13 has no colour: half the cells have a row)


def test_the_maps_have_colour_where_mapsdf_cases_have_none():
    for mine, theirs in ((C.sphere_map(), MSC.sphere_map()), (C.scene_map(), MSC.scene_map()), (C.far_map(), MSC.far_map())):
        assert np.array_equal(bits(mine.window), bits(theirs.window)) and mine.total == theirs.total and set(mine.store) == set(theirs.store)
        assert theirs.cwindow is None and mine.cwindow is not None and mine.colour_plane
        assert all(np.asarray(c).any() for _, c in mine.store.values())
        vol, cvol = mine.dense()
        assert (CO.f32(cvol[..., 3]) > 0).mean() > 0.3


# ---------------------------------------------------------------------------------------------- the cases' conditions
def test_random_colour_content_and_every_class_with_a_row():
    m = C.random_map()
    assert np.array_equal(bits(m.window), bits(MSC.random_map().window))        # the TSDF half is mapsdf_cases'
    lo, hi = m.bounds()
    assert (hi - lo <= 40).all()
    vol, cvol = m.dense()
    w, ch = CO.f32(cvol[..., 3]), CO.f32(cvol[..., :3])
    assert (w == 0).sum() > 100 and (w < 0).sum() > 20 and np.isnan(w).sum() > 20 and np.isinf(w).sum() > 20
    assert (~np.isfinite(ch) & (w > 0)[..., None]).sum() > 50               # NaN / Inf channels under a weight > 0
    rows = not_finite = 0
    with_row = np.zeros(len(C.CLASSES), np.int64)
    for box in (None, (lo - 8, hi + 8)):
        b = m.bounds() if box is None else box
        for n, pose in enumerate(MSC.random_views(m, b)):
            depth = C.class_depth(m, b, C.CAM_A, pose, MSC.RANDOM_GATE)
            lv, _, _ = C.frame_levels(C.CAM_A, depth, C.frame_rgba(C.CAM_A, n))
            V, N, If = lv[0]
            seen = dict(zip(C.CLASSES, MSC.classes(m, b, V, pose).sum(0)))
            assert all(seen[k] > 0 for k in C.CLASSES), seen
            with_row += C.rows_per_class(m, b, V, pose, MSC.RANDOM_GATE)
            r, J, ok = C.oracle_rows(m, b, V, If, pose, MSC.RANDOM_GATE)
            assert not (ok & ~C.tsdf_stands(m, b, V, pose, MSC.RANDOM_GATE)).any()
            rows += int(ok.sum())
            not_finite += int((ok & ~np.isfinite(r)).sum())
    with_row = dict(zip(C.CLASSES, with_row))
    print("rows", rows, "not finite", not_finite, "pixels whose TSDF corners let a row through, per class", with_row)
    assert {k for k in C.CLASSES if with_row[k] > 0} == set(C.RANDOM_ROW_CLASSES), with_row
    assert rows > 40 and not_finite > 5
    # ... and the sphere's frames reach the rest
    m = C.sphere_map()
    with_row = np.zeros(len(C.CLASSES), np.int64)
    for box in (m.bounds(), MSC.GROWN_BOX):
        for name, pose, depth in C.sphere_class_frames(m, box, C.CAM_A):
            with_row += C.rows_per_class(m, box, C.frame_levels(C.CAM_A, depth, C.frame_rgba(C.CAM_A))[0][0][0], pose, 0.1)
    with_row = dict(zip(C.CLASSES, with_row))
    print("the sphere", with_row)
    assert {k for k in C.CLASSES if with_row[k] > 0} == set(C.SPHERE_ROW_CLASSES), with_row
    assert set(C.RANDOM_ROW_CLASSES) | set(C.SPHERE_ROW_CLASSES) == set(C.ROW_CLASSES)


def test_the_two_stage_map_holds_bricks_with_and_without_a_colour_plane():
    m = C.two_stage_map()
    planes = [bool(np.asarray(c).any()) for _, c in m.store.values()]
    assert len(planes) == 32 and sum(planes) == 16 and m.cwindow is not None and m.colour_plane
    plane = bare = rows_plane = tsdf_bare = 0
    for name, pose, depth in C.two_stage_frames(m, C.CAM_A):
        lv, _, _ = C.frame_levels(C.CAM_A, depth, C.frame_rgba(C.CAM_A))
        V, N, If = lv[0]
        p, b = C.held_kinds(m, m.bounds(), V, pose)
        r, J, ok = C.oracle_rows(m, m.bounds(), V, If, pose, 0.1)
        stands = C.tsdf_stands(m, m.bounds(), V, pose, 0.1)
        plane, bare = plane + int(p.sum()), bare + int(b.sum())
        rows_plane += int((ok & p).sum())
        tsdf_bare += int((stands & b).sum())
        assert not (ok & b).any()                                          # corner 0 has no colour there: no photometric row
    print("pixels in held bricks with a plane", plane, "rows there", rows_plane, "without", bare, "with a TSDF row there", tsdf_bare)
    assert rows_plane > 50 and tsdf_bare > 50


def test_wall_walk_figures(oracle):
    vol, cvol, total, store = C.oracle_walk_map()
    assert tuple(total) == C.WALK_TOTAL and len(store) == C.WALK_HELD
    got = C.oracle_walk(oracle)
    for k, g in enumerate(got):
        print(C.WALK_BACK[k], g)
        assert g["rows_window"] == C.ROWS_WINDOW[k] and g["rows_map"] == C.ROWS_MAP[k] and g["rows_map"] > g["rows_window"]
        assert g["rows_window"] < 0.4 * g["rows_map"]                      # most of the wall in view lies in archived bricks
        for key, want in (("err_map_sdf", C.ERR_MAP_SDF), ("err_window_rgbd", C.ERR_WINDOW_RGBD), ("err_map_rgbd", C.ERR_MAP_RGBD)):
            assert g[key][:2] == pytest.approx(want[k], rel=0.02), (key, g[key], want[k])
        # the condition on the case
        assert g["err_map_rgbd"][1] <= 0.5 * min(g["err_map_sdf"][1], g["err_window_rgbd"][1]), g
        assert C.ERR_MAP_RGBD[k][1] <= 0.5 * min(C.ERR_MAP_SDF[k][1], C.ERR_WINDOW_RGBD[k][1])


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    at = hdr.index("---- Map volume colour term:")
    assert at > hdr.index("---- Map volume term:") and at > hdr.index("---- Volume colour term:")
    block = " ".join(hdr[at:hdr.index("int rpe_map_sdf_photo_rows(")].replace("\n *", " ").split())
    for what in ("VIRTUAL COLOUR VOLUME", "without a colour plane", "bit for bit", "ONCE per call", "RPE_ERR_STATE", "RPE_ERR_ARG", "2^24 bricks"):
        assert what in block, what
    window = " ".join(hdr[hdr.index("---- Volume colour term:"):hdr.index("int rpe_sdf_photo_rows(")].replace("\n *", " ").split())
    assert "rpe_icp_pyramid_map_sdf_rgbd" in window                              # "reads the dense window only" now points here
    text = open(os.path.join(UG.CSRC, "rpe_map_sdf_photo.hpp")).read()
    assert text.count("RPE_PRELOAD(") == 2                                        # one node per new kernel
    assert open(os.path.join(UG.CSRC, "rpe_sdf_photo.hpp")).read().rstrip().endswith('#include "rpe_map_sdf_photo.hpp"')
    api = open(os.path.join(UG.CSRC, "rpe_sdf_api.hip")).read()                   # the one host unit of both terms, window and map
    assert "build_grid(" not in api                                               # map_field lives once, beside build_grid
    assert open(os.path.join(UG.CSRC, "rpe_mapmesh_api.hip")).read().count("int rpeh::map_field(") == 1


def test_the_new_kernels_are_within_the_budget_taken():
    """no spill, no scratch.  The rows kernel and the photometric-only round: at most 128 registers (four waves per SIMD).  The combined
    round did not fit 128 without spills in six arrangements (DESIGN.md has their figures) and takes two waves per SIMD: at most 256"""
    rows = frontend_kernels()
    assert len(rows.get("map_sdf_photo_rows_kernel", [])) == 1 and len(rows.get("icp_map_sdf_photo_kernel", [])) == 4, sorted(rows)
    for r in rows["map_sdf_photo_rows_kernel"] + rows["icp_map_sdf_photo_kernel"]:
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        combined = "icp_map_sdf_photo_kernelILb1E" in r["mangled"]
        assert r["vgpr"] + r["agpr"] <= (256 if combined else 128), r
    assert sum("icp_map_sdf_photo_kernelILb1E" in r["mangled"] for r in rows["icp_map_sdf_photo_kernel"]) == 2
    assert rows["map_sdf_photo_rows_kernel"][0]["lds"] == 0


def test_the_round_kernel_finds_its_late_arguments_in_the_kernarg_segment(tmp_path):
    """icp_map_sdf_photo_kernel reads the view, the pose and the reduction's argument from the kernarg segment (rpe_map_sdf_photo.hpp
    map_photo_late_view, map_photo_late_pose -- rpe_frontend.hip late_pose_at at its offset --, late_finish_at), at the offsets of a struct that mirrors the argument list: the metadata
    must hold the arguments exactly there"""
    UG.built()
    layouts = kernarg_layouts(tmp_path, "icp_map_sdf_photo_kernel")
    assert len(layouts) == 4
    for layout in layouts:
        assert layout[:10] == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 80), (112, 36), (148, 16), (164, 4), (168, 48), (216, 136)], layout[:11]
    src = open(os.path.join(UG.CSRC, "rpe_map_sdf_photo.hpp")).read()
    assert "offsetof(MapSdfPhotoRoundArgs, fin) == 216 && sizeof(Finish) == 136" in src
    assert "offsetof(MapSdfPhotoRoundArgs, T) == 168 && sizeof(PoseF) == 48" in src
    assert "offsetof(MapSdfPhotoRoundArgs, P) == 32 && sizeof(MapSdfPhotoView) == 80" in src


def test_the_earlier_rounds_are_what_they_were():
    """the window's colour round and the map's geometric round keep their resources: the split of sdf_photo_row into gate and value, and
    the move of map_field, changed neither"""
    rows = frontend_kernels()
    assert sorted(r["vgpr"] for r in rows["icp_sdf_photo_kernel"]) == [110, 110, 124, 124]
    assert [r["vgpr"] for r in rows["icp_map_sdf_kernel"]] == [120, 120]
    for r in rows["icp_sdf_photo_kernel"] + rows["icp_map_sdf_kernel"] + rows["sdf_photo_rows_kernel"] + rows["map_sdf_rows_kernel"]:
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, r


def test_volume_map_sdf_color_track_cpp_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_map_sdf_color_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_map_sdf_color_track")])
