"""CPU: the map fuse as tests/mapfuse_oracle.py states it -- a composition of mapmesh_oracle.dense, rebuild_oracle.fuse and the split back
into window and bricks -- the conditions on the small scene of tests/mapfuse_cases.py, and the build surface: the entry point, the
Python and C++ names, the resources of every map_fuse_kernel instance, and rpe_rebuild.hip's kernels, which gave up their cull's text
to a shared header and must hold what they held."""
import os

import numpy as np

import isa_tools as T
import mapfuse_cases as C
import mapfuse_oracle as MF
import mapmesh_cases as MC
import mapmesh_oracle as MM
import rebuild_oracle as RO
import unit_gates as UG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_volume_map_fuse_keyframes"}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_store(a, b):
    return set(a) == set(b) and all(same(a[k][0], b[k][0]) and same(a[k][1], b[k][1]) for k in a)


def walked_map(colour=True):
    """a sphere's world uploaded at three stops of a short walk: a window with content and held bricks around it"""
    return MC.Map(None, C.DIMS, C.KW).fill(MC.sphere((10.2, 7.7, 8.4), 9.3), [(8, 0, 0), (0, 8, -8)], colour=colour)


# ---------------------------------------------------------------------------------------------- the build surface
def test_entry_point_and_names():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert "Map fuse" in hdr and "const int64_t lo[3], const int64_t hi[3], int64_t stats[4]);" in hdr
    from rgbd_pose_estimation_amd import api
    assert callable(api.Context.volume_map_fuse_keyframes)
    hpp = open(os.path.join(ROOT, "rgbd_pose_estimation_amd", "include", "pose", "DepthFrontEnd.hpp")).read()
    assert "MapFuseStats fuseKeyframesMap(" in hpp and "rpe_volume_map_fuse_keyframes(_ctx" in hpp
    # the archive's clear no longer calls itself the remedy after a loop closure
    assert "rpe_volume_map_fuse_keyframes" in hdr.split("int rpe_volume_archive_clear")[0].rsplit("/*", 1)[1]
    assert "volume_map_fuse_keyframes" in api.Context.volume_archive_clear.__doc__ and "fuseKeyframesMap" in hpp.split("void archiveClear")[0][-300:]


def test_every_instance_of_the_kernel_is_lean():
    """resource metadata of the built code object: <= 128 registers, no scratch, no spill, the cull's keep[] flags and little else in LDS"""
    UG.built()
    rows = [r for r in T.kernel_resources(UG.obj("rpe_frontend.hip")) if r["base"] == "map_fuse_kernel"]
    for r in rows:
        print(r["name"], {k: r[k] for k in ("vgpr", "agpr", "vgpr_spill", "sgpr_spill", "scratch", "lds")})
    assert len(rows) == 6, [r["name"] for r in rows]                                     # pass 1: colour or not; pass 2: clear x colour
    for r in rows:
        assert r["vgpr"] + r["agpr"] <= 128 and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert 1024 <= r["lds"] <= 2048, r


def test_the_rebuild_unit_holds_the_kernels_it_held():
    UG.built()
    assert T.kernel_bases(UG.obj("rpe_rebuild.hip")) == {"volume_fuse_kernel": 4, "attach_pack_kernel": 1}
    src = open(os.path.join(UG.CSRC, "rpe_rebuild.hip")).read()
    field = open(os.path.join(UG.CSRC, "rpe_volume_field.hpp")).read()
    assert "bool box_can_update(" not in src and field.count("bool box_can_update(") == 1 and field.count("bool edge_outside(") == 1
    assert "box_can_update(" in open(os.path.join(UG.CSRC, "rpe_mapfuse.hpp")).read()


# ---------------------------------------------------------------------------------------------- the composition
def test_the_windows_extent_after_a_shift_is_the_window_fuse():
    """box = the window's extent, nothing held: the virtual volume is the window and its origin the window's own after the shift (one
    rounding of origin + total * voxel_size), so the result is rebuild_oracle.fuse on the window's own geometry"""
    m = MC.Map(None, C.DIMS, C.KW, capacity=0)
    m.shift((8, -8, 0))
    G = MM.SO.geometry_after(m.dims, m.kw["voxel_size"], m.kw["origin"], m.kw["trunc"], m.kw["max_weight"], m.total)
    Gb = MM.geometry(m.kw, m.extent())
    assert same(G.o, Gb.o) and G.dim == Gb.dim
    assert not same(G.o, (np.asarray(C.KW["origin"], np.float32) + np.float32(0.05) * np.asarray(m.total, np.float32)))   # not two roundings
    for color in (False, True):
        want, cwant = RO.fuse(None, None, G, C.entries([0, 1, 2]), C.flags_of(True, color))
        w, cw, store, stats = MF.fuse(m.window, None, m.total, {}, m.extent(), m.kw, C.entries([0, 1, 2]), C.flags_of(True, color))
        assert same(w, want) and store == {} and stats == dict(bricks=12, archived=0, released=0) and (want[..., 1] > 0).sum() > 1000
        assert (cw is None and cwant is None) or same(cw, cwant)


def test_dense_then_split_is_the_identity():
    m = walked_map()
    assert len(m.store) >= 8 and m.cwindow is not None
    for box in (m.bounds(), m.extent(), (m.bounds()[0] - 8, m.bounds()[1] + [8, 0, 16])):
        w, cw, store, stats = MF.fuse(m.window, m.cwindow, m.total, m.store, box, m.kw, [], 0)
        assert same(w, m.window) and same(cw, m.cwindow) and same_store(store, m.store) and stats["archived"] == stats["released"] == 0


def test_the_small_scene_has_every_kind_of_brick():
    count, looked_at = C.update_counts()
    print(np.bincount(count.reshape(-1)), int((looked_at & (count == 0)).sum()))
    assert count.shape == (4, 4, 6)
    assert (count == 0).sum() >= 8 and (count == 1).sum() >= 8 and (count >= 2).sum() >= 8       # seen by none, by one, by more
    assert (looked_at & (count == 0)).sum() >= 4                      # in front of keyframe 0, in its image, and only behind its surface
    window = np.zeros(count.shape, bool)
    window[1:3, 1:3, 1:4] = True                                     # the window at total (0, 0, 0) inside the box from (-8, -8, -8)
    assert (count[window] > 0).any() and (count[~window] > 0).any() and (count[~window] == 0).any()


def test_clear_releases_accumulate_keeps_and_colour_follows_the_rules():
    m = walked_map()
    before = dict(m.store)
    box = m.bounds()
    # CLEAR without COLOR: the box's colour goes to zero, the colour window stays; held bricks nobody sees are released
    w, cw, store, stats = MF.fuse(m.window, m.cwindow, m.total, m.store, box, m.kw, C.entries([1]), C.flags_of(True, False))
    assert cw is not None and not cw.any() and stats["released"] > 0 and all(not c.any() for _, c in store.values())
    assert all(t.view(np.uint32).any() for t, _ in store.values())
    # without CLEAR: every held brick stays, unseen ones bit for bit, and new ones join
    w, cw, store, stats = MF.fuse(m.window, m.cwindow, m.total, m.store, box, m.kw, C.entries([1]), C.flags_of(False, True))
    assert stats["released"] == 0 and set(before) <= set(store)
    assert any(same(store[k][0], before[k][0]) for k in before) and any(not same(store[k][0], before[k][0]) for k in before)


# ---------------------------------------------------------------------------------------------- the use case
def test_the_walk_rebuilt_at_corrected_poses_the_figures():
    """tests/mapfuse_cases.py's figures recomputed with the oracle, and the claim: rebuilt at the corrected poses the whole map is
    better than as fused, within the margin of the true-pose map, and covers strictly more than today's route leaves"""
    u = C.oracle_use_case()
    print(u)
    assert u["box"] == C.USE_BOX and u["held"] == C.USE_HELD and u["keyframes"] == 13
    assert all(C.same_figures(u[k], C.FIGURES[k]) for k in C.FIGURES), {k: u[k] for k in C.FIGURES}
    assert (u["corrected"]["held"], u["corrected"]["archived"], u["corrected"]["released"]) == (C.USE_HELD_REBUILT, C.USE_ARCHIVED, C.USE_RELEASED)
    C.claim(u)
    assert u["corrected"]["share"] > 2 * u["today"]["share"]                              # the case is well chosen: strictly, and by far
    assert abs(C.MARGIN - 0.0049) < 1e-12


def test_the_cpp_front_end_compiles_with_the_new_call(tmp_path):
    """g++ on a translation unit that names DepthFrontEnd::fuseKeyframesMap with its defaults (syntax and types only: no GPU, no link)"""
    import subprocess
    src = tmp_path / "map_fuse.cpp"
    src.write_text('#include "DepthFrontEnd.hpp"\n'
                   "rpe::DepthFrontEnd::MapFuseStats rebuild(rpe::DepthFrontEnd& fe, const int64_t* lo, const int64_t* hi) {\n"
                   "  rpe::DepthFrontEnd::MapFuseStats a = fe.fuseKeyframesMap();\n"
                   "  rpe::DepthFrontEnd::MapFuseStats b = fe.fuseKeyframesMap({0, 1}, {}, false, true, false, lo, hi);\n"
                   "  a.written += b.bricks + b.archived + b.released;\n  return a;\n}\n")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsyntax-only", "-I", os.path.join(inc, "pose"), "-I", inc, str(src)])
