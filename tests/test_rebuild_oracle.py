"""CPU: the volume rebuilt from keyframes, as tests/rebuild_oracle.py states it -- the figures of tests/rebuild_cases.py recomputed and
the statement they carry (the map fused at the optimised poses is as good as the one fused at the true poses, the drifted one is
not) --, and the build surface: exported symbols, the header, the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import rebuild_cases as RC
import rebuild_oracle as RO
import unit_gates as UG
import volume_cases as VC
import volume_oracle as VO
from rgbd_pose_estimation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_keyframe_attach_frame", "rpe_keyframe_attach_host", "rpe_keyframe_attachment_info", "rpe_keyframe_attachment_download",
        "rpe_volume_fuse_keyframes"}


# ---------------------------------------------------------------------------------------------- the figures
def test_the_rebuilt_map_is_as_good_as_the_true_one_and_the_drifted_one_is_not():
    """The eight `small` shots fused into volume_cases.room_geometry() at the true, the drifted and the oracle loop's poses, raycast
    from the held-out pose.  The ordering holds for the median AND the 90th percentile on this scene: optimised strictly below
    drifted, truth not above optimised.  The GPU inherits the statement through bit equality (tests/test_gpu_rebuild.py)."""
    got = {n: RC.oracle_figures(n) for n in ("truth", "drifted", "optimised")}
    print(got)
    for n, (hits, med, p90) in got.items():
        fig = RC.FIGURES[n]
        assert abs(hits - fig[0]) <= 2 and med == pytest.approx(fig[1], rel=2e-2) and p90 == pytest.approx(fig[2], rel=2e-2), (n, got[n], fig)
    t, d, o = got["truth"], got["drifted"], got["optimised"]
    assert o[1] < d[1] and o[2] < d[2]
    assert t[1] <= o[1] and t[2] <= o[2]
    assert 5 * o[1] < d[1] and 4 * o[2] < d[2]                    # not by a hair: the drifted map is several times worse
    assert o[0] >= d[0] and min(t[0], d[0], o[0]) > 0.9 * RC.CAM[4] * RC.CAM[5]
    # the median is volume_cases.hit_depth_errors' own
    G, _, _ = RC.room()
    MV, _ = VO.raycast(RC.fused("optimised"), G, RC.CAM, VC.held_out_pose(), *VC.RAY)
    assert VC.hit_depth_errors(MV, VC.held_out_pose(), RC.CAM)[0] == o[1]


def test_the_oracle_is_the_loop_over_the_integrate_oracles_and_the_order_matters():
    (dims, s, o), ids = RC.VOLUMES["odd"], RC.LISTS["three"]
    G, _ = RC.geometry(dims, s, o, max_weight=2)
    c = RC.case()
    es = RC.entries([c.poses0[i] for i in ids], ids)
    vol, cvol = RO.fuse(None, None, G, es, RO.CLEAR | RO.COLOR)
    v, cv = G.empty(), CO.empty(G)
    for e in es:
        v, cv = CO.integrate(v, cv, G, RO.as_map(e["z"]), e["rgba"], e["cam"], e["pose"])
    assert np.array_equal(vol.view(np.uint32), v.view(np.uint32)) and np.array_equal(cvol, cv)
    assert (vol[..., 1] > 0).sum() > 1000 and (cvol[..., 3] != 0).sum() > 100
    # depth only: the tsdf half is the same, no colour volume comes back
    vd, none = RO.fuse(None, None, G, es, RO.CLEAR)
    assert none is None and np.array_equal(vd.view(np.uint32), vol.view(np.uint32))
    # without CLEAR the incoming volume is the start
    again, _ = RO.fuse(vd, None, G, es[:1], 0)
    assert np.array_equal(again.view(np.uint32), VO.integrate(vd, G, RO.as_map(es[0]["z"]), es[0]["cam"], es[0]["pose"]).view(np.uint32))
    # max_weight 2 with three observations: the clamp engages, the reversed list ends elsewhere
    rev, _ = RO.fuse(None, None, G, es[::-1], RO.CLEAR)
    assert (vd[..., 1] == 2).any() and not np.array_equal(rev.view(np.uint32), vd.view(np.uint32))


def test_the_wide_volume_gives_the_cull_something_to_cull():
    """per keyframe of the fan, and of the rolled fan, a good part of the kernel's bricks holds no voxel it updates; the blind keyframe
    updates none at all"""
    dims, s, o = RC.WIDE
    G, _ = RC.geometry(dims, s, o)
    c = RC.case()
    for poses in (c.truth[:4], RC.rolled_poses()):
        for e in RC.entries(poses, range(4)):
            _, mask = VO.integrate(G.empty(), G, RO.as_map(e["z"]), e["cam"], e["pose"], with_mask=True)
            share = RC.brick_update_share(G, mask)
            assert mask.any() and 0.4 < share < 1, share
    e = RC.entry(RC.shots()[0], RC.BLIND)
    assert not VO.integrate(G.empty(), G, RO.as_map(e["z"]), e["cam"], e["pose"], with_mask=True)[1].any()


# ---------------------------------------------------------------------------------------------- registers
# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_rebuild_entry_points():
    hdr = UG.check_entry_points(SYMS)
    assert "enum { RPE_FUSE_CLEAR = 1, RPE_FUSE_COLOR = 2, RPE_FUSE_NO_CULL = 4 };" in hdr
    assert (L.FUSE_CLEAR, L.FUSE_COLOR, L.FUSE_NO_CULL) == (1, 2, 4)
    assert "the caller fuses its own" not in hdr                     # the graph section no longer sends the user away


def test_rebuild_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_rebuild.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_rebuild")])
