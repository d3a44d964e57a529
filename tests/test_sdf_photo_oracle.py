"""CPU: the volume colour term as tests/sdf_photo_oracle.py states it.  Every gate of the rule removes exactly the pixels the text says,
on a tiny hand-made volume; the row is the derivative of the residual (central differences over one voxel); the figures of
tests/sdf_photo_cases.py -- coverage, the wall loop the volume term alone loses, the room loop -- recomputed; and the build surface: the
four entry points, the resources of the new kernels, the untouched volume-term kernel, the C++ example."""
import os
import re
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import isa_tools as T
import sdf_cases as SC
import sdf_oracle as SO
import sdf_photo_cases as C
import sdf_photo_oracle as SP
import photo_oracle as PH
import unit_gates as UG
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"rpe_sdf_photo_rows", "rpe_sdf_photo_normal_eq", "rpe_icp_sdf_rgbd", "rpe_icp_pyramid_sdf_rgbd"}
EYE = pose12(np.eye(3), np.zeros(3))
F = np.float32


# ---------------------------------------------------------------------------------------------- the gates, on a tiny volume
def tiny():
    """4 x 4 x 4 voxels of 0.1 m at the origin, trunc 0.3: the plane z = 0.2 (tsdf 0.5, 0.167, -0.167, -0.5 along z: unsaturated), every
    weight 1; a colour that differs along every axis, colour weight 1.  27 vertices, one well inside each of the 27 cells, seen from the
    identity pose with intensity 100"""
    G = VO.Geometry((4, 4, 4), 0.1, (0.0, 0.0, 0.0), 0.3, 64)
    vol = G.empty()
    zc = (np.arange(4) + 0.5) * 0.1
    vol[..., 0] = ((0.2 - zc) / 0.3).astype(F)[:, None, None]
    vol[..., 1] = 1
    k, j, i = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    cvol = CO.empty(G)
    cvol[..., 0], cvol[..., 1], cvol[..., 2] = CO.h(40 + 30 * i), CO.h(60 + 20 * j), CO.h(90 + 25 * k)
    cvol[..., 3] = CO.h(1.0)
    c = np.array([0.07, 0.17, 0.27])
    z, y, x = np.meshgrid(np.array([0.12, 0.2, 0.28]), c, c, indexing="ij")
    V = np.stack([x.ravel(), y.ravel(), z.ravel()], -1).astype(F)
    cell = np.floor(V.astype(np.float64) / 0.1 - 0.5).astype(int)          # i0 per axis, far from every cell face
    return G, vol, cvol, V, np.full(len(V), 100, F), cell


def touches(cell, voxel):
    """the pixels whose cell has `voxel` (i, j, k) among its eight corners"""
    d = np.array(voxel) - cell
    return ((d >= 0) & (d <= 1)).all(1)


def mask(vol, cvol, G, V, If, gate=0.1):
    return SP.rows(vol, cvol, G, V, If, EYE, gate)[2]


def test_every_pixel_of_the_tiny_scene_has_a_row_and_the_value_is_the_colour_fields():
    G, vol, cvol, V, If, cell = tiny()
    st = {}
    r, J, ok = SP.rows(vol, cvol, G, V, If, EYE, 0.1, st)
    assert ok.all() and np.isfinite(r).all() and np.isfinite(J).all()
    assert np.array_equal(np.stack(st["i0"], -1).astype(int), cell)
    # the interpolated luma against the luma of color_oracle's interpolated colour: the same field up to the order of two linear maps
    rgb, known = CO.color_field(cvol, G, V)
    assert known.all() and np.abs(st["value"] - SP.luma(rgb)).max() < 1e-3
    assert np.array_equal(r.view(np.uint32), (st["value"] - If).view(np.uint32))
    # the colour rises by 30 r / 20 g / 25 b levels per voxel along x / y / z: a = -gradient / s at the identity pose
    want = -np.array([0.299 * 30, 0.587 * 20, 0.114 * 25]) / 0.1
    assert np.abs(J[:, :3] - want).max() < 2e-2, (J[0, :3], want)
    assert np.allclose(J[:, 3:], np.cross(V.astype(np.float64), J[:, :3].astype(np.float64)), atol=1e-4)


def test_step_1_a_vertex_or_an_intensity_that_is_not_finite():
    G, vol, cvol, V, If, cell = tiny()
    for bad in (np.nan, np.inf):
        for axis in range(3):
            W = V.copy()
            W[5 + axis, axis] = bad
            assert np.array_equal(~mask(vol, cvol, G, W, If), np.arange(len(V)) == 5 + axis)
        I2 = If.copy()
        I2[11] = bad                                              # A = 0 gives the NaN
        assert np.array_equal(~mask(vol, cvol, G, V, I2), np.arange(len(V)) == 11)
    rgba = np.full((len(V), 4), 255, np.uint8)
    rgba[11, 3] = 0
    assert np.array_equal(~mask(vol, cvol, G, V, PH.intensity(rgba)), np.arange(len(V)) == 11)


def test_step_1_a_cell_on_the_volumes_last_voxel():
    G, vol, cvol, V, If, cell = tiny()
    for axis in range(3):
        W = V.copy()
        W[:, axis] = np.where(cell[:, axis] == 2, F(0.36), W[:, axis])   # g = 3.1: i0 = 3 = dim - 1, one past the last cell
        assert np.array_equal(~mask(vol, cvol, G, W, If), cell[:, axis] == 2)
        W[:, axis] = np.where(cell[:, axis] == 0, F(0.04), V[:, axis])   # g = -0.1: i0 = -1
        assert np.array_equal(~mask(vol, cvol, G, W, If), cell[:, axis] == 0)


@pytest.mark.parametrize("voxel", [(1, 1, 1), (0, 3, 2), (3, 0, 0)])
def test_step_2_one_corner_unknown_saturated_or_nan(voxel):
    G, vol, cvol, V, If, cell = tiny()
    hit = touches(cell, voxel)
    assert hit.any() and not hit.all()
    i, j, k = voxel
    for channel, value in ((1, 0.0), (0, 1.0), (0, -1.0), (0, np.nan)):
        v2 = vol.copy()
        v2[k, j, i, channel] = value
        assert np.array_equal(~mask(v2, cvol, G, V, If), hit), (channel, value)
    v2 = vol.copy()
    v2[k, j, i, 0] = np.nextafter(F(1.0), F(0.0))                  # just inside the band: the corner stands (the distance gate may not)
    assert mask(v2, cvol, G, V, If, 10.0).all()


def test_step_2_the_distance_gate_is_inclusive():
    G, vol, cvol, V, If, cell = tiny()
    st = {}
    SP.rows(vol, cvol, G, V, If, EYE, 0.1, st)
    res = np.abs(st["tsdf"] * G.tr)
    for p in (0, 22, 26):
        assert res[p] > 0
        assert np.array_equal(mask(vol, cvol, G, V, If, res[p]), res <= res[p]) and mask(vol, cvol, G, V, If, res[p])[p]
        below = np.nextafter(res[p], F(0))
        assert np.array_equal(mask(vol, cvol, G, V, If, below), res <= below) and not mask(vol, cvol, G, V, If, below)[p]
    # the slope and normal gates are NOT asked: a flat TSDF (len = 0: the volume term has no row) keeps its photometric row
    flat = vol.copy()
    flat[..., 0] = 0.25
    assert mask(flat, cvol, G, V, If).all()
    assert not SO.rows(flat, G, V, np.tile(F([0, 0, -1]), (len(V), 1)), EYE, 0.1, 0.0, False)[2].any()


@pytest.mark.parametrize("voxel", [(1, 1, 1), (2, 0, 3), (0, 2, 1)])
def test_step_3_one_corner_without_colour(voxel):
    G, vol, cvol, V, If, cell = tiny()
    hit = touches(cell, voxel)
    i, j, k = voxel
    for bits in (0x0000, 0x8000, 0xBC00, 0x7E00):                  # weight 0, -0, -1, NaN: none is > 0
        c2 = cvol.copy()
        c2[k, j, i, 3] = bits
        assert np.array_equal(~mask(vol, c2, G, V, If), hit), hex(bits)
    c2 = cvol.copy()
    c2[k, j, i, 3] = 0x0001                                        # the smallest subnormal is > 0
    assert mask(vol, c2, G, V, If).all()


@pytest.mark.parametrize("bits", [0x7E00, 0x7C00, 0xFC00], ids=["nan", "inf", "-inf"])
def test_step_3_a_colour_that_is_not_finite_propagates(bits):
    """PROPAGATES: no gate looks at a colour channel's value.  The row stands (it is counted), its r and J are not finite, and the
    record's sums are what fp64 makes of them -- on the GPU exactly as here"""
    G, vol, cvol, V, If, cell = tiny()
    hit = touches(cell, (1, 2, 1))
    for channel in range(3):
        c2 = cvol.copy()
        c2[1, 2, 1, channel] = bits
        r, J, ok = SP.rows(vol, c2, G, V, If, EYE, 0.1)
        assert ok.all()
        assert np.array_equal(~np.isfinite(r), hit) and np.array_equal(~np.isfinite(J).all(1), hit)
        rec, _ = SP.record(r, J, ok, C.WEIGHT)
        assert rec[28] == len(V) and not np.isfinite(rec[:28]).any()


def test_the_spoiled_volume_exercises_both_colour_cases():
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    assert np.array_equal(vol, SC.room_volume(SMALL_CAM)[3])                     # the TSDF half is sdf_cases' volume, bit for bit
    sp = C.spoiled_color(cvol)
    w = CO.f32(sp[..., 3])
    assert ((CO.f32(cvol[..., 3]) > 0) & (w == 0)).sum() > 50
    assert (~np.isfinite(CO.f32(sp[..., :3])) & (w > 0)[..., None]).sum() > 100
    V, N, If = C.frame_levels(SMALL_CAM, *C.frame(SMALL_CAM))[0]
    assert np.isnan(If).sum() > 100 and np.isnan(V[:, 2]).sum() > 100
    st = {}
    r, J, ok = SP.rows(SC.spoiled(vol), sp, G, V, If, VC.held_out_pose(), 0.1, st)
    lost = st["finite"] & st["cell"] & st["known"] & st["band"] & st["distance"] & st["intensity"] & ~st["colour"]
    print("rows", ok.sum(), "lost to a colour weight", lost.sum(), "rows that are not finite", (~np.isfinite(r[ok])).sum())
    assert ok.sum() > 0.6 * len(V) and lost.sum() > 500 and (~np.isfinite(r[ok])).sum() > 500


# ---------------------------------------------------------------------------------------------- the row is the derivative
def test_the_row_against_central_differences(oracle):
    """the row against central differences of the oracle's own residual, on the wall fused at the true poses: steps of one voxel
    (0.04 m) and 0.04 / 3 rad.  Per column: correlation > 0 (and its sign), and max |J - dr| / max |dr| under 3 x JAC_SEEN"""
    G, vol, cvol, poses, frames = C.wall_fused()
    cam = VC.HALF_CAM
    d, rgb = frames[C.JAC_FRAME]
    V = FO.frame_maps(d, cam, 1.0, *VC.RANGE)[0]
    If = PH.intensity(CO.frame_rgba(rgb).reshape(cam[5], cam[4], 4)).reshape(-1)
    pose = poses[C.JAC_FRAME]
    r0, J, ok0 = SP.rows(vol, cvol, G, V, If, pose, 0.1)
    worst = 0.0
    for k in range(6):
        h = C.JAC_STEP_T if k < 3 else C.JAC_STEP_R
        step = np.zeros(6)
        step[k] = h
        rp, _, okp = SP.rows(vol, cvol, G, V, If, oracle.gn_apply(step, pose), 0.1)
        rm, _, okm = SP.rows(vol, cvol, G, V, If, oracle.gn_apply(-step, pose), 0.1)
        m = ok0 & okp & okm
        dr = (rp[m].astype(np.float64) - rm[m].astype(np.float64)) / (2 * h)
        Jk = J[m, k].astype(np.float64)
        corr, ratio = np.corrcoef(Jk, dr)[0, 1], np.abs(Jk - dr).max() / np.abs(dr).max()
        print("column", k, "rows", int(m.sum()), "correlation", corr, "max |J - dr| / max |dr|", ratio)
        assert m.sum() > 0.9 * len(V)
        assert corr > 0 and (Jk * dr).sum() > 0
        assert ratio < C.JAC_BOUND
        worst = max(worst, ratio)
    assert worst == pytest.approx(C.JAC_SEEN, abs=0.01) and C.JAC_BOUND == 3 * C.JAC_SEEN


def test_record_is_the_sum_of_the_rows_of_both_terms():
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    V, N, If = C.frame_levels(SC.RAGGED_CAM, *C.frame(SC.RAGGED_CAM))[1]
    geo = SO.rows(vol, G, V, N, VC.held_out_pose(), 0.15, SC.COS_THR, True)
    pho = SP.rows(vol, cvol, G, V, If, VC.held_out_pose(), 0.15)
    rec, S = SP.combined(geo, pho, C.WEIGHT)
    lam = F(C.WEIGHT)
    Jg, rg = geo[1][geo[2]].astype(np.float64), geo[0][geo[2]].astype(np.float64)
    Jp, rp = (lam * pho[1][pho[2]]).astype(np.float64), (lam * pho[0][pho[2]]).astype(np.float64)
    H = Jg.T @ Jg + Jp.T @ Jp
    assert np.allclose(rec[:21], H[np.triu_indices(6)], rtol=1e-12)
    assert np.allclose(rec[21:27], Jg.T @ rg + Jp.T @ rp, rtol=1e-9, atol=1e-12)
    assert rec[27] == pytest.approx((rg * rg).sum(), rel=1e-12) and rec[28] == geo[2].sum()
    assert rec[29] == pytest.approx((rp * rp).sum(), rel=1e-12) and rec[30] == pho[2].sum() and (S[:31] >= np.abs(rec[:31])).all()
    # more photometric rows than geometric ones: the slope and normal gates are not asked
    assert (geo[2] & ~pho[2] & np.isfinite(If)).sum() == 0 and pho[2].sum() > geo[2].sum()


# ---------------------------------------------------------------------------------------------- the figures of sdf_photo_cases
@pytest.mark.parametrize("cam", [SMALL_CAM, SC.RAGGED_CAM], ids=["160x120", "161x119"])
def test_coverage_figures(cam):
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    shares = []
    for l, (V, N, If) in enumerate(C.frame_levels(cam, *C.frame(cam))):
        shares.append(float(SP.rows(vol, cvol, G, V, If, VC.held_out_pose(), VC.TRACK_GATES[l])[2].sum()) / len(V))
    print(cam[4], "x", cam[5], shares)
    assert shares == pytest.approx(C.COVER_ORACLE, abs=6e-3) and min(shares) >= C.COVER


def test_wall_loop_figures(oracle):
    poses, frames, geometry = C.loop_scene("wall")
    with_term, rows = C.oracle_loop(oracle, poses, frames, geometry, C.WEIGHT)
    alone, _ = C.oracle_loop(oracle, poses, frames, geometry, None)
    print("wall loop: with the term", with_term, "rows", rows, "the volume term alone", alone)
    assert with_term[0] <= 1e-3 and with_term[1] <= 1e-3                                  # within 1 mrad / 1 mm
    assert alone[0] > 10 * with_term[0] and alone[1] > 10 * with_term[1]                  # the volume term alone is lost
    assert with_term == pytest.approx(C.WALL_LOOP_RGBD, rel=0.02) and alone == pytest.approx(C.WALL_LOOP_SDF, rel=0.02)
    assert all(C.WALL_ROWS[0][0] <= g <= C.WALL_ROWS[0][1] and C.WALL_ROWS[1][0] <= p <= C.WALL_ROWS[1][1] for g, p in rows), rows
    assert C.wall_limit() == (2 * C.WALL_LOOP_RGBD[0], 2 * C.WALL_LOOP_RGBD[1])


def test_room_loop_figures(oracle):
    poses, frames, geometry = C.loop_scene("room")
    with_term, rows = C.oracle_loop(oracle, poses, frames, geometry, C.WEIGHT)
    print("room loop: with the term", with_term, "rows", rows, "the volume term's own", SC.TRACK_ORACLE)
    assert with_term[0] <= 2 * SC.TRACK_ORACLE[0] and with_term[1] <= 2 * SC.TRACK_ORACLE[1]
    assert with_term == pytest.approx(C.ROOM_LOOP_RGBD, rel=0.02)
    assert C.ROOM_LOOP_SDF == pytest.approx(SC.TRACK_ORACLE, rel=0.01)
    assert all(C.ROOM_ROWS[0][0] <= g <= C.ROOM_ROWS[0][1] and C.ROOM_ROWS[1][0] <= p <= C.ROOM_ROWS[1][1] for g, p in rows), rows
    assert C.room_limit() == (2 * C.ROOM_LOOP_RGBD[0], 2 * C.ROOM_LOOP_RGBD[1])


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert hdr.index("---- Volume colour term:") > hdr.index("---- Volume term:")
    block = " ".join(hdr[hdr.index("---- Volume colour term:"):hdr.index("int rpe_sdf_photo_rows(")].replace("\n *", " ").split())
    for what in ("voxel-size blend", "dense window only", "not weighted by voxel weight", "truncation band", "NO model", "NO rpe_photo_prepare",
                 "NOT gated"):
        assert what in block, what
    from rgbd_pose_estimation_amd import build as B
    # the host side is the volume term's unit, which states the four calls once for both terms: no unit of its own
    assert "rpe_sdf_api.hip" in B.SOURCES and dict((s, k) for s, k, _ in B.UNITS)["rpe_sdf_api.hip"] == "host"
    assert "rpe_sdf_photo_api.hip" not in B.SOURCES and not os.path.exists(os.path.join(UG.CSRC, "rpe_sdf_photo_api.hip"))
    src = open(os.path.join(UG.CSRC, "rpe_frontend.hip")).read()
    assert src.rstrip().endswith('#include "rpe_sdf_photo.hpp"')                   # compiled into the front end's unit: no new kernel unit
    text = open(os.path.join(UG.CSRC, "rpe_sdf_photo.hpp")).read()
    assert text.count("RPE_PRELOAD(") == 2                                        # one node per new kernel


def frontend_kernels():
    UG.built()
    rows = {}
    for r in T.kernel_resources(UG.obj("rpe_frontend.hip")):
        rows.setdefault(r["base"], []).append(r)
    return rows


def test_the_new_kernels_are_lean():
    """no spill, no scratch, at most 128 registers; no LDS in the rows kernel"""
    rows = frontend_kernels()
    assert len(rows.get("sdf_photo_rows_kernel", [])) == 1 and len(rows.get("icp_sdf_photo_kernel", [])) == 4, sorted(rows)
    for r in rows["sdf_photo_rows_kernel"] + rows["icp_sdf_photo_kernel"]:
        print(r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] + r["agpr"] <= 128, r
    assert rows["sdf_photo_rows_kernel"][0]["lds"] == 0


def kernarg_layouts(tmp_path, kernel):
    co = T.code_object(UG.obj("rpe_frontend.hip"), str(tmp_path))
    notes = subprocess.check_output([T.READELF, "--notes", co]).decode()
    out = []
    for m in re.finditer(r"\.name:\s+(\S*\d+%s\S*)\n" % kernel, notes):
        if m.group(1).endswith(".kd"):
            continue
        args = notes[notes.rfind(".args:", 0, m.start()):m.start()]
        out.append([(int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)", args)])
    return out


def test_the_round_kernel_finds_its_late_arguments_in_the_kernarg_segment(tmp_path):
    """icp_sdf_photo_kernel reads the pose and the reduction's argument from the kernarg segment (rpe_frontend.hip late_pose_at and
    late_finish_at, the pose's offset named by rpe_sdf_photo.hpp photo_late_pose), at the offsets of a struct that mirrors the argument list: the metadata must hold the arguments exactly there"""
    UG.built()
    layouts = kernarg_layouts(tmp_path, "icp_sdf_photo_kernel")
    assert len(layouts) == 4
    for layout in layouts:
        assert layout[:11] == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 8), (40, 8), (48, 36), (84, 16), (100, 4), (104, 48), (152, 136)], layout[:12]
    src = open(os.path.join(UG.CSRC, "rpe_sdf_photo.hpp")).read()
    assert "offsetof(SdfPhotoRoundArgs, fin) == 152 && sizeof(Finish) == 136" in src
    assert "offsetof(SdfPhotoRoundArgs, T) == 104 && sizeof(PoseF) == 48" in src


def test_the_volume_terms_round_kernel_is_what_it_was(tmp_path):
    """icp_sdf_kernel keeps its code: two instances, the resources and the kernarg layout tests/test_sdf_oracle.py holds it to"""
    rows = frontend_kernels()
    assert len(rows.get("icp_sdf_kernel", [])) == 2 and len(rows.get("sdf_rows_kernel", [])) == 1
    for r in rows["icp_sdf_kernel"]:
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, r
    layouts = kernarg_layouts(tmp_path, "icp_sdf_kernel")
    assert len(layouts) == 2
    for layout in layouts:
        assert layout[:8] == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 36), (68, 16), (84, 48), (136, 136)], layout[:9]


def test_volume_sdf_color_track_cpp_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_sdf_color_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_sdf_color_track")])
