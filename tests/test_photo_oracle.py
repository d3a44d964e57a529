"""CPU: the numpy statement of the photometric term (tests/photo_oracle.py) against itself -- its Jacobian row against central
differences of its own residual, the NaN rules on small hand-made maps, the figures of tests/photo_cases.py recomputed -- and the
cross-compiled library: exports, header, the C++ driver compiles."""
import os
import subprocess

import numpy as np
import pytest

import isa_tools as T
import photo_cases as PC
import photo_oracle as PH
import unit_gates as UG
import volume_cases as VC
from frontend_util import SMALL_CAM, pose12
from rgbd_pose_estimation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMS = {"rpe_model_color_upload", "rpe_model_color_from_frame", "rpe_photo_prepare", "rpe_photo_download", "rpe_photo_normal_eq",
        "rpe_photo_rows", "rpe_icp_rgbd", "rpe_icp_pyramid_rgbd"}


# ---------------------------------------------------------------------------------------------- the row is the residual's derivative
def test_jacobian_against_central_differences(oracle):
    case = PC.pair(PC.WALL, noise=0.0)
    IA, IB = PC.smooth_intensity(case[0], SMALL_CAM, PC.WALL), PC.smooth_intensity(case[3], SMALL_CAM, PC.WALL)
    V, _, _, If, MV, MN, pmap = PC.pair_oracle_maps(case, SMALL_CAM, IA, IB)
    p0 = case[3]
    _, J, ok0 = PH.rows(V, If, pmap, SMALL_CAM, p0, case[0], PC.PAIR_GATE)
    worst = []
    for k in range(6):
        h = PC.JAC_STEP_T if k < 3 else PC.JAC_STEP_R
        d = np.zeros(6)
        d[k] = h
        rp, _, okp = PH.rows(V, If, pmap, SMALL_CAM, oracle.gn_apply(d, p0), case[0], PC.PAIR_GATE)    # T <- exp(delta) T
        rm, _, okm = PH.rows(V, If, pmap, SMALL_CAM, oracle.gn_apply(-d, p0), case[0], PC.PAIR_GATE)
        m = ok0 & okp & okm
        assert m.sum() > 0.9 * ok0.sum() > 0.8 * len(V)
        dr = (rp[m].astype(np.float64) - rm[m]) / (2 * h)
        worst.append(float(np.abs(J[m, k] - dr).max() / np.abs(dr).max()))
    print("jacobian vs central differences, per column:", ["%.2e" % x for x in worst])
    assert max(worst) < PC.JAC_BOUND, worst
    assert max(worst) > PC.JAC_SEEN / 3, worst      # the figure on record is the figure seen


# ---------------------------------------------------------------------------------------------- NaN rules on hand-made maps
W_, H_ = 10, 8
TINY = (8.0, 8.0, 4.5, 3.5, W_, H_)
EYE = pose12(np.eye(3), np.zeros(3))


def _tiny(unknown=(), nan_normal=(), far=()):
    """a plane at z = 2 seen by TINY from the identity pose as model, a textured RGBA map; the frame looks at the same plane with
    every pixel's ray moved by (+0.25, +0.5) pixel, so that pixel (u, v) lands in the stencil (u, v) .. (u+1, v+1).
    unknown: model pixels with A = 0; nan_normal: with a NaN normal; far: 0.5 m behind the plane (beyond the gate)"""
    fx, fy, cx, cy, w, h = TINY
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = np.full((h, w), 2.0)
    for (a, b) in far:
        z[b, a] += 0.5
    MV = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1).reshape(-1, 3).astype(F)
    MN = np.tile(np.array([0, 0, -1], F), (w * h, 1))
    for (a, b) in nan_normal:
        MN[b * w + a] = np.nan
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[..., 0] = (20 * u + 3 * v).astype(np.uint8)
    rgba[..., 1] = (5 * u + 25 * v).astype(np.uint8)
    rgba[..., 2] = 77
    rgba[..., 3] = 255
    for (a, b) in unknown:
        rgba[b, a, 3] = 0
    zf = np.full((h, w), 2.0)
    V = np.stack([(u + 0.25 - cx) / fx * zf, (v + 0.5 - cy) / fy * zf, zf], -1).reshape(-1, 3).astype(F)
    If = np.full(w * h, 100.0, F)
    return V, If, PH.model_map(PH.intensity(rgba), MV, MN, EYE)


def _expected(bad_I=(), bad_zm=()):
    """pair mask by the text alone: stencil inside the map, its sixteen floats finite -- I is NaN at bad_I, gx beside it in x (and on
    the left / right border), gy beside it in y (and on the top / bottom border), zm at bad_zm"""
    nanI = np.zeros((H_, W_), bool)
    nangx, nangy, nanz = nanI.copy(), nanI.copy(), nanI.copy()
    nangx[:, [0, -1]] = True
    nangy[[0, -1], :] = True
    for (a, b) in bad_I:
        nanI[b, a] = True
        for da in (-1, 1):
            if 0 <= a + da < W_:
                nangx[b, a + da] = True
            if 0 <= b + da < H_:
                nangy[b + da, a] = True
    for (a, b) in bad_zm:
        nanz[b, a] = True
    bad = nanI | nangx | nangy | nanz
    ok = np.zeros((H_, W_), bool)
    for v in range(H_ - 1):
        for u in range(W_ - 1):
            ok[v, u] = not bad[v:v + 2, u:u + 2].any()
    return ok.reshape(-1)


@pytest.mark.parametrize("name,kw,exp", [
    ("border", {}, {}),
    ("unknown_colour", {"unknown": [(4, 4)]}, {"bad_I": [(4, 4)]}),
    ("nan_normal", {"nan_normal": [(3, 5), (6, 2)]}, {"bad_zm": [(3, 5), (6, 2)]}),
    ("depth_gate", {"far": [(5, 2)]}, {"bad_zm": [(5, 2)]}),
    ("all", {"unknown": [(2, 2)], "nan_normal": [(7, 5)], "far": [(5, 3)]}, {"bad_I": [(2, 2)], "bad_zm": [(7, 5), (5, 3)]}),
])
def test_nan_rules_remove_exactly_the_pairs_the_text_says(name, kw, exp):
    V, If, pmap = _tiny(**kw)
    r, J, ok = PH.rows(V, If, pmap, TINY, EYE, EYE, 0.1)
    want = _expected(**exp)
    assert np.array_equal(ok, want), (name, ok.reshape(H_, W_).astype(int), want.reshape(H_, W_).astype(int))
    assert want.sum() >= 10 and np.isfinite(r[ok]).all() and np.isfinite(J[ok]).all()
    assert np.isnan(r[~ok]).all() and np.isnan(J[~ok]).all()
    rec, S = PH.record(r, J, ok, 0.01)
    assert rec[28] == want.sum() and np.isfinite(rec).all() and (S[:28] >= np.abs(rec[:28])).all()


def test_frame_rules_and_the_gate_itself():
    V, If, pmap = _tiny()
    base = _expected()
    V2, If2 = V.copy(), If.copy()
    V2[13, 1] = np.nan          # a hole in the depth
    If2[24] = np.nan            # an unknown frame colour
    V2[35] = V[35] * F(1.04)    # 8 cm further along its ray: inside the gate of 0.1 m, outside one of 0.05 m
    ok = PH.rows(V2, If2, pmap, TINY, EYE, EYE, 0.1)[2]
    want = base.copy()
    want[[13, 24]] = False
    assert base[[13, 24, 35]].all() and np.array_equal(ok, want)
    ok = PH.rows(V2, If2, pmap, TINY, EYE, EYE, 0.05)[2]
    want[35] = False
    assert np.array_equal(ok, want)
    # behind the model camera, and outside its image
    back = pose12(np.diag([-1.0, 1.0, -1.0]), np.zeros(3))
    assert not PH.rows(V, If, pmap, TINY, back, EYE, 0.1)[2].any()
    assert not PH.rows(V, If, pmap, TINY, pose12(np.eye(3), np.array([5.0, 0, 0])), EYE, 10.0)[2].any()


def test_intensity_pyramid_and_block_mean():
    rng = np.random.default_rng(1)
    rgba = rng.integers(0, 256, (9, 13, 4)).astype(np.uint8)
    rgba[..., 3] = 255
    rgba[4, 6, 3] = 0
    I = PH.intensity_pyramid(PH.intensity(rgba), 3)
    assert [i.shape for i in I] == [(9, 13), (4, 6), (2, 3)]
    assert np.isnan(I[0]).sum() == 1 and np.isnan(I[1][2, 3]) and np.isnan(I[1]).sum() == 1 and np.isnan(I[2][1, 1])
    c = rgba[0, 0].astype(np.float64)
    assert abs(I[0][0, 0] - (0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2])) < 1e-4
    assert I[1][0, 0] == F((((I[0][0, 0] + I[0][0, 1]) + I[0][1, 0]) + I[0][1, 1]) * F(0.25))


# ---------------------------------------------------------------------------------------------- the figures of photo_cases.py
def _near(got, want, rel=0.05):
    return all(abs(g - w) <= rel * w for g, w in zip(got, want))


def test_wall_pair_figures(oracle):
    """ICP alone does not move in the wall's plane; with the term the pair is tracked"""
    start, icp = PC.oracle_pair(oracle, PC.WALL, None)
    _, rgbd = PC.oracle_pair(oracle, PC.WALL, PC.WEIGHT)
    print("wall pair: start", start, "ICP", icp, "RGB-D", rgbd)
    assert abs(start[0] - 0.01) < 1e-6 and abs(start[1] - 0.05) < 1e-6
    assert _near(icp, PC.PAIR_WALL_ICP) and _near(rgbd, PC.PAIR_WALL_RGBD), (icp, rgbd)
    assert icp[0] > start[0] / 2 and icp[1] > start[1] / 2 and rgbd[0] < 1e-4 and rgbd[1] < 1e-4
    case = PC.pair(PC.WALL)
    V, _, _, If, _, _, pmap = PC.pair_oracle_maps(case)
    ok = PH.rows(V, If, pmap, SMALL_CAM, case[3], case[0], PC.PAIR_GATE)[2]
    cover = ok.sum() / np.isfinite(V).all(1).sum()
    assert abs(cover - PC.PAIR_WALL_COVERAGE) < 0.005 and cover >= 0.8


def test_room_pair_figures(oracle):
    """where geometry holds all six degrees of freedom the term leaves the result in the same order"""
    _, rgbd = PC.oracle_pair(oracle, None, PC.WEIGHT)
    print("room pair: RGB-D", rgbd)
    assert _near(rgbd, PC.PAIR_ROOM_RGBD), rgbd
    assert rgbd[0] < 3 * PC.PAIR_ROOM_ICP[0] and rgbd[1] < 3 * PC.PAIR_ROOM_ICP[1]


def test_wall_loop_figures(oracle):
    """the tracking loop through the TSDF + colour volume on the wall, with and without the term"""
    poses = [PC.wall_pose(k) for k in range(PC.WALL_FRAMES)]
    frames = PC.loop_frames(poses, PC.WALL)
    rgbd = PC.oracle_loop(oracle, poses, frames, PC.wall_geometry(), PC.WEIGHT)
    icp = PC.oracle_loop(oracle, poses, frames, PC.wall_geometry(), None)
    print("wall loop: ICP", icp, "RGB-D", rgbd)
    assert _near(rgbd, PC.WALL_LOOP_RGBD) and _near(icp, PC.WALL_LOOP_ICP), (rgbd, icp)
    assert icp[1] > 0.1 and rgbd[0] < 5e-4 and rgbd[1] < 5e-4


# ---------------------------------------------------------------------------------------------- the cross-compiled library
def test_header_and_library_export_the_photometric_entry_points():
    hdr = UG.check_entry_points(SYMS)
    assert "RPE_PHOTO_FRAME = 0" in hdr and "RPE_PHOTO_MODEL = 1" in hdr and (L.PHOTO_FRAME, L.PHOTO_MODEL) == (0, 1)
    assert L.lib().rpe_abi_version() == 1


def test_icp_kernels_keep_their_unit():
    """the term is one new unit: the ICP unit still holds the fused and resident kernels only, and the new unit shares their
    per-pixel code (associate_pixel, pair_group) instead of restating it"""
    UG.built()
    assert set(T.kernel_bases(UG.obj("rpe_icp.hip"))) == {"icp_fused_kernel", "icp_resident_kernel"}
    src = open(os.path.join(ROOT, "rgbd_pose_estimation_amd", "csrc", "rpe_photo.hip")).read()
    assert "associate_pixel(" in src and "pair_group<" in src and "add_row2<" in src


def test_photometric_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "photo_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "photo_track")])
