"""CPU: pins the numpy statement of colour registration (tests/register_oracle.py) with cases whose answer is known without it,
recomputes the oracle figures the GPU thresholds are set from (tests/register_cases.py), checks the simulator's distorted colour camera
against the forward model, the library's export, that the registration kernels neither spill nor carry scratch, and that the C++ driver
compiles.

Two kinds of test live here.  Those that PIN THE ORACLE run numpy alone, so that the statement the device is held to stands on answers
known without the device, and do not need the library: test_identity_rig_returns_the_input_colour,
test_projection_is_the_written_expression_scalar_by_scalar, test_z_buffer_hides_the_far_one_of_two_points_on_one_ray,
test_bilinear_sample_and_quantise_on_a_ramp, test_integrate_gate_is_color_integrate_where_alpha_is_set_and_nothing_where_it_is_not,
test_registration_figures and test_accuracy_figures (the last three with the simulator's distorted camera).  Those that NEED THE
FEATURE in the sources: test_render_rgb_with_distortion_inverts_the_forward_model (simulator), the export and C++ driver tests (library, header, ctypes, DepthFrontEnd.hpp).  Everything on the device is in
tests/test_gpu_register.py."""
import os
import subprocess

import numpy as np

import color_cases as CC
import color_oracle as CO
import register_cases as RC
import register_oracle as RO
import unit_gates as UG
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, rot
from rgbd_pose_estimation_amd import _lib as L
from rgbd_pose_estimation_amd import simulator as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _small_frame(holes=False):
    p = VC.view(1)
    d = VC.depth_at(p, SMALL_CAM)
    if holes:
        d = d.copy()
        d[30:34, 50:57] = 0
        d[77, 100] = 0
    return p, d, FO.frame_maps(d, SMALL_CAM, 1.0, *VC.RANGE)[0]


def test_identity_rig_returns_the_input_colour():
    """the same camera, no distortion, identity pose: px = fx * (X / Z) + cx of a vertex X = (u - cx) / fx * Z is u up to a rounding,
    so the bilinear weights are within 1e-4 of 0 or 1 and q() gives the pixel's own byte.  The rule for the pixels the oracle leaves
    out, checked here: (1) no depth; (2) a projection whose floor lies outside 0 .. w - 2 x 0 .. h - 2 -- the last column and row, and
    pixels of column / row 0 whose px rounds below 0 -- so only INTERIOR pixels are promised; (3) with the occlusion test (cell 1), the
    far side of a depth edge: a pixel one of whose eight neighbours is nearer by more than the tolerance, because every pixel writes its
    z into the four cells around its projection.  A depth HOLE casts no shadow: pixels beside one keep their colour.  Every other
    pixel returns the input colour exactly."""
    p, d, V = _small_frame(holes=True)
    fx, fy, cx, cy, w, h = SMALL_CAM
    img = S.render_rgb(p[:9].reshape(3, 3), p[9:], SMALL_CAM)
    flat = img.reshape(-1, 3)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    interior = ((u >= 1) & (u <= w - 2) & (v >= 1) & (v <= h - 2)).reshape(-1)
    valid = np.isfinite(V).all(1)
    assert (~valid).sum() == 29
    # cell 0: rule (1) and (2) only
    out = RO.register(V, img, RO.Rig(SMALL_CAM, cell=0))
    must = interior & valid
    assert np.all(out[must, 3] == 255) and np.array_equal(out[must, :3], flat[must])
    assert np.all(out[~valid] == 0) and np.all(out[out[:, 3] == 0] == 0)
    # cell 1 with the default tolerance: rule (3) on top
    rig = RO.Rig(SMALL_CAM, cell=1)
    out1 = RO.register(V, img, rig)
    z = np.where(valid, V[:, 2], np.nan).reshape(h, w).astype(np.float64)
    pad = np.pad(z, 1, constant_values=np.nan)
    zmin = np.full_like(z, np.inf)
    for dv in (0, 1, 2):
        for du in (0, 1, 2):
            zmin = np.fmin(zmin, pad[dv:dv + h, du:du + w])
    with np.errstate(invalid="ignore"):
        edge = (z - zmin > 0.999 * (rig.occl_tol + rig.occl_tol_z2 * zmin * zmin)).reshape(-1)      # a hair inside, for fp32
        clear = (z - zmin < 0.5 * (rig.occl_tol + rig.occl_tol_z2 * zmin * zmin)).reshape(-1)
    got = out1[:, 3] == 255
    assert 50 < (must & edge).sum() < 2000
    assert np.all(got[must & clear]) and not (got & (out[:, 3] == 0)).any()
    assert np.array_equal(out1[got], out[got])                               # whatever is coloured is the cell-0 colour
    assert np.all(edge[must & ~got])                                         # only the far side of an edge is left out
    # a hole casts no shadow: the pixels around the holes keep their colour
    hole_nb = np.zeros((h, w), bool)
    for dv in (0, 1, 2):
        for du in (0, 1, 2):
            hole_nb |= np.isnan(pad[dv:dv + h, du:du + w])
    hole_nb = hole_nb.reshape(-1) & must & clear
    assert hole_nb.sum() > 20 and np.all(got[hole_nb]) and np.array_equal(out1[hole_nb, :3], flat[hole_nb])


def test_projection_is_the_written_expression_scalar_by_scalar():
    """a handful of vertices through project(), recomputed one float32 operation at a time"""
    rig = RO.Rig((438.75, 440.25, 240.5, 179.25, 480, 360), (-0.12, 0.05, 0.001, -0.0008, 0.01), tuple(RC.RIG_POSE), 0.9, 2)
    rng = np.random.default_rng(3)
    V = np.concatenate([rng.uniform([-2, -1.5, 0.5], [2, 1.5, 5], (40, 3)), [[np.nan, 0, 1], [0, 0, -1], [np.inf, 0, 1], [3, 3, 1]]]).astype(f32)
    P = RO.project(V, rig)
    R, t = np.asarray(rig.pose12[:9], f32), np.asarray(rig.pose12[9:], f32)
    k1, k2, p1, p2, k3 = [f32(x) for x in rig.dist]
    fx, fy, cx, cy = [f32(x) for x in rig.cam[:4]]
    two = f32(2.0)
    n_ok = 0
    for i, (X, Y, Z) in enumerate(V):
        with np.errstate(all="ignore"):
            kx = f32(f32(f32(R[0] * X) + f32(R[1] * Y)) + f32(R[2] * Z)) + t[0]
            ky = f32(f32(f32(R[3] * X) + f32(R[4] * Y)) + f32(R[5] * Z)) + t[1]
            kz = f32(f32(f32(R[6] * X) + f32(R[7] * Y)) + f32(R[8] * Z)) + t[2]
            ok = bool(np.isfinite([X, Y, Z]).all() and kz > 0)
            x, y = f32(kx / kz), f32(ky / kz)
            r2 = f32(f32(x * x) + f32(y * y))
            ok = ok and bool(r2 <= f32(0.9))
            rad = f32(f32(1.0) + f32(r2 * f32(k1 + f32(r2 * f32(k2 + f32(r2 * k3))))))
            xd = f32(f32(x * rad) + f32(f32(f32(two * p1) * f32(x * y)) + f32(p2 * f32(r2 + f32(two * f32(x * x))))))
            yd = f32(f32(y * rad) + f32(f32(p1 * f32(r2 + f32(two * f32(y * y)))) + f32(f32(two * p2) * f32(x * y))))
            px, py = f32(f32(fx * xd) + cx), f32(f32(fy * yd) + cy)
            ok = ok and bool(np.isfinite(px) and np.isfinite(py) and 0 <= np.floor(px) <= 478 and 0 <= np.floor(py) <= 358)
        assert ok == bool(P["ok"][i]), i
        if ok:
            n_ok += 1
            assert (px, py, kz) == (P["px"][i], P["py"][i], P["z"][i]), i
            assert (P["x0"][i], P["y0"][i]) == (int(np.floor(px)), int(np.floor(py)))
    assert 15 < n_ok < 40 and not P["ok"][-4:].any()


def test_z_buffer_hides_the_far_one_of_two_points_on_one_ray():
    """two points on the colour camera's axis, a wall behind a post: the far one is hidden by the test and coloured without it; a
    point whose own cell holds nothing nearer is visible whatever the tolerance"""
    cam = (100.0, 100.0, 8.0, 6.0, 16, 12)
    img = np.zeros((12, 16, 3), np.uint8)
    img[..., 0] = 200
    V = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [0.02, 0.0, 2.0], [0.05, 0.04, 0.9], [np.nan] * 3], f32)
    out = RO.register(V, img, RO.Rig(cam, cell=2, occl_tol=0.02, occl_tol_z2=0.01))
    # pixel 2 projects one colour pixel beside the post: still the post's cell neighbourhood (the four-cell splat), hidden too
    assert [int(a) for a in out[:, 3]] == [255, 0, 0, 255, 0]
    assert np.all(out[[0, 3], 0] == 200) and np.all(out[[1, 2, 4]] == 0)
    assert np.all(RO.register(V, img, RO.Rig(cam, cell=0))[:4, 3] == 255)
    # within the tolerance 0.02 + 0.01 * 1 of the nearest: visible
    V2 = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.03], [0.0, 0.0, 1.031]], f32)
    assert [int(a) for a in RO.register(V2, img, RO.Rig(cam, cell=2))[:, 3]] == [255, 255, 0]


def test_bilinear_sample_and_quantise_on_a_ramp():
    """an image linear in x and y is reproduced by the bilinear sample up to q()'s rounding"""
    cam = (50.0, 50.0, 10.0, 8.0, 20, 16)
    xx, yy = np.meshgrid(np.arange(20), np.arange(16))
    img = np.stack([10 * xx + 3, 5 * yy + 100, 4 * xx + 6 * yy], -1).astype(np.uint8)
    rng = np.random.default_rng(5)
    V = rng.uniform([-0.15, -0.12, 0.9], [0.15, 0.12, 1.1], (500, 3)).astype(f32)
    out, P, vis = RO.register(V, img, RO.Rig(cam, cell=0), with_info=True)
    assert vis.sum() > 400
    px, py = P["px"][vis].astype(np.float64), P["py"][vis].astype(np.float64)
    want = np.stack([10 * px + 3, 5 * py + 100, 4 * px + 6 * py], -1)
    assert np.all(np.abs(out[vis, :3] - want) <= 0.5 + 1e-3)
    bgr = RO.register(V, img[..., ::-1], RO.Rig(cam, cell=0), order="bgr")
    assert np.array_equal(bgr, out)


def test_render_rgb_with_distortion_inverts_the_forward_model():
    cam, dist = RC.COLOR_CAM, RC.DIST
    rays = S.undistort_rays(cam, dist)
    xd, yd = S.distort(rays[:, 0], rays[:, 1], dist)
    fx, fy, cx, cy, w, h = cam
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    assert np.abs(fx * xd + cx - u.reshape(-1)).max() < 1e-9 and np.abs(fy * yd + cy - v.reshape(-1)).max() < 1e-9
    # dist = None and all zeros: the registered image, bit for bit
    R, t = rot(0.05, -0.1, 0.02), np.array([0.1, -0.05, 0.2])
    assert np.array_equal(S.render_rgb(R, t, SMALL_CAM), S.render_rgb(R, t, SMALL_CAM, dist=(0, 0, 0, 0, 0)))
    assert not np.array_equal(S.render_rgb(R, t, SMALL_CAM), S.render_rgb(R, t, SMALL_CAM, dist=dist))


def _check(fig, want):
    for k in ("occluded_coloured", "visible_dropped"):
        assert fig[k] == want[k], (k, fig)
    for k in ("median", "p95", "p99"):
        assert abs(fig[k] - want[k]) <= 0.01 * max(want[k], 1.0), (k, fig)


def test_registration_figures():
    """the oracle figures behind register_cases.WITH_TEST / WITHOUT_TEST, and the two conditions on the oracle alone"""
    a = RC.registration_figures()
    b = RC.registration_figures(RC.without_test(RC.ROOM_RIG))
    print(f"with the occlusion test: {a}\nwithout: {b}")
    assert (a["valid"], a["in_image"], a["occluded"]) == (RC.VALID, RC.IN_IMAGE, RC.OCCLUDED)
    _check(a, RC.WITH_TEST)
    _check(b, RC.WITHOUT_TEST)
    visible = a["in_image"] - a["occluded"]
    assert a["occluded"] > 300
    assert a["occluded_coloured"] <= RC.MAX_OCCLUDED_COLOURED * a["occluded"]
    assert a["visible_dropped"] <= RC.MAX_VISIBLE_DROPPED * visible
    # what the test buys: without it every occluded pixel is coloured, and the tail of the error shows it
    assert b["occluded_coloured"] == b["occluded"] and b["p99"] > 5 * a["p99"]


def test_accuracy_figures():
    """the oracle figures behind register_cases.ACC_* (the GPU end-to-end test's thresholds) and NAIVE_*"""
    med, p95, cover = RC.oracle_accuracy("rig")
    print(f"registered through the rig: median {med}, p95 {p95}, coverage {cover:.4f}")
    assert np.allclose(med, RC.ORACLE_MEDIAN, atol=2e-3) and np.allclose(p95, RC.ORACLE_P95, atol=2e-2)
    assert abs(cover - RC.ORACLE_COVERAGE) < 2e-3
    nmed, np95, ncover = RC.oracle_accuracy("naive")
    print(f"used as if registered: median {nmed}, p95 {np95}, coverage {ncover:.4f}")
    assert np.allclose(nmed, RC.NAIVE_MEDIAN, atol=0.1) and np.allclose(np95, RC.NAIVE_P95, atol=0.5) and abs(ncover - RC.NAIVE_COVERAGE) < 2e-3
    # the rig brings the separate camera to the registered camera's figures; the naive route is an order of magnitude off
    assert np.all(RC.ORACLE_MEDIAN <= 1.1 * CC.ORACLE_MEDIAN) and np.all(RC.ORACLE_P95 <= 1.1 * CC.ORACLE_P95)
    assert np.all(nmed > 10 * med)


def test_integrate_gate_is_color_integrate_where_alpha_is_set_and_nothing_where_it_is_not():
    p, d, V = _small_frame()
    G = VO.Geometry((40, 32, 60), 0.1, (-2.0, -1.6, 0.0), 0.3, 64)
    rgba = CO.frame_rgba(S.render_rgb(p[:9].reshape(3, 3), p[9:], SMALL_CAM))
    v0, c0, band0 = CO.integrate(G.empty(), CO.empty(G), G, V, rgba, SMALL_CAM, p, with_band=True)
    v1, c1 = RO.integrate(G.empty(), CO.empty(G), G, V, rgba, SMALL_CAM, p)
    assert np.array_equal(c0, c1) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and band0.sum() > 1000
    gated = rgba.copy()
    gated[::3] = 0
    v2, c2, band2 = RO.integrate(G.empty(), CO.empty(G), G, V, gated, SMALL_CAM, p, with_band=True)
    assert np.array_equal(v2.view(np.uint32), v0.view(np.uint32))                    # the tsdf does not look at A
    assert 0.5 * band0.sum() < band2.sum() < 0.8 * band0.sum() and not (band2 & ~band0).any()
    assert np.array_equal(c2[band2], c0[band2]) and np.all(c2[~band2] == 0)
    none = np.zeros_like(rgba)
    assert np.all(RO.integrate(G.empty(), CO.empty(G), G, V, none, SMALL_CAM, p)[1] == 0)


def test_header_and_library_export_the_entry_point():
    hdr = UG.check_entry_points({"rpe_frame_register_color"})
    assert "} rpe_color_rig;" in hdr
    import ctypes as C
    # the ctypes mirror has the C struct's layout: camera 40 bytes, 5 + 12 + 1 doubles, an int padded to 8, 2 doubles
    assert C.sizeof(L.ColorRig) == 40 + 8 * 18 + 8 + 16 and L.ColorRig.cell.offset == 40 + 8 * 18 and L.ColorRig.occl_tol.offset == 40 + 8 * 19


def test_register_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "register_color.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "register_color")])
