"""Scenes shared by the colour-registration tests (CPU oracle and GPU): the room seen by a half-resolution depth camera and a
480 x 360 DISTORTED colour camera 50 mm beside it, the truth a registration is judged by (the texture at each depth pixel's vertex, and
whether the colour camera really sees that point: a ray cast from its centre), the end-to-end colour accuracy case of
tests/color_cases.py with every view's colour taken through the rig, and the oracle's own figures the thresholds are set from
(tests/test_register_oracle.py recomputes them)."""
import functools

import numpy as np

import color_cases as CC
import color_oracle as CO
import register_oracle as RO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, pose12, rot
from rgbd_pose_estimation_amd import simulator as S

DEPTH_CAM = VC.HALF_CAM                                           # 320 x 240
COLOR_CAM = (438.75, 438.75, 240.0, 180.0, 480, 360)             # the reference camera at three quarters of its resolution
DIST = (-0.12, 0.05, 0.001, -0.0008, 0.0)
RIG_POSE = pose12(rot(0.01, -0.015, 0.005), np.array([-0.05, 0.004, 0.002]))   # the colour camera 50 mm to the right, turned a little
ROOM_RIG = RO.Rig(COLOR_CAM, DIST, tuple(RIG_POSE), 0.0, 2, 0.02, 0.01)


def without_test(rig):
    return RO.Rig(rig.cam, rig.dist, rig.pose12, rig.r2_max, 0, rig.occl_tol, rig.occl_tol_z2)


def color_pose(p, rig=ROOM_RIG):
    """world -> colour camera (R, t) for the depth camera's pose p"""
    r = np.asarray(rig.pose12, np.float64)
    Rr, tr = r[:9].reshape(3, 3), r[9:]
    return Rr @ p[:9].reshape(3, 3), Rr @ p[9:] + tr


def color_image(p, rig=ROOM_RIG):
    """what the rig's colour camera delivers when the depth camera is at pose p"""
    Rk, tk = color_pose(p, rig)
    return S.render_rgb(Rk, tk, rig.cam, dist=rig.dist)


def world_points(V, p):
    """the depth vertices (camera frame) in the world, float64"""
    return (V.astype(np.float64) - p[9:]) @ p[:9].reshape(3, 3)


def truly_visible(V, p, rig=ROOM_RIG):
    """per depth pixel: does the colour camera see the vertex?  A ray from its centre through the point hits the room's first surface
    at the point itself (within 1 mm), not before it"""
    Rk, tk = color_pose(p, rig)
    Xk = world_points(V, p) @ Rk.T + tk
    ok = np.isfinite(Xk).all(1) & (Xk[:, 2] > 0)
    d = np.where(ok[:, None], Xk / np.where(ok, Xk[:, 2], 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    _, _, lam = S._cast(Rk, tk, rig.cam, None, d)          # one ray per DEPTH pixel from the colour centre (cam is not used then)
    return ok & (lam >= Xk[:, 2] - 1e-3)


def registration_figures(rig=ROOM_RIG, p=None):
    """the room pair: dict of in_image (pixels that project into the colour image), occluded (of those, truly hidden), occluded_coloured,
    visible_dropped, and median / p95 / p99 of |colour - texture at the vertex| over every channel of the coloured pixels"""
    p = VC.view(0) if p is None else p
    V = FO.frame_maps(VC.depth_at(p, DEPTH_CAM), DEPTH_CAM, 1.0, *VC.RANGE)[0]
    rgba, P, _ = RO.register(V, color_image(p, rig), rig, with_info=True)
    got = rgba[:, 3] == 255
    inimg = P["ok"]
    vis = truly_visible(V, p, rig)
    occl = inimg & ~vis
    err = np.abs(rgba[got, :3].astype(np.float64) - S.room_texture(world_points(V[got], p)))
    return dict(valid=int(np.isfinite(V).all(1).sum()), in_image=int(inimg.sum()), occluded=int(occl.sum()),
                occluded_coloured=int((occl & got).sum()), visible_dropped=int((inimg & vis & ~got).sum()),
                median=float(np.median(err)), p95=float(np.percentile(err, 95)), p99=float(np.percentile(err, 99)))


# The oracle on the room pair (view 0; test_register_oracle.py::test_registration_figures recomputes them), with the occlusion test and,
# for what it buys, without (cell 0): of VALID depth pixels, IN_IMAGE project into the colour image and OCCLUDED of those are hidden.
# (An fp64 one-view prototype gave 432 occluded, 970 dropped, 0.47 / 0.79 / 1.6 levels, and a p99 of 30 without the test.)
VALID, IN_IMAGE, OCCLUDED = 76800, 75458, 429
WITH_TEST = dict(occluded_coloured=0, visible_dropped=761, median=0.271, p95=0.676, p99=0.957)
WITHOUT_TEST = dict(occluded_coloured=429, visible_dropped=0, median=0.274, p95=0.698, p99=7.74)
# the conditions a registration must meet, whatever the figures: at most 1 % of the truly occluded pixels coloured, at most 3 % of the
# truly visible in-image pixels dropped
MAX_OCCLUDED_COLOURED, MAX_VISIBLE_DROPPED = 0.01, 0.03


def naive_as_registered(image, cam=DEPTH_CAM):
    """what a user does today: the colour image resized (nearest pixel) to the depth image's size and passed as if it were registered"""
    hc, wc = image.shape[:2]
    u = np.minimum(((np.arange(cam[4]) + 0.5) * wc / cam[4]).astype(np.int64), wc - 1)
    v = np.minimum(((np.arange(cam[5]) + 0.5) * hc / cam[5]).astype(np.int64), hc - 1)
    return np.ascontiguousarray(image[v][:, u])


@functools.lru_cache(maxsize=None)
def accuracy_frames():
    """[(pose, depth, colour camera image)] of the accuracy views (rendered once, shared by the tests)"""
    return [(VC.view(k), VC.depth_at(VC.view(k), DEPTH_CAM), color_image(VC.view(k))) for k in VC.ACC_VIEWS]


def oracle_accuracy(mode="rig"):
    """color_cases.oracle_color_accuracy with every view's colour taken through the rig and fused with the alpha gate ("rig"), or with
    the colour image used as if it were registered ("naive"): (median (3,), p95 (3,), coverage)"""
    cam = DEPTH_CAM
    dims, desc = VC.room_geometry(VC.ACC_VOXEL)
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    vol, cvol = G.empty(), CO.empty(G)
    for p, d, img in accuracy_frames():
        V = FO.frame_maps(d, cam, 1.0, *VC.RANGE)[0]
        rgba = RO.register(V, img, ROOM_RIG) if mode == "rig" else CO.frame_rgba(naive_as_registered(img))
        vol, cvol = RO.integrate(vol, cvol, G, V, rgba, cam, p)
    MV, _ = VO.raycast(vol, G, cam, VC.held_out_pose(), *VC.RAY)
    return CC.color_errors(CO.sample(cvol, G, MV), MV)


# The oracle's end-to-end figures per channel r, g, b (test_register_oracle.py::test_accuracy_figures recomputes them), beside the
# registered camera's of color_cases.py (median 0.446 / 0.376 / 0.432, p95 1.36 / 2.74 / 3.28, coverage 0.970).  The GPU is bit-exact with
# the oracle; the margin is x1.5 on the errors and -0.02 on the coverage, as there.
ORACLE_MEDIAN = np.array([0.457, 0.385, 0.449])
ORACLE_P95 = np.array([1.39, 2.85, 3.38])
ORACLE_COVERAGE = 0.962
ACC_MEDIAN, ACC_P95, ACC_COVERAGE = 1.5 * ORACLE_MEDIAN, 1.5 * ORACLE_P95, ORACLE_COVERAGE - 0.02
# the same run with the colour image used as if it were registered (naive_as_registered): twenty to forty times the error
NAIVE_MEDIAN = np.array([10.7, 20.1, 19.8])
NAIVE_P95 = np.array([44.7, 111.2, 129.6])
NAIVE_COVERAGE = 0.970
