"""Scenes shared by the colour tests (CPU oracle and GPU): the textured room of simulator.render_rgb fused at 4 cm from the accuracy
views of tests/volume_cases.py, the colour error of a model colour map against the texture at its vertices, and the oracle's own
figures the GPU accuracy threshold is set from (tests/test_color_oracle.py recomputes them)."""
import numpy as np

import color_oracle as CO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO
from rgbd_pose_estimation_amd import simulator as S


def rgb_at(p, cam):
    """the colour frame registered to volume_cases.depth_at(p, cam)"""
    return S.render_rgb(p[:9].reshape(3, 3), p[9:], cam)


def color_errors(MC, MV):
    """per channel (median, p95) of |model colour - room texture at the model vertex| over the pixels with a known colour, and the
    fraction of the hits (finite vertices) that have one"""
    MC = MC.reshape(-1, 4)
    hit = ~np.isnan(MV).any(1)
    known = hit & (MC[:, 3] == 255)
    err = np.abs(MC[known, :3].astype(np.float64) - S.room_texture(MV[known].astype(np.float64)))
    return np.median(err, 0), np.percentile(err, 95, axis=0), float(known.sum() / max(hit.sum(), 1))


def oracle_color_accuracy(cam=VC.HALF_CAM):
    """the oracle's run of the accuracy case: (median (3,), p95 (3,), coverage)"""
    dims, desc = VC.room_geometry(VC.ACC_VOXEL)
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    vol, cvol = G.empty(), CO.empty(G)
    for k in VC.ACC_VIEWS:
        p = VC.view(k)
        V = FO.frame_maps(VC.depth_at(p, cam), cam, 1.0, *VC.RANGE)[0]
        vol, cvol = CO.integrate(vol, cvol, G, V, CO.frame_rgba(rgb_at(p, cam)), cam, p)
    MV, _ = VO.raycast(vol, G, cam, VC.held_out_pose(), *VC.RAY)
    return color_errors(CO.sample(cvol, G, MV), MV)


# The oracle at HALF_CAM gives, per channel r, g, b: median 0.446 / 0.376 / 0.432, p95 1.36 / 2.74 / 3.28 levels, and a known colour on
# 0.970 of the hits (test_color_oracle.py::test_accuracy_figures recomputes them).  The GPU is bit-exact with the oracle; the margin is
# x1.5 on the errors and -0.02 on the coverage.
ORACLE_MEDIAN = np.array([0.446, 0.376, 0.432])
ORACLE_P95 = np.array([1.36, 2.74, 3.28])
ORACLE_COVERAGE = 0.970
ACC_MEDIAN, ACC_P95, ACC_COVERAGE = 1.5 * ORACLE_MEDIAN, 1.5 * ORACLE_P95, ORACLE_COVERAGE - 0.02
