"""numpy statement of the depth filter of include/rgbd_pose_hip.h Part 3 (rpe_frame_set_filter), the contract the F0 kernel of
csrc/rpe_filter.hip is held to BIT-EXACTLY.  Every expression is IEEE fp32 in the written order (the kernel is compiled without FMA
contraction); the spatial weights are made in double with libm's exp, which is Python's math.exp.  What follows the filter is the
existing statement: oracle/frontend_oracle.py's frame_maps and pyramid_oracle.py's pyramid on the filtered depth, float32 with scale 1."""
import math

import numpy as np

import pyramid_oracle as PO
from frontend_util import FO

F = np.float32
MAX_RADIUS = 4


def spatial_weights(radius, sigma_space):
    """ws[dy + r][dx + r] = (float)exp(-(double)(dx*dx + dy*dy) / (2 * sigma_space * sigma_space)), (2r + 1) x (2r + 1) float32."""
    r, s = int(radius), float(sigma_space)
    ws = np.empty((2 * r + 1, 2 * r + 1), F)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ws[dy + r, dx + r] = F(math.exp(-float(dx * dx + dy * dy) / (2 * s * s)))
    return ws


def bilateral(m, radius, sigma_space, depth_cut, depth_cut_z2):
    """m: metric depth (h, w) float32, NaN = invalid.  Per pixel with centre c: NaN stays NaN; cut = a + b * (c * c), inv = 1 / cut; over
    dy = -r .. r (outer), dx = -r .. r (inner), neighbours d inside the image: x = ((d - c) * inv)^2, counted iff x < 1 with
    wgt = ws * ((1 - x) * (1 - x)), num += wgt * d, den += wgt; out = num / den."""
    r = int(radius)
    a, b = F(depth_cut), F(depth_cut_z2)
    ws = spatial_weights(r, sigma_space)
    m = np.asarray(m, F)
    h, w = m.shape
    c = m
    pad = np.full((h + 2 * r, w + 2 * r), np.nan, F)      # a neighbour outside the image never counts: NaN fails x < 1
    pad[r:r + h, r:r + w] = m
    one = F(1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cut = (a + b * (c * c)).astype(F)
        inv = (one / cut).astype(F)
        num, den = np.zeros((h, w), F), np.zeros((h, w), F)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                d = pad[r + dy:r + dy + h, r + dx:r + dx + w]
                t = ((d - c) * inv).astype(F)
                x = (t * t).astype(F)
                keep = x < one
                wr = ((one - x) * (one - x)).astype(F)
                wgt = (ws[dy + r, dx + r] * wr).astype(F)
                num = np.where(keep, (num + (wgt * d).astype(F)).astype(F), num)
                den = np.where(keep, (den + wgt).astype(F), den)
        out = np.where(np.isnan(c), F(np.nan), (num / den).astype(F)).astype(F)
    assert out.dtype == F and num.dtype == F and den.dtype == F
    return out


def filtered_depth(depth, depth_scale, dmin, dmax, filt):
    """raw depth (uint16 or float32) -> the filtered metric depth of level 0; filt = (radius, sigma_space, depth_cut, depth_cut_z2)"""
    return bilateral(PO.metric_depth(depth, depth_scale, dmin, dmax), *filt)


def frame_maps(depth, cam, depth_scale, dmin, dmax, max_jump, filt):
    """rpe_frame_set_depth with the filter on: F1 on the filtered depth (float32, scale 1; (dmin, dmax) applied again)."""
    return FO.frame_maps(filtered_depth(depth, depth_scale, dmin, dmax, filt), cam, 1.0, dmin, dmax, max_jump)


def frame_pyramid(depth, cam, depth_scale, dmin, dmax, max_jump, levels, filt):
    """rpe_frame_set_depth_pyramid with the filter on: per level (metric depth, vertex, normal, bearing)."""
    return PO.frame_pyramid(filtered_depth(depth, depth_scale, dmin, dmax, filt), cam, 1.0, dmin, dmax, max_jump, levels)
