"""numpy statement of the coarse-to-fine pyramids of include/rgbd_pose_hip.h Part 3 (rpe_frame_set_depth_pyramid,
rpe_model_build_pyramid, rpe_icp_pyramid), the contract the F1p / F2p kernels of csrc/rpe_frontend.hip are held to BIT-EXACTLY.
The per-level maps are oracle/frontend_oracle.py's frame_maps / to_world on each level; this file adds what is new: the level
camera, the depth downsample and the model resize.  Every expression is IEEE fp32 in the written order (the kernels are compiled
without FMA contraction)."""
import numpy as np

from frontend_util import FO

F = np.float32


def level_camera(cam, level):
    """fp64 camera of a level: level 0 is the camera itself, level l >= 1 has f / 2^l and c_l = (c + 0.5) / 2^l - 0.5 (level-l pixel u
    is centred on level-0 coordinate 2^l u + (2^l - 1) / 2)."""
    fx, fy, cx, cy, w, h = cam
    if level == 0:
        return (float(fx), float(fy), float(cx), float(cy), int(w), int(h))
    s = float(1 << level)
    return (fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5, int(w) >> level, int(h) >> level)


def metric_depth(depth, depth_scale, dmin, dmax):
    """level 0: depth * scale in fp32, NaN outside (dmin, dmax)."""
    with np.errstate(invalid="ignore"):
        z = depth.astype(F) * F(depth_scale)
        return np.where((z > F(dmin)) & (z < F(dmax)), z, F(np.nan)).astype(F)


def downsample_depth(z, max_jump):
    """level l -> l+1: c = z[2v, 2u]; NaN if c is NaN, else the mean of the block's valid depths within max_jump of c, summed in the
    order (2v,2u) (2v,2u+1) (2v+1,2u) (2v+1,2u+1) with 0 for an excluded pixel."""
    h, w = z.shape[0] // 2, z.shape[1] // 2
    a, b = z[0:2 * h:2, 0:2 * w:2], z[0:2 * h:2, 1:2 * w:2]
    e, f = z[1:2 * h:2, 0:2 * w:2], z[1:2 * h:2, 1:2 * w:2]
    mj = F(max_jump)
    with np.errstate(invalid="ignore", divide="ignore"):
        keep = [np.abs(x - a) <= mj for x in (a, b, e, f)]          # False for NaN members (and everywhere when a is NaN)
        s = np.where(keep[0], a, F(0))
        for x, k in zip((b, e, f), keep[1:]):
            s = (s + np.where(k, x, F(0))).astype(F)
        cnt = sum(k.astype(np.int32) for k in keep).astype(F)
        out = (s / cnt).astype(F)
    return np.where(np.isnan(a), F(np.nan), out).astype(F)


def depth_pyramid(depth, depth_scale, dmin, dmax, max_jump, levels):
    z = [metric_depth(depth, depth_scale, dmin, dmax)]
    for _ in range(1, levels):
        z.append(downsample_depth(z[-1], max_jump))
    return z


def frame_pyramid(depth, cam, depth_scale, dmin, dmax, max_jump, levels):
    """per level: (metric depth (h_l, w_l), vertex, normal, bearing maps (w_l*h_l, 3))."""
    out = []
    for l, z in enumerate(depth_pyramid(depth, depth_scale, dmin, dmax, max_jump, levels)):
        V, N, B = FO.frame_maps(z, level_camera(cam, l), 1.0, dmin, dmax, max_jump)
        out.append((z, V, N, B))
    return out


def _valid(X):
    return ~np.isnan(X).any(-1)


def resize_model(MV, MN, w, h):
    """model level l (w*h, 3) -> level l+1 (KinectFusion): block a = (2u,2v), b = (2u+1,2v), c = (2u,2v+1), d = (2u+1,2v+1); vertex valid iff
    all four are, value (((a + b) + c) + d) * 0.25; normal valid iff all four are, the same sum over its length (NaN at length 0)."""
    def blocks(X):
        X = X.reshape(h, w, 3)
        hh, ww = h // 2, w // 2
        return (X[0:2 * hh:2, 0:2 * ww:2], X[0:2 * hh:2, 1:2 * ww:2], X[1:2 * hh:2, 0:2 * ww:2], X[1:2 * hh:2, 1:2 * ww:2])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b, c, d = blocks(MV)
        ok = _valid(a) & _valid(b) & _valid(c) & _valid(d)
        V = np.where(ok[..., None], (((a + b) + c) + d) * F(0.25), F(np.nan)).astype(F)
        a, b, c, d = blocks(MN)
        ok = _valid(a) & _valid(b) & _valid(c) & _valid(d)
        s = (((a + b) + c) + d).astype(F)
        ln = np.sqrt(s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1] + s[..., 2] * s[..., 2])
        ok &= ln > F(0)
        N = np.where(ok[..., None], s / ln[..., None], F(np.nan)).astype(F)
    return V.reshape(-1, 3), N.reshape(-1, 3)


def model_pyramid(MV, MN, cam, levels):
    out = [(MV, MN)]
    for l in range(1, levels):
        w, h = level_camera(cam, l - 1)[4:]
        out.append(resize_model(*out[-1], w, h))
    return out
