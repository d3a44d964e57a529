"""numpy statement of the colour half of the TSDF volume of include/rgbd_pose_hip.h Part 3 ("Colour": rpe_frame_set_color,
rpe_volume_integrate_color, rpe_model_sample_color, rpe_volume_mesh_colors), the contract the C1-C3 kernels of csrc/rpe_color.hip are
held to BIT-EXACTLY.  Every intermediate is IEEE fp32 in the written order.  A colour volume is an array of shape (d2, d1, d0, 4) of
binary16 BIT PATTERNS (uint16): [..., :3] = r, g, b, [..., 3] = the colour weight wc; Context.volume_color_download returns the same
bits as float16.  A frame colour is (h*w, 4) uint8 RGBA, as the device holds it.  Like tests/volume_oracle.py, integrate and the field
can run on a z-slab window [k0, k0 + len(vol)) of a larger volume."""
import numpy as np

import volume_oracle as VO
from frontend_util import FO

F = np.float32
QNAN16 = np.uint16(0x7E00)


def h(x):
    """fp32 -> binary16 bits: round to nearest even, subnormals kept, overflow to +-Inf, every NaN to the quiet NaN 0x7e00"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        b = x.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(x), QNAN16, b).astype(np.uint16)


def f32(bits):
    """binary16 bits -> fp32 (exact)"""
    return np.asarray(bits, np.uint16).view(np.float16).astype(F)


def empty(G):
    d0, d1, d2 = G.dim
    return np.zeros((d2, d1, d0, 4), np.uint16)


def frame_rgba(rgb, order="rgb"):
    """C1: (h, w, 3) uint8 in `order` -> (h*w, 4) uint8 RGBA with A = 255"""
    a = np.asarray(rgb, np.uint8).reshape(-1, 3)
    if order == "bgr":
        a = a[:, ::-1]
    return np.concatenate([a, np.full((len(a), 1), 255, np.uint8)], 1)


def blend(c, wc, o, W):
    """one observation o (n, 3) fp32 blended into the colours c (n, 3) of weight wc (n,), all fp32: the new (colour, weight) as
    binary16 bits"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nc = h((c * wc[:, None] + o) / (wc[:, None] + F(1.0)))
        nw = h(np.fmin(wc + F(1.0), W))                          # fminf: a NaN weight becomes W
    return nc, nw


def integrate(vol, cvol, G, V, rgba, cam, pose12, k0=0, with_band=False):
    """C2: (tsdf volume, colour volume) with the frame (level-0 vertex map V (h*w, 3), colour rgba (h*w, 4)) fused in under pose12.
    The tsdf half is volume_oracle.integrate's; the colour half recomputes sdf and the pixel of each updated voxel and blends the band
    voxels (sdf <= tr).  vol / cvol may be the z-slab window [k0, k0 + len(vol)) of the volume."""
    out, up = VO.integrate(vol, G, V, cam, pose12, k0, with_mask=True)
    fx, fy, cx, cy, w, h_ = FO._cam(cam)
    R, t = FO._pose_f(pose12)
    px, py, pz = VO.voxel_centres(G, k0, k0 + vol.shape[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qx = R[0] * px + R[1] * py + R[2] * pz + t[0]
        qy = R[3] * px + R[4] * py + R[5] * pz + t[1]
        qz = R[6] * px + R[7] * py + R[8] * pz + t[2]
        uf = np.floor(fx * (qx / qz) + cx + F(0.5))
        vf = np.floor(fy * (qy / qz) + cy + F(0.5))
        j = np.where(up, vf, F(0)).astype(np.int64) * w + np.where(up, uf, F(0)).astype(np.int64)
        sdf = V[j, 2] - qz
        band = up & (sdf <= G.tr)
        o = rgba[j[band], :3].astype(F)
        c = f32(cvol[band][:, :3])
        wc = f32(cvol[band][:, 3])
        nc, nw = blend(c, wc, o, G.W)
    cout = cvol.copy()
    sel = cout[band]
    sel[:, :3] = nc
    sel[:, 3] = nw
    cout[band] = sel
    return (out, cout, band) if with_band else (out, cout)


def color_field(cvol, G, X, k0=0):
    """C at world points X (n, 3): (r, g, b (n, 3) fp32, known (n,)).  F's g, i0, a and in-range rule; known iff in range and all 8
    corner colour weights are > 0; F's lerp order per channel.  cvol may be the z-slab window [k0, k0 + len(cvol)), every voxel outside
    it without colour."""
    d0, d1, d2 = G.dim
    X = np.asarray(X, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(X[:, a] - G.o[a]) / G.s - F(0.5) for a in range(3)]
        i0 = [np.floor(x) for x in g]
        ok = np.ones(len(X), bool)
        for a in range(3):
            ok &= (i0[a] >= F(0)) & (i0[a] <= F(G.dim[a] - 2))
        ok &= (i0[2] >= F(k0)) & (i0[2] <= F(k0 + cvol.shape[0] - 2))
        ax, ay, az = [g[a] - i0[a] for a in range(3)]
    i, j, k = [np.where(ok, i0[a], F(0)).astype(np.int64) for a in range(3)]
    k = np.where(ok, k - k0, 0)
    flat = cvol.reshape(-1, 4)
    base = (k * d1 + j) * d0 + i
    v = {}
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                v[di, dj, dk] = f32(flat[base + di + dj * d0 + dk * d0 * d1])
    for c in v.values():
        ok &= c[:, 3] > F(0)
    lerp = VO._lerp
    with np.errstate(invalid="ignore", over="ignore"):
        t = {key: c[:, :3] for key, c in v.items()}
        ax, ay, az = ax[:, None], ay[:, None], az[:, None]
        c00, c10 = lerp(t[0, 0, 0], t[1, 0, 0], ax), lerp(t[0, 1, 0], t[1, 1, 0], ax)
        c01, c11 = lerp(t[0, 0, 1], t[1, 0, 1], ax), lerp(t[0, 1, 1], t[1, 1, 1], ax)
        c0, c1 = lerp(c00, c10, ay), lerp(c01, c11, ay)
        rgb = lerp(c0, c1, az)
    return rgb, ok


def quantise(x):
    """q(x) = (uint8)floorf(fminf(fmaxf(x, 0.0f), 255.0f) + 0.5f): NaN gives 0, +Inf 255"""
    x = np.asarray(x, F)
    return np.floor(np.fmin(np.fmax(x, F(0.0)), F(255.0)) + F(0.5)).astype(np.uint8)


def sample(cvol, G, X, k0=0):
    """C3: (n, 4) uint8 RGBA of C at X: (q(r), q(g), q(b), 255) where known, (0, 0, 0, 0) where unknown or at a NaN point"""
    rgb, known = color_field(cvol, G, X, k0)
    out = np.zeros((len(known), 4), np.uint8)
    out[known, :3] = quantise(rgb[known])
    out[known, 3] = 255
    return out


def windows_sample(windows, G, X):
    """C3 at X of a colour volume held as z-slab windows [(k0, cvol), ...], no colour outside them"""
    out = np.zeros((len(X), 4), np.uint8)
    for k0, cvol in windows:
        _, known = color_field(cvol, G, X, k0)
        out[known] = sample(cvol, G, X[known], k0)
    return out
