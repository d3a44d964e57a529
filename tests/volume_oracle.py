"""numpy statement of the TSDF volume of include/rgbd_pose_hip.h Part 3 (rpe_volume_integrate, rpe_volume_raycast), the contract the
V1 / V2 kernels of csrc/rpe_volume.hip are held to BIT-EXACTLY.  Vectorised over voxels (integrate) and over rays (raycast); every
intermediate is IEEE fp32 in the written order (the kernels are compiled without FMA contraction).  A volume is an array of shape
(d2, d1, d0, 2): [..., 0] = tsdf, [..., 1] = weight, the layout rpe_volume_download returns."""
import numpy as np

from frontend_util import FO

F = np.float32


class Geometry:
    """the descriptor's doubles cast to fp32 once"""

    def __init__(self, dims, voxel_size, origin, trunc, max_weight):
        self.dim = tuple(int(d) for d in dims)
        self.o = np.asarray(origin, np.float64).astype(F)
        self.s, self.tr, self.W = F(voxel_size), F(trunc), F(max_weight)

    def empty(self):
        d0, d1, d2 = self.dim
        return np.zeros((d2, d1, d0, 2), F)


def voxel_centres(G, k0=0, k1=None):
    """per axis: o + ((float)i + 0.5f) * s, shaped to broadcast over (k1 - k0, d1, d0): the z-slab window [k0, k1) of the volume"""
    k1 = G.dim[2] if k1 is None else k1
    c = [G.o[a] + (np.arange(G.dim[a], dtype=F) + F(0.5)) * G.s for a in range(2)]
    c.append(G.o[2] + (np.arange(k0, k1).astype(F) + F(0.5)) * G.s)
    return c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]


def integrate(vol, G, V, cam, pose12, k0=0, with_mask=False):
    """V1: a new volume with the frame (level-0 vertex map V, (h*w, 3)) of camera cam fused in under pose12 (Xc = R Xw + t).
    vol may be the z-slab window [k0, k0 + len(vol)) of the volume; with_mask also returns the updated voxels (d2, d1, d0) bool."""
    fx, fy, cx, cy, w, h = FO._cam(cam)
    R, t = FO._pose_f(pose12)
    px, py, pz = voxel_centres(G, k0, k0 + vol.shape[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qx = R[0] * px + R[1] * py + R[2] * pz + t[0]
        qy = R[3] * px + R[4] * py + R[5] * pz + t[1]
        qz = R[6] * px + R[7] * py + R[8] * pz + t[2]
        ok = qz > F(0)
        uf = np.floor(fx * (qx / qz) + cx + F(0.5))
        vf = np.floor(fy * (qy / qz) + cy + F(0.5))
        ok &= (uf >= F(0)) & (uf <= F(w - 1)) & (vf >= F(0)) & (vf <= F(h - 1))
        j = np.where(ok, vf, F(0)).astype(np.int64) * w + np.where(ok, uf, F(0)).astype(np.int64)
        d = V[j, 2]
        ok &= ~np.isnan(d)
        sdf = d - qz
        ok &= sdf >= -G.tr
        f = np.fmin(F(1.0), sdf / G.tr)                          # fminf: a NaN operand gives the other one
        ts, wt = vol[..., 0], vol[..., 1]
        nts = (ts * wt + f) / (wt + F(1.0))
        nwt = np.fmin(wt + F(1.0), G.W)                          # a NaN weight becomes W
    out = vol.copy()
    out[..., 0] = np.where(ok, nts, ts)
    out[..., 1] = np.where(ok, nwt, wt)
    return (out, ok) if with_mask else out


def _lerp(x, y, t):
    return x + (y - x) * t


def cell(G, X):
    """the cell of world points X (n, 3) fp32: g = (p - o) / s - 0.5f, i0 = floorf(g), a = g - i0 per axis; (in range (n,), [i0 per axis]
    as fp32, [a per axis]) -- in range iff 0 <= i0 <= dim - 2 on every axis"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(X[:, a] - G.o[a]) / G.s - F(0.5) for a in range(3)]
        i0 = [np.floor(x) for x in g]
        ok = np.ones(len(X), bool)
        for a in range(3):
            ok &= (i0[a] >= F(0)) & (i0[a] <= F(G.dim[a] - 2))
        return ok, i0, [g[a] - i0[a] for a in range(3)]


def field(vol, G, X, k0=0):
    """F at world points X (n, 3): (value (n,), known (n,)).  vol may be the z-slab window [k0, k0 + len(vol)) of the volume, every
    voxel outside it unobserved (weight 0): a point whose cell reaches outside the window is unknown."""
    d0, d1, d2 = G.dim
    ok, i0, (ax, ay, az) = cell(G, X)
    with np.errstate(invalid="ignore"):
        ok &= (i0[2] >= F(k0)) & (i0[2] <= F(k0 + vol.shape[0] - 2))
    i, j, k =[np.where(ok, i0[a], F(0)).astype(np.int64) for a in range(3)]
    k = np.where(ok, k - k0, 0)
    flat = vol.reshape(-1, 2)
    base = (k * d1 + j) * d0 + i
    v = {}
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                v[di, dj, dk] = flat[base + di + dj * d0 + dk * d0 * d1]
    for c in v.values():
        ok &= c[:, 1] > F(0)
    t = {key: c[:, 0] for key, c in v.items()}
    c00, c10 = _lerp(t[0, 0, 0], t[1, 0, 0], ax), _lerp(t[0, 1, 0], t[1, 1, 0], ax)
    c01, c11 = _lerp(t[0, 0, 1], t[1, 0, 1], ax), _lerp(t[0, 1, 1], t[1, 1, 1], ax)
    c0, c1 = _lerp(c00, c10, ay), _lerp(c01, c11, ay)
    return _lerp(c0, c1, az), ok


def windows_field(windows, G, X):
    """F at X of a volume held as z-slab windows [(k0, vol), ...], unobserved (weight 0) outside them"""
    val, known = np.zeros(len(X), F), np.zeros(len(X), bool)
    for k0, vol in windows:
        v, kn = field(vol, G, X, k0)
        val = np.where(kn, v, val)
        known |= kn
    return val, known


def raycast(vol, G, cam, pose12, dmin, dmax):
    """V2: world vertex and normal maps ((h*w, 3) each) of the view pose12 with camera cam over camera depths (dmin, dmax).  vol is
    the volume or a list of its z-slab windows [(k0, slab), ...], unobserved outside them."""
    fld = (lambda X: windows_field(vol, G, X)) if isinstance(vol, list) else (lambda X: field(vol, G, X))
    fx, fy, cx, cy, w, h = FO._cam(cam)
    R, t = FO._pose_f(pose12)
    xn = np.broadcast_to(((np.arange(w, dtype=F) - cx) / fx)[None, :], (h, w)).reshape(-1)
    yn = np.broadcast_to(((np.arange(h, dtype=F) - cy) / fy)[:, None], (h, w)).reshape(-1)
    n = w * h
    zh = np.full(n, np.nan, F)
    live = np.arange(n)
    prev = np.zeros(n, bool)
    Fp, zp = np.zeros(n, F), np.zeros(n, F)
    s, lo, hi = G.s, F(dmin), F(dmax)
    k = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while live.size:
            z = lo + F(k) * s
            if not z < hi:
                break
            X = FO._to_world(R, t, np.stack([xn[live] * z, yn[live] * z, np.full(live.size, z, F)], -1))
            Fk, known = fld(X)
            hit = known & prev[live] & (Fp[live] > F(0)) & (Fk <= F(0))
            hl = live[hit]
            zh[hl] = zp[hl] + s * (Fp[hl] / (Fp[hl] - Fk[hit]))
            prev[live], Fp[live], zp[live] = known, Fk, z
            live = live[~hit]
            k += 1
        ok = ~np.isnan(zh)
        MV = np.full((n, 3), np.nan, F)
        MN = np.full((n, 3), np.nan, F)
        idx = np.nonzero(ok)[0]
        z = zh[idx]
        P = FO._to_world(R, t, np.stack([xn[idx] * z, yn[idx] * z, z], -1)).astype(F)
        MV[idx] = P
        samples = []
        for a in range(3):
            for sign in (1, -1):
                Q = P.copy()
                Q[:, a] = P[:, a] + s if sign > 0 else P[:, a] - s
                samples.append(fld(Q))
        good = np.ones(len(idx), bool)
        for _, kn in samples:
            good &= kn
        gx, gy, gz = [samples[2 * a][0] - samples[2 * a + 1][0] for a in range(3)]
        ln = np.sqrt(gx * gx + gy * gy + gz * gz)
        good &= ln > F(0)
        N = np.stack([gx / ln, gy / ln, gz / ln], -1)
        MN[idx] = np.where(good[:, None], N, F(np.nan))
    return MV, MN
