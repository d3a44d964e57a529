"""numpy statement of the mesh extraction of include/rgbd_pose_hip.h Part 3 (rpe_volume_mesh), the contract the kernels of
csrc/rpe_mesh.hip are held to BIT-EXACTLY.  Vectorised over voxels; every intermediate is IEEE fp32 in the written order.  A volume is
an array of shape (d2, d1, d0, 2), the layout rpe_volume_download returns; the triangle tables come from scripts/gen_mc_tables.py."""
import importlib.util
import os

import numpy as np

import volume_oracle as VO

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "scripts", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
_TRIS, TRI_COUNT, MAX_TRIS = GEN.tables()
TRI_COUNT = np.array(TRI_COUNT, np.int64)
TRI_EDGES = np.full((256, MAX_TRIS, 3), -1, np.int64)
for _c, _t in enumerate(_TRIS):
    if _t:
        TRI_EDGES[_c, : len(_t)] = _t
EDGE_OWNER = np.array(GEN.OWNER, np.int64)         # corner n = di + 2 dj + 4 dk of the owner voxel
EDGE_AXIS = np.array(GEN.AXIS, np.int64)


def _shift(a, d):
    """a[k - dk, j - dj, i - di] for d = (di, dj, dk) >= 0, zero where that leaves the array"""
    di, dj, dk = d
    out = np.zeros_like(a)
    d2, d1, d0 = a.shape
    out[dk:, dj:, di:] = a[: d2 - dk, : d1 - dj, : d0 - di]
    return out


def cases(vol, wmin):
    """per voxel (d2, d1, d0) uint8: the case of the cube it is corner 0 of; 0 where the cube is inactive or does not exist"""
    d2, d1, d0 = vol.shape[:3]
    ts, w = vol[..., 0], vol[..., 1]
    with np.errstate(invalid="ignore"):
        known = (w >= F(wmin)) & np.isfinite(ts)
        inside = ts <= F(0)
    c = np.zeros((d2, d1, d0), np.int64)
    if min(d0, d1, d2) < 2:
        return c.astype(np.uint8)
    act = np.ones((d2 - 1, d1 - 1, d0 - 1), bool)
    m = np.zeros((d2 - 1, d1 - 1, d0 - 1), np.int64)
    for n in range(8):
        di, dj, dk = n & 1, (n >> 1) & 1, (n >> 2) & 1
        sl = (slice(dk, d2 - 1 + dk), slice(dj, d1 - 1 + dj), slice(di, d0 - 1 + di))
        act &= known[sl]
        m |= inside[sl].astype(np.int64) << n
    c[:-1, :-1, :-1] = np.where(act, m, 0)
    return c.astype(np.uint8)


def used_edges(case):
    """per voxel: bit a set iff the voxel's edge along axis a carries a vertex (crossed and in an active cube)"""
    c = case.astype(np.int64)
    used = np.zeros(case.shape, np.int64)
    for e in range(12):
        a, b = GEN.EDGES[e]
        o = EDGE_OWNER[e]
        d = (o & 1, (o >> 1) & 1, (o >> 2) & 1)
        diff = (((c >> a) ^ (c >> b)) & 1).astype(bool)        # the edge crossed, seen from this cube
        used |= _shift(diff, d).astype(np.int64) << EDGE_AXIS[e]  # ... marked at its owner voxel
    return used.astype(np.uint8)


def mesh(vol, G, min_weight=1.0, k0=0, id0=0):
    """(vertices (V, 3) f32, normals (V, 3) f32, triangles (T, 3) int32) of rpe_volume_mesh.  vol may be the z-slab window
    [k0, k0 + len(vol)) of a volume whose slabs k0 - 1 and k0 + len(vol) (where they exist) are unobserved: then no active cube
    reaches outside it, and the window's part of the mesh is this one, with its vertex ids starting at id0 (the vertices of the slabs
    before k0)."""
    d0, d1 = G.dim[:2]
    case = cases(vol, min_weight)
    used = used_edges(case)
    flat_used = used.reshape(-1).astype(np.int64)
    bits = ((flat_used[:, None] >> np.arange(3)) & 1).astype(bool)     # (nvox, 3)
    vox, axis = np.nonzero(bits)                                        # voxel order, then axis: the vertex order
    ts = vol.reshape(-1, 2)[:, 0]
    strides = np.array([1, d0, d0 * d1], np.int64)
    i, j, k = vox % d0, (vox // d0) % d1, vox // (d0 * d1) + k0
    ijk = np.stack([i, j, k], -1)
    Fa, Fb = ts[vox], ts[vox + strides[axis]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = Fa / (Fa - Fb)
        P = np.empty((len(vox), 3), F)
        for a in range(3):
            centre = G.o[a] + (ijk[:, a].astype(F) + F(0.5)) * G.s
            along = G.o[a] + ((ijk[:, a].astype(F) + F(0.5)) + t) * G.s
            P[:, a] = np.where(axis == a, along, centre)
        N = normals(vol, G, P, k0)
    counts = bits.sum(1)
    first = id0 + np.cumsum(counts) - counts                            # first vertex id per voxel
    ntri = TRI_COUNT[case.reshape(-1)]
    cube = np.repeat(np.arange(ntri.size), ntri)
    r = np.arange(cube.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    edges = TRI_EDGES[case.reshape(-1)[cube], r]                        # (T, 3)
    o = EDGE_OWNER[edges]
    owner = cube[:, None] + (o & 1) + ((o >> 1) & 1) * d0 + ((o >> 2) & 1) * d0 * d1
    ax = EDGE_AXIS[edges]
    lower = flat_used[owner] & ((1 << ax) - 1)
    ids = first[owner] + (lower & 1) + ((lower >> 1) & 1)
    assert ids.size == 0 or ids.max() < 2 ** 31
    return P, N, ids.astype(np.int32).reshape(-1, 3)


def normals(vol, G, P, k0=0):
    """the raycast's model normal at P: central differences of F over +- s per axis, normalised; NaN if a sample is unknown or the
    length is 0.  vol may be a z-slab window from k0, unobserved outside (volume_oracle.field)."""
    s = G.s
    samples = []
    for a in range(3):
        for sign in (1, -1):
            Q = P.copy()
            Q[:, a] = P[:, a] + s if sign > 0 else P[:, a] - s
            samples.append(VO.field(vol, G, Q, k0))
    good = np.ones(len(P), bool)
    for _, kn in samples:
        good &= kn
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gx, gy, gz = [samples[2 * a][0] - samples[2 * a + 1][0] for a in range(3)]
        ln = np.sqrt(gx * gx + gy * gy + gz * gz)
        good &= ln > F(0)
        N = np.stack([gx / ln, gy / ln, gz / ln], -1).astype(F)
    return np.where(good[:, None], N, F(np.nan)).astype(F)
