"""Volumes shared by the mesh tests (CPU oracle and GPU): analytic signed distance fields (plane, sphere, torus) sampled at the voxel
centres, a slab with unknown regions, and seeded noise with every awkward value the conventions name.  Each builder returns
(Geometry, volume, volume_init keywords); the volume is (d2, d1, d0, 2) float32, the layout of rpe_volume_download / upload."""
import numpy as np

import volume_oracle as VO

f32 = np.float32


def geometry(dims, voxel_size, origin, trunc=None, max_weight=16):
    trunc = 3 * voxel_size if trunc is None else trunc
    desc = dict(voxel_size=voxel_size, origin=tuple(origin), trunc=trunc, max_weight=max_weight)
    return VO.Geometry(dims, voxel_size, origin, trunc, max_weight), desc


def sdf_volume(G, sdf, weight=1.0):
    """tsdf = clip(sdf / tr, -1, 1) at the voxel centres (sdf evaluated in float64), every weight `weight`"""
    px, py, pz = [c.astype(np.float64) for c in VO.voxel_centres(G)]
    vol = G.empty()
    vol[..., 0] = np.clip(sdf(px, py, pz) / float(G.tr), -1.0, 1.0)
    vol[..., 1] = weight
    return vol


SPHERE_R = 0.5
TORUS_R, TORUS_r = 0.42, 0.16
PLANE_N, PLANE_D = np.array([0.2, -0.35, 1.0]) / np.linalg.norm([0.2, -0.35, 1.0]), 0.07


def sphere():
    G, desc = geometry((30, 28, 26), 0.05, (-0.76, -0.69, -0.66))
    return G, sdf_volume(G, lambda x, y, z: np.sqrt(x * x + y * y + z * z) - SPHERE_R), desc


def torus():
    G, desc = geometry((34, 33, 17), 0.04, (-0.67, -0.65, -0.33))
    return G, sdf_volume(G, lambda x, y, z: np.sqrt((np.sqrt(x * x + y * y) - TORUS_R) ** 2 + z * z) - TORUS_r), desc


def plane():
    """the plane n . p = d, free side n . p > d"""
    G, desc = geometry((20, 18, 22), 0.05, (-0.5, -0.45, -0.55))
    return G, sdf_volume(G, lambda x, y, z: PLANE_N[0] * x + PLANE_N[1] * y + PLANE_N[2] * z - PLANE_D), desc


def slab():
    """a tilted plane with a box of unobserved voxels (weight 0) and a patch of weight 1 among weight 3"""
    G, vol, desc = plane()
    vol[..., 1] = 3.0
    vol[5:14, 4:9, 6:12] = 0.0              # unknown: tsdf and weight 0
    vol[:, 10:16, 12:18, 1] = 1.0           # seen once: filtered by min_weight > 1
    return G, vol, desc


def noise(dims=(23, 17, 19), seed=11):
    """uniform tsdf in [-1, 1] with 8 % exact zeros (both signs), 3 % NaN, 2 % +-Inf; weights from {-1, 0, 0.5, 1, 2, 7} (mostly >= 1)"""
    rng = np.random.default_rng(seed)
    G, desc = geometry(dims, 0.03, (-0.3, -0.2, 0.1))
    vol = G.empty()
    n = vol[..., 0].size
    t = rng.uniform(-1, 1, n).astype(f32)
    u = rng.random(n)
    t[u < 0.04] = f32(0.0)
    t[(u >= 0.04) & (u < 0.08)] = f32(-0.0)
    t[(u >= 0.08) & (u < 0.11)] = np.nan
    t[(u >= 0.11) & (u < 0.12)] = np.inf
    t[(u >= 0.12) & (u < 0.13)] = -np.inf
    w = rng.choice(np.array([-1, 0, 0.5, 1, 2, 7], f32), n, p=[0.02, 0.03, 0.05, 0.3, 0.3, 0.3])
    vol[..., 0] = t.reshape(vol.shape[:3])
    vol[..., 1] = w.reshape(vol.shape[:3])
    return G, vol, desc


def mesh_edges(T):
    """(undirected edges with their triangle counts, directed edges) of a triangle list"""
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    und, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    return und, cnt, d


def euler(V, T):
    und, _, _ = mesh_edges(T)
    return len(V) - len(und) + len(T)


def face_normals(V, T):
    P = V.astype(np.float64)
    return np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
