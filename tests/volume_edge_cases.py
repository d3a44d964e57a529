"""Edge cases of the TSDF volume and the mesh, shared by the CPU oracle tests and the GPU tests: each tie of the written conventions
built exactly (an axis-aligned pose, a voxel size of 0.25, dyadic origins and pixel-centred principal points, so that every voxel
centre, pixel coordinate and sample is exact in fp32), the lane tails of integrate, volumes filled with awkward bits, the chunk counts
of the mesh scan, the large volume's windows and the maximum volume's checkerboard."""
import numpy as np

import mesh_cases as MC
import volume_oracle as VO
from frontend_util import FO, pose12

f32 = np.float32
IDENTITY = pose12(np.eye(3), np.zeros(3))
S = 0.25                                   # voxel size and raycast step of the tie cases
W_BITS = np.array([0x7fc00000, 0x7f800001, 0x7fa00005, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff],
                  np.uint32)              # qNaN, sNaN, sNaN with payload, negative qNaN with payload, +Inf, -Inf, -0, denormals


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- integrate ties
# dims (11, 10, 14), origin (-1.125, -1.125, -0.625), s = 0.25, tr = 0.75, identity pose: voxel centres x = y = -1 + 0.25 i,
# z = -0.5 + 0.25 k, and the camera point is the centre itself.  Camera 8 x 8, f = 4, c = 3.5: pixel coordinate 4 x / z + 3.5.
# Depth 1.0 on rows 0..3, 1.5 on rows 4..7 (float metres, scale 1).
TIE_CAM = (4.0, 4.0, 3.5, 3.5, 8, 8)
TIE_RANGE = (0.25, 4.0, 10.0)


def integrate_ties(max_weight=16):
    G, desc = MC.geometry((11, 10, 14), S, (-1.125, -1.125, -0.625), trunc=3 * S, max_weight=max_weight)
    depth = np.full((8, 8), 1.0, f32)
    depth[4:] = 1.5
    return G, desc, depth


def centre(G, i, j, k):
    return tuple(float(G.o[a] + (f32(x) + f32(0.5)) * G.s) for a, x in enumerate((i, j, k)))


# name -> (voxel (i, j, k), (tsdf, weight) after one frame into the zero volume, or None where the voxel is skipped), by hand:
#   u_minus_half: x = -1, z = 1: pixel coordinate 4 * -1 + 3.5 = -0.5 exactly, floor(0) = column 0 is in; depth 1, sdf 0
#   u_w_minus_half: x = 1, z = 1: 7.5 = w - 0.5, floor(8) = column 8 is out
#   v_minus_half / v_h_minus_half: the same on y (z = 1: row 0 has depth 1; row 8 is out)
#   z_zero: k = 2, the camera z is 0 (not > 0): skipped
#   sdf_zero: z = 1 on a row of depth 1: sdf 0, f = 0, tsdf 0
#   sdf_minus_tr: z = 1.75 on depth 1: sdf = -0.75 = -tr is kept, f = -1;   sdf_below_minus_tr: z = 2 on depth 1: skipped
#   sdf_minus_tr_far: z = 2.25 on depth 1.5: sdf = -tr again, f = -1
#   f_one: z = 0.25, y = -0.25 (row coordinate -0.5: row 0, depth 1): sdf / tr = 1 exactly
#   f_clamped: z = 0.25, y = 0 (row coordinate 3.5: row 4, depth 1.5): sdf / tr = 5/3 > 1, f = 1
INTEGRATE_TIES = {
    "u_minus_half": ((0, 3, 6), (0.0, 1.0)),
    "u_w_minus_half": ((8, 3, 6), None),
    "v_minus_half": ((4, 0, 6), (0.0, 1.0)),
    "v_h_minus_half": ((4, 8, 6), None),
    "z_zero": ((4, 3, 2), None),
    "sdf_zero": ((4, 2, 6), (0.0, 1.0)),
    "sdf_minus_tr": ((4, 2, 9), (-1.0, 1.0)),
    "sdf_below_minus_tr": ((4, 2, 10), None),
    "sdf_minus_tr_far": ((4, 6, 11), (-1.0, 1.0)),
    "f_one": ((4, 3, 3), (1.0, 1.0)),
    "f_clamped": ((4, 4, 3), (1.0, 1.0)),
}


def pixel_coord(G, i, j, k):
    """(u, v) pixel coordinates fx * x / z + cx of voxel (i, j, k) of integrate_ties, in fp32 as the convention has them"""
    x, y, z = [f32(c) for c in centre(G, i, j, k)]
    fx, fy, cx, cy, _, _ = FO._cam(TIE_CAM)
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(fx * (x / z) + cx), f32(fy * (y / z) + cy)


def tie_counts(G, vol_after):
    """how often each tie occurs over the whole volume (fp32, as the convention computes it): pixel coordinates of exactly -0.5 or
    size - 0.5, camera z of exactly 0, sdf of exactly 0 or -tr, sdf / tr of exactly 1 and above 1 among the updated voxels"""
    px, py, pz = VO.voxel_centres(G)
    px, py, pz = np.broadcast_arrays(px, py, pz)
    fx, fy, cx, cy, w, h = FO._cam(TIE_CAM)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * (px / pz) + cx, fy * (py / pz) + cy
        depth = np.where(v < f32(3.5), f32(1.0), f32(1.5))
        sdf = depth - pz
    up = vol_after[..., 1] > 0
    return {"u_minus_half": int((u == f32(-0.5)).sum()), "u_w_minus_half": int((u == f32(w - 0.5)).sum()),
            "v_minus_half": int((v == f32(-0.5)).sum()), "v_h_minus_half": int((v == f32(h - 0.5)).sum()),
            "z_zero": int((pz == 0).sum()), "sdf_zero": int((up & (sdf == 0)).sum()), "sdf_minus_tr": int((up & (sdf == -G.tr)).sum()),
            "f_one": int((up & (sdf / G.tr == 1)).sum()), "f_clamped": int((up & (sdf / G.tr > 1)).sum())}


# ---------------------------------------------------------------------------------------------------------------- raycast ties
# Layered fields: every voxel of layer k holds tsdf T[k] (weight 1), so F depends on z alone.  Identity pose, camera 7 x 7, f = 8,
# c = 3 (the centre pixel's ray is the z axis), dmin = 0.125: sample k is at z = 0.125 + 0.25 k, exactly the centre of layer k, so
# F(z_k) = T[k] on every ray that stays inside the volume (a lerp of equal values and a weight of 0 are exact).
RAY_CAM = (8.0, 8.0, 3.0, 3.0, 7, 7)
RAY_DMIN = 0.125


def z_k(k):
    return RAY_DMIN + S * k


def layered(T, dims=None, origin=(-0.625, -0.625, 0.0)):
    T = np.asarray(T, f32)
    dims = (5, 5, len(T)) if dims is None else dims
    G, desc = MC.geometry(dims, S, origin, max_weight=16)
    vol = G.empty()
    vol[..., 0] = T[:, None, None]
    vol[..., 1] = 1.0
    return G, vol, desc


def _inf_nan_hit(with_inf=True):
    """rays of slope x = 2 z (pixel u = 4 of the camera f = 2, c = (0, 1)): one step moves two voxels in x.  Sample 2 of that ray
    lies in the cell (6, 0, 2) with a = 0.5 on every axis; its far corner (7, 1, 3) holds +Inf, so F = +Inf there; sample 3, in the
    cell (8, 0, 3), misses that voxel and gives F = 0: Fp = +Inf > 0 >= Fk, z* = z2 + s * (Inf / Inf) = NaN, the ray ends with no hit.
    Without the Inf voxel the same ray hits at z2 + s = 1.0."""
    G, desc = MC.geometry((12, 4, 8), S, (-0.25, -0.25, 0.0), max_weight=16)
    vol = G.empty()
    vol[..., 0] = np.where(np.arange(8) <= 3, f32(0.5), f32(-0.5))[:, None, None]
    vol[..., 1] = 1.0
    if with_inf:
        vol[3, 1, 7, 0] = np.inf
    return G, vol, desc


INF_CAM = (2.0, 2.0, 0.0, 1.0, 6, 3)
INF_PIXEL = 1 * 6 + 4                      # (u, v) = (4, 1): xn = 2, yn = 0


def raycast_ties():
    """name -> (G, vol, desc, cam, dmin, dmax, expected (vertex z of the centre ray or None for no hit, normal of the centre ray:
    a 3-tuple, 'nan' or None))"""
    c = {}
    c["f_next_plus_zero"] = layered([1, 0.5, 0.0, -0.5, -1, -1, -1, -1]) + (RAY_CAM, RAY_DMIN, 3.0, (z_k(2), (0.0, 0.0, -1.0)))
    # -0 survives the trilinear only where every lerp that starts from it moves towards a negative value by t = 0: layer 2 is -0 with
    # its +x and +y neighbours of the centre column at -0.25, so that F(z_2) = -0 on the centre ray (Fp / (Fp - -0) = 1 again)
    G, vol, desc = layered([1, 0.5, -0.0, -0.5, -1, -1, -1, -1])
    vol[2, 2, 3, 0] = vol[2, 3, 2, 0] = -0.25
    c["f_next_minus_zero"] = (G, vol, desc, RAY_CAM, RAY_DMIN, 3.0, (z_k(2), None))
    # the first sample is known and <= 0: no hit there (there is no previous sample); the crossing after it is found
    c["first_sample_inside"] = layered([-0.5, 0.5, -0.5, -1, -1, -1]) + (RAY_CAM, RAY_DMIN, 3.0, (z_k(1) + 0.125, (0.0, 0.0, -1.0)))
    # dmax - dmin < s: one sample, no hit although the field crosses right after it
    c["one_sample"] = layered([0.5, -0.5, -1, -1]) + (RAY_CAM, RAY_DMIN, RAY_DMIN + 0.2, (None, None))
    # the hit's second sample is in the last cell (i0 == dim - 2)
    c["last_cell_hit"] = layered([1, 1, 1, 0.5, -0.5, -1]) + (RAY_CAM, RAY_DMIN, 3.0, (z_k(3) + 0.125, (0.0, 0.0, -1.0)))
    # the crossing lies between the last two layers: the sample there has i0 = dim - 1 and is unknown
    c["beyond_last_cell"] = layered([1, 1, 1, 1, 0.5, -0.5]) + (RAY_CAM, RAY_DMIN, 3.0, (None, None))
    # dim 2 on x: the centre ray has i0 = 0 = dim - 2 and a = 0.5; the x samples of the normal leave the volume: vertex, NaN normal
    c["dim2_x"] = layered([1, 0.5, -0.5, -1, -1, -1], (2, 5, 6), (-0.25, -0.625, 0.0)) + (RAY_CAM, RAY_DMIN, 3.0, (z_k(1) + 0.125, "nan"))
    # unobserved voxels beside the hit: column i = 4 (x = 0.5) has weight 0; the centre ray's cells never touch it, its +x normal
    # sample (x = 0.25, cell i0 = 3) does
    G, vol, desc = layered([1, 0.5, -0.5, -1, -1, -1])
    vol[:, :, 4] = 0.0
    c["beside_unknown"] = (G, vol, desc, RAY_CAM, RAY_DMIN, 3.0, (z_k(1) + 0.125, "nan"))
    # F(z* + s) == F(z* - s) and F constant in x, y: a zero-length gradient, NaN normal with the vertex kept
    c["zero_gradient"] = layered([1, 0.5, 0.0, 0.5, 1, 1]) + (RAY_CAM, RAY_DMIN, 3.0, (z_k(2), "nan"))
    c["inf_makes_z_nan"] = _inf_nan_hit() + (INF_CAM, 0.25, 3.0, (None, None))
    return c


CENTRE_PIXEL = 3 * 7 + 3


# ---------------------------------------------------------------------------------------------------------------- lane tails
# integrate's lanes own 4 voxels: nvox % 4 in {0, 1, 2, 3}, d0 of 2, 3 and 5, the smallest volume and the thin ones
TAIL_DIMS = [(2, 2, 2), (4, 3, 5), (5, 3, 7), (2, 5, 7), (3, 5, 5), (3, 3, 3), (5, 7, 9), (2, 3, 3), (1024, 2, 2), (2, 1024, 2),
             (2, 2, 1024)]
TAIL_CAM = (40.0, 40.0, 31.5, 23.5, 64, 48)


def tail_scene(dims, max_weight=16, seed=0):
    """(G, desc, depth, pose): the volume spans about 1 m on its longest axis, 1.5 m in front of a 64 x 48 camera that sees all of
    it; the depth is a tilted plane through it with holes (0 = invalid), so that voxels in front, in the band and behind occur"""
    s = 1.0 / max(dims)
    ext = np.array(dims, np.float64) * s
    G, desc = MC.geometry(dims, s, tuple(-ext / 2), trunc=0.1, max_weight=max_weight)
    fx, fy, cx, cy, w, h = TAIL_CAM
    u = np.arange(w)[None, :]
    v = np.arange(h)[:, None]
    depth = (1.5 + 0.6 * (u - cx) / w + 0.3 * (v - cy) / h).astype(f32)
    rng = np.random.default_rng(seed)
    depth.reshape(-1)[rng.integers(0, depth.size, depth.size // 10)] = 0
    return G, desc, depth, pose12(np.eye(3), np.array([0.0, 0.0, 1.5]))


TAIL_RANGE = (0.1, 10.0, 10.0)


def awkward(G, seed, max_weight):
    """a volume of awkward bits: tsdf from NaNs (quiet, signalling, with payloads), +-Inf, +-0, denormals and ordinary values;
    weights negative, -1 (then w + 1 = 0), 0, denormal, 1, W - 1, W, above W, +-Inf and NaNs"""
    rng = np.random.default_rng(seed)
    vol = G.empty()
    n = vol[..., 0].size
    t = rng.uniform(-1.5, 1.5, n).astype(f32)
    pick = rng.random(n) < 0.4
    t.view(np.uint32)[pick] = rng.choice(W_BITS, int(pick.sum()))
    wv = np.array([-2.5, -1.0, 0.0, 1e-40, 1.0, max_weight - 1, max_weight, max_weight + 0.5, 2 * max_weight, np.inf, -np.inf], f32)
    w = rng.choice(wv, n)
    pick = rng.random(n) < 0.15
    w.view(np.uint32)[pick] = rng.choice(W_BITS[:4], int(pick.sum()))
    vol[..., 0] = t.reshape(vol.shape[:3])
    vol[..., 1] = w.reshape(vol.shape[:3])
    return vol


def integrate_matches(got, before, want, ok):
    """the comparison rule of integrate into an uploaded volume: a skipped voxel keeps its bits (NaN payloads included); an updated
    voxel has the oracle's bits, except that two NaN results are equal (the convention does not fix NaN payloads).  Returns the
    number of offending voxels."""
    g, b, o = got.view(np.uint32), before.view(np.uint32), want.view(np.uint32)
    skipped_bad = (g != b).any(-1) & ~ok
    both_nan = np.isnan(got) & np.isnan(want)
    updated_bad = ((g != o) & ~both_nan).any(-1) & ok
    return int(skipped_bad.sum() + updated_bad.sum())


# ---------------------------------------------------------------------------------------------------------------- mesh chunks
CHUNK = 4096


def gyroid(dims, period=9.0, seed=0):
    """weight 1 everywhere, tsdf a gyroid-like field of about `period` voxels, clipped to [-1, 1]: vertices in every chunk"""
    rng = np.random.default_rng(seed)
    G, desc = MC.geometry(dims, 0.02, (-0.3, -0.2, 0.1))
    ph = rng.uniform(0, 6.28, 3)
    k = 2 * np.pi / (period * 0.02)
    vol = MC.sdf_volume(G, lambda x, y, z: 0.05 * (np.sin(k * x + ph[0]) * np.cos(k * y) + np.sin(k * y + ph[1]) * np.cos(k * z)
                                                     + np.sin(k * z + ph[2]) * np.cos(k * x)))
    return G, vol, desc


def sparse_256(n=256):
    """an n^3 volume (4096 chunks at 256), weight 1, tsdf 1 but for small spheres of radius 2.2 voxels around the first voxel,
    the last voxel and chunk boundaries (a chunk is 16 rows of 256: cubes at j = 15 mod 16 straddle two chunks)"""
    G, desc = MC.geometry((n, n, n), 0.01, (0.0, 0.0, 0.0))
    vol = G.empty()
    vol[..., 0] = 1.0
    vol[..., 1] = 1.0
    centres = [(1.5, 1.5, 1.5), (n - 2.5, n - 2.5, n - 2.5), (100.5, 15.5, 7.0), (n - 4.0, 31.5, 128.0), (3.0, n - 16.5, n - 3.0)]
    for ci, cj, ck in centres:
        lo = [max(0, int(c) - 4) for c in (ck, cj, ci)]
        sl = tuple(slice(l, min(n, l + 9)) for l in lo)
        kk, jj, ii = np.meshgrid(*[np.arange(s.start, s.stop) for s in sl], indexing="ij")
        r = np.sqrt((ii - ci) ** 2 + (jj - cj) ** 2 + (kk - ck) ** 2) - 2.2
        vol[sl + (0,)] = np.minimum(vol[sl + (0,)], np.clip(r / 3.0, -1, 1).astype(f32))
    return G, vol, desc


# ---------------------------------------------------------------------------------------------------------------- checkerboard
def checkerboard_slab(d0, d1, parity):
    """one z slab of the checkerboard: tsdf +0.5 where i + j + k is even, -0.5 where odd (k's parity given), weight 1"""
    p = (np.arange(d0)[None, :] + np.arange(d1)[:, None] + parity) & 1
    s = np.empty((d1, d0, 2), f32)
    s[..., 0] = np.where(p == 0, f32(0.5), f32(-0.5))
    s[..., 1] = 1.0
    return s


def checkerboard(dims):
    d0, d1, d2 = dims
    vol = np.empty((d2, d1, d0, 2), f32)
    slabs = [checkerboard_slab(d0, d1, 0), checkerboard_slab(d0, d1, 1)]
    for k in range(d2):
        vol[k] = slabs[k & 1]
    return vol


def checkerboard_counts(dims):
    """every lattice edge joins opposite signs and every cube is active: vertices = the x + y + z edges, 4 triangles per cube"""
    d0, d1, d2 = dims
    nv = (d0 - 1) * d1 * d2 + d0 * (d1 - 1) * d2 + d0 * d1 * (d2 - 1)
    return nv, 4 * (d0 - 1) * (d1 - 1) * (d2 - 1)


# ---------------------------------------------------------------------------------------------------------------- large volume
# 1024 x 1024 x 544 voxels of 1/128 m from the origin: slab k starts at byte 8 * 2^20 * k, so k = 256 and k = 512 are the byte
# offsets 2^31 and 2^32.  Analytic content in z-slab windows, weight 0 everywhere else.
LARGE_DIMS = (1024, 1024, 544)
LARGE_S = 1.0 / 128
LARGE_WINDOWS = [(250, 262), (506, 518), (534, 544)]


def large_geometry():
    return MC.geometry(LARGE_DIMS, LARGE_S, (0.0, 0.0, 0.0), trunc=3 * LARGE_S, max_weight=16)


def large_window(G, k0, k1, seed):
    """slabs [k0, k1): a bumpy surface z = z0(x, y) across the middle of the window, tsdf = clip((z0 - z) / tr) (free side in front
    of a camera looking along +z), weight 1.  The windows do not touch, so unobserved slabs separate them."""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 6.28, 2)
    px, py, pz = [c.astype(np.float64) for c in VO.voxel_centres(G, k0, k1)]
    z0 = float(G.o[2]) + (0.5 * (k0 + k1)) * float(G.s) + 2.5 * float(G.s) * np.sin(7.0 * px + ph[0]) * np.cos(5.0 * py + ph[1])
    vol = np.empty((k1 - k0, G.dim[1], G.dim[0], 2), f32)
    vol[..., 0] = np.clip((z0 - pz) / float(G.tr), -1.0, 1.0)
    vol[..., 1] = 1.0
    return vol
