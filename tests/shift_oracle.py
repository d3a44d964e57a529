"""numpy statement of the moving volume of include/rgbd_pose_hip.h Part 3 ("Moving volume": rpe_volume_shift, rpe_volume_geometry,
rpe_volume_follow, rpe_volume_mesh_box), the contract csrc/rpe_shift.hip, rpe_shift_api.hip and the box predicate of rpe_mesh.hip are
held to BIT-EXACTLY.  A volume is (d2, d1, d0, 2) float32, a colour volume (d2, d1, d0, 4) uint16 (or float16), as the downloads
return them; a shift is (di, dj, dk) voxels along +x, +y, +z."""
import numpy as np

import mesh_oracle as MO
import volume_oracle as VO

F = np.float32


def _ranges(n, s):
    """(destination slice, source slice) along an axis of n voxels moved by s: new[i] = old[i + s] where 0 <= i + s < n"""
    lo, hi = max(0, -s), min(n, n - s)
    if lo >= hi:
        return slice(0, 0), slice(0, 0)
    return slice(lo, hi), slice(lo + s, hi + s)


def shift(vol, cvol, d):
    """(volume, colour volume or None) after rpe_volume_shift(d): the bits moved as they are, zeros elsewhere"""
    di, dj, dk = (int(x) for x in d)
    out = []
    for a in (vol, cvol):
        if a is None:
            out.append(None)
            continue
        d2, d1, d0 = a.shape[:3]
        (zd, zs), (yd, ys), (xd, xs) = _ranges(d2, dk), _ranges(d1, dj), _ranges(d0, di)
        b = np.zeros_like(a)
        b.view(np.uint32 if a.dtype == F else np.uint16)[zd, yd, xd] = a.view(np.uint32 if a.dtype == F else np.uint16)[zs, ys, xs]
        out.append(b)
    return out[0], out[1]


def origin_after(origin, voxel_size, total):
    """origin_now: origin + (double)total * voxel_size per axis, in double as written"""
    return np.array([float(origin[a]) + float(int(total[a])) * float(voxel_size) for a in range(3)], np.float64)


def geometry_after(dims, voxel_size, origin, trunc, max_weight, total):
    """the fp32 geometry every kernel sees after a total shift: ONE rounding of origin_now"""
    return VO.Geometry(dims, voxel_size, origin_after(origin, voxel_size, total), trunc, max_weight)


def follow(pose12, look_ahead, granule, origin_now, dims, voxel_size):
    """rpe_volume_follow: the five lines of the header, in double (python floats), in the written order"""
    P = [float(x) for x in np.asarray(pose12, np.float64).reshape(12)]
    R, t = P[:9], P[9:]
    p = [0.0 - t[0], 0.0 - t[1], float(look_ahead) - t[2]]
    out = np.zeros(3, np.int32)
    for a in range(3):
        c = R[a] * p[0] + R[3 + a] * p[1] + R[6 + a] * p[2]
        centre = float(origin_now[a]) + 0.5 * int(dims[a]) * float(voxel_size)
        v = (c - centre) / float(voxel_size)
        out[a] = int(granule) * int(np.trunc(v / int(granule)))
    return out


def full_box(G):
    return (0, 0, 0), tuple(d - 1 for d in G.dim)


def leaving_boxes(dims, d):
    """the cubes of the window that a shift d loses, as at most three disjoint boxes [(lo, hi), ...]: a cube stays iff all its corners
    stay, per axis index >= d (d > 0) or index < dim - 1 + d (d < 0).  Axis by axis: the slab that leaves along the axis, restricted
    on the axes before it to what stays there.  Together with the cubes of the window after the shift they partition the cubes."""
    keep = []
    for a in range(3):
        n, s = int(dims[a]) - 1, int(d[a])
        lo, hi = (min(s, n), n) if s > 0 else (0, max(n + s, 0))
        keep.append((lo, hi))
    boxes = []
    for a in range(3):
        n = int(dims[a]) - 1
        for lo_a, hi_a in ((0, keep[a][0]), (keep[a][1], n)):
            if lo_a >= hi_a:
                continue
            lo = [keep[b][0] if b < a else 0 for b in range(3)]
            hi = [keep[b][1] if b < a else int(dims[b]) - 1 for b in range(3)]
            lo[a], hi[a] = lo_a, hi_a
            if all(l < h for l, h in zip(lo, hi)):
                boxes.append((tuple(lo), tuple(hi)))
    return boxes


def mesh_box(vol, G, min_weight, lo, hi):
    """rpe_volume_mesh_box: mesh_oracle.mesh with the case of every cube outside lo <= (i, j, k) < hi set to 0"""
    d0, d1 = G.dim[:2]
    case = MO.cases(vol, min_weight)
    box = np.zeros(case.shape, bool)
    box[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    case = np.where(box, case, 0).astype(np.uint8)
    used = MO.used_edges(case)
    flat_used = used.reshape(-1).astype(np.int64)
    bits = ((flat_used[:, None] >> np.arange(3)) & 1).astype(bool)
    vox, axis = np.nonzero(bits)
    ts = vol.reshape(-1, 2)[:, 0]
    strides = np.array([1, d0, d0 * d1], np.int64)
    ijk = np.stack([vox % d0, (vox // d0) % d1, vox // (d0 * d1)], -1)
    Fa, Fb = ts[vox], ts[vox + strides[axis]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = Fa / (Fa - Fb)
        P = np.empty((len(vox), 3), F)
        for a in range(3):
            centre = G.o[a] + (ijk[:, a].astype(F) + F(0.5)) * G.s
            along = G.o[a] + ((ijk[:, a].astype(F) + F(0.5)) + t) * G.s
            P[:, a] = np.where(axis == a, along, centre)
        N = MO.normals(vol, G, P)
    counts = bits.sum(1)
    first = np.cumsum(counts) - counts
    ntri = MO.TRI_COUNT[case.reshape(-1)]
    cube = np.repeat(np.arange(ntri.size), ntri)
    r = np.arange(cube.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    edges = MO.TRI_EDGES[case.reshape(-1)[cube], r]
    o = MO.EDGE_OWNER[edges]
    owner = cube[:, None] + (o & 1) + ((o >> 1) & 1) * d0 + ((o >> 2) & 1) * d0 * d1
    ax = MO.EDGE_AXIS[edges]
    lower = flat_used[owner] & ((1 << ax) - 1)
    ids = first[owner] + (lower & 1) + ((lower >> 1) & 1)
    return P, N, ids.astype(np.int32).reshape(-1, 3), cube
