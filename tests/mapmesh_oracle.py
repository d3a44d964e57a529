"""numpy statement of the map mesh of include/rgbd_pose_hip.h Part 3 ("Map mesh": rpe_volume_map_bounds, rpe_volume_map_mesh), the
contract csrc/rpe_mapmesh.hip and rpe_mapmesh_api.hip are held to BIT EXACTLY.  The map is archive_oracle's model -- (window, colour
window or None, total shift, store) -- seen as a sparse grid of world voxels; a box of it is a dense VIRTUAL volume, and the map mesh
is mesh_oracle.mesh and color_oracle.sample of that volume, permuted into brick order.  No convention of the mesh is restated here:
only the virtual volume and the order."""
import numpy as np

import archive_oracle as AO
import color_oracle as CO
import mesh_oracle as MO
import shift_oracle as SO

BRICK = AO.BRICK


def bounds(total, dims, store):
    """rpe_volume_map_bounds: (lo, hi) int64, the world-voxel bounding box of the window and every held brick"""
    lo = [int(total[a]) for a in range(3)]
    hi = [int(total[a]) + int(dims[a]) for a in range(3)]
    for key in store:
        for a in range(3):
            lo[a] = min(lo[a], BRICK * int(key[a]))           # python's * and the keys are exact for negative bricks too
            hi[a] = max(hi[a], BRICK * int(key[a]) + BRICK)
    return np.array(lo, np.int64), np.array(hi, np.int64)


def _paste(dst, src, at, lo, hi):
    """src, whose voxel (0, 0, 0) is world voxel `at`, into dst = the box [lo, hi), where they overlap"""
    a = [max(int(at[x]), int(lo[x])) for x in range(3)]
    b = [min(int(at[x]) + src.shape[2 - x], int(hi[x])) for x in range(3)]
    if any(p >= q for p, q in zip(a, b)):
        return
    d = tuple(slice(a[x] - int(lo[x]), b[x] - int(lo[x])) for x in (2, 1, 0))
    s = tuple(slice(a[x] - int(at[x]), b[x] - int(at[x])) for x in (2, 1, 0))
    dst[d] = src[s]


def dense(window, cwindow, total, store, box):
    """the virtual volume of the box: (tsdf (n2, n1, n0, 2) float32, colour (n2, n1, n0, 4) uint16), the window's bits where it covers,
    the held bricks' where the store holds them, zeros elsewhere"""
    lo, hi = (np.asarray(b, np.int64) for b in box)
    n = [int(hi[a] - lo[a]) for a in range(3)]
    assert all(int(x) % BRICK == 0 for x in list(lo) + list(hi)) and all(BRICK <= x <= 1 << 20 for x in n), box
    vol = np.zeros((n[2], n[1], n[0], 2), np.uint32)
    cvol = np.zeros((n[2], n[1], n[0], 4), np.uint16)
    _paste(vol, np.ascontiguousarray(window).view(np.uint32), total, lo, hi)
    if cwindow is not None:
        _paste(cvol, np.ascontiguousarray(cwindow).view(np.uint16), total, lo, hi)
    for key, (t, c) in store.items():
        at = [BRICK * int(k) for k in key]
        _paste(vol, np.ascontiguousarray(t).view(np.uint32), at, lo, hi)
        _paste(cvol, np.ascontiguousarray(c).view(np.uint16), at, lo, hi)
    return vol.view(np.float32), cvol


def geometry(kw, box):
    """the fp32 geometry of the box's virtual volume: kw = the init descriptor (voxel_size, origin, trunc, max_weight); the origin is
    origin + (double)lo * voxel_size, rounded once (shift_oracle.geometry_after with lo for the total)"""
    lo, hi = box
    dims = tuple(int(hi[a]) - int(lo[a]) for a in range(3))
    return SO.geometry_after(dims, kw["voxel_size"], kw["origin"], kw["trunc"], kw["max_weight"], [int(x) for x in lo])


def rank(dims):
    """per voxel of a dense volume, by its flat index: its position in MAP order -- bricks ascending by (bz, by, bx), inside a brick
    (z, y, x) with x fastest"""
    d0, d1, d2 = dims
    k, j, i = np.meshgrid(np.arange(d2), np.arange(d1), np.arange(d0), indexing="ij")
    nb0, nb1 = d0 // BRICK, d1 // BRICK
    brick = ((k // BRICK) * nb1 + j // BRICK) * nb0 + i // BRICK
    local = ((k % BRICK) * BRICK + j % BRICK) * BRICK + i % BRICK
    return (brick * BRICK ** 3 + local).reshape(-1).astype(np.int64)


def owners(vol, min_weight):
    """of mesh_oracle.mesh(vol): per vertex its owner voxel (flat index) and axis, per triangle its cube (flat index of the corner-0
    voxel) and its place in the cube's table entry, all in the dense order"""
    case = MO.cases(vol, min_weight)
    used = MO.used_edges(case).reshape(-1).astype(np.int64)
    vox, axis = np.nonzero(((used[:, None] >> np.arange(3)) & 1).astype(bool))
    ntri = MO.TRI_COUNT[case.reshape(-1)]
    cube = np.repeat(np.arange(ntri.size), ntri)
    r = np.arange(cube.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    return vox, axis, cube, r


def permutation(vol, min_weight):
    """(pv, pt): the map mesh's vertex n is the dense mesh's vertex pv[n], its triangle m the dense mesh's triangle pt[m]"""
    d2, d1, d0 = vol.shape[:3]
    rk = rank((d0, d1, d2))
    vox, axis, cube, r = owners(vol, min_weight)
    pv = np.argsort(rk[vox] * 3 + axis, kind="stable")
    pt = np.argsort(rk[cube] * 8 + r, kind="stable")
    return pv, pt


def permute(vol, min_weight, V, N, T, C=None):
    """a dense mesh of vol (mesh_oracle.mesh's, or rpe_volume_mesh's) in map order, ids renumbered"""
    pv, pt = permutation(vol, min_weight)
    assert len(pv) == len(V) and len(pt) == len(T)
    inv = np.empty(len(pv), np.int64)
    inv[pv] = np.arange(len(pv))
    Tm = inv[np.asarray(T, np.int64)[pt]].astype(np.int32).reshape(-1, 3)
    return V[pv], N[pv], Tm, None if C is None else C[pv]


def mesh(window, cwindow, total, store, box, kw, min_weight=1.0, colour=True):
    """rpe_volume_map_mesh(box) and rpe_volume_mesh_colors after it: (vertices, normals, triangles, RGBA8 colours or None)"""
    vol, cvol = dense(window, cwindow, total, store, box)
    G = geometry(kw, box)
    V, N, T = MO.mesh(vol, G, min_weight)
    C = CO.sample(cvol, G, V) if colour else None
    return permute(vol, min_weight, V, N, T, C)
