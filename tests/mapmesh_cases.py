"""Cases of the map mesh, shared by tests/test_mapmesh_oracle.py (CPU) and tests/test_gpu_mapmesh.py: the model of a map beside a
context (Map), worlds to fill it with -- content that is a function of the WORLD voxel, uploaded window by window while the window
walks, so that the map ends up holding the world wherever the window has been -- and the use case: the walk of tests/archive_cases.py,
meshed at its end as a whole map and as the window alone."""
import numpy as np

import archive_cases as AC
import archive_oracle as AO
import color_oracle as CO
import mapmesh_oracle as MM
import mesh_oracle as MO
import shift_cases as SC
import shift_oracle as SO
import volume_oracle as VO
from frontend_util import FO

F32 = np.float32
KW = dict(voxel_size=0.03, origin=(-0.7, 0.3, 1.1), trunc=0.09, max_weight=16.0)


class Map:
    """archive_oracle's model of a map -- window, colour window, total, store -- and, if ctx is given, the same calls on a context"""

    def __init__(self, ctx, dims, kw=KW, capacity=256):
        self.ctx, self.dims, self.kw = ctx, tuple(dims), dict(kw)
        d0, d1, d2 = dims
        self.window, self.cwindow, self.total, self.store = np.zeros((d2, d1, d0, 2), F32), None, (0, 0, 0), {}
        self.colour_plane = False            # the pool has a colour plane: a brick was archived while a colour volume existed
        if ctx is not None:
            ctx.volume_init(dims, **kw)
            if capacity:
                ctx.volume_archive(capacity)

    def upload(self, vol, cvol=None):
        self.window = np.ascontiguousarray(vol, F32)
        if self.ctx is not None:
            self.ctx.volume_upload(self.window)
        if cvol is not None:
            self.cwindow = np.ascontiguousarray(cvol).view(np.uint16)
            if self.ctx is not None:
                self.ctx.volume_color_upload(self.cwindow.view(np.float16))
        return self

    def shift(self, d):
        held = set(self.store)
        self.window, self.cwindow, self.total = AO.shift(self.window, self.cwindow, self.total, d, self.store)
        self.colour_plane = self.colour_plane or (self.cwindow is not None and bool(set(self.store) - held))
        if self.ctx is not None:
            self.ctx.volume_shift(d)
        return self

    def fill(self, world, path, colour=True):
        """upload world(total) at every stop of the path of shifts"""
        for d in [None] + list(path):
            if d is not None:
                self.shift(d)
            vol, cvol = world(self.total, self.dims)
            self.upload(vol, cvol if colour else None)
        return self

    def extent(self):
        lo = np.array(self.total, np.int64)
        return lo, lo + np.array(self.dims, np.int64)

    def bounds(self):
        return MM.bounds(self.total, self.dims, self.store)

    def has_colour(self):
        return self.cwindow is not None or self.colour_plane

    def dense(self, box=None):
        return MM.dense(self.window, self.cwindow, self.total, self.store, self.bounds() if box is None else box)

    def mesh(self, box=None, min_weight=1.0):
        """(V, N, T, C or None) of the oracle"""
        return MM.mesh(self.window, self.cwindow, self.total, self.store, self.bounds() if box is None else box, self.kw, min_weight,
                       colour=self.has_colour())


# ---------------------------------------------------------------------------------------------- worlds
def grids(total, dims):
    """world voxel coordinates X, Y, Z of a window at `total`, shaped (d2, d1, d0)"""
    d0, d1, d2 = dims
    Z, Y, X = np.meshgrid(np.arange(d2) + int(total[2]), np.arange(d1) + int(total[1]), np.arange(d0) + int(total[0]), indexing="ij")
    return X, Y, Z


def colours(X, Y, Z):
    """a colour per world voxel; one voxel in 13 has no colour weight"""
    c = np.empty(X.shape + (4,), np.uint16)
    c[..., 0], c[..., 1], c[..., 2] = CO.h((X * 7 % 256).astype(F32)), CO.h((Y * 11 % 256).astype(F32)), CO.h((Z * 13 % 256).astype(F32))
    c[..., 3] = CO.h(np.where((X + 3 * Y + 5 * Z) % 13 == 0, 0, 2).astype(F32))
    return c


def world_of(tsdf_weight):
    """a world whose {tsdf, weight} are tsdf_weight(X, Y, Z) of the world voxel"""
    def world(total, dims):
        X, Y, Z = grids(total, dims)
        t, w = tsdf_weight(X, Y, Z)
        return np.stack([np.broadcast_to(t, X.shape), np.broadcast_to(w, X.shape)], -1).astype(F32), colours(X, Y, Z)
    return world


def sphere(centre, radius, weight=2.0):
    """the truncated distance (3 voxels) to a sphere, in voxels of the world grid"""
    def f(X, Y, Z):
        d = np.sqrt((X - centre[0]) ** 2.0 + (Y - centre[1]) ** 2.0 + (Z - centre[2]) ** 2.0) - radius
        return np.clip(d / 3.0, -1.0, 1.0), weight
    return world_of(f)


def slab(axis, lo, hi, sign):
    """sign * min(w - lo, hi - w) / 3 along one axis, clipped: EXACTLY 0 on the layers w = lo and w = hi"""
    def f(X, Y, Z):
        w = (X, Y, Z)[axis]
        return np.clip(sign * np.minimum(w - lo, hi - w) / 3.0, -1.0, 1.0), 2.0
    return world_of(f)


# a 16^3 window that visits the eight octants of [-16, 16)^3: negative and positive shifts, a diagonal one, negative world bricks
OCTANTS = [(-16, 0, 0), (0, -16, 0), (16, 0, 0), (0, 16, -16), (-16, 0, 0), (0, -16, 0), (16, 0, 0)]
# the sphere passes through the corner where the eight bricks around world voxel (8, 8, 8) meet, and through the planes 0 and +-8
SPHERE = ((0.3, -0.3, 0.2), float(np.sqrt(7.2 ** 2 + 7.8 ** 2 + 7.3 ** 2)))


def edge_t(vol, min_weight=1.0):
    """per vertex of mesh_oracle.mesh(vol), in its order: (owner voxel (i, j, k), axis, t = Fa / (Fa - Fb))"""
    d2, d1, d0 = vol.shape[:3]
    vox, axis, _, _ = MM.owners(vol, min_weight)
    ts = vol.reshape(-1, 2)[:, 0]
    Fa, Fb = ts[vox], ts[vox + np.array([1, d0, d0 * d1])[axis]]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = Fa / (Fa - Fb)
    return np.stack([vox % d0, (vox // d0) % d1, vox // (d0 * d1)], -1), axis, t


def cube_ijk(vol, min_weight=1.0):
    """per triangle of mesh_oracle.mesh(vol), in its order: its cube's corner-0 voxel (i, j, k)"""
    d2, d1, d0 = vol.shape[:3]
    _, _, cube, _ = MM.owners(vol, min_weight)
    return np.stack([cube % d0, (cube // d0) % d1, cube // (d0 * d1)], -1)


def triangle_words(V, N, T, normals=True):
    """each triangle as its 9 position words (and 9 normal words), sorted: a multiset that does not know vertex ids or order"""
    P = np.ascontiguousarray(V[T.reshape(-1)]).view(np.uint32).reshape(-1, 9)
    if normals and N is not None:
        P = np.concatenate([P, np.ascontiguousarray(N[T.reshape(-1)]).view(np.uint32).reshape(-1, 9)], 1)
    return P[np.lexsort(P.T[::-1])] if len(P) else P


def contains(big, small):
    """the sorted rows of `small` are a sub-multiset of the sorted rows of `big` (triangle_words)"""
    rows = lambda a: np.ascontiguousarray(a).view([("", a.dtype)] * a.shape[1]).reshape(-1)
    ub, cb = np.unique(rows(big), return_counts=True)
    us, cs = np.unique(rows(small), return_counts=True)
    at = np.searchsorted(ub, us)
    at = np.minimum(at, len(ub) - 1)
    return len(ub) > 0 and bool((ub[at] == us).all() and (cb[at] >= cs).all())


# ---------------------------------------------------------------------------------------------- the use case
# The walk of tests/archive_cases.py out and back (a 64^3 window at 4 cm, every frame fused at its true pose, the archive on).  At its
# end the map is meshed whole (the bounds) and the window alone; figures() says what each mesh shows of the room.
WMIN = 1.0


def oracle_walk():
    """archive_cases.oracle_walk(True) without its raycasts, and with the store handed out: (window, total, store)"""
    total, store = (0, 0, 0), {}
    G = SC.geometry(total)
    vol = G.empty()
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = SO.follow(p, SC.LOOK_AHEAD, AC.GRANULE, SO.origin_after(SC.first_origin(), AC.VOXEL, total), AC.DIMS, AC.VOXEL)
            if sh.any():
                vol, _, total = AO.shift(vol, None, total, sh, store)
                G = SC.geometry(total)
        vol = VO.integrate(vol, G, FO.frame_maps(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)[0], AC.CAM, p)
    return vol, total, store


def room_samples(step=AC.VOXEL):
    """points on the room's true surfaces, one per step^2 of area: the six walls on a grid, the spheres on a spiral"""
    lo, hi, spheres = SC.S.default_room()
    pts = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        gb, gc = np.meshgrid(np.arange(lo[b] + step / 2, hi[b], step), np.arange(lo[c] + step / 2, hi[c], step), indexing="ij")
        for side in (lo[a], hi[a]):
            q = np.empty(gb.shape + (3,))
            q[..., a], q[..., b], q[..., c] = side, gb, gc
            pts.append(q.reshape(-1, 3))
    for sx, sy, sz, r in spheres:
        n = int(4 * np.pi * r * r / (step * step))
        k = np.arange(n) + 0.5
        z, phi = 1 - 2 * k / n, k * np.pi * (3 - np.sqrt(5))
        pts.append(np.array([sx, sy, sz]) + r * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1))
    return np.concatenate(pts)


def figures(V, T):
    """dict(triangles, share = the part of the room's true surface area (room_samples) within one voxel of a mesh vertex, median = the
    median distance of the mesh's vertices to the true surfaces, in metres)"""
    from scipy.spatial import cKDTree
    S = room_samples()
    near = cKDTree(np.asarray(V, np.float64)).query(S, distance_upper_bound=AC.VOXEL)[0]
    return dict(triangles=int(len(T)), share=float(np.isfinite(near).mean()), median=float(np.median(SC.surface_distance(V))))


def window_triangles_away_from_the_last_layer(window, V, T, min_weight=WMIN):
    """of mesh_oracle.mesh(window) = (V, ., T): the position words of the triangles whose cube does not touch the window's last layer on
    any axis (those cubes have all eight corners in the window AND are cubes of the map's box whatever lies beyond)"""
    d2, d1, d0 = window.shape[:3]
    cube = cube_ijk(window, min_weight)
    keep = (cube + 1 < np.array([d0, d1, d2]) - 1).all(1)             # its far corners lie before the last layer
    return triangle_words(V, None, T[keep], normals=False)


def oracle_use_case():
    """the walk, the two meshes and their figures"""
    window, total, store = oracle_walk()
    kw = SC.desc()
    box = MM.bounds(total, AC.DIMS, store)
    Vm, Nm, Tm, _ = MM.mesh(window, None, total, store, box, kw, WMIN, colour=False)
    Vw, Nw, Tw = MO.mesh(window, SC.geometry(total), WMIN)
    return dict(digest=AC.digest(window), total=tuple(int(x) for x in total), held=len(store), box=box, map=(Vm, Nm, Tm), window=(Vw, Nw, Tw),
                window_bits=window, figures_map=figures(Vm, Tm), figures_window=figures(Vw, Tw))


# ---- the figures (oracle_use_case, measured on the CPU; tests/test_mapmesh_oracle.py recomputes them).  The walk ends where it began,
# total (0, 0, 0), with 507 bricks held; the map's bounds are 136 x 64 x 64 voxels from world voxel (0, 0, 0): the window's own corner,
# so both meshes have the same fp32 origin and a triangle of both has the same position words.
BOX = ((0, 0, 0), (136, 64, 64))
HELD = 507
# The whole map shows 3.3 x the triangles of the window and 2.9 x the surface: 16.7 % of the room's 150 m^2 (walls and spheres; the
# camera never sees most of it) against 5.7 %.  The vertices lie where the surfaces are, either way: the median distance is 0.7 mm.
TRIANGLES_MAP, TRIANGLES_WINDOW = 39445, 11786
SHARE_MAP, SHARE_WINDOW = 0.1666, 0.0568
MEDIAN_MAP, MEDIAN_WINDOW = 0.00066, 0.00068
