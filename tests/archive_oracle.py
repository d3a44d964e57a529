"""numpy statement of the volume archive of include/rgbd_pose_hip.h Part 3 ("Volume archive": rpe_volume_archive, the shift with the
archive on, rpe_volume_archive_info / _download / _clear), the contract csrc/rpe_archive.hip and rpe_archive_api.hip are held to BIT
EXACTLY.  The model: ONE unbounded store of bricks, a dict {(bx, by, bz) world brick: (tsdf brick (8, 8, 8, 2) float32, colour brick
(8, 8, 8, 4) uint16)}.  A shift writes the non-zero leaving bricks into it, moves the window as shift_oracle.shift does, and takes the
entering bricks out.  Volumes are laid out as the downloads return them, (d2, d1, d0, c); a brick is 8 x 8 x 8 voxels aligned in world
voxel coordinates: world voxel = total shift + window index, world brick = world voxel / 8."""
import numpy as np

import shift_oracle as SO

BRICK = 8


def bricks_of(dims):
    assert all(int(d) % BRICK == 0 for d in dims), dims
    return tuple(int(d) // BRICK for d in dims)


def leaving_boxes(nb, s):
    """the bricks of a window of nb bricks per axis that have no destination inside it after a move by s bricks (new index = old
    index - s), as at most three disjoint boxes [(lo, hi), ...], hi exclusive: axis by axis, the slab that leaves along the axis,
    restricted on the axes before it to what stays there (shift_oracle.leaving_boxes does the same for cubes)"""
    keep = []
    for a in range(3):
        lo = min(max(0, int(s[a])), nb[a])
        keep.append((lo, max(lo, min(nb[a], nb[a] + int(s[a])))))
    boxes = []
    for a in range(3):
        for lo_a, hi_a in ((0, keep[a][0]), (keep[a][1], nb[a])):
            lo = [keep[b][0] if b < a else 0 for b in range(3)]
            hi = [keep[b][1] if b < a else nb[b] for b in range(3)]
            lo[a], hi[a] = lo_a, hi_a
            if all(l < h for l, h in zip(lo, hi)):
                boxes.append((tuple(lo), tuple(hi)))
    return boxes


def bricks_in(boxes):
    """the bricks of the boxes, box after box, x fastest: the order the occupancy kernel numbers them in"""
    return [(x, y, z) for lo, hi in boxes for z in range(lo[2], hi[2]) for y in range(lo[1], hi[1]) for x in range(lo[0], hi[0])]


def leaving_bricks(dims, d):
    """window bricks (bx, by, bz) that a shift of d voxels pushes out"""
    return bricks_in(leaving_boxes(bricks_of(dims), [int(x) // BRICK for x in d]))


def entering_bricks(dims, d):
    """bricks of the window AFTER a shift of d voxels that were not in the window before it"""
    return bricks_in(leaving_boxes(bricks_of(dims), [-(int(x) // BRICK) for x in d]))


def _cut(a, b):
    x, y, z = (BRICK * int(v) for v in b)
    return a[z:z + BRICK, y:y + BRICK, x:x + BRICK]


def shift(window, cwindow, total, d, store):
    """(window, colour window or None, total) after rpe_volume_shift(d) with the archive on; `store` is updated in place.
    cwindow is uint16 (or float16) or None"""
    d = [int(x) for x in d]
    total = [int(x) for x in total]
    dims = window.shape[2], window.shape[1], window.shape[0]
    assert all(x % BRICK == 0 for x in d) and all(x % BRICK == 0 for x in total)
    if not any(d):
        return window, cwindow, tuple(total)
    w32 = np.ascontiguousarray(window).view(np.uint32)
    c16 = None if cwindow is None else np.ascontiguousarray(cwindow).view(np.uint16)
    for b in leaving_bricks(dims, d):
        t = _cut(w32, b)
        c = None if c16 is None else _cut(c16, b)
        if t.any() or (c is not None and c.any()):                  # any 32-bit word of either volume: bits, not weights
            key = tuple(total[a] // BRICK + b[a] for a in range(3))
            assert key not in store, key                                # the window is the only holder of what it covers
            store[key] = (t.copy().view(np.float32), np.zeros((BRICK, BRICK, BRICK, 4), np.uint16) if c is None else c.copy())
    window, cwindow = SO.shift(window, cwindow, d)
    total = [total[a] + d[a] for a in range(3)]
    w32 = window.view(np.uint32)
    c16 = None if cwindow is None else cwindow.view(np.uint16)
    for b in entering_bricks(dims, d):
        key = tuple(total[a] // BRICK + b[a] for a in range(3))
        if key in store:
            t, c = store.pop(key)
            _cut(w32, b)[...] = t.view(np.uint32)
            if c16 is not None:
                _cut(c16, b)[...] = c
    return window, cwindow, tuple(total)


def download(store):
    """rpe_volume_archive_download: (coords (n, 3) int64 as (bx, by, bz), tsdf (n, 8, 8, 8, 2) float32, colour (n, 8, 8, 8, 4) uint16),
    sorted by (bz, by, bx)"""
    keys = sorted(store, key=lambda k: (k[2], k[1], k[0]))
    n = len(keys)
    coords = np.array(keys, np.int64).reshape(n, 3)
    tsdf = np.zeros((n, BRICK, BRICK, BRICK, 2), np.float32)
    colour = np.zeros((n, BRICK, BRICK, BRICK, 4), np.uint16)
    for i, k in enumerate(keys):
        tsdf[i], colour[i] = store[k]
    return coords, tsdf, colour


def covered(total, dims):
    """the world bricks the window covers"""
    nb = bricks_of(dims)
    return {(int(total[0]) // BRICK + x, int(total[1]) // BRICK + y, int(total[2]) // BRICK + z)
            for z in range(nb[2]) for y in range(nb[1]) for x in range(nb[0])}
