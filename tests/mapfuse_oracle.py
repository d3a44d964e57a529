"""numpy statement of the map fuse of include/rgbd_pose_hip.h Part 3 ("Map fuse": rpe_volume_map_fuse_keyframes), the contract
csrc/rpe_mapfuse.hpp and rpe_mapfuse_api.hip are held to BIT EXACTLY.  A pure composition, no arithmetic of its own: the box's dense
virtual volume (mapmesh_oracle.dense), rebuild_oracle.fuse on the box's geometry (mapmesh_oracle.geometry), and the result split back
into the window's part and the bricks outside it: such a brick is held afterwards iff any 32-bit word of its tsdf or colour brick is
non-zero (the archive's own rule for a leaving brick).  The map is archive_oracle's model: window, colour window or None, total, store."""
import numpy as np

import archive_oracle as AO
import mapmesh_oracle as MM
import rebuild_oracle as RO

BRICK = AO.BRICK
CLEAR, COLOR, NO_CULL = RO.CLEAR, RO.COLOR, RO.NO_CULL


def split(vol, cvol, box, window, cwindow, total, store):
    """the dense box (vol, cvol) written back into the map: (window, cwindow, store) -- new arrays and a new dict.  cvol None = the box's
    colour is all zero; a colour window exists afterwards iff cwindow is given"""
    lo, hi = (np.asarray(b, np.int64) for b in box)
    vol32 = np.ascontiguousarray(vol).view(np.uint32)
    c16 = np.zeros(vol32.shape[:3] + (4,), np.uint16) if cvol is None else np.ascontiguousarray(cvol).view(np.uint16)
    dims = window.shape[2], window.shape[1], window.shape[0]
    wlo = np.array([int(x) for x in total], np.int64)
    whi = wlo + np.array(dims, np.int64)
    w32 = np.ascontiguousarray(window).view(np.uint32).copy()
    MM._paste(w32, vol32, lo, wlo, whi)
    cw = None
    if cwindow is not None:
        cw = np.ascontiguousarray(cwindow).view(np.uint16).copy()
        MM._paste(cw, c16, lo, wlo, whi)
    out = dict(store)
    inside = AO.covered(total, dims)
    for bz in range(int(lo[2]) // BRICK, int(hi[2]) // BRICK):
        for by in range(int(lo[1]) // BRICK, int(hi[1]) // BRICK):
            for bx in range(int(lo[0]) // BRICK, int(hi[0]) // BRICK):
                key = (bx, by, bz)
                if key in inside:
                    continue
                at = (bx - int(lo[0]) // BRICK, by - int(lo[1]) // BRICK, bz - int(lo[2]) // BRICK)
                t, c = AO._cut(vol32, at), AO._cut(c16, at)
                if t.any() or c.any():
                    out[key] = (t.copy().view(np.float32), c.copy())
                else:
                    out.pop(key, None)
    return w32.view(np.float32), cw, out


def fuse(window, cwindow, total, store, box, kw, entries, flags):
    """the map after rpe_volume_map_fuse_keyframes(entries, flags, box): (window, cwindow or None, store, stats).  COLOR creates the
    colour window, zero-filled, if there is none; CLEAR zeroes the box's colour even without COLOR (rebuild_oracle.fuse hands None back:
    all zero) and never removes the colour window.  stats: bricks of the box, slots newly taken, slots released"""
    vol, cvol = MM.dense(window, cwindow, total, store, box)
    G = MM.geometry(kw, box)
    vol, cvol = RO.fuse(vol, cvol, G, entries, flags)
    if flags & COLOR and cwindow is None:
        cwindow = np.zeros(window.shape[:3] + (4,), np.uint16)
    w, cw, out = split(vol, cvol, box, window, cwindow, total, store)
    lo, hi = box
    stats = dict(bricks=int(np.prod([(int(hi[a]) - int(lo[a])) // BRICK for a in range(3)])), archived=len(set(out) - set(store)),
                 released=len(set(store) - set(out)))
    return w, cw, out, stats
