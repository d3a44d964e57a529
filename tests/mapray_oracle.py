"""numpy statement of the map raycast of include/rgbd_pose_hip.h Part 3 ("Map raycast": rpe_volume_map_raycast), the contract the
map_raycast_kernel / map_occupancy_kernel of csrc/rpe_frontend.hip and rpe_mapmesh_api.hip are held to BIT EXACTLY.  It is a
composition of existing statements and restates none of them: the virtual volume of a box of the map (mapmesh_oracle.dense /
geometry), the raycast of a dense volume (volume_oracle.raycast), the colour field at points (color_oracle.sample)."""
import numpy as np

import color_oracle as CO
import mapmesh_oracle as MM
import volume_oracle as VO

F = np.float32


def raycast(window, cwindow, total, store, box, kw, cam, pose12, dmin, dmax, colour=False):
    """rpe_volume_map_raycast(box): (vertex map, normal map, (h*w, 3) float32 each, RGBA8 colour map (h*w, 4) uint8 or None)"""
    vol, cvol = MM.dense(window, cwindow, total, store, box)
    G = MM.geometry(kw, box)
    MV, MN = VO.raycast(vol, G, cam, pose12, dmin, dmax)
    return MV, MN, CO.sample(cvol, G, MV) if colour else None


def cells(G, X):
    """i0 of F's cell at the points X (n, 3), int64; rows of NaN points are meaningless"""
    with np.errstate(invalid="ignore"):
        g = np.stack([(X[:, a].astype(F) - G.o[a]) / G.s - F(0.5) for a in range(3)], -1)
    return np.nan_to_num(np.floor(g)).astype(np.int64)
