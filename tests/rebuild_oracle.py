"""numpy statement of rpe_volume_fuse_keyframes (include/rgbd_pose_hip.h Part 3, "Keyframe depth and rebuilding the volume"): the loop
over tests/volume_oracle.py integrate / tests/color_oracle.py integrate that the header's contract names, and nothing more.  An entry
is dict(z (h*w,) float32 depth plane, NaN = invalid; rgba (h*w, 4) uint8 or None; cam; pose (12,))."""
import numpy as np

import color_oracle as CO
import volume_oracle as VO

CLEAR, COLOR, NO_CULL = 1, 2, 4


def as_map(z):
    """the vertex map whose z column is the plane: what the integrate oracles read"""
    V = np.zeros((np.asarray(z).size, 3), np.float32)
    V[:, 2] = np.asarray(z, np.float32).reshape(-1)
    return V


def fuse(vol, cvol, G, entries, flags):
    """(vol, cvol) after the call; cvol None = no colour volume.  vol / cvol are ignored with CLEAR."""
    if flags & CLEAR:
        vol, cvol = G.empty(), None
    if flags & COLOR and cvol is None:
        cvol = CO.empty(G)
    for e in entries:
        if flags & COLOR:
            vol, cvol = CO.integrate(vol, cvol, G, as_map(e["z"]), e["rgba"], e["cam"], e["pose"])
        else:
            vol = VO.integrate(vol, G, as_map(e["z"]), e["cam"], e["pose"])
    return vol, cvol
