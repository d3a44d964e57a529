"""numpy statement of THE FUSE'S CULL (csrc/rpe_volume_field.hpp: edge_outside, box_can_update), the decision volume_fuse_kernel
(rpe_rebuild.hip) and map_fuse_kernel (rpe_mapfuse.hpp) take per brick and list entry.  Every intermediate is IEEE fp32 in the written
order, as in tests/volume_oracle.py; vectorised over cases (one row per brick and entry).  A camera is the tuple of arrays (fx, fy, cx,
cy fp32; width, height int), a pose the arrays R (n, 9) and t (n, 3) fp32.

variant= names a DELIBERATELY WRONG form of the rule, for tests/test_cull_oracle.py to show that the case set tells it from the rule:
  "no_fabs"        the box's half extent in the camera frame without the magnitudes of R
  "centre_behind"  "every centre behind the camera" decided on the box's centre alone
  "zh_for_zl"      the far z in place of the near z where the extreme ratio x / z lies at the near one
The variants live in test code only; the library has one form."""
import numpy as np

import volume_oracle as VO

F = np.float32
EPS = F(1.0) / F(262144.0)                                      # kCullEps
VARIANTS = ("no_fabs", "centre_behind", "zh_for_zl")


def edge_outside(xlo, xhi, zl, zh, f, c, size, variant=None):
    inf = F(np.inf)
    zn = zh if variant == "zh_for_zl" else zl
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rmax = np.where(xhi >= F(0), np.where(zn > F(0), xhi / zn, inf), xhi / zh)
        rmin = np.where(xlo <= F(0), np.where(zn > F(0), xlo / zn, -inf), xlo / zh)
        umax, umin = f * rmax + c + F(0.5), f * rmin + c + F(0.5)
        return (umax + (F(1) + EPS * np.abs(umax)) < F(0)) | (umin - (F(1) + EPS * np.abs(umin)) > size.astype(F))


def box_can_update(lo, hi, cam, R, t, variant=None):
    """lo, hi (n, 3) fp32: per axis the centres of the brick's first and last voxel.  (n,) bool: False = the entry is skipped"""
    fx, fy, cx, cy, w, h = cam
    lo, hi, R, t = (np.asarray(x, F) for x in (lo, hi, R, t))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c, hx, a = F(0.5) * (lo + hi), F(0.5) * (hi - lo), np.fmax(np.abs(lo), np.abs(hi))
        l, u, q = [], [], []
        for r in range(3):
            R0, R1, R2 = R[:, 3 * r], R[:, 3 * r + 1], R[:, 3 * r + 2]
            qr = R0 * c[:, 0] + R1 * c[:, 1] + R2 * c[:, 2] + t[:, r]
            if variant == "no_fabs":
                e = R0 * hx[:, 0] + R1 * hx[:, 1] + R2 * hx[:, 2]
            else:
                e = np.abs(R0) * hx[:, 0] + np.abs(R1) * hx[:, 1] + np.abs(R2) * hx[:, 2]
            m = EPS * (np.abs(R0) * a[:, 0] + np.abs(R1) * a[:, 1] + np.abs(R2) * a[:, 2] + np.abs(t[:, r]))
            q.append(qr); l.append(qr - e - m); u.append(qr + e + m)
        behind = (q[2] if variant == "centre_behind" else u[2]) <= F(0)
        out = behind | edge_outside(l[0], u[0], l[2], u[2], fx, cx, w, variant) | edge_outside(l[1], u[1], l[2], u[2], fy, cy, h, variant)
    return ~out


def centre(G_o, G_s, i):
    """voxel_project's own expression for the centre of voxel index i (any shape broadcast against o and s)"""
    return G_o + (np.asarray(i).astype(F) + F(0.5)) * G_s


def brick_box(T, form):
    """lo, hi (n, 3) of the rows of a brick table (tests/cull_cases.py BRICK) as a kernel forms them: "rebuild" = the brick's last voxel
    inside the volume, min(i0 + n, dim) - 1 (volume_fuse_kernel); "map" = i0 + 7 (map_fuse_kernel, bricks of 8 x 8 x 8)"""
    last = np.minimum(T["i0"] + T["n"], T["dim"]) - 1 if form == "rebuild" else T["i0"] + 7
    s = T["s"][:, None]
    return centre(T["o"], s, T["i0"]), centre(T["o"], s, last)


def decide(T, form, variant=None):
    """box_can_update of every row of a brick table, the box formed as `form` says"""
    lo, hi = brick_box(T, form)
    return box_can_update(lo, hi, (T["fx"], T["fy"], T["cx"], T["cy"], T["w"], T["h"]), T["R"], T["t"], variant)


FAR = F(1e30)                                                     # the one valid depth, far beyond every volume


def far_plane(cam):
    """the vertex map of an all-valid depth plane at FAR: every voxel that projects into the image is updated"""
    V = np.zeros((int(cam[4]) * int(cam[5]), 3), F)
    V[:, 2] = FAR
    return V


def updated(G, cam, pose):
    """(d2, d1, d0) bool: the voxels that pass volume_oracle.integrate's projection test with all depth valid"""
    return VO.integrate(G.empty(), G, far_plane(cam), cam, pose, with_mask=True)[1]


def brick_counts(mask, brick):
    """per brick of the volume (x fastest, then y, then z; ragged ends included): how many of its voxels the mask holds"""
    d2, d1, d0 = mask.shape
    n = [-(-d // b) for d, b in zip((d0, d1, d2), brick)]
    pad = np.zeros((n[2] * brick[2], n[1] * brick[1], n[0] * brick[0]), np.int64)
    pad[:d2, :d1, :d0] = mask
    return pad.reshape(n[2], brick[2], n[1], brick[1], n[0], brick[0]).sum((1, 3, 5)).reshape(-1)


def needed(G, brick, cam, pose):
    """per brick of the volume, in the order of brick_counts: does any voxel of it update with all depth valid?"""
    return brick_counts(updated(G, cam, pose), brick) > 0
