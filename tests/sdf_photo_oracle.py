"""numpy statement of the volume colour term of include/rgbd_pose_hip.h Part 3 ("Volume colour term": rpe_sdf_photo_rows,
rpe_sdf_photo_normal_eq, rpe_icp_sdf_rgbd, rpe_icp_pyramid_sdf_rgbd), the contract the kernels of csrc/rpe_sdf_photo.hpp are held to:
BIT-EXACTLY for everything per pixel (cell, gates, the corners' luma, value, gradient, row -- IEEE fp32 in the written order, no FMA
contraction) and to a rounding bound for the sums.  Composed from sdf_oracle (the cell and the TSDF gates: its stages), color_oracle
(f32, the corner layout: a colour volume is (d2, d1, d0, 4) binary16 bit patterns) and photo_oracle (intensity, intensity_pyramid,
record).  The geometric row beside it is sdf_oracle.rows, unchanged."""
import numpy as np

import color_oracle as CO
import photo_oracle as PH
import sdf_oracle as SO
import volume_oracle as VO
from frontend_util import FO

F = np.float32
NAN = F(np.nan)
L = VO._lerp


def luma(c):
    """(n, 4) fp32 {r, g, b, wc} of a corner -> ((0.299 r + 0.587 g) + 0.114 b), the photometric term's intensity on 0 .. 255"""
    return ((F(0.299) * c[:, 0] + F(0.587) * c[:, 1]) + F(0.114) * c[:, 2]).astype(F)


def rows(vol, cvol, G, V, If, pose12, dist_thr, stages=None):
    """steps 1-5 per frame pixel: V (n, 3) the frame's vertices, If (n,) its intensity.  Returns r (n,), J (n, 6) -- UNSCALED, NaN
    where the pixel has no row -- and the row mask.  stages receives sdf_oracle's masks (finite, cell, known, band, distance ...) and
    intensity (If finite), colour (all eight colour weights > 0), value (Iv).  A colour channel that is NaN or Inf under a weight > 0 is
    NOT gated: it propagates into r and J of a row that stands (and is counted), as any other value would."""
    V, If = np.asarray(V, F), np.asarray(If, F).reshape(-1)
    R, t = FO._pose_f(pose12)
    st = {}
    # steps 1-2 and the TSDF gates of step 2 are the volume term's: its stages at this gate (slope and normal gates are not asked)
    SO.rows(vol, G, V, np.zeros_like(V), pose12, dist_thr, 0.0, False, st)
    d0, d1, d2 = G.dim
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inside = st["finite"] & st["cell"]
        W = FO._to_world(R, t, V)
        g = [(W[:, a] - G.o[a]) / G.s - F(0.5) for a in range(3)]
        ax, ay, az = [g[a] - st["i0"][a] for a in range(3)]
        i, j, k = [np.where(inside, st["i0"][a], F(0)).astype(np.int64) for a in range(3)]
        flat = cvol.reshape(-1, 4)
        base = (k * d1 + j) * d0 + i
        c = {(di, dj, dk): CO.f32(flat[base + di + dj * d0 + dk * d0 * d1]) for dk in (0, 1) for dj in (0, 1) for di in (0, 1)}
        colour = np.ones(len(V), bool)
        for corner in c.values():
            colour &= corner[:, 3] > F(0)
        Y = {key: luma(corner) for key, corner in c.items()}
        Iv = L(L(L(Y[0, 0, 0], Y[1, 0, 0], ax), L(Y[0, 1, 0], Y[1, 1, 0], ax), ay),
               L(L(Y[0, 0, 1], Y[1, 0, 1], ax), L(Y[0, 1, 1], Y[1, 1, 1], ax), ay), az)
        gx = L(L(Y[1, 0, 0] - Y[0, 0, 0], Y[1, 1, 0] - Y[0, 1, 0], ay), L(Y[1, 0, 1] - Y[0, 0, 1], Y[1, 1, 1] - Y[0, 1, 1], ay), az)
        gy = L(L(Y[0, 1, 0] - Y[0, 0, 0], Y[1, 1, 0] - Y[1, 0, 0], ax), L(Y[0, 1, 1] - Y[0, 0, 1], Y[1, 1, 1] - Y[1, 0, 1], ax), az)
        gz = L(L(Y[0, 0, 1] - Y[0, 0, 0], Y[1, 0, 1] - Y[1, 0, 0], ax), L(Y[0, 1, 1] - Y[0, 1, 0], Y[1, 1, 1] - Y[1, 1, 0], ax), ay)
        mx, my, mz = gx / G.s, gy / G.s, gz / G.s
        a = [-((R[3 * m] * mx + R[3 * m + 1] * my) + R[3 * m + 2] * mz) for m in range(3)]
        r = Iv - If
        x, y, z = V[:, 0], V[:, 1], V[:, 2]
        J = np.stack([a[0], a[1], a[2], y * a[2] - z * a[1], z * a[0] - x * a[2], x * a[1] - y * a[0]], -1)
        intensity = np.isfinite(If)
        ok = inside & intensity & st["known"] & st["band"] & st["distance"] & colour
    assert r.dtype == F and J.dtype == F and Iv.dtype == F
    if stages is not None:
        stages.update(st, intensity=intensity, colour=colour, value=Iv, tsdf=st["value"])
    return np.where(ok, r, NAN).astype(F), np.where(ok[:, None], J, NAN).astype(F), ok


def record(r, J, ok, weight):
    """the record of rpe_sdf_photo_normal_eq: photo_oracle.record of the rows scaled by float32(weight)"""
    return PH.record(r, J, ok, weight)


def combined(geo, pho, weight):
    """the combined round's record from the two terms' rows (r, J, ok): H | g of both (27), [27] geometric cost, [28] geometric rows,
    [29] photometric cost, [30] photometric rows -- and, per entry, the sum of the products' magnitudes"""
    rg, Sg = SO.record(*geo)
    rp, Sp = PH.record(*pho, weight)
    rec, S = np.zeros(32), np.zeros(32)
    rec[:27], S[:27] = rg[:27] + rp[:27], Sg[:27] + Sp[:27]
    rec[27:29], S[27:29] = rg[27:29], Sg[27:29]
    rec[29:31], S[29:31] = rp[27:29], Sp[27:29]
    return rec, S


def icp_sdf_rgbd(oracle_lib, vol, cvol, G, V, N, If, pose, iters, dist_thr, cos_thr, weight, use_normals=True, tol=0.0):
    """the loop of rpe_icp_sdf_rgbd on one level in the oracles: both terms' rows (numpy fp32), their fp64 record, the C oracle's solve
    and exp-map.  weight = None: the volume term alone.  Returns the pose and per round (geometric rows, photometric rows, |delta|)."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for _ in range(iters):
        geo = SO.rows(vol, G, V, N, p, dist_thr, cos_thr, use_normals)
        if weight is None:
            rec, pcnt = SO.record(*geo)[0], 0
        else:
            rec, _ = combined(geo, rows(vol, cvol, G, V, If, p, dist_thr), weight)
            pcnt = int(rec[30])
        d, _ = oracle_lib.gn_solve(rec[:29])
        p = oracle_lib.gn_apply(d, p)
        hist.append((int(rec[28]), pcnt, float(np.linalg.norm(d))))
        if np.linalg.norm(d) < tol:
            break
    return p, hist


def icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, frame_pyr, fint, pose, iters, gates, cos_thr, weight, use_normals=True):
    """coarse to fine over len(iters) levels: frame_pyr = pyramid_oracle.frame_pyramid's levels, fint = photo_oracle.intensity_pyramid
    of the frame.  Returns the pose and level 0's history."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for l in range(len(iters) - 1, -1, -1):
        if iters[l] < 1:
            continue
        _, V, N, _ = frame_pyr[l]
        p, hist = icp_sdf_rgbd(oracle_lib, vol, cvol, G, V, N, fint[l].reshape(-1), p, iters[l], gates[l], cos_thr, weight, use_normals)
    return p, hist
