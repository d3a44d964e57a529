"""numpy statement of the volume term of include/rgbd_pose_hip.h Part 3 ("Volume term": rpe_sdf_rows, rpe_sdf_normal_eq, rpe_icp_sdf,
rpe_icp_pyramid_sdf), the contract the kernels sdf_rows_kernel and icp_sdf_kernel of csrc/rpe_frontend.hip are held to: BIT-EXACTLY for
everything per pixel (world point, cell, corner gates, value, gradient, row -- every expression is IEEE fp32 in the written order,
the rule is compiled without FMA contraction), and to a rounding bound for the sums (record() returns the fp64 sums of the exact
products of the fp32 rows and, per entry, the sum of their magnitudes).  Built on volume_oracle (the geometry's casts, the lerp) and
frontend_oracle (the pose's cast, to_world); a volume is (d2, d1, d0, 2) as rpe_volume_download returns it."""
import numpy as np

import photo_oracle as PH
import volume_oracle as VO
from frontend_util import FO

F = np.float32
NAN = F(np.nan)
L = VO._lerp


def rows(vol, G, V, N, pose12, dist_thr, cos_thr, use_normals=True, stages=None):
    """steps 1-8 per frame pixel: V, N (n, 3) the frame's vertices and normals in its camera.  Returns r (n,), J (n, 6) -- NaN where the
    pixel has no row -- and the row mask.  stages (a dict) receives the mask of every gate on its own: finite, cell, known, band,
    distance, slope, normal_finite, cosine, and nan_tsdf (a corner's tsdf is NaN)."""
    R, t = FO._pose_f(pose12)
    gate, c, k = F(dist_thr), F(cos_thr), F(G.tr / G.s)
    V, N = np.asarray(V, F), np.asarray(N, F)
    d0, d1, d2 = G.dim
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        finite = np.isfinite(V).all(1)
        W = FO._to_world(R, t, V)
        g = [(W[:, a] - G.o[a]) / G.s - F(0.5) for a in range(3)]
        i0 = [np.floor(x) for x in g]
        cell = np.ones(len(V), bool)
        for a in range(3):
            cell &= (i0[a] >= F(0)) & (i0[a] <= F(G.dim[a] - 2))
        ax, ay, az = [g[a] - i0[a] for a in range(3)]
        inside = finite & cell
        i, j, kk = [np.where(inside, i0[a], F(0)).astype(np.int64) for a in range(3)]
        flat = vol.reshape(-1, 2)
        base = (kk * d1 + j) * d0 + i
        v = {(di, dj, dk): flat[base + di + dj * d0 + dk * d0 * d1] for dk in (0, 1) for dj in (0, 1) for di in (0, 1)}
        known, band, nan_tsdf = np.ones(len(V), bool), np.ones(len(V), bool), np.zeros(len(V), bool)
        for corner in v.values():
            known &= corner[:, 1] > F(0)
            band &= np.abs(corner[:, 0]) < F(1.0)
            nan_tsdf |= np.isnan(corner[:, 0])
        T = {key: corner[:, 0] for key, corner in v.items()}
        D = L(L(L(T[0, 0, 0], T[1, 0, 0], ax), L(T[0, 1, 0], T[1, 1, 0], ax), ay),
              L(L(T[0, 0, 1], T[1, 0, 1], ax), L(T[0, 1, 1], T[1, 1, 1], ax), ay), az)
        r = D * G.tr
        distance = np.abs(r) <= gate
        gx = L(L(T[1, 0, 0] - T[0, 0, 0], T[1, 1, 0] - T[0, 1, 0], ay), L(T[1, 0, 1] - T[0, 0, 1], T[1, 1, 1] - T[0, 1, 1], ay), az)
        gy = L(L(T[0, 1, 0] - T[0, 0, 0], T[1, 1, 0] - T[1, 0, 0], ax), L(T[0, 1, 1] - T[0, 0, 1], T[1, 1, 1] - T[1, 0, 1], ax), az)
        gz = L(L(T[0, 0, 1] - T[0, 0, 0], T[1, 0, 1] - T[1, 0, 0], ax), L(T[0, 1, 1] - T[0, 1, 0], T[1, 1, 1] - T[1, 1, 0], ax), ay)
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        slope = ln > F(0)
        nx, ny, nz = gx * k, gy * k, gz * k
        a = [-((R[3 * m] * nx + R[3 * m + 1] * ny) + R[3 * m + 2] * nz) for m in range(3)]
        normal_finite = np.isfinite(N).all(1)
        cosine = (-((a[0] * N[:, 0] + a[1] * N[:, 1]) + a[2] * N[:, 2])) / (ln * k) >= c
        ok = inside & known & band & distance & slope
        if use_normals:
            ok = ok & normal_finite & cosine
        x, y, z = V[:, 0], V[:, 1], V[:, 2]
        J = np.stack([a[0], a[1], a[2], y * a[2] - z * a[1], z * a[0] - x * a[2], x * a[1] - y * a[0]], -1)
    assert r.dtype == F and J.dtype == F and D.dtype == F
    if stages is not None:
        stages.update(finite=finite, cell=cell, known=known, band=band, distance=distance, slope=slope, normal_finite=normal_finite,
                      cosine=cosine, nan_tsdf=nan_tsdf, i0=i0, value=D)
    return np.where(ok, r, NAN).astype(F), np.where(ok[:, None], J, NAN).astype(F), ok


def record(r, J, ok):
    """the record of rpe_sdf_normal_eq from the fp32 rows: fp64 sums of the EXACT products -- H upper triangle (21) | g (6) | [27] sum
    r^2 | [28] rows -- and, per entry, the sum of the products' magnitudes (photo_oracle.record with the weight 1)"""
    return PH.record(r, J, ok, 1.0)


def icp_sdf(oracle_lib, vol, G, V, N, pose, iters, dist_thr, cos_thr, use_normals=True, tol=0.0):
    """the loop of rpe_icp_sdf on one level in the oracles: rows (numpy fp32), their fp64 record, the C oracle's solve and exp-map.
    Returns the pose and per round (rows, |delta|, cost)."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for _ in range(iters):
        rec, _ = record(*rows(vol, G, V, N, p, dist_thr, cos_thr, use_normals))
        d, _ = oracle_lib.gn_solve(rec[:29])
        p = oracle_lib.gn_apply(d, p)
        hist.append((int(rec[28]), float(np.linalg.norm(d)), float(rec[27])))
        if np.linalg.norm(d) < tol:
            break
    return p, hist


def icp_pyramid_sdf(oracle_lib, vol, G, frame_pyr, pose, iters, gates, cos_thr, use_normals=True):
    """coarse to fine over len(iters) levels: frame_pyr = pyramid_oracle.frame_pyramid's levels.  Returns the pose and level 0's history."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for l in range(len(iters) - 1, -1, -1):
        if iters[l] < 1:
            continue
        _, V, N, _ = frame_pyr[l]
        p, hist = icp_sdf(oracle_lib, vol, G, V, N, p, iters[l], gates[l], cos_thr, use_normals)
    return p, hist
