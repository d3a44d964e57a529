"""numpy statement of the photometric term of include/rgbd_pose_hip.h Part 3 ("Photometric term": rpe_photo_prepare, rpe_photo_rows,
rpe_photo_normal_eq, rpe_icp_rgbd), the contract the kernels of csrc/rpe_photo.hip are held to: BIT-EXACTLY for everything per pixel
(intensity pyramid, model map, residual and Jacobian row -- every expression is IEEE fp32 in the written order, the kernels are compiled
without FMA contraction), and to a rounding bound for the sums (record() returns the fp64 sums of the exact products of the fp32 rows
and, per entry, the sum of their magnitudes)."""
import numpy as np

from frontend_util import FO

F = np.float32
NAN = F(np.nan)


def intensity(rgba):
    """(h, w, 4) uint8 RGBA -> (h, w) float32: ((0.299 r + 0.587 g) + 0.114 b), NaN where A = 0"""
    c = np.asarray(rgba)
    r, g, b = c[..., 0].astype(F), c[..., 1].astype(F), c[..., 2].astype(F)
    i = ((F(0.299) * r + F(0.587) * g) + F(0.114) * b).astype(F)
    return np.where(c[..., 3] != 0, i, NAN).astype(F)


def downsample(I):
    """level l -> l+1: (((a + b) + c) + d) * 0.25 over a = (2u,2v), b = (2u+1,2v), c = (2u,2v+1), d = (2u+1,2v+1); NaN if any is"""
    h, w = I.shape[0] // 2, I.shape[1] // 2
    a, b = I[0:2 * h:2, 0:2 * w:2], I[0:2 * h:2, 1:2 * w:2]
    c, d = I[1:2 * h:2, 0:2 * w:2], I[1:2 * h:2, 1:2 * w:2]
    with np.errstate(invalid="ignore"):
        return ((((a + b) + c) + d) * F(0.25)).astype(F)


def intensity_pyramid(I0, levels):
    """[(h_l, w_l) float32] from a level-0 intensity image (intensity(rgba), or any float image for the derivative checks)"""
    out = [np.asarray(I0, F)]
    for _ in range(1, levels):
        out.append(downsample(out[-1]))
    return out


def model_map(I, MV, MN, mpose12):
    """one level of the model photometric map, (h*w, 4) float32 {I, gx, gy, zm}: central differences of I (NaN on the border or beside
    a NaN), zm = z of the model vertex in the model camera, NaN where the model normal is"""
    h, w = I.shape
    Rm, tm = FO._pose_f(mpose12)
    gx, gy = np.full((h, w), NAN, F), np.full((h, w), NAN, F)
    with np.errstate(invalid="ignore"):
        if w > 2:
            gx[:, 1:-1] = F(0.5) * (I[:, 2:] - I[:, :-2])
        if h > 2:
            gy[1:-1, :] = F(0.5) * (I[2:, :] - I[:-2, :])
        zm = (((Rm[6] * MV[:, 0] + Rm[7] * MV[:, 1]) + Rm[8] * MV[:, 2]) + tm[2]).astype(F)
    zm = np.where(np.isnan(MN).any(1), NAN, zm).astype(F)
    return np.stack([I.reshape(-1), gx.reshape(-1), gy.reshape(-1), zm], -1).astype(F)


def model_maps(I0, model_pyr, mpose12):
    """every level: model_pyr = [(MV_l, MN_l)] as pyramid_oracle.model_pyramid returns it"""
    return [model_map(I, MV, MN, mpose12) for I, (MV, MN) in zip(intensity_pyramid(I0, len(model_pyr)), model_pyr)]


def _lerp(p, q, s):
    return (p + (q - p) * s).astype(F)


def rows(V, If, pmap, mcam, pose12, mpose12, dist_thr):
    """steps 1-5 per frame pixel: V (n, 3) frame vertices, If (n,) frame intensity, pmap (w*h, 4) the model map of the level.
    Returns r (n,), J (n, 6) -- unscaled, NaN where there is no pair -- and the pair mask."""
    fx, fy, cx, cy, w, h = FO._cam(mcam)
    R, t = FO._pose_f(pose12)
    Rm, tm = FO._pose_f(mpose12)
    d = F(dist_thr)
    V, If = np.asarray(V, F), np.asarray(If, F).reshape(-1)
    n = len(V)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(V).all(1) & np.isfinite(If)
        W = FO._to_world(R, t, V)
        wx, wy, wz = W[:, 0], W[:, 1], W[:, 2]
        px = Rm[0] * wx + Rm[1] * wy + Rm[2] * wz + tm[0]
        py = Rm[3] * wx + Rm[4] * wy + Rm[5] * wz + tm[1]
        pz = Rm[6] * wx + Rm[7] * wy + Rm[8] * wz + tm[2]
        ok &= pz > F(0)
        xs, ys = fx * (px / pz) + cx, fy * (py / pz) + cy
        x0, y0 = np.floor(xs), np.floor(ys)
        ok &= (x0 >= F(0)) & (x0 <= F(w - 2)) & (y0 >= F(0)) & (y0 <= F(h - 2))
        j = np.where(ok, y0, 0).astype(np.int64) * w + np.where(ok, x0, 0).astype(np.int64)
        pick = lambda o: pmap[np.where(ok, j + o, 0)]   # noqa: E731
        m00, m10, m01, m11 = pick(0), pick(1), pick(w), pick(w + 1)
        for m in (m00, m10, m01, m11):
            ok &= np.isfinite(m).all(1) & (np.abs(m[:, 3] - pz) <= d)
        a, b = xs - x0, ys - y0
        bil = lambda k: _lerp(_lerp(m00[:, k], m10[:, k], a), _lerp(m01[:, k], m11[:, k], a), b)   # noqa: E731
        Is, Gx, Gy = bil(0), bil(1), bil(2)
        r = Is - If
        gfx, gfy = Gx * fx, Gy * fy
        qx, qy, qz = gfx / pz, gfy / pz, -((gfx * px + gfy * py) / (pz * pz))
        A = [[-((Rm[3 * i] * R[3 * k] + Rm[3 * i + 1] * R[3 * k + 1]) + Rm[3 * i + 2] * R[3 * k + 2]) for k in range(3)] for i in range(3)]
        ax, ay, az = [(qx * A[0][k] + qy * A[1][k]) + qz * A[2][k] for k in range(3)]
        x, y, z = V[:, 0], V[:, 1], V[:, 2]
        J = np.stack([ax, ay, az, y * az - z * ay, z * ax - x * az, x * ay - y * ax], -1)
    assert r.dtype == F and J.dtype == F and len(r) == n
    return np.where(ok, r, NAN).astype(F), np.where(ok[:, None], J, NAN).astype(F), ok


def record(r, J, ok, weight):
    """the record of rpe_photo_normal_eq from the fp32 rows r' = lam * r, J' = lam * J (lam = float32(weight)): fp64 sums of the EXACT
    products (a product of two fp32 values is exact in fp64) -- H upper triangle (21) | g (6) | [27] sum r'^2 | [28] pairs -- and, per
    entry, the sum of the products' magnitudes"""
    lam = F(weight)
    rp = (lam * r[ok]).astype(F).astype(np.float64)
    Jp = (lam * J[ok]).astype(F).astype(np.float64)
    rec, S = np.zeros(32), np.zeros(32)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            p = Jp[:, a] * Jp[:, b]
            rec[k], S[k] = p.sum(), np.abs(p).sum()
            k += 1
        p = Jp[:, a] * rp
        rec[21 + a], S[21 + a] = p.sum(), np.abs(p).sum()
    rec[27] = S[27] = (rp * rp).sum()
    rec[28] = S[28] = float(ok.sum())
    return rec, S


def icp_rgbd(oracle_lib, V, N, B, If, MV, MN, pmap, mcam, pose, mpose, iters, dist_thr, cos_thr, weight, tol=0.0):
    """the loop of rpe_icp_rgbd on one level in the oracles: associate (numpy fp32) + point-to-plane normal equations (C oracle), the
    photometric record above, H and g added, solve, exp-map.  weight = None: ICP alone.  Returns the pose and per round
    (geometric pairs, photometric pairs, |delta|)."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for _ in range(iters):
        XW, XC, _, _, NC, cnt = FO.associate(V, N, B, MV, MN, mcam, p, mpose, dist_thr, cos_thr, True)
        ne = oracle_lib.gn_normal_eq(1, XW, XC, NC, pose=p)
        pcnt = 0
        if weight is not None:
            rec, _ = record(*rows(V, If, pmap, mcam, p, mpose, dist_thr), weight)
            ne[:27] += rec[:27]
            pcnt = int(rec[28])
        d, _ = oracle_lib.gn_solve(ne)
        p = oracle_lib.gn_apply(d, p)
        hist.append((cnt, pcnt, float(np.linalg.norm(d))))
        if np.linalg.norm(d) < tol:
            break
    return p, hist


def icp_pyramid_rgbd(oracle_lib, frame_pyr, fint, model_pyr, pmaps, cam, pose, mpose, iters, gates, cos_thr, weight):
    """coarse to fine over len(iters) levels: frame_pyr = pyramid_oracle.frame_pyramid's levels, fint = intensity_pyramid of the frame,
    model_pyr / pmaps the model's levels"""
    import pyramid_oracle as PO
    p = np.array(pose, np.float64).copy()
    for l in range(len(iters) - 1, -1, -1):
        if iters[l] < 1:
            continue
        _, V, N, B = frame_pyr[l]
        p, _ = icp_rgbd(oracle_lib, V, N, B, fint[l].reshape(-1), *model_pyr[l], None if pmaps is None else pmaps[l], PO.level_camera(cam, l), p,
                        mpose, iters[l], gates[l], cos_thr, weight)
    return p
