"""numpy statement of the robust volume terms of include/rgbd_pose_hip.h Part 3 ("Robust volume terms": rpe_sdf_set_robust and what it
does to the normal-equation calls and loops of the four volume terms; rpe_sdf_robust_weights / rpe_map_sdf_robust_weights), the contract
the kernels of csrc/rpe_sdf_robust.hpp are held to: the weights BIT EXACTLY (csrc/rpe_sdf_robust_rule.hpp: IEEE fp32 in the written
order, no FMA contraction), the sums to the siblings' rounding bound.  A composition: the rows are sdf_oracle.rows and
sdf_photo_oracle.rows, unchanged; the map forms are the same statements on mapsdf_oracle.virtual / mapsdf_photo_oracle.virtual's dense
volumes of the box.  Only the weight and the weighted record are stated here."""
import numpy as np

import sdf_oracle as SO
import sdf_photo_oracle as SP

F = np.float32
NAN = F(np.nan)
NONE, HUBER, TUKEY = 0, 1, 3        # RPE_ROBUST_NONE / _HUBER / _TUKEY


def huber(r, k):
    """s = fabsf(r); w = s <= k ? 1.0f : k / s"""
    r, k = np.asarray(r, F), F(k)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(r)
        w = np.where(s <= k, F(1.0), k / s)
    assert w.dtype == F
    return w


def tukey(r, k):
    """u = r / k; q = 1.0f - u * u; w = fabsf(r) < k ? q * q : 0.0f"""
    r, k = np.asarray(r, F), F(k)
    with np.errstate(invalid="ignore", over="ignore"):
        u = r / k
        q = F(1.0) - u * u
        w = np.where(np.abs(r) < k, q * q, F(0.0))
    assert w.dtype == F
    return w


def weights(kind, r, k, ok=None):
    """the plane of weights of rows r: NaN where a pixel has no row (ok; None: where r is NaN), as the hook writes it.  kind NONE or
    k = 0 (a photometric plane with photo_k = 0): 1 for every row.  A row whose residual is not finite (a colour channel that is NaN or
    Inf under a weight > 0 goes through) gets what the rule makes of it"""
    r = np.asarray(r, F)
    ok = ~np.isnan(r) if ok is None else ok
    if kind == NONE or k == 0:
        w = np.ones_like(r)
    else:
        w = {HUBER: huber, TUKEY: tukey}[kind](r, k)
    return np.where(ok, w, NAN).astype(F)


def record(r, J, ok, w, lam=None):
    """the weighted record from the fp32 rows and fp32 weights: fp64 sums of w J J (H, 21) | w J r (g, 6) | [27] sum w r^2 | [28] EVERY
    row that passed the gates, weight 0 included -- and, per entry, the sum of the products' magnitudes.  lam: the photometric rows are
    r' = lam r, J' = lam J in fp32 first (photo_oracle.record); the weight is that of the UNSCALED r"""
    rp, Jp = r[ok], J[ok]
    if lam is not None:
        rp, Jp = (F(lam) * rp).astype(F), (F(lam) * Jp).astype(F)
    rp, Jp, wd = rp.astype(np.float64), Jp.astype(np.float64), np.asarray(w, F)[ok].astype(np.float64)
    rec, S = np.zeros(32), np.zeros(32)
    k = 0
    for a in range(6):
        x = wd * Jp[:, a]                        # exact in fp64: two floats
        for b in range(a, 6):
            p = x * Jp[:, b]
            rec[k], S[k] = p.sum(), np.abs(p).sum()
            k += 1
        p = x * rp
        rec[21 + a], S[21 + a] = p.sum(), np.abs(p).sum()
    rec[27] = S[27] = ((wd * rp) * rp).sum()
    rec[28] = S[28] = float(ok.sum())
    return rec, S


def geometric(vol, G, V, N, pose12, dist_thr, cos_thr, kind, k, use_normals=True):
    """(rows, weights, record, magnitudes) of the weighted volume term of one level"""
    geo = SO.rows(vol, G, V, N, pose12, dist_thr, cos_thr, use_normals)
    w = weights(kind, geo[0], k, geo[2])
    return geo, w, *record(*geo, w)


def photometric(vol, cvol, G, V, If, pose12, dist_thr, lam, kind, photo_k):
    """the same of the weighted photometric rows alone: the record of rpe_sdf_photo_normal_eq under the setting"""
    pho = SP.rows(vol, cvol, G, V, If, pose12, dist_thr)
    w = weights(kind, pho[0], photo_k, pho[2])
    return pho, w, *record(*pho, w, lam)


def combined(vol, cvol, G, V, N, If, pose12, dist_thr, cos_thr, lam, kind, k, photo_k, use_normals=True):
    """the combined round's record laid out as sdf_photo_oracle.combined's, and the magnitudes"""
    _, _, rg, Sg = geometric(vol, G, V, N, pose12, dist_thr, cos_thr, kind, k, use_normals)
    _, _, rp, Sp = photometric(vol, cvol, G, V, If, pose12, dist_thr, lam, kind, photo_k)
    rec, S = np.zeros(32), np.zeros(32)
    rec[:27], S[:27] = rg[:27] + rp[:27], Sg[:27] + Sp[:27]
    rec[27:29], S[27:29] = rg[27:29], Sg[27:29]
    rec[29:31], S[29:31] = rp[27:29], Sp[27:29]
    return rec, S


def icp_sdf(oracle_lib, vol, G, V, N, pose, iters, dist_thr, cos_thr, kind, k, use_normals=True, tol=0.0):
    """sdf_oracle.icp_sdf with the weighted record.  Returns the pose and per round (rows, |delta|, weighted cost)."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for _ in range(iters):
        rec = geometric(vol, G, V, N, p, dist_thr, cos_thr, kind, k, use_normals)[2]
        d, _ = oracle_lib.gn_solve(rec[:29])
        p = oracle_lib.gn_apply(d, p)
        hist.append((int(rec[28]), float(np.linalg.norm(d)), float(rec[27])))
        if np.linalg.norm(d) < tol:
            break
    return p, hist


def icp_pyramid_sdf(oracle_lib, vol, G, frame_pyr, pose, iters, gates, cos_thr, kind, k, use_normals=True):
    """sdf_oracle.icp_pyramid_sdf with the weighted record: the same k at every level"""
    p = np.array(pose, np.float64).copy()
    hist = []
    for l in range(len(iters) - 1, -1, -1):
        if iters[l] < 1:
            continue
        _, V, N, _ = frame_pyr[l]
        p, hist = icp_sdf(oracle_lib, vol, G, V, N, p, iters[l], gates[l], cos_thr, kind, k, use_normals)
    return p, hist


def icp_sdf_rgbd(oracle_lib, vol, cvol, G, V, N, If, pose, iters, dist_thr, cos_thr, lam, kind, k, photo_k, use_normals=True, tol=0.0):
    """sdf_photo_oracle.icp_sdf_rgbd with the weighted record.  Returns the pose and per round (geometric rows, photometric rows, |delta|)."""
    p = np.array(pose, np.float64).copy()
    hist = []
    for _ in range(iters):
        rec, _ = combined(vol, cvol, G, V, N, If, p, dist_thr, cos_thr, lam, kind, k, photo_k, use_normals)
        d, _ = oracle_lib.gn_solve(rec[:29])
        p = oracle_lib.gn_apply(d, p)
        hist.append((int(rec[28]), int(rec[30]), float(np.linalg.norm(d))))
        if np.linalg.norm(d) < tol:
            break
    return p, hist


def icp_pyramid_sdf_rgbd(oracle_lib, vol, cvol, G, frame_pyr, fint, pose, iters, gates, cos_thr, lam, kind, k, photo_k, use_normals=True):
    p = np.array(pose, np.float64).copy()
    hist = []
    for l in range(len(iters) - 1, -1, -1):
        if iters[l] < 1:
            continue
        _, V, N, _ = frame_pyr[l]
        p, hist = icp_sdf_rgbd(oracle_lib, vol, cvol, G, V, N, fint[l].reshape(-1), p, iters[l], gates[l], cos_thr, lam, kind, k, photo_k,
                               use_normals)
    return p, hist
