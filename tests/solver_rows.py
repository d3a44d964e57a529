"""The Gauss-Newton normal equations of the five residual kinds as plain numpy in np.longdouble (CPU only): Jacobian rows, the 29-entry
record, the majorant S on which rounding acts, an emulation of the kernels' precision plan with planted defects, and dyadic problems on
which no rounding can occur.  Independent of the C++ oracle (oracle/orc_gn.hpp): tests/test_solver_rows_oracle.py holds the two against
each other.

Record: H upper triangle row-major (21) | g = J^T W r (6) | sum w r^2 | sum w.  Conventions of oracle/orc_gn.hpp: p = R x + t,
T <- exp(delta) T, dp / ddelta = [I | -[p]x], so a residual a . p has the row [a ; p x a].

THE BOUND.  |device - record| <= c u S + (C64 + D) 2^-53 S64 entrywise, u = 2^-24 (fp32 arrays) or 2^-53 (fp64 arrays).
 S    the record formed over MAGNITUDE rows: every sum inside a Jacobian entry replaced by the sum of the absolute values of its terms
      ((p x n).x -> |p_y| |n_z| + |p_z| |n_y|), |r| for r.  The scale on which the array-dtype roundings act.
 c    roundings in the array dtype that one summed product goes through, counted in the code and doubled (C below).
 S64  the same sums with the fp64 part's own magnitudes: |R| |x| + |t| for |p| and the magnitudes of the residual's terms for |r| (the
      point-to-plane residual n . (p - Xc) is a cancelling sum of terms of size |n| (|p| + |Xc|)).  The transform and the residual are
      formed in fp64 (rpe_reduce.hpp transform: 3 fused multiply-adds; the residual: a subtraction and up to 3 more): 7 roundings of
      2^-53 relative to THOSE magnitudes, doubled: C64 = 14.  For fp32 arrays this term is five orders below the first; for fp64 arrays
      it is what bounds g and the cost near the optimum, where |r| is a thousandth of its terms.
 D    the fp64 additions between a per-group sum and the record (a thread's trips, 6 reduce-scatter levels of the wave, up to 8 waves,
      one record per workgroup): reduction_depth().  Negligible for fp32 arrays, part of the error for fp64 arrays.

Counting c (rpe_residuals.hpp, rpe_joint.hip).  Every count is of relative roundings u of a summed product w J_a J_b (or w J_a r, w r r),
measured against the product of the MAGNITUDE rows; an FMA is one rounding; a reciprocal or reciprocal square root of the hardware is
taken at 1 ulp (documented for v_rcp_f32 / v_rsq_f32; it cannot be measured on a CPU).  A span is what shares one array-dtype partial
sum: P kShare correspondences in two lanes (one-launch kernels), P correspondences in one lane (joint kernel).  The joint kernel
multiplies w by the term's scale: + 1.  The largest entry's count is doubled for slack.
 point-to-plane  J_a = (p x n)_k: p rounded 1, product 1, subtraction 1 = 3 (n is exact).  H: 3 + 3, w J_a 1, chain 2 kShare = 4 FMAs,
                 lane add 1 = 12, joint 13.  g: 3 + 1 + r rounded 1 + 4 + 1 = 10.  cost: r 2, w r 1, 4, 1 = 8.                  c = 26
 point-to-point  17 structured sums.  w p p^T: p 2, w p 1, chain 2, lane 1 = 6 (joint: chain 4, scale 1, one addition in expand_into: 9).
                 p x w r: p 1, r 1, w r 1, two products and a subtraction 2, chain 2, lane 1 = 8 (joint: two FMAs per correspondence,
                 chain 8, scale 1 = 12).  cost: r 2, w r 1, chain 3 x 2, lane 1 = 10 (joint 10).                               c = 24
 normal-normal   the rotation block of point-to-point with q = R Nw for p (joint kernel only).                                  c = 24
 reprojection    1 / p_z: p 1, reciprocal 1 = 2.  g_1 = -(p_x ipz) ipz: 1 + 2 + 1 + 2 + 1 = 7.  Largest J entry p_z ipz - p_x g_1:
                 max(3, 1 + 7 + 1) + FMA 1 = 10.  H: 10 + 10, w J_a 1, chain 2 rows x 2 = 4, lane 1 = 26, joint 27.  r = n inv: n 1, inv =
                 ipz rcp(bv_z) 2 + 1 + 1 = 4, product 1 = 6; g: 10 + 1 + 6 + 5 = 22.                                           c = 54
 bearing         1 / |p|: three FMAs and the reciprocal square root = 4.  e_k (tangent_basis): addition, reciprocal, product, FMA = 4.
                 a_k = (e_k - rho h_k) inv against (|e_k| + |rho| |h_k|) / |p|: the e part 4 + FMA 1 + inv 4 + product 1 = 10; the rho h part
                 rho = d inv (d rounded 1, inv 4, product 1 = 6), h = p inv (p 1, inv 4 = 5), FMA 1, inv 4, product 1 = 17; the larger,
                 17.  J_a = (p x a)_k: p 1 + 17 + product and subtraction 2 = 20.  H: 20 + 20,
                 weight w |bv|^2 3 FMAs + product = 4, w J_a 1, chain 2 rows x 2 kShare = 16, lane 1 = 62, joint 63.             c = 126
                 (above the 64 the issue hoped for: the sharpness list of the bearing kind in tests/test_solver_rows_oracle.py is shorter.)
tests/test_solver_rows_oracle.py checks that the plan itself (emulate, without FMA: more roundings than the device) stays inside c / 2, so
that c is not a fit to the device's output."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "solver_rows needs an np.longdouble with at least 64 bits of mantissa (x87 extended or better)"

P2P, P2PLANE, BEARING, NORMAL, REPROJ = 0, 1, 2, 3, 4          # = L.RES_* = oracle GN_*
NAMES = {P2P: "p2p", P2PLANE: "p2plane", BEARING: "bearing", NORMAL: "normal", REPROJ: "reproj"}
ROWS_PER = {P2P: 3, P2PLANE: 1, BEARING: 2, NORMAL: 3, REPROJ: 2}
K_SHARE = {P2P: 1, P2PLANE: 2, BEARING: 4, NORMAL: 1, REPROJ: 1}   # groups per widening, normal_eq_kernel
C = {P2P: 24, P2PLANE: 26, BEARING: 126, NORMAL: 24, REPROJ: 54}
C64 = 14
K_REPROJ_MIN_Z = 1e-6
# bearing: how far the array-dtype tangent basis (Duff et al., formed from bv as given) is off the true tangent plane, in units of u.
# Measured on the CPU with numpy division over the bearings of the cases below: 0.540 u (fp32), 0.902 u (fp64); the larger, times 4.
BEARING_DELTA_U = 3.61


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def group_width(dtype):
    return 4 if np.dtype(dtype) == np.float32 else 2


def reduction_depth(n, dtype):
    """fp64 additions between a per-group sum and the record, from above: trips x workgroups <= ceil(groups / 256) + 1, 6 levels in the
    wave, 8 waves."""
    groups = (n + group_width(dtype) - 1) // group_width(dtype)
    return (groups + 255) // 256 + 1 + 6 + 8


class Rows:
    """J, r, w: (m, 6), (m,), (m,) rows of the valid correspondences; Jm, rm the magnitude rows; Jf, rf those of the fp64 part (S64);
    wc, idx: weight and index of the valid correspondences (slot 28 sums wc)."""

    def __init__(self, J, r, w, Jm, rm, Jf, rf, wc, idx, per):
        self.J, self.r, self.w, self.Jm, self.rm, self.Jf, self.rf, self.wc, self.idx, self.per = J, r, w, Jm, rm, Jf, rf, wc, idx, per


def _cols(a, work):
    a = np.asarray(a)
    return a[:, 0].astype(work), a[:, 1].astype(work), a[:, 2].astype(work)


def valid(kind, arrays, pose, mask=None):
    """The kernels' own validity: b column not all NaN, mask == 1, reprojection: p_z and bv_z above kReprojMinZ."""
    a, b = np.asarray(arrays[0]), np.asarray(arrays[1])
    ok = ~np.isnan(b).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask) == 1
    if kind == REPROJ:
        pose = np.asarray(pose, np.float64)
        with np.errstate(invalid="ignore"):
            pz = a.astype(np.float64) @ pose[6:9] + pose[11]
            ok &= (pz > K_REPROJ_MIN_Z) & (b[:, 2].astype(np.float64) > K_REPROJ_MIN_Z)
    return ok


def tangent_basis(bx, by, bz):
    """rpe_residuals.hpp tangent_basis in the arithmetic of the arguments' dtype."""
    one = bx.dtype.type(1)
    sg = np.where(bz < 0, -one, one)
    a = -one / (sg + bz)
    bxa = bx * a
    c = bxa * by
    return (sg * bx * bxa + one, sg * c, -sg * bx), (c, by * by * a + sg, -by)


def _cross_rows(ax, ay, az, px, py, pz):
    """[a ; p x a]"""
    return [ax, ay, az, py * az - pz * ay, pz * ax - px * az, px * ay - py * ax]


def _cross_mag(ax, ay, az, px, py, pz):
    return [ax, ay, az, py * az + pz * ay, pz * ax + px * az, px * ay + py * ax]


def _kind_rows(kind, p, pm_list, x, b, c, R, work):
    """rows of one kind: list over row slots of (J6, r, [ (Jmag6, rmag) for pm in pm_list ]).  p: transformed point (3 columns), pm_list:
    magnitudes to use for |p| (the value's own, the fp64 part's)."""
    zero, one = np.zeros_like(p[0]), np.ones_like(p[0])
    out = []
    if kind in (P2P, NORMAL):
        eye = [(one, zero, zero), (zero, one, zero), (zero, zero, one)]
        for k in range(3):
            J = _cross_rows(*eye[k], *p)
            if kind == NORMAL:
                J[0] = J[1] = J[2] = zero
            mags = []
            for i, pm in enumerate(pm_list):
                Jm = _cross_mag(*eye[k], *pm)
                if kind == NORMAL:
                    Jm[0] = Jm[1] = Jm[2] = zero
                mags.append((Jm, np.abs(p[k] - b[k]) if i == 0 else pm[k] + np.abs(b[k])))
            out.append((J, p[k] - b[k], mags))
    elif kind == P2PLANE:
        J = _cross_rows(*c, *p)
        r = c[0] * (p[0] - b[0]) + c[1] * (p[1] - b[1]) + c[2] * (p[2] - b[2])
        ca = [np.abs(v) for v in c]
        mags = [(_cross_mag(*ca, *pm), np.abs(r) if i == 0 else sum(ca[k] * (pm[k] + np.abs(b[k])) for k in range(3))) for i, pm in enumerate(pm_list)]
        out.append((J, r, mags))
    elif kind == BEARING:
        bn = np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
        e1, e2 = tangent_basis(b[0] / bn, b[1] / bn, b[2] / bn)      # the exact tangent plane of bv
        ln = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        h = [v / ln for v in p]
        for e in (e1, e2):
            rho = e[0] * h[0] + e[1] * h[1] + e[2] * h[2]
            a = [(e[k] - rho * h[k]) / ln for k in range(3)]
            mags = []
            for i, pm in enumerate(pm_list):
                rm = np.abs(rho) if i == 0 else sum(np.abs(e[k]) * pm[k] for k in range(3)) / ln
                am = [(np.abs(e[k]) + rm * pm[k] / ln) / ln for k in range(3)]
                mags.append((_cross_mag(*am, *pm), rm))
            out.append((_cross_rows(*a, *p), rho, mags))
    elif kind == REPROJ:
        ipz = one / p[2]
        for q in range(2):
            g = -p[q] * ipz * ipz
            a = (ipz, zero, g) if q == 0 else (zero, ipz, g)
            r = p[q] / p[2] - b[q] / b[2]
            mags = []
            for i, pm in enumerate(pm_list):
                gm = pm[q] * ipz * ipz
                am = (ipz, zero, gm) if q == 0 else (zero, ipz, gm)
                rm = np.abs(r) if i == 0 else (pm[q] * np.abs(b[2]) + np.abs(b[q]) * pm[2]) / (p[2] * np.abs(b[2]))
                mags.append((_cross_mag(*am, *pm), rm))
            out.append((_cross_rows(*a, *p), r, mags))
    else:
        raise ValueError(kind)
    return out


def rows(kind, arrays, pose, mask=None, weight=None, dtype=np.float32, work=LD):
    """arrays = (a, b, c): world points | camera points or bearings | camera normals (point-to-plane); normal-normal: (Nw, Nc, None).
    The arrays are taken in `dtype` as given, the arithmetic is in `work` (np.longdouble)."""
    a, b = np.asarray(arrays[0], dtype), np.asarray(arrays[1], dtype)
    c = None if len(arrays) < 3 or arrays[2] is None else np.asarray(arrays[2], dtype)
    idx = np.flatnonzero(valid(kind, (a, b), pose, mask))
    pose = np.asarray(pose, np.float64).astype(work)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    x, bb = _cols(a[idx], work), _cols(b[idx], work)
    cc = None if c is None else _cols(c[idx], work)
    tt = np.zeros(3, work) if kind == NORMAL else t
    p = [R[k, 0] * x[0] + R[k, 1] * x[1] + R[k, 2] * x[2] + tt[k] for k in range(3)]
    pf = [np.abs(R[k, 0]) * np.abs(x[0]) + np.abs(R[k, 1]) * np.abs(x[1]) + np.abs(R[k, 2]) * np.abs(x[2]) + np.abs(tt[k]) for k in range(3)]
    wc = np.ones(len(idx), work) if weight is None else np.asarray(weight, dtype)[idx].astype(work)
    w = wc * (bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]) if kind == BEARING else wc
    slots = _kind_rows(kind, p, [[np.abs(v) for v in p], pf], x, bb, cc, R, work)
    stack = lambda get: np.concatenate([np.stack(get(s), axis=1) for s in slots]) if len(idx) else np.zeros((0, 6), work)
    cat = lambda get: np.concatenate([get(s) for s in slots]) if len(idx) else np.zeros(0, work)
    per = len(slots)
    return Rows(stack(lambda s: s[0]), cat(lambda s: s[1]), np.tile(w, per), stack(lambda s: s[2][0][0]), cat(lambda s: s[2][0][1]),
                stack(lambda s: s[2][1][0]), cat(lambda s: s[2][1][1]), wc, idx, per)


def _pack(J, r, w, wc):
    out = np.zeros(29, J.dtype)
    wJ = J * w[:, None]
    H = wJ.T @ J
    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[k] = H[a, b]; k += 1
    out[21:27] = wJ.T @ r
    out[27] = np.sum(w * r * r)
    out[28] = np.sum(wc)
    return out


def record(rw):
    """(rec29, S29)"""
    return _pack(rw.J, rw.r, rw.w, rw.wc), _pack(rw.Jm, rw.rm, np.abs(rw.w), np.abs(rw.wc))


def floor64(rw):
    """S64: the majorant of the fp64 part"""
    return _pack(rw.Jf, rw.rf, np.abs(rw.w), np.abs(rw.wc))


def bearing_extra(rw, dtype):
    """the additive term of the bearing kind: the array-dtype basis is off the tangent plane by delta, so rho is off by delta absolutely:
    delta sum w J^_a for g, 2 delta sum w |rho| for the cost"""
    d = BEARING_DELTA_U * unit(dtype)
    out = np.zeros(29, LD)
    out[21:27] = d * (rw.Jm * np.abs(rw.w)[:, None]).sum(axis=0)
    out[27] = 2 * d * np.sum(np.abs(rw.w) * rw.rm)
    return out


def bound(kind, rw, n, dtype, c=None):
    """entrywise bound of a single-kind record over slots 0..28 (slot 28: exact when the weights are all 1 -- the caller's check)"""
    _, S = record(rw)
    tol = (C[kind] if c is None else c) * unit(dtype) * S + (C64 + reduction_depth(n, dtype)) * 2.0 ** -53 * floor64(rw)
    if kind == BEARING:
        tol = tol + bearing_extra(rw, dtype)
    return tol


def measured_delta(bv, dtype):
    """max |e_i . bv^| of the array-dtype basis over the valid bearings, in units of u"""
    b = np.asarray(bv, dtype)
    b = b[~np.isnan(b).all(axis=1)]
    e1, e2 = tangent_basis(b[:, 0], b[:, 1], b[:, 2])
    bl = b.astype(LD)
    bl = bl / np.sqrt((bl * bl).sum(axis=1))[:, None]
    d = max(np.abs(sum(e[k].astype(LD) * bl[:, k] for k in range(3))).max() for e in (e1, e2))
    return float(d / unit(dtype))


# ---------------------------------------------------------------------------------------------- the precision plan
DEFECTS = ("residual_in_dtype", "pose_fp32", "drop", "double", "g0", "negate_min_H")


def emulate(kind, arrays, pose, mask=None, weight=None, dtype=np.float32, share=None, order=0, defect=None, scale=1.0, chunk=1 << 16):
    """The precision plan of rpe_residuals.hpp in numpy: transform and what cancels in fp64, rounded to the array dtype; J and the products
    in the array dtype; partial sums in the array dtype over P * share correspondences in two lanes; those summed in fp64 (order 0:
    pairwise, 1: one after the other from the back).  No FMA, numpy division for the hardware reciprocals: not the device's bits, the
    plan's error size.  defect: one of DEFECTS, never device code."""
    T = np.dtype(dtype).type
    share = K_SHARE[kind] if share is None else share
    a, b = np.asarray(arrays[0], dtype), np.asarray(arrays[1], dtype)
    c = None if len(arrays) < 3 or arrays[2] is None else np.asarray(arrays[2], dtype)
    idx = np.flatnonzero(valid(kind, (a, b), pose, mask))
    if defect == "drop":
        idx = idx[:-1]
    elif defect == "double":
        idx = np.concatenate([idx, idx[-1:]])
    pose = np.asarray(pose, np.float64)
    if defect == "pose_fp32":
        pose = pose.astype(np.float32).astype(np.float64)
    R, t = pose[:9].reshape(3, 3), (np.zeros(3) if kind == NORMAL else pose[9:])
    L = group_width(dtype) * share
    lanes = []
    for lo in range(0, len(idx), chunk - chunk % L):
        sel = idx[lo:lo + chunk - chunk % L]
        x = _cols(a[sel], np.float64)
        bT, b64 = _cols(b[sel], T), _cols(b[sel], np.float64)
        pd = [R[k, 0] * x[0] + R[k, 1] * x[1] + R[k, 2] * x[2] + t[k] for k in range(3)]
        p = [v.astype(T) for v in pd]
        wc = np.ones(len(sel), T) if weight is None else np.asarray(weight, dtype)[sel]
        w = T(scale) * wc
        inexact = defect == "residual_in_dtype"
        zero, one = np.zeros(len(sel), T), np.ones(len(sel), T)
        slots = []
        if kind in (P2P, NORMAL):
            eye = [(one, zero, zero), (zero, one, zero), (zero, zero, one)]
            for k in range(3):
                J = _cross_rows(*eye[k], *p)
                if kind == NORMAL:
                    J[0] = J[1] = J[2] = zero
                slots.append((J, p[k] - bT[k] if inexact else (pd[k] - b64[k]).astype(T)))
        elif kind == P2PLANE:
            nT, n64 = _cols(c[sel], T), _cols(c[sel], np.float64)
            if inexact:
                r = nT[0] * (p[0] - bT[0]) + nT[1] * (p[1] - bT[1]) + nT[2] * (p[2] - bT[2])
            else:
                r = (n64[0] * (pd[0] - b64[0]) + n64[1] * (pd[1] - b64[1]) + n64[2] * (pd[2] - b64[2])).astype(T)
            slots.append((_cross_rows(*nT, *p), r))
        elif kind == BEARING:
            e1, e2 = tangent_basis(*bT)
            inv = one / np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
            h = [v * inv for v in p]
            w = w * (bT[0] * bT[0] + bT[1] * bT[1] + bT[2] * bT[2])
            for e in (e1, e2):
                if inexact:
                    d = e[0] * p[0] + e[1] * p[1] + e[2] * p[2]
                else:
                    d = (e[0].astype(np.float64) * pd[0] + e[1].astype(np.float64) * pd[1] + e[2].astype(np.float64) * pd[2]).astype(T)
                rho = d * inv
                slots.append((_cross_rows(*[(e[k] - rho * h[k]) * inv for k in range(3)], *p), rho))
        elif kind == REPROJ:
            ipz = one / p[2]
            inv = ipz * (one / bT[2])
            for q in range(2):
                num = p[q] * bT[2] - bT[q] * p[2] if inexact else (pd[q] * b64[2] - b64[q] * pd[2]).astype(T)
                g = -(p[q] * ipz) * ipz
                av = (ipz, zero, g) if q == 0 else (zero, ipz, g)
                slots.append((_cross_rows(*av, *p), num * inv))
        else:
            raise ValueError(kind)
        m = len(sel)
        pad = (-m) % L
        terms = np.zeros((len(slots), m + pad, 29), T)
        for s, (J, r) in enumerate(slots):
            k = 0
            for i in range(6):
                wa = w * J[i]
                for j in range(i, 6):
                    terms[s, :m, k] = wa * J[j]; k += 1
                terms[s, :m, 21 + i] = wa * r
            terms[s, :m, 27] = (w * r) * r
        terms[0, :m, 28] = wc
        terms = terms.reshape(len(slots), -1, L // 2, 2, 29)
        acc = np.zeros((terms.shape[1], 2, 29), T)
        for j in range(L // 2):
            for s in range(len(slots)):
                acc = acc + terms[s, :, j]
        lanes.append((acc[:, 0] + acc[:, 1]).astype(np.float64))
    lane = np.concatenate(lanes) if lanes else np.zeros((0, 29))
    rec = lane.sum(axis=0) if order == 0 else (np.cumsum(lane[::-1], axis=0)[-1] if len(lane) else np.zeros(29))
    if defect == "g0":            # (normal-normal has no translation block: its first gradient entry is g[3])
        rec[24 if kind == NORMAL else 21] *= 1 + 1e-3
    elif defect == "negate_min_H":
        # the smallest entry that is not a structural zero (reprojection: J_1 and J_2 cancel in H[2][5] for every correspondence; what the
        # arithmetic leaves there is rounding): the smallest above 1e-5 of the largest -- "about 2e-5 of the maximum" in the scenes
        nz = np.flatnonzero(np.abs(rec[:21]) >= 1e-5 * np.abs(rec[:21]).max())
        rec[nz[np.argmin(np.abs(rec[nz]))]] *= -1
    return rec


# ---------------------------------------------------------------------------------------------- exact problems
class Exact:
    pass


def exact_problem(n, seed, dtype=np.float32):
    """Dyadic inputs on which no operation of the kernels rounds: world points k / 4 (|k| <= 8), R a signed permutation, t in quarters,
    normals in halves (not unit), Xc = p - k / 8, masks 0 / 1, weights in {0.5, 1, 2} (term scales {0.5, 1, 4} are the caller's).  Every
    summed product is a multiple of 2^-10; the function asserts that the magnitudes of any span's partial sum (8 correspondences, the widest) stay
    below 2^22 of that quantum (two bits left for the terms of a joint record, scales up to 4 included) and the whole sum below 2^53."""
    rng = np.random.default_rng(seed)
    E = Exact()
    perm, sign = rng.permutation(3), rng.choice([-1.0, 1.0], 3)
    E.R = np.zeros((3, 3)); E.R[np.arange(3), perm] = sign
    E.t = rng.integers(-4, 5, 3) / 4.0
    E.pose = np.concatenate([E.R.reshape(9), E.t])
    E.Q = (rng.integers(-8, 9, (n, 3)) / 4.0).astype(dtype)
    p = E.Q.astype(np.float64) @ E.R.T + E.t
    E.P = (p - rng.integers(-4, 5, (n, 3)) / 8.0).astype(dtype)
    E.N = (rng.integers(-2, 3, (n, 3)) / 2.0).astype(dtype)
    E.M = (rng.integers(-2, 3, (n, 3)) / 2.0).astype(dtype)
    E.mask = (rng.random(n) < 0.7).astype(np.int16)
    E.mask[rng.integers(0, n)] = 1
    E.weight = rng.choice([0.5, 1.0, 2.0], n).astype(dtype)
    E.n, E.dtype = n, dtype
    q = 2.0 ** 10
    for kind, arr in ((P2P, (E.Q, E.P, None)), (P2PLANE, (E.Q, E.P, E.N)), (NORMAL, (E.M, E.N, None))):
        rw = rows(kind, arr, E.pose, None, E.weight, dtype, work=np.float64)
        per, m = rw.per, len(rw.idx)
        for col in range(28):
            if col < 21:
                a, b = [(i, j) for i in range(6) for j in range(i, 6)][col]
                tm = rw.w * rw.Jm[:, a] * rw.Jm[:, b]
            elif col < 27:
                tm = rw.w * rw.Jm[:, col - 21] * rw.rm
            else:
                tm = rw.w * rw.rm * rw.rm
            tm = 4.0 * tm.reshape(per, m).sum(axis=0)               # the largest term scale
            assert np.array_equal(tm * q, np.rint(tm * q)), (kind, col)
            span = np.add.reduceat(tm, np.arange(0, m, 8)) if m else tm
            assert span.max(initial=0.0) * q < 2.0 ** 22, (kind, col, span.max())
            assert tm.sum() * q < 2.0 ** 53
    return E


def exact_record(E, terms, mask=None, weight=None):
    """the record of a (joint) objective on an exact problem, terms = [(kind, scale)]: fp64 is exact here (asserted budget)"""
    tot = np.zeros(29)
    arr = {P2P: (E.Q, E.P, None), P2PLANE: (E.Q, E.P, E.N), NORMAL: (E.M, E.N, None)}
    for kind, scale in terms:
        rec, _ = record(rows(kind, arr[kind], E.pose, mask, weight, E.dtype, work=np.float64))
        tot[:28] += scale * rec[:28]
        tot[28] += rec[28]
    return tot + 0.0


# ---------------------------------------------------------------------------------------------- the scenes both test files use
SIZES_B = [1, 5, 9, 63, 64, 65, 257, 1000, 4099]
FAMILIES = ("far", "near")
_scenes = {}


def scene(family, n, dtype, dressed):
    """far: util.scene_full defaults at a perturbed pose; near: n3d = 0.002, n2d = 0.5, nnl_deg = 0.2, no outliers, at the true pose.
    dressed: with a mask, weights and 5 % NaN columns (camera points and bearings).  Returns (scene, pose12, mask, weight)."""
    import util
    key = (family, n, np.dtype(dtype).name, dressed)
    if key not in _scenes:
        seed = 7000 + n + (500000 if family == "near" else 0) + (250000 if dressed else 0)
        nan = 0.05 if dressed and n >= 20 else 0.0
        if family == "near":
            sc = util.scene_full(seed, n, dtype, n2d=0.5, n3d=0.002, nnl_deg=0.2, outliers=0.0, nan_frac=nan)
        else:
            sc = util.scene_full(seed, n, dtype, nan_frac=nan)
        rng = np.random.default_rng(seed)
        Rp, tp = (sc.R, sc.t) if family == "near" else util.perturbed_pose(rng, sc.R, sc.t)
        mask = weight = None
        if dressed:
            if nan:
                sc.U[rng.permutation(n)[: max(1, int(nan * n))]] = np.nan
            mask = (rng.uniform(size=n) < 0.7).astype(np.int16)
            mask[0] = 1
            if n > 1 and not np.isnan(sc.P[n - 1]).all():
                mask[n - 1] = 1
            weight = rng.uniform(0.1, 2.0, n).astype(dtype)
        _scenes[key] = (sc, np.concatenate([np.asarray(Rp, np.float64).reshape(9), np.asarray(tp, np.float64)]), mask, weight)
    return _scenes[key]


def kind_arrays(sc, kind):
    return {P2P: (sc.Q, sc.P, None), P2PLANE: (sc.Q, sc.P, sc.N), BEARING: (sc.Q, sc.U, None), NORMAL: (sc.M, sc.N, None),
            REPROJ: (sc.Q, sc.U, None)}[kind]


def reference(kind, arrays, pose, n, dtype, mask=None, weight=None):
    """(rec29, S29, bound29, valid correspondences) of one kind, np.longdouble"""
    rw = rows(kind, arrays, pose, mask, weight, dtype)
    rec, S = record(rw)
    return rec, S, bound(kind, rw, n, dtype), len(rw.idx)


def joint_reference(refs_scales):
    """the same for a joint record from [(reference(...), scale)]: the bound is the sum of the terms' bounds times their scales (the + 1
    of scale x w is inside every c); slot 28 adds the terms' weight sums unscaled"""
    rec, S, tol = np.zeros(29, LD), np.zeros(29, LD), np.zeros(29, LD)
    for (r, s, t, _), scale in refs_scales:
        rec[:28] += scale * r[:28]; S[:28] += scale * s[:28]; tol[:28] += scale * t[:28]
        rec[28] += r[28]; S[28] += s[28]; tol[28] += t[28]
    return rec, S, tol, None


def assert_within(got, ref, dtype, weighted, what=""):
    """|got - rec| <= bound entrywise over slots 0..27; slot 28 exact without weights, within the bound with them.  Returns the worst
    error in units of u S (entries with S = 0 must be exact: their bound is 0) and as a fraction of the bound."""
    rec, S, tol, _ = ref
    err = np.abs(np.asarray(got[:29], np.float64).astype(LD) - rec)
    bad = np.flatnonzero(err[:28] > tol[:28])
    assert len(bad) == 0, (what, "entries", bad.tolist(), "error / bound", [float(err[i] / tol[i]) if tol[i] > 0 else math.inf for i in bad])
    if weighted:
        assert err[28] <= tol[28], (what, "weight sum", float(err[28]), float(tol[28]))
    else:
        assert got[28] == float(rec[28]), (what, "count", got[28], float(rec[28]))
    pos = tol[:28] > 0
    return (float(np.max(err[:28][pos] / (unit(dtype) * S[:28][pos]))), float(np.max(err[:28][pos] / tol[:28][pos]))) if pos.any() else (0.0, 0.0)


def check_record(kind, got, arrays, pose, n, dtype, mask=None, weight=None, what=""):
    """the entrywise check of a single-kind device record in one call"""
    return assert_within(got, reference(kind, arrays, pose, n, dtype, mask, weight), dtype, weight is not None, (what, NAMES[kind], n))
