"""The numpy statement of the keyframe graph (include/rgbd_pose_hip.h Part 3, "Keyframe graph") on top of tests/feature_oracle.py: the
edges, the fp32 rows in the kernel's operation order, the records as fp64 sums of the exact products of those rows (with the sums of
the products' magnitudes, for the rounding bound), the dense solve, the gated Gauss-Newton loop and the apply step.  Links and rows
are the GPU's bits; records and poses are held to bounds derived in tests/test_gpu_graph.py."""
import numpy as np

import feature_oracle as FE
import keyframe_oracle as KO

F32, F64 = np.float32, np.float64
RECORD = 92
MIN_MATCHES = 12


# ---------------------------------------------------------------------------------------------- the graph
def link(keyframes, first=0, mopt=KO.MOPT, min_matches=MIN_MATCHES, edges=()):
    """[(j, i, a, b)] ordered by (j, i): the edges in `edges` whose newer keyframe is < first, and for every j >= first and i < j the
    match list of j's descriptors (the frame's) against i's (the model's), kept with >= min_matches pairs"""
    out = [e for e in edges if e[0] < first]
    for j in range(max(first, 1), len(keyframes)):
        for i in range(j):
            a, b, _, _ = FE.match(keyframes[j]["desc"], keyframes[i]["desc"], *mopt)
            if len(a) >= min_matches:
                out.append((j, i, a.astype(np.int32), b.astype(np.int32)))
    return out


# ---------------------------------------------------------------------------------------------- the fp32 rows
def corrections(poses, poses0):
    """(K, 12) float32: C_k = R_k^T R0_k row-major | c_k = R_k^T (t0_k - t_k), in fp64 and cast; a pose with the store's bits gives the
    identity exactly"""
    out = np.zeros((len(poses), 12), F32)
    for k, (p, p0) in enumerate(zip(poses, poses0)):
        p, p0 = np.asarray(p, F64), np.asarray(p0, F64)
        if np.array_equal(p, p0):
            out[k, [0, 4, 8]] = 1
            continue
        R, R0 = p[:9].reshape(3, 3), p0[:9].reshape(3, 3)
        out[k, :9] = (R.T @ R0).reshape(9).astype(F32)
        out[k, 9:] = (R.T @ (p0[9:] - p[9:])).astype(F32)
    return out


def rotate(C12, x):
    """((C[3r] x0 + C[3r+1] x1) + C[3r+2] x2), every product and sum rounded to fp32 on its own; x (n, 3) float32"""
    C = C12.astype(F32)
    x = x.astype(F32)
    return np.stack([(C[3 * r] * x[:, 0] + C[3 * r + 1] * x[:, 1]) + C[3 * r + 2] * x[:, 2] for r in range(3)], 1).astype(F32)


def transform(C12, x):
    return (rotate(C12, x) + C12[9:].astype(F32)[None, :]).astype(F32)


def gate_sq(gate):
    g = F32(gate)
    return F32(g * g)


def pair_rows(keyframes, edge, corr, gate):
    """(X, Y, r (n, 3) float32, counted (n,) bool) of one edge"""
    j, i, a, b = edge
    xa, xb = keyframes[j]["xw"][a], keyframes[i]["xw"][b]
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y = transform(corr[j], xa), transform(corr[i], xb)
        r = (X - Y).astype(F32)
        s = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(F32)
        ok = np.isfinite(xa).all(1) & np.isfinite(xb).all(1) & (s < gate_sq(gate))
    return X, Y, r, ok


def residuals(keyframes, edges, poses, poses0, gate):
    """(pairs, 3) float32, NaN where the pair does not count: what rpe_graph_residuals gives"""
    corr = corrections(poses, poses0)
    out = []
    for e in edges:
        _, _, r, ok = pair_rows(keyframes, e, corr, gate)
        out.append(np.where(ok[:, None], r, F32(np.nan)).astype(F32))
    return np.concatenate(out) if out else np.zeros((0, 3), F32)


# ---------------------------------------------------------------------------------------------- the records
def raw_sums(X, Y, r, ok):
    """the 38 sums of csrc/rpe_graph.hip over the counted pairs, in fp64 from the fp32 rows, and the sums of the terms' magnitudes
    (for a difference of two products: of both products)"""
    X, Y, r = X[ok].astype(F64), Y[ok].astype(F64), r[ok].astype(F64)
    n = len(X)
    t, m = [np.ones(n), (r * r).sum(1)], [np.ones(n), (r * r).sum(1)]
    for c in range(3):
        t.append(r[:, c]); m.append(np.abs(r[:, c]))
    for c in range(3):
        u, v = (c + 1) % 3, (c + 2) % 3
        t.append(r[:, u] * X[:, v] - r[:, v] * X[:, u]); m.append(np.abs(r[:, u] * X[:, v]) + np.abs(r[:, v] * X[:, u]))
    for c in range(3):
        u, v = (c + 1) % 3, (c + 2) % 3
        t.append(Y[:, u] * r[:, v] - Y[:, v] * r[:, u]); m.append(np.abs(Y[:, u] * r[:, v]) + np.abs(Y[:, v] * r[:, u]))
    for Z in (X, Y):
        for c in range(3):
            t.append(Z[:, c]); m.append(np.abs(Z[:, c]))
    for Z in (X, Y):
        for (u, v) in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            t.append(Z[:, u] * Z[:, v]); m.append(np.abs(Z[:, u] * Z[:, v]))
    for u in range(3):
        for v in range(3):
            t.append(X[:, u] * Y[:, v]); m.append(np.abs(X[:, u] * Y[:, v]))
    return np.array([x.sum() for x in t], F64), np.array([x.sum() for x in m], F64)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], F64)


def tangent_map(p):
    """M = [[R^T, -R^T [t]x], [0, R^T]]: the world-frame Jacobian [-I, [X]x] times M is dX/d(upsilon, omega) of the left update"""
    R, t = np.asarray(p[:9], F64).reshape(3, 3), np.asarray(p[9:], F64)
    M = np.zeros((6, 6))
    M[:3, :3] = R.T
    M[3:, 3:] = R.T
    M[:3, 3:] = -R.T @ skew(t)
    return M


def sym6(q):
    return np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]], F64)


def world_blocks(w, magnitude=False):
    """(g_j, g_i, H_jj, H_ii, H_ji) in the world frame from the 38 sums; magnitude: every coefficient's absolute value (w = the
    magnitudes' sums): an entrywise bound's image"""
    s = (lambda x: np.abs(x)) if magnitude else (lambda x: x)
    n, Sr, SrX, SYr, SX, SY = w[0], w[2:5], w[5:8], w[8:11], w[11:14], w[14:17]
    QX, QY, XY = sym6(w[17:23]), sym6(w[23:29]), w[29:38].reshape(3, 3)
    gj = np.concatenate([s(-Sr), SrX])
    gi = np.concatenate([Sr, SYr])
    I = np.eye(3)

    def self_block(S, Q):
        H = np.zeros((6, 6))
        H[:3, :3] = n * I
        H[:3, 3:] = s(-skew(S))
        H[3:, :3] = s(skew(S))
        H[3:, 3:] = np.trace(Q) * I + s(-Q)
        return H

    Hji = np.zeros((6, 6))
    Hji[:3, :3] = s(-n * I)
    Hji[:3, 3:] = s(skew(SY))
    Hji[3:, :3] = s(-skew(SX))
    Hji[3:, 3:] = XY.T + s(-np.trace(XY) * I)
    return gj, gi, self_block(SX, QX), self_block(SY, QY), Hji


def pack(count, cost, gj, gi, Hjj, Hii, Hji):
    iu = np.triu_indices(6)
    return np.concatenate([[count, cost], gj, gi, Hjj[iu], Hii[iu], Hji.reshape(36)])


def record(w, pj, pi, magnitude=False):
    """the RECORD doubles of one edge at the poses pj / pi; magnitude: w = the magnitudes' sums, every matrix entrywise absolute"""
    Mj, Mi = tangent_map(pj), tangent_map(pi)
    if magnitude:
        Mj, Mi = np.abs(Mj), np.abs(Mi)
    gj, gi, Hjj, Hii, Hji = world_blocks(w, magnitude)
    return pack(w[0], w[1], Mj.T @ gj, Mi.T @ gi, Mj.T @ Hjj @ Mj, Mi.T @ Hii @ Mi, Mj.T @ Hji @ Mi)


def records(keyframes, edges, poses, poses0, gate):
    """(records (edges, RECORD), magnitudes (edges, RECORD)): per entry the record and the image of the sums of magnitudes"""
    corr = corrections(poses, poses0)
    rec, mag = np.zeros((len(edges), RECORD)), np.zeros((len(edges), RECORD))
    for e, edge in enumerate(edges):
        w, m = raw_sums(*pair_rows(keyframes, edge, corr, gate))
        rec[e] = record(w, poses[edge[0]], poses[edge[1]])
        mag[e] = record(m, poses[edge[0]], poses[edge[1]], magnitude=True)
    return rec, mag


def unpack(rec):
    """(g_j, g_i, H_jj, H_ii, H_ji) of one record, the diagonal blocks symmetric"""
    iu = np.triu_indices(6)
    out = []
    for o in (14, 35):
        H = np.zeros((6, 6))
        H[iu] = rec[o:o + 21]
        out.append(H + np.triu(H, 1).T)
    return rec[2:8], rec[8:14], out[0], out[1], rec[56:92].reshape(6, 6)


# ---------------------------------------------------------------------------------------------- solve, loop, apply
def fixed_set(K, ji, rec, anchor):
    """the anchor and the lowest id of every other component; components over the edges with >= 1 counted pair"""
    root = list(range(K))

    def find(k):
        while root[k] != k:
            k = root[k]
        return k

    for (j, i), r in zip(ji, rec):
        if r[0] >= 1:
            x, y = find(j), find(i)
            if x != y:
                root[max(x, y)] = min(x, y)
    ra = find(anchor)
    return np.array([(k == anchor) if find(k) == ra else (k == find(k)) for k in range(K)], bool)


def system(K, ji, rec):
    """the dense 6K x 6K matrix and the 6K gradient"""
    H, g = np.zeros((6 * K, 6 * K)), np.zeros(6 * K)
    for (j, i), r in zip(ji, rec):
        gj, gi, Hjj, Hii, Hji = unpack(r)
        sj, si = slice(6 * j, 6 * j + 6), slice(6 * i, 6 * i + 6)
        g[sj] += gj
        g[si] += gi
        H[sj, sj] += Hjj
        H[si, si] += Hii
        H[sj, si] += Hji
        H[si, sj] += Hji.T
    return H, g


def solve(K, ji, rec, fixed):
    """delta (K, 6) by numpy.linalg.solve over the keyframes that are on an edge and not fixed; None when the matrix is singular"""
    H, g = system(K, ji, rec)
    on = np.zeros(K, bool)
    for j, i in ji:
        on[j] = on[i] = True
    free = np.flatnonzero(on & ~np.asarray(fixed, bool))
    d = np.zeros((K, 6))
    if len(free) == 0:
        return d
    idx = (6 * free[:, None] + np.arange(6)[None, :]).reshape(-1)
    A = H[np.ix_(idx, idx)]
    if np.linalg.matrix_rank(A, tol=1e-10 * np.abs(A).max()) < len(idx):
        return None
    d[free] = np.linalg.solve(A, -g[idx]).reshape(-1, 6)
    return d


def se3_exp(a):
    v, w = np.asarray(a[:3], F64), np.asarray(a[3:], F64)
    th = np.linalg.norm(w)
    W = skew(w)
    if th < 1e-10:
        return np.eye(3) + W, v + 0.5 * W @ v
    A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * W + B * W @ W, (np.eye(3) + B * W + Cc * W @ W) @ v


def left_update(d, p):
    Rd, td = se3_exp(d)
    R, t = p[:9].reshape(3, 3), p[9:]
    return np.concatenate([(Rd @ R).reshape(9), Rd @ t + td])


def optimize(keyframes, edges, poses0, gates, anchor=0, tol=0.0):
    """(poses (K, 12), stats [(counted pairs, cost, |delta|)]) of the gated Gauss-Newton loop; None when a round is singular"""
    K = len(keyframes)
    ji = [(e[0], e[1]) for e in edges]
    poses0 = [np.asarray(p, F64).copy() for p in poses0]
    P = [p.copy() for p in poses0]
    stats, fixed = [], None
    for r, gate in enumerate(gates):
        rec, _ = records(keyframes, edges, P, poses0, gate)
        if r == 0:
            fixed = fixed_set(K, ji, rec, anchor)
        d = solve(K, ji, rec, fixed)
        if d is None:
            return None
        P = [p if fixed[k] else left_update(d[k], p) for k, p in enumerate(P)]
        stats.append((int(rec[:, 0].sum()), float(rec[:, 1].sum()), float(np.linalg.norm(d))))
        if stats[-1][2] < tol:
            break
    return np.array(P), stats


def apply(keyframes, poses, poses0):
    """the keyframes of the store after the apply step: xw <- C xw + c, nw <- C nw in the fp32 order"""
    corr = corrections(poses, poses0)
    with np.errstate(invalid="ignore", over="ignore"):
        return [dict(k, xw=transform(corr[n], k["xw"]), nw=rotate(corr[n], k["nw"])) for n, k in enumerate(keyframes)]
