"""Adversarial inputs for the pyramid kernels (F1p / F2p of csrc/rpe_frontend.hip): depth maps that put the 2 x 2 jump gate on its
edges, and model maps with partial NaNs, cancelling normals and infinities.  Shared by the CPU oracle cases and the GPU parity tests."""
import numpy as np

F = np.float32
GRID = 0.125      # gate-stress depths lie on a 1/8 grid in [1, 2): every difference of two of them (or of one +-1 ulp) is exact


def gate_stress_depth(w, h, seed, u16=False, hole_frac=0.1):
    """(i) every level-0 2 x 2 block: top-left a on the 1/8 grid, the other three at offsets from a drawn from {0, +-mj, +-mj +- 1 ulp,
    +-2 mj} (mj = 0.125; u16: scale 0.125 and offsets of 0, +-1, +-2 units), with holes.  Ties at exactly max_jump = 0.125 happen only
    from level 0 to 1; deeper levels see means with dense exclusion patterns.  Returns (depth, scale)."""
    rng = np.random.default_rng(seed)
    hb, wb = (h + 1) // 2, (w + 1) // 2
    if u16:
        a = rng.integers(10, 14, (hb, wb))                 # 1.25 .. 1.625 m at scale 0.125
        off = rng.choice(np.array([0, 1, -1, 2, -2]), (hb, wb, 4))
        off[..., 0] = 0
        z = (a[..., None] + off).astype(np.uint16)
    else:
        a = (rng.integers(10, 14, (hb, wb)) * GRID).astype(F)
        mj = F(GRID)
        up, dn = np.nextafter(a + mj, F(np.inf)), np.nextafter(a + mj, F(-np.inf))
        upn, dnn = np.nextafter(a - mj, F(np.inf)), np.nextafter(a - mj, F(-np.inf))
        cand = np.stack([a, a + mj, a - mj, up, dn, upn, dnn, a + 2 * mj, a - 2 * mj], -1).astype(F)
        pick = rng.integers(0, cand.shape[-1], (hb, wb, 4))
        pick[..., 0] = 0
        z = np.take_along_axis(cand, pick, -1)
    blocks = z.reshape(hb, wb, 2, 2).transpose(0, 2, 1, 3).reshape(2 * hb, 2 * wb)[:h, :w].copy()
    blocks.reshape(-1)[rng.random(h * w) < hole_frac] = 0
    return np.ascontiguousarray(blocks), (0.125 if u16 else 1.0)


def uniform_depth(w, h, seed, u16, dmin, dmax, hole_frac=0.3):
    """(ii) independent uniform depths in (dmin, dmax), hole_frac of them 0 (invalid); u16 in millimetres."""
    rng = np.random.default_rng(seed)
    if u16:
        z = rng.integers(int(dmin * 1000) + 1, int(dmax * 1000), (h, w)).astype(np.uint16)
    else:
        z = rng.uniform(dmin, dmax, (h, w)).astype(F)
    z[rng.random((h, w)) < hole_frac] = 0
    return z, (0.001 if u16 else 1.0)


def range_edge_depth(w, h, seed, u16, dmin, dmax):
    """(iii) depths at the ends of the valid range: one unit (u16 at scale 0.001) or one ulp (f32) either side of dmin and dmax, and on
    them, mixed with in-range depths."""
    rng = np.random.default_rng(seed)
    if u16:
        lo, hi = int(round(dmin * 1000)), int(round(dmax * 1000))
        edges = np.array([lo - 1, lo, lo + 1, hi - 1, hi, hi + 1])
        z = rng.integers(lo + 1, hi, (h, w))
        pick = rng.random((h, w)) < 0.6
        z[pick] = rng.choice(edges, int(pick.sum()))
        return z.astype(np.uint16), 0.001
    lo, hi = F(dmin), F(dmax)
    edges = np.array([np.nextafter(lo, F(0)), lo, np.nextafter(lo, F(np.inf)), np.nextafter(hi, F(0)), hi, np.nextafter(hi, F(np.inf))], F)
    z = rng.uniform(dmin, dmax, (h, w)).astype(F)
    pick = rng.random((h, w)) < 0.6
    z[pick] = rng.choice(edges, int(pick.sum()))
    return z, 1.0


def model_edge_maps(w, h, seed):
    """World vertex / normal maps (w*h, 3) of random 8 x 8 tiles, each with one pattern: plain; one NaN component of a vertex and of a
    normal; normals of alternating sign that cancel at level 1, 2 or 3; +-Inf vertex components; +-Inf normal components; vertices
    near FLT_MAX whose sums overflow; and in a quarter of the tiles whole-NaN holes.  Tiles are clipped at the right and bottom edges."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-2.0, 2.0, (h, w, 3)).astype(F)
    V[..., 2] += F(3.0)
    N = rng.normal(size=(h, w, 3)) * 0.2 + np.array([0.0, 0.0, -1.0])
    N = (N / np.linalg.norm(N, axis=-1, keepdims=True)).astype(F)
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            tv, tn = V[ty:ty + 8, tx:tx + 8], N[ty:ty + 8, tx:tx + 8]
            th, tw = tv.shape[:2]
            pix = lambda k: (rng.integers(0, th, k), rng.integers(0, tw, k))   # noqa: E731
            kind = int(rng.integers(0, 8))
            if kind == 1:
                y, x = pix(2)
                tv[y[0], x[0], rng.integers(0, 3)] = np.nan
                tn[y[1], x[1], rng.integers(0, 3)] = np.nan
            elif kind in (2, 3, 4):
                step = kind - 2                               # cancel at level step + 1
                n0 = tn[0, 0].copy()
                sign = np.where((np.arange(tw) >> step) & 1, F(-1), F(1)).astype(F)
                tn[:] = n0[None, None, :] * sign[None, :, None]
            elif kind == 5:
                y, x = pix(3)
                tv[y, x, rng.integers(0, 3, 3)] = rng.choice(np.array([np.inf, -np.inf], F), 3)
            elif kind == 6:
                y, x = pix(3)
                tn[y, x, rng.integers(0, 3, 3)] = rng.choice(np.array([np.inf, -np.inf], F), 3)
            elif kind == 7:
                tv[:] = rng.choice(np.array([-3e38, 3e38], F), tv.shape)
            if rng.random() < 0.25:
                y, x = pix(2)
                tv[y[0], x[0]] = np.nan
                tn[y[1], x[1]] = np.nan
    return V.reshape(-1, 3), N.reshape(-1, 3)
