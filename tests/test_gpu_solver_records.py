"""-m gpu: the 29-entry records of the Gauss-Newton normal-equation kernels (rpe_normal_eq.hip, rpe_residuals.hpp, rpe_joint.hip) held
ENTRY BY ENTRY -- not by a max-norm against the record's largest entry:
 (a) dyadic problems on which no operation rounds: the record equals the reference as numbers, at every size at which a thread makes
     another number of trips, the shared widening ends with another number of groups left over, or the ragged tail has another length;
     one Gauss-Newton step through the resident, the per-launch and the device loop from those records;
 (b) noisy scenes: |record - reference| <= c u S + ... per entry (tests/solver_rows.py derives c per kind and says what S is), all five
     residual kinds, both flavours, far from and at the optimum;
 (c) bearing and reprojection, which cannot be exact: one correspondence switched on at a time, at every index a block, a trip or the tail
     begins or ends with;
 (d) 307 200 correspondences with and without the last one: the two records differ by that correspondence's own products.
tests/test_solver_rows_oracle.py (CPU) shows that the reference agrees with the C++ oracle, that the precision plan alone stays inside
half the bound, and which planted defects the bound sees."""
import functools

import numpy as np
import pytest

from rgbd_pose_estimation_amd import _lib as L, api
import solver_rows as SR
import util
from test_gpu_clean_first import _ctx

pytestmark = pytest.mark.gpu

TWO_WG = {"RPE_BLOCK": "256", "RPE_MAX_BLOCKS": "2"}          # a trip covers 512 groups
TWO_WG_512 = {"RPE_BLOCK": "512", "RPE_MAX_BLOCKS": "2"}
GUARD = {"RPE_GUARD_ALWAYS": "1"}
DT = {False: np.float32, True: np.float64}


def edge_sizes(P):
    return [1, 2, 3, 4, 5, 7, 8, 9, 256 * P - 1, 256 * P, 256 * P + 1, 512 * P + 1, P * (2 * 512 + 257) + P - 1, P * (3 * 512 + 1) + 1,
            P * 4 * 512 + P - 1, P * (5 * 512 + 511) + 1]


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(*envs):
        env = {k: v for e in envs for k, v in e.items()}
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _ctx(env)
        return made[key]

    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _exact(n, f64):
    return SR.exact_problem(n, 100 + n, DT[f64])


def _load_exact(ctx, E, f64):
    ctx.load(L.F64 if f64 else L.F32, xw=E.Q, xc=E.P, nw=E.M, nc=E.N)
    for mod in (L.MOD_33, L.MOD_NN):
        ctx.upload_mask(mod, E.mask); ctx.upload_weight(mod, E.weight)


FLAGS = [0, L.USE_MASK, L.USE_WEIGHT, L.USE_MASK | L.USE_WEIGHT]
JOINT_EXACT = [[(L.RES_P2P, 1.0)], [(L.RES_P2PLANE, 0.5)], [(L.RES_P2P, 0.5), (L.RES_NORMAL, 4.0)], [(L.RES_P2PLANE, 4.0), (L.RES_NORMAL, 0.5)]]


def _moments_ref(E, mask, weight):
    ok = ~np.isnan(E.P).all(axis=1) & (True if mask is None else mask == 1)
    w = (np.ones(E.n) if weight is None else weight.astype(np.float64))[ok]
    Q, P = E.Q.astype(np.float64)[ok], E.P.astype(np.float64)[ok]
    return np.concatenate([[w.sum()], (w[:, None] * Q).sum(0), (w[:, None] * P).sum(0), ((w[:, None] * P).T @ Q).reshape(9),
                           [np.sum(w[:, None] * P * P)], [ok.sum()]])


def _exact_checks(ctx, E, what, moments=True):
    for flags in FLAGS:
        mask = E.mask if flags & L.USE_MASK else None
        weight = E.weight if flags & L.USE_WEIGHT else None
        for kind in (L.RES_P2P, L.RES_P2PLANE):
            rec, _ = ctx.normal_eq(kind, E.pose, flags=flags)
            ref = SR.exact_record(E, [(kind, 1.0)], mask, weight)
            assert np.array_equal(rec[:29], ref), (what, E.n, "normal_eq", kind, flags, np.flatnonzero(rec[:29] != ref), rec[:29] - ref)
        for terms in JOINT_EXACT:
            rec = ctx.normal_eq_joint(terms, E.pose, flags=flags)
            ref = SR.exact_record(E, terms, mask, weight)
            assert np.array_equal(rec[:29], ref), (what, E.n, "joint", terms, flags, np.flatnonzero(rec[:29] != ref), rec[:29] - ref)
        if moments:
            m = ctx.p2p_moments(flags)
            assert np.array_equal(m, _moments_ref(E, mask, weight)), (what, E.n, "moments", flags)


@pytest.mark.parametrize("flavour", ["clean_first", "guarded"])
@pytest.mark.parametrize("geometry", ["two_wg_256", "two_wg_512", "default"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_exact_problems_equal_the_reference_as_numbers(ctxs, f64, geometry, flavour):
    """(a) rec[:29] -- the weight sum in slot 28 included -- is array_equal to the reference: normal_eq (point-to-point, point-to-plane),
    normal_eq_joint (those two, and each with a normal-normal term, dyadic scales), p2p_moments; no flags, mask, weight, both.  With two
    workgroups of 256 (512) threads the sizes make a thread take 0 to 6 trips, threads of one launch unequal numbers of trips, the shared
    widening end with every number of groups left over, and thread 0 of workgroup 0 take a ragged tail of every length."""
    P = SR.group_width(DT[f64])
    env = {"two_wg_256": TWO_WG, "two_wg_512": TWO_WG_512, "default": {}}[geometry]
    ctx = ctxs(env, GUARD if flavour == "guarded" else {})
    for n in ([4099, 307200] if geometry == "default" else edge_sizes(P)):
        E = _exact(n, f64)
        _load_exact(ctx, E, f64)
        _exact_checks(ctx, E, (geometry, flavour))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_exact_problems_with_nan_marked_columns(ctxs, f64):
    """(a) guarded flavour: camera points marked "no measurement" (all-NaN columns) contribute nothing -- the record is that of the
    remaining correspondences, as numbers -- in full groups, at block and trip edges and in the ragged tail."""
    P = SR.group_width(DT[f64])
    ctx = ctxs(TWO_WG, GUARD)
    for n in edge_sizes(P):
        E0 = _exact(n, f64)
        E = SR.Exact()
        E.__dict__.update(E0.__dict__)
        E.P = E0.P.copy()
        rng = np.random.default_rng(n)
        idx = np.unique(np.concatenate([rng.integers(0, n, max(1, n // 9)), [n - 1] if n > 1 else [], [min(n - 1, 256 * P)] if n > 2 else []]).astype(int))
        if len(idx) == n:
            idx = idx[1:]
        E.P[idx] = np.nan
        _load_exact(ctx, E, f64)
        _exact_checks(ctx, E, "nan", moments=False)


@pytest.mark.parametrize("kind", [L.RES_P2P, L.RES_P2PLANE], ids=["p2p", "p2plane"])
def test_one_step_from_exact_records_is_the_same_on_every_path(ctxs, kind):
    """(a) gn_refine(max_iter = 1, tol = 0) with the resident loop (in registers up to 4096 correspondences under RPE_MAX_BLOCKS = 2,
    streaming at 4099) and with one launch per iteration: the same pose and cost bit for bit, the cost equal to rec[27]; the device loop:
    that cost exactly, its pose within 1e-12 (the device's solve rounds differently from the host's)."""
    few = {"RPE_MAX_BLOCKS": "2"}
    res, per = ctxs(few), ctxs(few, {"RPE_RESIDENT": "0"})
    for n in (64, 1023, 4096, 4099):
        E = _exact(n, False)
        out = []
        for ctx in (res, per):
            _load_exact(ctx, E, False)
            rec, _ = ctx.normal_eq(kind, E.pose, flags=L.USE_MASK | L.USE_WEIGHT)
            assert np.array_equal(rec[:29], SR.exact_record(E, [(kind, 1.0)], E.mask, E.weight))
            p, it, step, cost = ctx.gn_refine([kind], E.pose, flags=L.USE_MASK | L.USE_WEIGHT, max_iter=1, tol=0.0)
            assert it == 1 and cost == rec[27] and step > 0, (n, it, cost, rec[27])
            pd, itd, _, costd = ctx.gn_refine_device([(kind, 1.0)], E.pose, flags=L.USE_MASK | L.USE_WEIGHT, max_iter=1, tol=0.0)
            assert itd == 1 and costd == rec[27] and np.max(np.abs(pd - p)) <= 1e-12, (n, costd, rec[27], np.max(np.abs(pd - p)))
            out.append(p)
        assert np.array_equal(out[0], out[1]), (n, out[0] - out[1])
    assert res.resident_state()["lost"] == 0 and res.resident_state()["enabled"]


# ---------------------------------------------------------------------------------------------- (b)
ARR_MOD = {L.RES_P2P: L.MOD_33, L.RES_P2PLANE: L.MOD_33, L.RES_BEARING: L.MOD_23, L.RES_REPROJ: L.MOD_23, L.RES_NORMAL: L.MOD_NN}
COMBOS = [(L.RES_P2P,), (L.RES_NORMAL,), (L.RES_P2P, L.RES_BEARING), (L.RES_P2PLANE, L.RES_BEARING), (L.RES_P2P, L.RES_NORMAL),
          (L.RES_BEARING, L.RES_NORMAL), (L.RES_P2P, L.RES_BEARING, L.RES_NORMAL), (L.RES_P2PLANE, L.RES_BEARING, L.RES_NORMAL)]   # test_gpu_joint.py
SCALES = [1.0, 0.3, 1.7, 0.6]                                   # not dyadic: scale x w rounds


@functools.lru_cache(maxsize=None)
def _ref(kind, family, n, f64, dressed):
    sc, pose, mask, weight = SR.scene(family, n, DT[f64], dressed)
    return SR.reference(kind, SR.kind_arrays(sc, kind), pose, n, DT[f64], mask, weight)


@pytest.mark.parametrize("family", SR.FAMILIES)
@pytest.mark.parametrize("flavour", ["clean_first", "guarded"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_records_within_the_entrywise_bound(ctxs, f64, flavour, family):
    """(b) |got - ref| <= c u S + (C64 + D) 2^-53 S64 (+ the bearing kind's delta term) for EVERY entry 0..27 -- the gradient and the
    cost on their own scale, an H entry that is 2e-5 of the largest on its own -- and the weight sum exact without weights, within c u
    sum w with them: normal_eq for the four kinds it has, normal_eq_joint for the term sets of test_gpu_joint.py with scales that round;
    each scene plain and with mask, weights and 5 % NaN columns.  The worst error in units of u S is printed per kind."""
    ctx = ctxs(GUARD if flavour == "guarded" else {})
    worst = {}
    for n in SR.SIZES_B:
        for dressed in (False, True):
            sc, pose, mask, weight = SR.scene(family, n, DT[f64], dressed)
            ctx.load(L.F64 if f64 else L.F32, xw=sc.Q, xc=sc.P, bv=sc.U, nw=sc.M, nc=sc.N)
            flags = 0
            if dressed:
                flags = L.USE_MASK | L.USE_WEIGHT
                for mod in (L.MOD_23, L.MOD_33, L.MOD_NN):
                    ctx.upload_mask(mod, mask); ctx.upload_weight(mod, weight)
            for kind in (L.RES_P2P, L.RES_P2PLANE, L.RES_BEARING, L.RES_REPROJ):
                rec, _ = ctx.normal_eq(kind, pose, flags=flags)
                r = SR.assert_within(rec, _ref(kind, family, n, f64, dressed), DT[f64], dressed, ("normal_eq", SR.NAMES[kind], n, dressed))
                worst[SR.NAMES[kind]] = np.maximum(worst.get(SR.NAMES[kind], 0.0), r)
            for combo in COMBOS:
                terms = [(k, SCALES[i]) for i, k in enumerate(combo)]
                rec = ctx.normal_eq_joint(terms, pose, flags=flags)
                ref = SR.joint_reference([(_ref(k, family, n, f64, dressed), s) for k, s in terms])
                r = SR.assert_within(rec, ref, DT[f64], dressed, ("joint", combo, n, dressed))
                name = "joint " + "+".join(SR.NAMES[k] for k in combo)
                worst[name] = np.maximum(worst.get(name, 0.0), r)
    for name, r in worst.items():
        print(f"{'f64' if f64 else 'f32'} {flavour} {family}: {name}: worst error {r[0]:.3f} u S, {r[1]:.4f} of the bound   (c = "
              + "+".join(str(SR.C[k]) for k in SR.NAMES if SR.NAMES[k] in name.replace("joint ", "").split("+")) + ")")


# ---------------------------------------------------------------------------------------------- (c)
def _edge_indices(n, P):
    full = n // P
    idx = [0, 1, P - 1, P, 256 * P - 1, 256 * P, 512 * P - 1, 512 * P, (full - 1) * P, full * P - 1] + list(range(full * P, n))
    return sorted(set(i for i in idx if 0 <= i < n))


@pytest.mark.parametrize("kind", [L.RES_BEARING, L.RES_REPROJ], ids=["bearing", "reproj"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_one_correspondence_at_a_time(ctxs, f64, kind):
    """(c) The kinds that cannot be exact (hardware reciprocal, reciprocal square root): exactly ONE correspondence switched on -- by
    its mask, by its weight, and (guarded flavour) by marking every other bearing NaN -- at the first and last index of a group, of a
    workgroup's first trip, of a trip of the grid, of the last full group, and at every index of the ragged tail (two workgroups of 256
    threads).  The record is that correspondence's row products within the bound of (b); the count is 1, or its weight, exactly."""
    P = SR.group_width(DT[f64])
    worst = np.zeros(2)
    for n in (4099, P * (2 * 512 + 257) + P - 1):
        sc = util.scene_full(900 + n, n, DT[f64])
        pose = api.pose12(*util.perturbed_pose(np.random.default_rng(n), sc.R, sc.t))
        wts = np.random.default_rng(n + 1).uniform(0.1, 2.0, n).astype(DT[f64])
        clean, guarded = ctxs(TWO_WG), ctxs(TWO_WG, GUARD)
        for c in (clean, guarded):
            c.load(L.F64 if f64 else L.F32, xw=sc.Q, bv=sc.U)
        for i in _edge_indices(n, P):
            one = (sc.Q[i:i + 1], sc.U[i:i + 1], None)
            for mode in ("mask", "weight", "nan"):
                mask = weight = None
                ctx, flags = clean, 0
                if mode == "mask":
                    mask = np.zeros(n, np.int16); mask[i] = 1
                    ctx.upload_mask(L.MOD_23, mask); flags = L.USE_MASK
                elif mode == "weight":
                    weight = np.zeros(n, DT[f64]); weight[i] = wts[i]
                    ctx.upload_weight(L.MOD_23, weight); flags = L.USE_WEIGHT
                else:
                    ctx = guarded
                    U = np.full_like(sc.U, np.nan); U[i] = sc.U[i]
                    ctx.upload(L.BV, U)
                rec, _ = ctx.normal_eq(kind, pose, flags=flags)
                ref = SR.reference(kind, one, pose, n, DT[f64], None, None if weight is None else weight[i:i + 1])
                worst = np.maximum(worst, SR.assert_within(rec, ref, DT[f64], False, (SR.NAMES[kind], n, i, mode)))   # (count: exact in every mode)
                assert rec[28] == (ref[3] if weight is None else ref[3] * float(wts[i])), (n, i, mode, rec[28])
    print(f"{'f64' if f64 else 'f32'} {SR.NAMES[kind]}: one correspondence at a time, worst error {worst[0]:.3f} u S, {worst[1]:.4f} of the bound   (c = {SR.C[kind]})")


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("kind", [L.RES_P2PLANE, L.RES_BEARING], ids=["p2plane", "bearing"])
def test_the_last_correspondence_at_full_size(ctxs, kind):
    """(d) 307 200 correspondences, fp32, default geometry: the record of the arrays and the record with the last valid correspondence masked
    off differ by that correspondence's own row products, within the bound evaluated on the whole sum; the counts differ by exactly 1.  (The
    max-norm checks pass a record that lost it: its products are 1e-6 of the largest entry.)"""
    n = 307200
    sc, pose, _, _ = SR.scene("far", n, np.float32, False)
    arr = SR.kind_arrays(sc, kind)
    last = int(np.flatnonzero(SR.valid(kind, arr, pose))[-1])
    ctx = ctxs({})
    ctx.load(L.F32, xw=sc.Q, xc=sc.P, bv=sc.U, nc=sc.N)
    whole, _ = ctx.normal_eq(kind, pose)
    mask = np.ones(n, np.int16); mask[last] = 0
    ctx.upload_mask(ARR_MOD[kind], mask)
    less, _ = ctx.normal_eq(kind, pose, flags=L.USE_MASK)
    ref = _ref(kind, "far", n, False, False)
    own, S1, _, cnt = SR.reference(kind, tuple(None if a is None else a[last:last + 1] for a in arr), pose, n, np.float32)
    assert cnt == 1 and whole[28] == less[28] + 1 == float(ref[0][28])
    err = np.abs((whole[:28] - less[:28]).astype(SR.LD) - own[:28])
    print(SR.NAMES[kind], "difference of the two records against the correspondence's own products, worst error / bound of the whole sum:",
          float(np.max(err / ref[2][:28])), " products / bound:", float(np.max(np.abs(own[:28]) / ref[2][:28])))
    assert (err <= ref[2][:28]).all(), np.flatnonzero(err > ref[2][:28])
    assert (np.abs(own[:28]) > ref[2][:28]).any()           # ... and the bound on the whole sum sees them
    SR.assert_within(whole, ref, np.float32, False, (SR.NAMES[kind], n))
