"""CPU: the numpy statement of the solver's normal equations (tests/solver_rows.py) against the C++ oracle, the precision plan against its
bound, the planted defects against the same bound, and the exact problems.  What tests/test_gpu_solver_records.py asserts of the device
rests on these: the reference is right (a), the bound is not a fit to the device (b), and it is sharp enough to see a defect (c)."""
import numpy as np
import pytest

import solver_rows as SR

KINDS = [SR.P2P, SR.P2PLANE, SR.BEARING, SR.REPROJ, SR.NORMAL]
DTYPES = [np.float32, np.float64]
ids = dict(ids=lambda v: SR.NAMES[v] if isinstance(v, int) else getattr(v, "__name__", str(v)))


def _cases(kind, dtype, sizes=SR.SIZES_B, families=SR.FAMILIES):
    for fam in families:
        for dressed in (False, True):
            for n in sizes:
                sc, pose, mask, weight = SR.scene(fam, n, dtype, dressed)
                yield fam, dressed, n, SR.kind_arrays(sc, kind), pose, mask, weight


def _ratio(err, tol):
    """largest error / bound over the entries; an error where the bound is 0 counts as infinite"""
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("kind", KINDS, **ids)
def test_two_references_agree(oracle, kind, dtype):
    """(a) record(rows) in np.longdouble and oracle.gn_normal_eq (C++) agree entrywise to 1e-12 S on every scene of the GPU file.  (The
    oracle forms p and the residuals that cancel against it in long double for this: in plain fp64 its g carried up to 0.25 x 2^-53 S64,
    4e-12 S at n = 1 near the optimum.)"""
    worst = 0.0
    for fam, dressed, n, arr, pose, mask, weight in _cases(kind, dtype):
        ref, S = SR.record(SR.rows(kind, arr, pose, mask, weight, dtype))
        orc = oracle.gn_normal_eq(kind, arr[0], arr[1], arr[2], mask=mask, weight=weight, pose=pose, in_f64=dtype == np.float64)
        err = np.abs(orc - ref)
        assert (err <= 1e-12 * S).all(), (fam, dressed, n, np.flatnonzero(err > 1e-12 * S))
        worst = max(worst, _ratio(err, S))
    print(SR.NAMES[kind], np.dtype(dtype).name, "oracle - record, worst / S:", worst)


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("kind", KINDS, **ids)
def test_the_plan_stays_inside_half_the_bound(kind, dtype):
    """(b) emulate -- the precision plan without FMA -- is within c / 2 of the bound on every scene, in both summation orders and with the
    joint kernel's one-group spans, so c is not fitted to the device.  Measured worst error / bound(c / 2): 0.07 (bearing) to 0.48
    (normal-normal, fp64); in units of u S for fp32 arrays 3.4 (point-to-point), 3.0 (point-to-plane), 5.3 (reprojection), 2.1
    (normal-normal), 6.1 (bearing, far scenes); the bearing kind reaches 556 u S at n = 9 at the optimum, which is its delta term."""
    worst = 0.0
    for fam, dressed, n, arr, pose, mask, weight in _cases(kind, dtype):
        rw = SR.rows(kind, arr, pose, mask, weight, dtype)
        ref, _ = SR.record(rw)
        tol = SR.bound(kind, rw, n, dtype, c=SR.C[kind] / 2)
        for share, order in ((None, 0), (None, 1), (1, 0)):
            err = np.abs(SR.emulate(kind, arr, pose, mask, weight, dtype, share=share, order=order) - ref)
            assert (err <= tol).all(), (fam, dressed, n, share, order, np.flatnonzero(err > tol))
            worst = max(worst, _ratio(err, tol))
    print(SR.NAMES[kind], np.dtype(dtype).name, "emulate, worst error / bound(c / 2):", worst)


def test_the_basis_is_off_the_tangent_plane_by_the_documented_delta():
    """BEARING_DELTA_U is four times what the array-dtype basis measures over the test's bearings (numpy division; the hardware
    reciprocal's ulp cannot be measured here)."""
    for dtype in DTYPES:
        d = max(SR.measured_delta(SR.scene(f, n, dtype, dr)[0].U, dtype) for f in SR.FAMILIES for dr in (False, True) for n in SR.SIZES_B)
        print(np.dtype(dtype).name, "delta / u:", d)
        assert 4 * d <= SR.BEARING_DELTA_U + 1e-9 and d > 0.25


def _defect_ratio(kind, dtype, defect, case):
    fam, dressed, n, arr, pose, mask, weight = case
    rw = SR.rows(kind, arr, pose, mask, weight, dtype)
    if len(rw.idx) == 0:
        return None
    ref, _ = SR.record(rw)
    return _ratio(np.abs(SR.emulate(kind, arr, pose, mask, weight, dtype, defect=defect) - ref), SR.bound(kind, rw, n, dtype))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("kind", KINDS, **ids)
def test_planted_defects_exceed_the_bound(kind, dtype):
    """(c) Every planted defect of emulate exceeds the full bound in at least one entry:
     * a dropped and a doubled correspondence: every kind, dtype, scene and n, and 307 200 (point-to-plane, bearing; fp32).  Measured
       smallest excess: 3.2 x the bound (bearing, 307 200), 4.5 x (point-to-plane, 307 200);
     * the smallest |H| entry negated: everywhere;
     * g scaled by 1 + 1e-3: far scenes, and fp64 arrays everywhere.  Near the optimum g is what is left of a cancelling sum, and a
       thousandth of it is below u S for fp32 arrays (bearing 0.03 - 0.8 of the bound, point-to-point 0.77 at n = 4099): not asserted;
     * the pose rounded to fp32: fp64 arrays everywhere; fp32 arrays near the optimum for point-to-point, point-to-plane and
       reprojection (>= 2.2 x).  In the far scenes |r| is 5 cm and metres for the outliers, and 6e-8 of |p| is 0.1 - 0.9 of the bound;
     * the residual formed in the array dtype: fp32 arrays, near the optimum, n <= 64, point-to-point and point-to-plane (the kinds whose
       header says so).  Not asserted: reprojection is seen up to n = 63 and misses at 64 (0.90), normal-normal cancels two digits only,
       the bearing kind's delta term is the size of this defect; for fp64 arrays it IS the plan."""
    f32 = dtype == np.float32
    worst = {}

    def held(defect, cases):
        for case in cases:
            r = _defect_ratio(kind, dtype, defect, case)
            if r is not None:
                assert r > 1.0, (defect, case[:3], r)
                worst[defect] = min(worst.get(defect, np.inf), r)

    for defect in ("drop", "double", "negate_min_H"):
        held(defect, _cases(kind, dtype))
    if f32 and kind in (SR.P2PLANE, SR.BEARING):
        sc, pose, _, _ = SR.scene("far", 307200, dtype, False)
        for defect in ("drop", "double"):
            held(defect, [("far", False, 307200, SR.kind_arrays(sc, kind), pose, None, None)])
    held("g0", _cases(kind, dtype, families=SR.FAMILIES if not f32 else ("far",)))
    if not f32:
        held("pose_fp32", _cases(kind, dtype))
    elif kind in (SR.P2P, SR.P2PLANE, SR.REPROJ):
        held("pose_fp32", _cases(kind, dtype, families=("near",)))
    if f32 and kind in (SR.P2P, SR.P2PLANE):
        held("residual_in_dtype", _cases(kind, dtype, sizes=[n for n in SR.SIZES_B if n <= 64], families=("near",)))
    print(SR.NAMES[kind], np.dtype(dtype).name, "smallest defect / bound:", {k: round(v, 2) for k, v in worst.items()})


EXACT_TERMS = [[(SR.P2P, 1.0)], [(SR.P2PLANE, 1.0)], [(SR.P2P, 0.5), (SR.NORMAL, 4.0)], [(SR.P2PLANE, 4.0), (SR.NORMAL, 0.5)]]


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("n", [5, 4099, 1000003])
def test_exact_problems_equal_the_reference_as_numbers(n, dtype):
    """(d) On the dyadic problems the emulation, in two summation orders and two span widths, equals the reference as numbers
    (np.array_equal: a negative zero is a zero), with mask and weights and without."""
    E = SR.exact_problem(n, 11 + n, dtype)
    arr = {SR.P2P: (E.Q, E.P, None), SR.P2PLANE: (E.Q, E.P, E.N), SR.NORMAL: (E.M, E.N, None)}
    big = n > 4099          # (a million correspondences: the dressed problem, two term sets, the two orders)
    for mask, weight in ((None, None), (E.mask, E.weight))[big:]:
        for terms in EXACT_TERMS[1:3] if big else EXACT_TERMS:
            ref = SR.exact_record(E, terms, mask, weight)
            assert mask is not None or ref[28] == len(terms) * n
            for share, order in ((None, 0), (None, 1), (1, 1))[:2 if big else 3]:
                got = np.zeros(29)
                for kind, scale in terms:
                    got += SR.emulate(kind, arr[kind], E.pose, mask, weight, dtype, share=share, order=order, scale=scale)
                assert np.array_equal(got, ref), (terms, share, order, np.flatnonzero(got != ref))
    # and the longdouble statement gives the same numbers as the fp64 one
    for kind in arr:
        a, _ = SR.record(SR.rows(kind, arr[kind], E.pose, E.mask, E.weight, dtype)) if n <= 4099 else (None, None)
        if a is not None:
            assert np.array_equal(a.astype(np.float64), SR.exact_record(E, [(kind, 1.0)], E.mask, E.weight))
