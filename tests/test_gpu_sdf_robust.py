"""GPU: the robust volume terms (csrc/rpe_sdf_robust.hpp, rpe_sdf_api.hip) against tests/sdf_robust_oracle.py.  The planes of weights
are held BIT FOR BIT -- NaN for NaN -- at scales taken from the oracle's own residuals, so that both kinds are hit at their edge; the
records of all four forms to the siblings' rounding bound with exact row counts; kind NONE after a robust call to the bits before it;
the loops of tests/sdf_robust_cases.py to the oracle's figures x2; the argument rules; and a round whose weights are all 0."""
import os
import subprocess

import numpy as np
import pytest

import mapmesh_oracle as MM
import mapsdf_cases as MSC
import mapsdf_photo_cases as MPC
import sdf_cases as SC
import sdf_oracle as SO
import sdf_photo_cases as SPC
import sdf_photo_oracle as SP
import sdf_robust_cases as RC
import sdf_robust_oracle as RO
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L
from test_gpu_mapsdf_photo import cut_box, set_frame as map_set_frame
from test_gpu_photo import close, raises, same
from test_gpu_sdf_photo import BOUND, check_record, load as window_load, volumes as window_volumes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"huber": L.ROBUST_HUBER, "tukey": L.ROBUST_TUKEY}
LAM = SPC.WEIGHT
FLOOR = 1e-6


def an_abs_r(r, ok, fallback):
    """a scale EQUAL to an |r| of the frame's own rows (the median one), so that s <= k against s < k and Tukey's exact zero are hit"""
    a = np.abs(r[ok & np.isfinite(r)])
    a = a[a >= 1e-4]                                                          # (a frame at its true pose has |r| below the floor of k)
    return float(np.sort(a)[len(a) // 2]) if len(a) else fallback


# ---------------------------------------------------------------------------------------------- weight planes, bit for bit
@pytest.mark.parametrize("kind", list(KINDS))
def test_window_weight_planes_are_bit_exact(gpu_ctx_factory, kind):
    """RAGGED_CAM 161 x 119 (n no multiple of 4, ragged levels, several workgroups), the three poses of sdf_cases -- the third leaves
    the volume: NaN planes -- geometric and photometric, k = an |r| of the frame, a k above the gate and the floor"""
    ctx = gpu_ctx_factory()
    volume = window_volumes()["room"]
    _, _, G, vol, cvol = volume
    lv = window_load(ctx, SC.RAGGED_CAM, volume)
    K = KINDS[kind]
    at_edge = rows = nans = 0
    kg_last, kp_last = 0.01, 5.0
    for pose in SC.poses():
        for l, (V, N, If) in enumerate(lv):
            gate = VC.TRACK_GATES[l]
            r, _, ok = SO.rows(vol, G, V, N, pose, gate, SC.COS_THR, True)
            kg_last = kg = an_abs_r(r, ok, kg_last)
            for k in (kg, 1.0, FLOOR):
                ctx.sdf_set_robust(K, k, 0.0)
                got = ctx.sdf_robust_weights(pose, l, gate, SC.COS_THR, True)
                want = RO.weights(K, r, k, ok)
                assert got.shape == (len(V),) and same(got, want), (kind, l, k, int(np.isnan(got).sum()), int((~ok).sum()))
                if k == 1.0:
                    assert (got[ok] == 1).all() or kind == "tukey"           # above the gate: Huber is 1 everywhere
            at_edge += int((np.abs(r[ok]) == np.float32(kg)).sum())
            rows += int(ok.sum())
            nans += int((~ok).sum())
            rp, _, okp = SP.rows(vol, cvol, G, V, If, pose, gate)
            kp_last = kp = an_abs_r(rp, okp, kp_last)
            for pk in (kp, 1000.0, FLOOR, 0.0):
                ctx.sdf_set_robust(K, 0.05, pk)
                got = ctx.sdf_robust_weights(pose, l, gate, photo=True)
                assert same(got, RO.weights(K, rp, pk, okp)), (kind, "photo", l, pk)
            at_edge += int((np.abs(rp[okp]) == np.float32(kp)).sum())
    print(kind, "rows", rows, "pixels without", nans, "rows with |r| == k", at_edge)
    assert rows > 10000 and nans > 10000 and at_edge >= 6
    ctx.sdf_set_robust(L.ROBUST_NONE)
    got = ctx.sdf_robust_weights(SC.poses()[0], 0, 0.1, SC.COS_THR, True)
    assert np.array_equal(np.isnan(got), np.isnan(ctx.sdf_rows(SC.poses()[0], 0, 0.1, SC.COS_THR, True)[0])) and (got[~np.isnan(got)] == 1).all()


def map_dense(m, box):
    vol, cvol = m.dense(box)
    return vol, cvol, MM.geometry(m.kw, box)


def check_map_planes(ctx, m, box, lv, pose, gate, fallback=(0.01, 5.0)):
    """both kinds, geometric and photometric, at every level of the frame set on ctx; returns (rows, rows at the edge)"""
    b = m.bounds() if box is None else box
    vol, cvol, G = map_dense(m, b)
    rows = edge = 0
    for l, (V, N, If) in enumerate(lv):
        r, _, ok = SO.rows(vol, G, V, N, pose, gate, MSC.COS_THR, True)
        rp, _, okp = SP.rows(vol, cvol, G, V, If, pose, gate)
        kg, kp = an_abs_r(r, ok, fallback[0]), an_abs_r(rp, okp, fallback[1])
        for K in KINDS.values():
            for k, pk in ((kg, kp), (1.0, 0.0), (FLOOR, FLOOR)):
                ctx.sdf_set_robust(K, k, pk)
                got = ctx.map_sdf_robust_weights(pose, l, gate, MSC.COS_THR, True, box=box)
                assert same(got, RO.weights(K, r, k, ok)), ("geometric", K, l, k)
                got = ctx.map_sdf_robust_weights(pose, l, gate, photo=True, box=box)
                assert same(got, RO.weights(K, rp, pk, okp)), ("photometric", K, l, pk)
        rows += int(ok.sum()) + int(okp.sum())
        edge += int((np.abs(r[ok]) == np.float32(kg)).sum()) + int((np.abs(rp[okp]) == np.float32(kp)).sum())
    return rows, edge


@pytest.mark.parametrize("which", ["sphere", "random", "two stages", "far origin"])
def test_map_weight_planes_are_bit_exact(gpu_ctx_factory, which):
    """the small maps of mapsdf_photo_cases -- window, held and absent bricks; random content with NaN / Inf colour under a weight > 0,
    whose rows go through the rule; bricks held without a colour plane; |o| / s = 2^22 -- on the bounds and on a box that cuts the
    window"""
    ctx = gpu_ctx_factory()
    rows = edge = 0
    if which == "random":
        m = MPC.random_map(ctx)
        for box in (None, cut_box(m)):
            b = m.bounds() if box is None else box
            for n, pose in enumerate(MSC.random_views(m, b)[:2]):
                lv, _, _ = map_set_frame((ctx,), MPC.class_depth(m, b, MPC.CAM_A, pose, MSC.RANDOM_GATE, every=box is None), MPC.CAM_A, n)
                a, e = check_map_planes(ctx, m, box, lv, pose, MSC.RANDOM_GATE)
                rows, edge = rows + a, edge + e
    else:
        m = {"sphere": MPC.sphere_map, "two stages": MPC.two_stage_map, "far origin": MPC.far_map}[which](ctx)
        frames = {"sphere": lambda: MSC.sphere_frames(m, MPC.CAM_A), "two stages": lambda: MPC.two_stage_frames(m, MPC.CAM_A),
                  "far origin": lambda: MSC.far_frames(m, MPC.CAM_A)}[which]()
        rng = MSC.FAR_RANGE if which == "far origin" else MPC.RANGE
        for box in (None, cut_box(m)):
            for name, pose, depth in frames[:3]:
                lv, _, _ = map_set_frame((ctx,), depth, MPC.CAM_A, rng=rng)
                a, e = check_map_planes(ctx, m, box, lv, pose, 0.1)
                rows, edge = rows + a, edge + e
    print(which, "rows", rows, "at the edge", edge)
    assert (rows > 30 and edge >= 1) if which == "random" else (rows > 100 and edge >= 2)   # (random content passes the normal gate rarely)


# ---------------------------------------------------------------------------------------------- records
def check_forms(ctx, vol, cvol, G, lv, pose, gates, K, k, pk, calls, cos=SC.COS_THR):
    """the geometric record, the photometric-only record with photo_k on and off, and the combined round through its costs, counts
    and step, each against the oracle's: counts exact, sums within BOUND of the magnitudes.  calls = (normal_eq, photo_normal_eq, icp_rgbd)"""
    normal_eq, photo_normal_eq, icp_rgbd = calls
    worst = 0.0
    for l, (V, N, If) in enumerate(lv):
        gate = gates[l]
        ctx.sdf_set_robust(K, k, pk)
        geo, w, rec, S = RO.geometric(vol, G, V, N, pose, gate, cos, K, k)
        got = normal_eq(pose, l, gate, cos, True)
        assert got[28] == rec[28] == geo[2].sum() and got[29] == 16 * 2.0 ** -24
        worst = max(worst, check_record(got, rec, S, slice(0, 28), ("geometric", K, l)))
        for photo_k in (pk, 0.0):
            ctx.sdf_set_robust(K, k, photo_k)
            pho, wp, prec, pS = RO.photometric(vol, cvol, G, V, If, pose, gate, LAM, K, photo_k)
            got = photo_normal_eq(pose, l, gate, LAM)
            assert got[28] == prec[28] == pho[2].sum()
            worst = max(worst, check_record(got, prec, pS, slice(0, 28), ("photometric", K, l, photo_k)))
        ctx.sdf_set_robust(K, k, pk)
        crec, cS = RO.combined(vol, cvol, G, V, N, If, pose, gate, cos, LAM, K, k, pk)
        if l == 0:
            p, it, step, cost, rows, pcost, prows = icp_rgbd(pose, LAM, 1, 0.0, gate, cos, True)
            assert it == 1 and (rows, prows) == (int(crec[28]), int(crec[30]))
            worst = max(worst, check_record(np.array([cost, pcost]), crec[[27, 29]], cS[[27, 29]], slice(0, 2), ("costs", K)))
    return worst


@pytest.mark.parametrize("kind", list(KINDS))
def test_window_records_within_the_rounding_bound(gpu_ctx_factory, oracle, kind):
    ctx = gpu_ctx_factory()
    volume = window_volumes()["room"]
    _, _, G, vol, cvol = volume
    lv = window_load(ctx, SC.RAGGED_CAM, volume)
    K, worst = KINDS[kind], 0.0
    for pose in SC.poses()[:2]:
        V, N, If = lv[0]
        r, _, ok = SO.rows(vol, G, V, N, pose, 0.1, SC.COS_THR, True)
        rp, _, okp = SP.rows(vol, cvol, G, V, If, pose, 0.1)
        k, pk = an_abs_r(r, ok, 0.01), an_abs_r(rp, okp, 5.0)
        assert ok.sum() > 0.2 * len(V) and okp.sum() > 0.2 * len(V)
        worst = max(worst, check_forms(ctx, vol, cvol, G, lv, pose, VC.TRACK_GATES, K, k, pk,
                                       (ctx.sdf_normal_eq, ctx.sdf_photo_normal_eq, ctx.icp_sdf_rgbd)))
        # one round is the oracle's step
        ctx.sdf_set_robust(K, k, pk)
        po, hist = RO.icp_sdf_rgbd(oracle, vol, cvol, G, V, N, If, pose, 1, 0.1, SC.TRACK_COS, LAM, K, k, pk)
        p = ctx.icp_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, SC.TRACK_COS)[0]
        assert close(p, po, 1e-6), (p, po)
        po, hist = RO.icp_sdf(oracle, vol, G, V, N, pose, 1, 0.1, SC.TRACK_COS, K, k)
        p, it, step, cost, m = ctx.icp_sdf(pose, 1, 0.0, 0.1, SC.TRACK_COS)
        assert close(p, po, 1e-6) and m == hist[-1][0] and abs(step - hist[-1][1]) < 1e-6
    print(kind, "worst error / (2^-24 S):", worst, "of the bound's", BOUND / 2.0 ** -24)


@pytest.fixture(scope="module")
def scene(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    return ctx, MPC.scene_map(ctx)


@pytest.mark.parametrize("kind", list(KINDS))
def test_map_records_within_the_rounding_bound(scene, oracle, kind):
    ctx, m = scene
    K, worst = KINDS[kind], 0.0
    try:
        for cam in MPC.CAMS.values():
            lv, _, _ = map_set_frame((ctx,), MSC.scene_depth(cam), cam)
            for box in (None, MSC.grown(m)):
                b = m.bounds() if box is None else box
                vol, cvol, G = map_dense(m, b)
                V, N, If = lv[0]
                for pose in (MSC.scene_pose(), MSC.scene_start()):
                    r, _, ok = SO.rows(vol, G, V, N, pose, 0.1, 0.8, True)
                    rp, _, okp = SP.rows(vol, cvol, G, V, If, pose, 0.1)
                    k, pk = an_abs_r(r, ok, 0.01), an_abs_r(rp, okp, 5.0)
                    calls = (lambda *a: ctx.map_sdf_normal_eq(*a, box=box), lambda *a: ctx.map_sdf_photo_normal_eq(*a, box=box),
                             lambda *a: ctx.icp_map_sdf_rgbd(*a, box=box))
                    worst = max(worst, check_forms(ctx, vol, cvol, G, lv, pose, (0.1, 0.1, 0.1), K, k, pk, calls, 0.8))
                    ctx.sdf_set_robust(K, k, pk)
                    po, hist = RO.icp_sdf_rgbd(oracle, vol, cvol, G, V, N, If, pose, 1, 0.1, 0.8, LAM, K, k, pk)
                    assert close(ctx.icp_map_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, 0.8, box=box)[0], po, 1e-6)
                    po, hist = RO.icp_sdf(oracle, vol, G, V, N, pose, 1, 0.1, 0.8, K, k)
                    p, it, step, cost, rows = ctx.icp_map_sdf(pose, 1, 0.0, 0.1, 0.8, box=box)
                    assert close(p, po, 1e-6) and rows == hist[-1][0] > 20
    finally:
        ctx.sdf_set_robust(L.ROBUST_NONE)                                     # the context is the module's
    print(kind, "worst error / (2^-24 S):", worst)


def all_records(ctx, pose):
    """the records of the four forms (the map's on its bounds), the combined rounds through one-round loops, and a two-round loop on
    the map (the window of this map sees too little of the small frame for a loop of its own)"""
    out = [ctx.sdf_normal_eq(pose, 0, 0.1, 0.8, True), ctx.sdf_photo_normal_eq(pose, 0, 0.1, LAM),
           np.array(ctx.icp_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, 0.8)[0]), np.array(ctx.icp_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, 0.8)[1:], np.float64)]
    out += [ctx.map_sdf_normal_eq(pose, 0, 0.1, 0.8, True), ctx.map_sdf_photo_normal_eq(pose, 0, 0.1, LAM),
            np.array(ctx.icp_map_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, 0.8)[0]), np.array(ctx.icp_map_sdf_rgbd(pose, LAM, 1, 0.0, 0.1, 0.8)[1:], np.float64),
            np.array(ctx.icp_map_sdf(pose, 2, 0.0, 0.1, 0.8)[0])]
    return out


def test_kind_none_gives_the_bits_it_gave_and_a_wide_huber_the_unweighted_sums(scene):
    """the setter leaves nothing behind: records and loop results with kind NONE after robust calls are bit-identical to those before
    them.  With Huber and k above every |r| (1 m, 10 000 levels) every weight is 1: the records are within the bound of the UNWEIGHTED
    oracle's"""
    ctx, m = scene
    cam = MPC.CAM_A
    lv, _, _ = map_set_frame((ctx,), MSC.scene_depth(cam), cam)
    pose = MSC.scene_start()
    assert ctx.sdf_robust() == (L.ROBUST_NONE, 0.0, 0.0)
    before = all_records(ctx, pose)
    for K in KINDS.values():
        ctx.sdf_set_robust(K, 0.02, 8.0)
        during = all_records(ctx, pose)
        assert not np.array_equal(during[0], before[0]) and not np.array_equal(during[4], before[4])      # the weight did something
        assert during[0][28] == before[0][28] and during[5][28] == before[5][28]                             # ... but not to the row counts
    ctx.sdf_set_robust(L.ROBUST_NONE)
    after = all_records(ctx, pose)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # a wide Huber against the unweighted oracle, window (= the map's window here: dense rows of the context's own volume) and map
    ctx.sdf_set_robust(L.ROBUST_HUBER, 1.0, 10000.0)
    try:
        vol, cvol, G = map_dense(m, m.bounds())
        V, N, If = lv[0]
        rec, S = SO.record(*SO.rows(vol, G, V, N, pose, 0.1, 0.8, True))
        got = ctx.map_sdf_normal_eq(pose, 0, 0.1, 0.8, True)
        assert got[28] == rec[28] > 50
        check_record(got, rec, S, slice(0, 28), "wide huber, map")
        prec, pS = SP.record(*SP.rows(vol, cvol, G, V, If, pose, 0.1), LAM)
        got = ctx.map_sdf_photo_normal_eq(pose, 0, 0.1, LAM)
        assert got[28] == prec[28] > 50
        check_record(got, prec, pS, slice(0, 28), "wide huber, map colour")
        wvol, wcvol, wG = map_dense(m, m.extent())
        rec, S = SO.record(*SO.rows(wvol, wG, V, N, pose, 0.1, 0.8, True))
        got = ctx.sdf_normal_eq(pose, 0, 0.1, 0.8, True)
        assert got[28] == rec[28]
        check_record(got, rec, S, slice(0, 28), "wide huber, window")
        prec, pS = SP.record(*SP.rows(wvol, wcvol, wG, V, If, pose, 0.1), LAM)
        got = ctx.sdf_photo_normal_eq(pose, 0, 0.1, LAM)
        assert got[28] == prec[28]
        check_record(got, prec, pS, slice(0, 28), "wide huber, window colour")
    finally:
        ctx.sdf_set_robust(L.ROBUST_NONE)


# ---------------------------------------------------------------------------------------------- the loops
def within(e, want):
    lim = RC.limit(want)
    return e[0] <= lim[0] and e[1] <= lim[1]


def test_the_intruder_on_the_window(gpu_ctx_factory):
    """sdf_robust_cases' frames under its settings: every loop ends within 2 x the oracle's recorded error, the clean frame's robust
    loops included; and the conditions on the case hold on the device too"""
    ctx = gpu_ctx_factory()
    dims, desc, G, vol = SC.room_volume(RC.WINDOW_CAM)
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    end = {}
    for f in RC.FRAMES:
        ctx.frame_set_depth(RC.window_depth(f), RC.WINDOW_CAM, 1.0, *VC.RANGE, levels=RC.LEVELS)
        for s, (kind, k) in RC.SETTINGS.items():
            ctx.sdf_set_robust(kind, k)
            p, its, step, cost, m = ctx.icp_pyramid_sdf(RC.window_start(), VC.TRACK_ITERS, VC.TRACK_GATES, 0.0, RC.COS_THR)
            end[f, s] = e = VC.pose_error(p, RC.window_truth())
            print(f, "|", s, "| %.3g mrad / %.3g mm" % (1e3 * e[0], 1e3 * e[1]), "oracle", RC.WINDOW_ORACLE[f][s], "rows", m)
            assert its == VC.TRACK_ITERS and m > 1000
            assert within(e, RC.WINDOW_ORACLE[f][s]), (f, s, e, RC.WINDOW_ORACLE[f][s])
    clean, plain, tukey = end["clean", "none"], end["intruder 8 cm", "none"], end["intruder 8 cm", "tukey 50 mm"]
    assert tukey[0] <= 2 * clean[0] and tukey[1] <= 2 * clean[1] and plain[0] >= 4 * tukey[0] and plain[1] >= 4 * tukey[1]


def test_the_intruder_with_colour(gpu_ctx_factory):
    """the textured wall: without a weight the intruder takes the frame 150 mm off; with both weights the loop ends where the clean
    frame's does.  (The weight on the geometric rows alone does not pay here and loses the frame in the oracle: its end is printed,
    not asserted)"""
    ctx = gpu_ctx_factory()
    G, vol, cvol, _, _ = SPC.wall_fused(RC.COLOUR_CAM)
    dims, desc = SPC.loop_scene("wall")[2]
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(np.ascontiguousarray(cvol).view(np.float16))
    for intruder in (False, True):
        d, rgb = RC.colour_frame(intruder)
        ctx.frame_set_depth(d, RC.COLOUR_CAM, 1.0, *VC.RANGE, levels=RC.LEVELS)
        ctx.frame_set_color(rgb)
        for s, (kind, k, pk) in RC.COLOUR_SETTINGS.items():
            ctx.sdf_set_robust(kind, k, pk)
            try:
                p = ctx.icp_pyramid_sdf_rgbd(RC.colour_start(), LAM, VC.TRACK_ITERS, VC.TRACK_GATES, 0.0, RC.COS_THR)[0]
            except L.RpeError as err:
                assert intruder and s == "tukey 50 mm" and err.code == L.RPE_ERR_DEGENERATE, (intruder, s, str(err))
                print("intruder |", s, "| lost:", err)
                continue
            e = VC.pose_error(p, RC.colour_truth())
            print("intruder" if intruder else "clean", "|", s, "|", e, "oracle", RC.COLOUR_ORACLE[intruder][s])
            if not (intruder and s == "tukey 50 mm"):
                assert within(e, RC.COLOUR_ORACLE[intruder][s]), (intruder, s, e)


def test_the_intruder_on_the_map(gpu_ctx_factory):
    """mapsdf_photo_cases' walk along the wall, assembled on the device as its own test does, and the frame of its first evaluated
    position with the intruder, against the window and the archived bricks"""
    ctx = gpu_ctx_factory()
    ctx.volume_init(MPC.WALK_DIMS, **MPC.WALK_KW)
    ctx.volume_archive(1024)
    for n in range(MPC.WALK_FRAMES):
        if n:
            ctx.volume_shift((MPC.WALK_STEP, 0, 0))
        d, rgb = MPC.walk_frame(MPC.walk_pose(n), n)
        ctx.frame_set_depth(d, MPC.WALK_CAM, 1.0, *VC.RANGE, levels=1)
        ctx.frame_set_color(rgb)
        ctx.volume_integrate_color(MPC.walk_pose(n))
    assert ctx.volume_archive_info()["held"] == MPC.WALK_HELD
    ctx.sdf_set_robust(L.ROBUST_TUKEY, 0.05, 25.0)                            # set before the frames and the shifts to come: it survives them
    for intruder in (False, True):
        d, rgb = RC.map_frame(intruder)
        ctx.frame_set_depth(d, RC.MAP_CAM, 1.0, *VC.RANGE, levels=RC.LEVELS)
        ctx.frame_set_color(rgb)
        for s, (kind, k, pk) in RC.COLOUR_SETTINGS.items():
            if intruder and s == "tukey 50 mm":
                continue                                                      # DOES NOT PAY, and ends anywhere
            ctx.sdf_set_robust(kind, k, pk)
            p = ctx.icp_pyramid_map_sdf_rgbd(MPC.walk_start(RC.MAP_POSITION), LAM, MPC.WALK_ITERS, MPC.WALK_GATES, 0.0, MPC.COS_THR)[0]
            e = VC.pose_error(p, RC.map_truth())
            print("intruder" if intruder else "clean", "|", s, "|", e, "oracle", RC.MAP_ORACLE[intruder][s])
            assert within(e, RC.MAP_ORACLE[intruder][s]), (intruder, s, e)


# ---------------------------------------------------------------------------------------------- arguments, state, the empty round
def test_argument_rules_and_the_getters_round_trip(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    assert ctx.sdf_robust() == (L.ROBUST_NONE, 0.0, 0.0)
    ctx.sdf_set_robust(L.ROBUST_HUBER, 0.0125, 7.5)
    assert ctx.sdf_robust() == (L.ROBUST_HUBER, 0.0125, 7.5)
    for bad in ((L.ROBUST_CAUCHY, 0.05, 0.0), (7, 0.05, 0.0), (-1, 0.05, 0.0), (L.ROBUST_TUKEY, 0.5e-6, 0.0), (L.ROBUST_TUKEY, 0.0, 0.0),
                (L.ROBUST_HUBER, float("nan"), 0.0), (L.ROBUST_HUBER, float("inf"), 0.0), (L.ROBUST_HUBER, -0.05, 0.0),
                (L.ROBUST_HUBER, 0.05, -1.0), (L.ROBUST_TUKEY, 0.05, float("nan")), (L.ROBUST_TUKEY, 0.05, 0.5e-6)):
        raises(L.RPE_ERR_ARG, ctx.sdf_set_robust, *bad)
        assert ctx.sdf_robust() == (L.ROBUST_HUBER, 0.0125, 7.5)              # a refused call leaves the setting as it was
    with pytest.raises(L.RpeError) as e:
        ctx.sdf_set_robust(L.ROBUST_CAUCHY, 0.05)
    assert "CAUCHY" in str(e.value)
    ctx.sdf_set_robust(L.ROBUST_TUKEY, FLOOR, FLOOR)                          # the floor itself is good
    assert ctx.sdf_robust() == (L.ROBUST_TUKEY, FLOOR, FLOOR)
    # the context's: a new volume, a new frame and a shift leave it
    dims, desc, G, vol = SC.room_volume()
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    ctx.frame_set_depth(SC.frame_depth(SC.RAGGED_CAM), SC.RAGGED_CAM, 1.0, *VC.RANGE, levels=2)
    ctx.volume_shift((1, 0, -1))
    assert ctx.sdf_robust() == (L.ROBUST_TUKEY, FLOOR, FLOOR)
    # the hook's own rules are the rows calls'
    held = VC.held_out_pose()
    raises(L.RPE_ERR_STATE, ctx.sdf_robust_weights, held, 2)                  # the frame has 2 levels
    raises(L.RPE_ERR_ARG, ctx.sdf_robust_weights, held, 0, -0.1)
    raises(L.RPE_ERR_STATE, ctx.sdf_robust_weights, held, 0, 0.1, 0.9, True, True)      # photo: no frame colour
    ctx.sdf_set_robust(L.ROBUST_NONE, 123.0, -5.0)                            # with NONE the scales are not read
    assert ctx.sdf_robust() == (L.ROBUST_NONE, 0.0, 0.0)


def test_a_round_whose_weights_are_all_zero_is_degenerate(gpu_ctx_factory):
    """Tukey with k at the floor, on a level chosen so that the oracle has no row inside it: every weight is exactly 0, the record's
    sums are 0 with the row count as it was, and the loop returns RPE_ERR_DEGENERATE as any round without a solution does"""
    ctx = gpu_ctx_factory()
    volume = window_volumes()["room"]
    _, _, G, vol, cvol = volume
    lv = window_load(ctx, SC.RAGGED_CAM, volume)
    pose = SC.poses()[1]
    level = None
    for l in (2, 1, 0):
        V, N, If = lv[l]
        r, _, ok = SO.rows(vol, G, V, N, pose, VC.TRACK_GATES[l], SC.COS_THR, True)
        if ok.sum() > 100 and np.abs(r[ok]).min() >= np.float32(FLOOR):
            level = l
            break
    assert level is not None
    ctx.sdf_set_robust(L.ROBUST_TUKEY, FLOOR)
    w = ctx.sdf_robust_weights(pose, level, VC.TRACK_GATES[level], SC.COS_THR, True)
    assert (w[ok] == 0).all() and np.isnan(w[~ok]).all()
    ne = ctx.sdf_normal_eq(pose, level, VC.TRACK_GATES[level], SC.COS_THR, True)
    assert ne[28] == ok.sum() and (ne[:28] == 0).all()
    iters = tuple(1 if l in (0, level) else 0 for l in range(level + 1))     # coarse to fine: the chosen level's round comes first
    with pytest.raises(L.RpeError) as e:
        ctx.icp_pyramid_sdf(pose, iters, VC.TRACK_GATES[:level + 1], 0.0, SC.COS_THR)
    assert e.value.code == L.RPE_ERR_DEGENERATE
    ctx.sdf_set_robust(L.ROBUST_NONE)
    assert ctx.icp_pyramid_sdf(pose, iters, VC.TRACK_GATES[:level + 1], 0.0, SC.COS_THR)[4] > 100      # and nothing is left behind


# ---------------------------------------------------------------------------------------------- C++
def test_volume_sdf_robust_track_cpp_runs(tmp_path):
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_sdf_robust_track")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_sdf_robust_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "volume_sdf_robust_track: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
