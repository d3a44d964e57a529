"""GPU parity of the keyframe store (csrc/rpe_keyframe.hip) against tests/keyframe_oracle.py, BIT FOR BIT -- what a keyframe keeps, the
counts and the ranking of a frame against every keyframe, one keyframe's match list and solver slots -- on every case of
tests/keyframe_cases.py; the new path tied to the tested one (a keyframe put back as the model through the existing API gives the same
lists, slots and relocalisation); the edges (one keyframe, a full store, keyframes of 0 .. 4096 keypoints side by side, no frame
keypoint, mixed cameras, equal counts, clear and reuse, what the store survives, every error code); and end to end:
rpe_relocalize_keyframes is rpe_run fed the oracle's matches of the oracle's winner."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import feature_oracle as FE
import keyframe_cases as KC
import keyframe_oracle as KO
import util
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RELOC = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, **FC.RELOC_THRE)
SOLVER = dict(method=api.M_SK_PROSAC, ls=api.LS_SHINJI_INLIERS)
MOPTS = [KO.MOPT, (64, 8, 10, True), (0, 8, 10, False), (256, 8, 10, False), (256, 8, 10, True)]


def same(a, b):
    """bit for bit, every NaN where the other has one"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32))


def same_keyframe(g, k):
    return (np.array_equal(g["xy"], k["xy"]) and g["desc"].dtype == np.uint32 and np.array_equal(g["desc"], k["desc"])
            and same(g["xw"], k["xw"]) and same(g["nw"], k["nw"]))


def kw(mopt):
    return dict(max_dist=mopt[0], ratio=(mopt[1], mopt[2]), cross_check=mopt[3])


def add_host(ctx, k, pose=None, w=160, h=120):
    return ctx.keyframe_add_host(k["xy"], k["desc"], k["xw"], k["nw"], np.arange(12.0) if pose is None else pose, w, h)


def code_of(fn, *a, **kwargs):
    try:
        fn(*a, **kwargs)
    except L.RpeError as e:
        return e.code
    return L.RPE_OK


def check_query(ctx, desc, keyframes, mopt):
    counts, order = ctx.keyframes_query(**kw(mopt))
    oc, oo = KO.query(desc, keyframes, mopt)
    assert np.array_equal(counts, oc) and np.array_equal(order, oo), (mopt, counts.tolist(), oc.tolist(), order.tolist(), oo.tolist())
    return oc, oo


def check_match(ctx, q, kid, k, mopt, fxy=None, fd=None):
    """keyframe_match(kid) against the oracle's lists and slots"""
    if fxy is None:
        fxy, fd = q.features()
    o = KO.match(fxy, fd, q.V, q.N, q.B, q.w, k, mopt)
    m = ctx.keyframe_match(kid, **kw(mopt))
    assert m == len(o["fi"]) == ctx.n
    fi, mi, d1, d2, w = ctx.matches()
    assert np.array_equal(fi, o["fi"]) and np.array_equal(mi, o["mi"]) and np.array_equal(d1, o["d1"]) and np.array_equal(d2, o["d2"])
    assert np.array_equal(w, o["w"])
    if m:
        for slot, key in ((L.XW, "XW"), (L.XC, "XC"), (L.BV, "BV"), (L.NW, "NW"), (L.NC, "NC")):
            assert same(ctx.download(slot), o[key]), key
    return o


# ---------------------------------------------------------------------------------------------- the store
@pytest.mark.parametrize("cam", ["small", "half"])
def test_keyframe_add_keeps_the_oracles_keyframe(gpu_ctx_factory, cam):
    ctx = gpu_ctx_factory()
    r = KC.room(cam)
    assert ctx.keyframes_len() == 0
    for i, (s, k) in enumerate(zip(r.shots, r.keyframes)):
        assert s.as_model(ctx) == len(k["xy"])
        assert ctx.keyframe_add() == i and ctx.keyframes_len() == i + 1
        g = ctx.keyframe(i)
        assert same_keyframe(g, k)
        # ... and what the same context says of its model side
        xy, _, desc = ctx.features(L.FEAT_MODEL)
        pix = xy[:, 1].astype(np.int64) * s.w + xy[:, 0]
        assert np.array_equal(g["xy"], xy) and np.array_equal(g["desc"], desc)
        assert same(g["xw"], ctx.frame_download(L.MAP_MODEL_VERTEX)[pix]) and same(g["nw"], ctx.frame_download(L.MAP_MODEL_NORMAL)[pix])
        assert np.array_equal(g["pose12"], s.pose) and (g["width"], g["height"]) == (s.w, s.h)
    for i, k in enumerate(r.keyframes):                     # the store grew in between: the early keyframes are still what they were
        assert same_keyframe(ctx.keyframe(i), k)


def test_keyframe_from_a_tracked_frame(gpu_ctx_factory):
    """model_from_frame + model_color_from_frame + detect(MODEL) + keyframe_add: the frame's own keypoints, its vertices in the world"""
    ctx = gpu_ctx_factory()
    s = KC.room("small").shots[2]
    s.as_frame(ctx)
    ctx.model_from_frame(s.pose)
    ctx.model_color_from_frame()
    n = ctx.features_detect(L.FEAT_MODEL)
    kid = ctx.keyframe_add()
    g = ctx.keyframe(kid)
    xy, desc = s.features()
    assert n == len(xy) and np.array_equal(g["xy"], xy) and np.array_equal(g["desc"], desc)
    pix = xy[:, 1].astype(np.int64) * s.w + xy[:, 0]
    assert same(g["xw"], ctx.frame_download(L.MAP_MODEL_VERTEX)[pix]) and np.allclose(g["xw"], s.MV[pix], atol=1e-5)


# ---------------------------------------------------------------------------------------------- the query
@pytest.mark.parametrize("cam", ["small", "half"])
def test_query_counts_and_order(gpu_ctx_factory, cam):
    ctx = gpu_ctx_factory()
    r = KC.room(cam)
    r.fill(ctx)
    for i, q in enumerate(r.queries):
        q.as_frame(ctx)
        xy, desc = q.features()
        assert ctx.features_detect(L.FEAT_FRAME) == len(xy)
        oc, oo = check_query(ctx, desc, r.keyframes, KO.MOPT)
        assert oc.tolist() == KC.FIGURES[cam]["queries"][i]["counts"]
        for mopt in MOPTS[1:] if i in (0, 6) else MOPTS[1:2]:
            check_query(ctx, desc, r.keyframes, mopt)
    assert KO.query(desc, r.keyframes, MOPTS[1])[0].tolist() != oc.tolist()          # the cross-check removes something


def test_query_ties_of_a_repeated_texture(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    shots, kfs, q = KC.tiled_store()
    for s in shots:
        s.as_model(ctx)
        ctx.keyframe_add()
    q.as_frame(ctx)
    xy, desc = q.features()
    assert ctx.features_detect(L.FEAT_FRAME) == len(xy)
    oc, oo = check_query(ctx, desc, kfs, (256, 2, 1, False))
    assert oc.tolist() == KC.TILED["counts"] and oo.tolist() == [0, 1, 2]            # equal counts: the ids decide
    oc, oo = check_query(ctx, desc, kfs, (256, 2, 1, True))
    assert oc.tolist() == KC.TILED["cross_counts"] and oo.tolist() == KC.TILED["cross_order"]
    check_query(ctx, desc, kfs, KO.MOPT)
    for kid in range(3):
        o = check_match(ctx, q, kid, kfs[kid], (256, 2, 1, False), xy, desc)
        assert (o["d1"] == o["d2"]).sum() > len(o["fi"]) / 2
        check_match(ctx, q, kid, kfs[kid], (256, 2, 1, True), xy, desc)


def test_the_same_keyframe_twice(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    ids = [1, 3, 1, 0, 3]
    for i in ids:
        add_host(ctx, r.keyframes[i])
    q = r.queries[3]
    q.as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    counts, order = ctx.keyframes_query()
    oc, oo = check_query(ctx, q.features()[1], [r.keyframes[i] for i in ids], KO.MOPT)
    assert counts[0] == counts[2] and counts[1] == counts[4] and order.tolist().index(0) + 1 == order.tolist().index(2)
    assert order.tolist().index(1) + 1 == order.tolist().index(4)


# ---------------------------------------------------------------------------------------------- one keyframe's matches
@pytest.mark.parametrize("cam", ["small", "half"])
def test_keyframe_match_is_the_oracle_and_the_model_path(gpu_ctx_factory, cam):
    ctx, old = gpu_ctx_factory(), gpu_ctx_factory()
    r = KC.room(cam)
    r.fill(ctx)
    q = r.queries[0]
    for c in (ctx, old):
        q.as_frame(c)
        c.features_detect(L.FEAT_FRAME)
    fxy, fd = q.features()
    for kid in (1, 0, 6):
        for mopt in (KO.MOPT, (64, 8, 10, True)):
            o = check_match(ctx, q, kid, r.keyframes[kid], mopt, fxy, fd)
            assert len(o["fi"]) >= 12
            lists = ctx.matches()
            slots = [ctx.download(s) for s in (L.XW, L.XC, L.BV, L.NW, L.NC)]
            # the same keyframe put back as the model through the existing API
            r.shots[kid].as_model(old)
            assert old.features_match(**kw(mopt)) == len(o["fi"])
            assert all(np.array_equal(a, b) for a, b in zip(lists, old.matches()))
            assert all(same(a, old.download(s)) for a, s in zip(slots, (L.XW, L.XC, L.BV, L.NW, L.NC)))
    # the query and the single match agree
    counts, _ = ctx.keyframes_query()
    assert [ctx.keyframe_match(k) for k in range(8)] == counts.tolist()


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("cam", ["small", "half"])
def test_relocalize_keyframes_is_rpe_run_on_the_oracles_winner(gpu_ctx_factory, oracle, cam):
    ctx = gpu_ctx_factory()
    r = KC.room(cam)
    r.fill(ctx)
    for i, q in enumerate(r.queries):
        fig = KC.FIGURES[cam]["queries"][i]
        fxy, fd = q.features()
        counts, order = KO.query(fd, r.keyframes)
        runs = {}

        def run(k):
            o = KO.match(fxy, fd, q.V, q.N, q.B, q.w, r.keyframes[k])
            w3 = np.repeat(o["w"][:, None], 3, axis=1)
            ref = api.run(SOLVER["method"], L.F32, xw=o["XW"], xc=o["XC"], bv=o["BV"], nw=o["NW"], nc=o["NC"], weights=w3, f=q.cam[0],
                          ls=SOLVER["ls"], score_mode=L.SCORE_EXACT, **RELOC)
            runs[k] = (o, ref)
            return ref["max_votes"], ref

        win, ref = KO.walk(counts, order, KC.CANDIDATES, KC.MIN_MATCHES, run)
        q.as_frame(ctx)
        got = ctx.relocalize_keyframes(candidates=KC.CANDIDATES, min_matches=KC.MIN_MATCHES, **SOLVER, **RELOC)
        e = VC.pose_error(got["pose12"], q.pose)
        print(cam, i, "keyframe", got["keyframe"], "votes", got["max_votes"], "iters", got["iters"], "error", e, "oracle", fig["reloc"])
        o = runs[win][0]
        assert got["keyframe"] == win and got["matches"] == len(o["fi"]) == counts[win]
        assert got["max_votes"] == ref["max_votes"] and got["iters"] == ref["iters"] and np.array_equal(got["masks"], ref["masks"])
        # the slots and the match list are the winner's
        assert same(ctx.download(L.XW), o["XW"]) and same(ctx.download(L.XC), o["XC"]) and same(ctx.download(L.NW), o["NW"])
        assert np.array_equal(ctx.matches()[1], o["mi"])
        assert e[0] < 2 * fig["reloc"][0] and e[1] < 2 * fig["reloc"][1]
        assert e[0] < KC.RELOC_BOUND[0] and e[1] < KC.RELOC_BOUND[1]


def test_one_candidate_is_relocalize_against_that_keyframe(gpu_ctx_factory):
    ctx, old = gpu_ctx_factory(), gpu_ctx_factory()
    r = KC.room("small")
    r.fill(ctx)
    for i in (0, 6):
        q = r.queries[i]
        q.as_frame(ctx)
        got = ctx.relocalize_keyframes(candidates=1, **SOLVER, **RELOC)
        assert got["keyframe"] == int(np.argmax(KC.FIGURES["small"]["queries"][i]["counts"]))
        q.as_frame(old)
        r.shots[got["keyframe"]].as_model(old)
        ref = old.relocalize(SOLVER["method"], ls=SOLVER["ls"], **RELOC)
        assert got["matches"] == ref["matches"] and got["max_votes"] == ref["max_votes"] and got["iters"] == ref["iters"]
        assert np.array_equal(got["masks"], ref["masks"])
        assert util.rot_err(got["pose12"][:9].reshape(3, 3), ref["pose12"][:9].reshape(3, 3)) < util.ROT_TOL_RAD
        assert util.trans_rel_err(got["pose12"][9:], ref["pose12"][9:]) < util.TRANS_REL_TOL


def test_two_cameras_in_one_store(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    store = KC.two_camera_store()
    for i, (s, k) in enumerate(store):
        s.as_model(ctx)
        assert ctx.keyframe_add() == i
    kfs = [k for _, k in store]
    for i, (s, k) in enumerate(store):
        g = ctx.keyframe(i)
        assert same_keyframe(g, k) and (g["width"], g["height"]) == (s.w, s.h)
    for (cam, i), fig in KC.TWO_CAMERA.items():
        q = KC.room(cam).queries[i]
        q.as_frame(ctx)
        fxy, fd = q.features()
        ctx.features_detect(L.FEAT_FRAME)
        oc, _ = check_query(ctx, fd, kfs, KO.MOPT)
        assert oc.tolist() == fig["counts"]
        check_query(ctx, fd, kfs, (64, 8, 10, True))
        check_match(ctx, q, 1, kfs[1], KO.MOPT, fxy, fd)
        check_match(ctx, q, 0, kfs[0], (64, 8, 10, True), fxy, fd)
        got = ctx.relocalize_keyframes(**SOLVER, **RELOC)
        e = VC.pose_error(got["pose12"], q.pose)
        assert (got["keyframe"], got["max_votes"], got["iters"]) == (fig["keyframe"], fig["votes"], fig["iters"])
        assert e[0] < KC.RELOC_BOUND[0] and e[1] < KC.RELOC_BOUND[1]


# ---------------------------------------------------------------------------------------------- edges
def sized_keyframe(desc_pool, count, seed):
    """`count` descriptors drawn (with repeats) from real ones, a bit flipped here and there: distances of every size, many ties"""
    rng = np.random.default_rng(seed)
    d = desc_pool[rng.integers(0, len(desc_pool), count)].copy()
    flip = rng.random(count) < 0.5
    d[flip, rng.integers(0, 8, int(flip.sum()))] ^= np.uint32(1) << rng.integers(0, 32, int(flip.sum())).astype(np.uint32)
    xy = np.stack([rng.integers(0, 64, count), rng.integers(0, 48, count)], 1).astype(np.int32)
    return dict(xy=xy, desc=d, xw=rng.normal(size=(count, 3)).astype(F32), nw=rng.normal(size=(count, 3)).astype(F32))


def test_keyframes_of_every_size_in_one_store(gpu_ctx_factory):
    """0, 1, 255, 256, 257 and 4096 keypoints side by side (and an empty one last): the workgroups' quarters, their tails and the
    offsets; the cross-check runs over the whole packed store"""
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    q = r.queries[0]
    fxy, fd = q.features()
    pool = np.concatenate([fd, r.keyframes[0]["desc"], r.keyframes[1]["desc"]])
    kfs = [sized_keyframe(pool, n, 40 + j) for j, n in enumerate((0, 1, 255, 256, 257, 4096, 2, 3, 0))]
    for j, k in enumerate(kfs):
        assert add_host(ctx, k) == j
    for j, k in enumerate(kfs):
        assert same_keyframe(ctx.keyframe(j), k)
    q.as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    for mopt in MOPTS + [(256, 2, 1, False), (256, 2, 1, True), (256, 65536, 1, False)]:
        oc, _ = check_query(ctx, fd, kfs, mopt)
        assert oc[0] == oc[-1] == 0
    assert KO.query(fd, kfs, (256, 8, 10, False))[0][1] == len(fd)                   # one keypoint: d2 = 257, everything passes
    for j, k in enumerate(kfs):
        check_match(ctx, q, j, k, (256, 2, 1, False), fxy, fd)
        check_match(ctx, q, j, k, (256, 2, 1, True), fxy, fd)
    assert ctx.n == 0 and len(ctx.matches()[0]) == 0                                  # the last keyframe is empty: an empty problem


def test_one_keyframe(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    r.shots[0].as_model(ctx)
    ctx.keyframe_add()
    q = r.queries[0]
    q.as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    counts, order = ctx.keyframes_query()
    assert counts.tolist() == [KC.FIGURES["small"]["queries"][0]["counts"][0]] and order.tolist() == [0]
    check_match(ctx, q, 0, r.keyframes[0], KO.MOPT)
    got = ctx.relocalize_keyframes(candidates=5, **SOLVER, **RELOC)
    assert got["keyframe"] == 0 and got["matches"] == counts[0]


def test_a_full_store_and_one_more(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    q = r.queries[0]
    fxy, fd = q.features()
    kfs = []
    for i in range(L.MAX_KEYFRAMES):
        k = KC.tiny_keyframe(i, count=i % 5)
        if i % 7 == 3 and len(k["desc"]):
            k["desc"][0] = fd[i]                                                     # some keyframes hold a keypoint of the frame
        kfs.append(k)
        assert add_host(ctx, k) == i
    assert ctx.keyframes_len() == L.MAX_KEYFRAMES
    assert code_of(add_host, ctx, kfs[1]) == L.RPE_ERR_STATE                         # the refusal of one more, from either entry
    r.shots[0].as_model(ctx)
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE and ctx.keyframes_len() == L.MAX_KEYFRAMES
    q.as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    for mopt in (KO.MOPT, (64, 8, 10, True), (256, 8, 10, False)):
        oc, oo = check_query(ctx, fd, kfs, mopt)
    assert oc.max() > 0 and (oc == 0).sum() > 50
    for j in (0, 3, 4, 255):
        assert same_keyframe(ctx.keyframe(j), kfs[j])
        check_match(ctx, q, j, kfs[j], (256, 8, 10, False), fxy, fd)


def test_a_frame_without_keypoints(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    r.fill(ctx)
    f = KC.flat_query()
    f.as_frame(ctx)
    assert ctx.features_detect(L.FEAT_FRAME) == 0
    for mopt in (KO.MOPT, (64, 8, 10, True)):
        counts, order = ctx.keyframes_query(**kw(mopt))
        assert counts.tolist() == [0] * 8 and order.tolist() == list(range(8))
        assert ctx.keyframe_match(3, **kw(mopt)) == 0 and ctx.n == 0 and len(ctx.matches()[0]) == 0
    # degenerate: the best-ranked id and its count come back, the pose is left alone
    p = np.arange(12, dtype=np.float64)
    it, kf, m, mv = api.C.c_int(50), api.C.c_int(-1), api.C.c_int(-1), api.C.c_int(0)
    mask = np.zeros(3 * L.MAX_KEYPOINTS, np.int16)
    rc = L.lib().rpe_relocalize_keyframes(ctx._h, None, None, 3, api.M_SK_PROSAC, 0.05, 3.0, 0.1, api.C.byref(it), 0.99, 1, 0, 12, api._p(p),
                                          api.C.byref(kf), api.C.byref(m), api.C.byref(mv), api._p(mask))
    assert rc == L.RPE_ERR_DEGENERATE and (kf.value, m.value) == (0, 0) and np.array_equal(p, np.arange(12)) and it.value == 50


def test_min_matches_and_the_keyframe_named_when_degenerate(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    r.fill(ctx)
    q = r.queries[5]
    q.as_frame(ctx)
    counts = KC.FIGURES["small"]["queries"][5]["counts"]                              # [13, 57, 165, 7, 13, 287, 18, 14]
    with pytest.raises(L.RpeError) as ei:
        ctx.relocalize_keyframes(min_matches=max(counts) + 1, **SOLVER, **RELOC)
    assert ei.value.code == L.RPE_ERR_DEGENERATE and (ei.value.keyframe, ei.value.matches) == (5, max(counts))
    # min_matches ends the walk: with 166 only keyframe 5 is tried, with 12 the three best are -- here the same winner either way
    a = ctx.relocalize_keyframes(candidates=8, min_matches=166, **SOLVER, **RELOC)
    b = ctx.relocalize_keyframes(candidates=1, min_matches=12, **SOLVER, **RELOC)
    assert a["keyframe"] == b["keyframe"] == 5 and a["max_votes"] == b["max_votes"] and np.array_equal(a["masks"], b["masks"])
    assert a["matches"] == max(counts)


def test_clear_and_reuse_and_what_the_store_survives(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    r.fill(ctx)
    q = r.queries[2]
    q.as_frame(ctx)
    fxy, fd = q.features()
    ctx.features_detect(L.FEAT_FRAME)
    before = ctx.keyframes_query()
    # a new frame, a new model, a new detection on both sides and a volume: the store is what it was
    r.queries[4].as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    r.shots[7].as_model(ctx)
    ctx.volume_init((32, 32, 32), voxel_size=0.1, origin=(-1.6, -1.6, 0.0), trunc=0.3)
    for i, k in enumerate(r.keyframes):
        assert same_keyframe(ctx.keyframe(i), k)
    q.as_frame(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    after = ctx.keyframes_query()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the keyframe match list: there after keyframe_match, gone after a new frame detection, a model-side match or a clear
    assert ctx.keyframe_match(2) == before[0][2] and len(ctx.matches()[0]) == before[0][2]
    ctx.features_detect(L.FEAT_FRAME)
    assert code_of(ctx.matches) == L.RPE_ERR_STATE
    ctx.keyframe_match(2)
    m = ctx.features_match()                                                          # against the model side (shot 7)
    assert m == len(FE.match(fd, r.keyframes[7]["desc"])[0]) and np.array_equal(ctx.matches()[1], FE.match(fd, r.keyframes[7]["desc"])[1])
    ctx.keyframe_match(2)
    ctx.keyframes_clear()
    assert ctx.keyframes_len() == 0 and code_of(ctx.matches) == L.RPE_ERR_STATE
    assert code_of(ctx.keyframes_query) == L.RPE_ERR_STATE and code_of(ctx.keyframe_match, 0) == L.RPE_ERR_STATE
    # reuse: ids start again, in another order
    for j, i in enumerate((5, 2)):
        assert add_host(ctx, r.keyframes[i], r.shots[i].pose, r.shots[i].w, r.shots[i].h) == j
    counts, order = ctx.keyframes_query()
    assert counts.tolist() == [before[0][5], before[0][2]] and same_keyframe(ctx.keyframe(1), r.keyframes[2])
    check_match(ctx, q, 1, r.keyframes[2], KO.MOPT, fxy, fd)


def test_state_and_argument_errors(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    s, q, k = r.shots[0], r.queries[0], r.keyframes[0]
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE                              # no model
    s.as_frame(ctx)
    ctx.model_from_frame(s.pose)
    ctx.model_color_from_frame()
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE                              # a model, no detection on it
    assert code_of(ctx.keyframes_query) == L.RPE_ERR_STATE and code_of(ctx.keyframe_match, 0) == L.RPE_ERR_STATE   # empty store
    assert code_of(ctx.relocalize_keyframes, api.M_SK_PROSAC) == L.RPE_ERR_STATE
    assert code_of(ctx.keyframe, 0) == L.RPE_ERR_ARG
    ctx.features_detect(L.FEAT_MODEL)
    assert ctx.keyframe_add() == 0
    ctx.model_color_from_frame()                                                      # drops the model's features
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE and ctx.keyframes_len() == 1
    assert code_of(ctx.keyframes_query) == L.RPE_ERR_STATE and code_of(ctx.keyframe_match, 0) == L.RPE_ERR_STATE   # no frame features
    ctx.features_detect(L.FEAT_FRAME)
    own = KO.query(s.features()[1], [k])[0].tolist()                                 # the frame is the keyframe's own view
    assert ctx.keyframes_query()[0].tolist() == own and own[0] > 0.9 * len(k["xy"])
    assert code_of(ctx.keyframe_match, 1) == L.RPE_ERR_ARG and code_of(ctx.keyframe_match, -1) == L.RPE_ERR_ARG
    assert code_of(ctx.keyframe, 1) == L.RPE_ERR_ARG and code_of(ctx.keyframe, -1) == L.RPE_ERR_ARG
    for bad in (dict(max_dist=-1), dict(max_dist=257), dict(ratio=(0, 10)), dict(ratio=(8, 0)), dict(ratio=(8, 65537)), dict(cross_check=2)):
        assert code_of(ctx.keyframes_query, **bad) == L.RPE_ERR_ARG, bad
        assert code_of(ctx.keyframe_match, 0, **bad) == L.RPE_ERR_ARG, bad
        assert code_of(ctx.relocalize_keyframes, api.M_SK_PROSAC, **bad) == L.RPE_ERR_ARG, bad
    for bad in (dict(candidates=0), dict(min_matches=3), dict(min_matches=L.MAX_KEYPOINTS + 1), dict(threshold=0), dict(max_keypoints=0)):
        assert code_of(ctx.relocalize_keyframes, api.M_SK_PROSAC, **bad) == L.RPE_ERR_ARG, bad
    assert code_of(ctx.relocalize_keyframes, 10) == L.RPE_ERR_ARG and code_of(ctx.relocalize_keyframes, -1) == L.RPE_ERR_ARG
    lib, h = L.lib(), ctx._h
    p12, one = np.arange(12.0), np.zeros(8, np.int32)
    xy, de, xw = np.array([[63, 47]], np.int32), np.zeros((1, 8), np.uint32), np.zeros((1, 3), F32)
    P = api._p
    assert lib.rpe_keyframe_add_host(h, -1, P(xy), P(de), P(xw), P(xw), P(p12), 64, 48, None) == L.RPE_ERR_ARG
    assert lib.rpe_keyframe_add_host(h, L.MAX_KEYPOINTS + 1, P(xy), P(de), P(xw), P(xw), P(p12), 64, 48, None) == L.RPE_ERR_ARG
    assert lib.rpe_keyframe_add_host(h, 1, None, P(de), P(xw), P(xw), P(p12), 64, 48, None) == L.RPE_ERR_ARG
    assert lib.rpe_keyframe_add_host(h, 1, P(xy), P(de), P(xw), P(xw), None, 64, 48, None) == L.RPE_ERR_ARG
    assert lib.rpe_keyframe_add_host(h, 1, P(xy), P(de), P(xw), P(xw), P(p12), 0, 48, None) == L.RPE_ERR_ARG
    assert lib.rpe_keyframe_add_host(h, 1, P(xy), P(de), P(xw), P(xw), P(p12), 63, 48, None) == L.RPE_ERR_ARG      # xy outside the image
    assert lib.rpe_keyframes_query(h, None, None, P(one)) == L.RPE_ERR_ARG and lib.rpe_keyframes_count(h, None) == L.RPE_ERR_ARG
    assert ctx.keyframes_len() == 1
    assert lib.rpe_keyframe_add_host(h, 1, P(xy), P(de), P(xw), P(xw), P(p12), 64, 48, None) == L.RPE_OK            # id may be NULL
    assert lib.rpe_keyframe_add_host(h, 0, None, None, None, None, P(p12), 64, 48, None) == L.RPE_OK                # count = 0 is legal
    assert ctx.keyframes_len() == 3 and len(ctx.keyframe(2)["xy"]) == 0 and ctx.keyframe(1)["xy"].tolist() == [[63, 47]]
    assert ctx.keyframes_query()[0].tolist()[0] == own[0]                             # the failed calls left the store alone


# ---------------------------------------------------------------------------------------------- C++
def test_keyframe_reloc_cpp(tmp_path):
    """DepthFrontEnd::addKeyframe / queryKeyframes / matchKeyframe / relocalizeKeyframes from plain C++ (tests/cpp/keyframe_reloc.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "keyframe_reloc")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "keyframe_reloc.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "keyframe_reloc: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
