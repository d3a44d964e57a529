"""GPU parity of the oriented descriptor (csrc/rpe_feature_oriented.hip) against tests/oriented_oracle.py, BIT FOR BIT -- keypoints,
scores, descriptors and angle bins of both sides, the match list, the five solver slots -- on every pair of tests/oriented_cases.py at
two camera sizes; the edges (steered samples outside the image on every side, zero moments, holes in the model colour, a cap of 1, no
keypoint, more survivors than the cap, a last describe workgroup that is not full); the upright path untouched; the invalidation rules
and every new error; rpe_relocalize of a rolled frame is rpe_run fed the oracle's matches, and lost with the upright descriptor; an
oriented keyframe store; the C++ front end."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import feature_oracle as FE
import keyframe_cases as KC
import keyframe_oracle as KO
import oriented_cases as OC
import oriented_oracle as OO
import test_gpu_feature as TG
import test_gpu_keyframes as TK
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELOC = TG.RELOC
code_of = TG.code_of


def check_side(ctx, which, xy, sc, de, bins):
    TG.check_side(ctx, which, xy, sc, de)
    g = ctx.features_angles(which)
    assert g.dtype == np.int32 and g.shape == bins.shape and np.array_equal(g, bins), which


def check_pair(ctx, p, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS), mopt=OC.MOPT):
    """test_gpu_feature.check_pair in oriented mode: detect both sides, match, and hold everything to the oracle; returns its dict"""
    o = OC.oracle(p, fopt, mopt)
    p.upload(ctx)
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    assert ctx.features_descriptor() == L.DESC_ORIENTED
    assert ctx.features_detect(L.FEAT_FRAME, *fopt) == len(o["fxy"])
    assert ctx.features_detect(L.FEAT_MODEL, *fopt) == len(o["mxy"])
    check_side(ctx, L.FEAT_FRAME, o["fxy"], o["fs"], o["fd"], o["fb"])
    check_side(ctx, L.FEAT_MODEL, o["mxy"], o["ms"], o["md"], o["mb"])
    m = ctx.features_match(mopt[0], (mopt[1], mopt[2]), mopt[3])
    assert m == len(o["fi"]) == ctx.n
    fi, mi, d1, d2, w = ctx.matches()
    assert np.array_equal(fi, o["fi"]) and np.array_equal(mi, o["mi"]) and np.array_equal(d1, o["d1"]) and np.array_equal(d2, o["d2"])
    assert np.array_equal(w, o["w"])
    if m:
        for slot, key in ((L.XW, "XW"), (L.XC, "XC"), (L.BV, "BV"), (L.NW, "NW"), (L.NC, "NC")):
            assert TG.same(ctx.download(slot), o[key]), key
    return o


# ---------------------------------------------------------------------------------------------- bit for bit, every pair and size
@pytest.mark.parametrize("motion", sorted(OC.MOTIONS))
@pytest.mark.parametrize("cam", ["small", "half"])
def test_pairs_bit_exact(gpu_ctx_factory, cam, motion):
    o = check_pair(gpu_ctx_factory(), OC.pair(cam, motion))
    assert len(o["fi"]) == OC.FIGURES[(cam, motion)]["oriented"][0] and len(np.unique(o["fb"])) > 16


def test_cross_check_and_other_options(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = OC.pair("small", "roll1.2")
    check_pair(ctx, p, fopt=(30, 300), mopt=(40, 9, 10, True))
    check_pair(ctx, p, fopt=(1, FE.MAX_KEYPOINTS), mopt=(256, 1, 1, False))


# ---------------------------------------------------------------------------------------------- edges
def test_steered_samples_outside_every_edge_and_zero_moments(gpu_ctx_factory):
    """corners at exactly 16 px from each edge in bins whose steered offsets reach 17 px: those samples read 0; lone dots have zero
    moments, a 32-way tie, bin 0"""
    p, placed, lone = OC.edge_pair()
    h, w = p.cam[5], p.cam[4]
    o = check_pair(gpu_ctx_factory(), p)
    for xy, bins in ((o["fxy"], o["fb"]), (o["mxy"], o["mb"])):
        at = {(int(u), int(v)): int(b) for (u, v), b in zip(xy, bins)}
        for edge, spots in placed.items():
            outside = 0
            for u, v, b in spots:
                assert at.get((u, v)) == b, (edge, u, v, b)
                P = OO.steer(np.array([b]))[0]
                X, Y = u + P[:, (0, 2)], v + P[:, (1, 3)]
                outside += int({"left": X < 0, "right": X >= w, "top": Y < 0, "bottom": Y >= h}[edge].sum())
            assert outside >= 1, edge
        found = [at[d] for d in lone if d in at]
        assert len(found) >= 3 and not any(found)


def test_model_colour_with_holes_inside_the_discs(gpu_ctx_factory):
    p = OC.holes_pair()
    o = check_pair(gpu_ctx_factory(), p)
    known = p.model_rgba[..., 3] != 0
    assert len(o["mxy"]) > 100 and all((~known[v + OO.DISC[:, 1], u + OO.DISC[:, 0]]).any() for u, v in o["mxy"])


def test_cap_of_one_and_a_flat_frame(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    o = check_pair(ctx, OC.pair("small", "roll0.6"), fopt=(FE.THRESHOLD, 1), mopt=(256, 8, 10, False))
    assert len(o["fxy"]) == len(o["mxy"]) == 1
    o = check_pair(ctx, FC.flat_pair())
    assert len(o["fxy"]) == 0 and len(o["mxy"]) > 0 and len(o["fi"]) == 0 and ctx.n == 0
    assert len(ctx.features_angles(L.FEAT_FRAME)) == 0


@pytest.mark.parametrize("cap", [FE.MAX_KEYPOINTS, 1001])
def test_more_survivors_than_the_cap(gpu_ctx_factory, cap):
    """4096: every describe workgroup is full; 1001: the last one holds a single keypoint"""
    p = FC.overcap_pair()
    o = check_pair(gpu_ctx_factory(), p, fopt=(FE.THRESHOLD, cap))
    assert len(o["fxy"]) == len(o["mxy"]) == cap and (cap == FE.MAX_KEYPOINTS or cap % 4 != 0)


@pytest.mark.parametrize("cap", [2, 3, 5])
def test_keypoint_counts_around_a_describe_workgroup(gpu_ctx_factory, cap):
    o = check_pair(gpu_ctx_factory(), OC.pair("small", "roll3.0"), fopt=(FE.THRESHOLD, cap))
    assert len(o["fxy"]) == len(o["mxy"]) == cap


# ---------------------------------------------------------------------------------------------- the upright path
def test_upright_is_untouched(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("small", "wide1")
    assert ctx.features_descriptor() == L.DESC_UPRIGHT
    o = TG.check_pair(ctx, p)
    for which, key in ((L.FEAT_FRAME, "fxy"), (L.FEAT_MODEL, "mxy")):
        a = ctx.features_angles(which)
        assert a.shape == (len(o[key]),) and not a.any()
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    ctx.features_detect(L.FEAT_FRAME)
    assert ctx.features_angles(L.FEAT_FRAME).any()
    ctx.features_set_descriptor(L.DESC_UPRIGHT)
    TG.check_pair(ctx, p)                                   # the same bits again
    assert not ctx.features_angles(L.FEAT_FRAME).any()


# ---------------------------------------------------------------------------------------------- invalidation and errors
def test_a_change_of_kind_drops_features_and_matches(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = OC.pair("small", "roll0.6")
    p.upload(ctx)

    def both():
        ctx.features_detect(L.FEAT_FRAME); ctx.features_detect(L.FEAT_MODEL)
        assert ctx.features_match() >= 0
        return ctx.features(L.FEAT_FRAME), ctx.matches()

    for kind, other in ((L.DESC_UPRIGHT, L.DESC_ORIENTED), (L.DESC_ORIENTED, L.DESC_UPRIGHT)):
        f, m = both()
        ctx.features_set_descriptor(kind)                   # the same kind: nothing goes
        assert ctx.features_descriptor() == kind
        assert all(np.array_equal(a, b) for a, b in zip(f, ctx.features(L.FEAT_FRAME)))
        assert all(np.array_equal(a, b) for a, b in zip(m, ctx.matches())) and len(ctx.features_angles(L.FEAT_MODEL)) > 0
        for bad in (-1, 2, 7):
            assert code_of(ctx.features_set_descriptor, bad) == L.RPE_ERR_ARG
        assert ctx.features_descriptor() == kind and len(ctx.features(L.FEAT_FRAME)[0]) == len(f[0])   # the failed calls changed nothing
        ctx.features_set_descriptor(other)
        assert ctx.features_descriptor() == other
        for which in (L.FEAT_FRAME, L.FEAT_MODEL):
            assert code_of(ctx.features, which) == L.RPE_ERR_STATE and code_of(ctx.features_angles, which) == L.RPE_ERR_STATE
        assert code_of(ctx.matches) == L.RPE_ERR_STATE and code_of(ctx.features_match) == L.RPE_ERR_STATE
    assert code_of(ctx.features_angles, 2) == L.RPE_ERR_ARG


def test_a_keyframe_store_has_one_kind(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    q = r.queries[0]
    solver = dict(method=api.M_SK_PROSAC, ls=api.LS_SHINJI_INLIERS, **RELOC)
    assert ctx.keyframes_descriptor() == -1
    r.shots[0].as_model(ctx)
    assert ctx.keyframe_add() == 0 and ctx.keyframes_descriptor() == L.DESC_UPRIGHT
    q.as_frame(ctx)
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    # (1) a keyframe of the other kind into a non-empty store
    r.shots[1].as_model(ctx)
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE
    assert code_of(TK.add_host, ctx, OC.keyframe(r.shots[1])) == L.RPE_ERR_STATE
    assert ctx.keyframes_len() == 1 and ctx.keyframes_descriptor() == L.DESC_UPRIGHT
    # (2) frame features of the other kind
    assert ctx.features_detect(L.FEAT_FRAME) > 0
    assert code_of(ctx.keyframes_query) == L.RPE_ERR_STATE and code_of(ctx.keyframe_match, 0) == L.RPE_ERR_STATE
    # (3) the context's kind differs from the store's
    assert code_of(ctx.relocalize_keyframes, **solver) == L.RPE_ERR_STATE
    ctx.features_set_descriptor(L.DESC_UPRIGHT)
    assert ctx.relocalize_keyframes(**solver)["keyframe"] == 0            # the kinds agree again
    # clear forgets the kind: the store takes the other one, from either entry
    ctx.keyframes_clear()
    assert ctx.keyframes_descriptor() == -1
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    assert TK.add_host(ctx, OC.keyframe(r.shots[1])) == 0 and ctx.keyframes_descriptor() == L.DESC_ORIENTED
    r.shots[2].as_model(ctx)
    assert ctx.keyframe_add() == 1
    ctx.features_set_descriptor(L.DESC_UPRIGHT)
    r.shots[3].as_model(ctx)
    assert code_of(ctx.keyframe_add) == L.RPE_ERR_STATE and code_of(TK.add_host, ctx, r.keyframes[3]) == L.RPE_ERR_STATE
    assert ctx.features_detect(L.FEAT_FRAME) > 0 and code_of(ctx.keyframes_query) == L.RPE_ERR_STATE
    assert code_of(ctx.relocalize_keyframes, **solver) == L.RPE_ERR_STATE
    ctx.keyframes_clear()
    assert ctx.keyframes_descriptor() == -1 and ctx.keyframe_add() == 0 and ctx.keyframes_descriptor() == L.DESC_UPRIGHT


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("motion", ["roll0.6", "wide2_rz-0.7"])
def test_relocalize_a_rolled_frame(gpu_ctx_factory, motion):
    """oriented: rpe_relocalize is rpe_run on the oracle's matches and lands within oriented_cases.RELOC_BOUND; upright, the same call
    is lost"""
    ctx = gpu_ctx_factory()
    p = OC.pair("half", motion)
    o = OC.oracle(p)
    p.upload(ctx)
    kw = dict(ls=api.LS_SHINJI_INLIERS, **RELOC)
    try:
        up = ctx.relocalize(api.M_SK_PROSAC, **kw)
        e = VC.pose_error(up["pose12"], p.pb)
        print(motion, "upright:", up["matches"], "matches,", e)
        assert not (e[0] <= 0.3)
    except L.RpeError as err:
        assert err.code == L.RPE_ERR_DEGENERATE
    assert not ctx.features_angles(L.FEAT_FRAME).any()
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    got = ctx.relocalize(api.M_SK_PROSAC, **kw)             # detects again on both sides: the kind changed
    w3 = np.repeat(o["w"][:, None], 3, axis=1)
    ref = api.run(api.M_SK_PROSAC, L.F32, xw=o["XW"], xc=o["XC"], bv=o["BV"], nw=o["NW"], nc=o["NC"], weights=w3, f=p.cam[0],
                  ls=api.LS_SHINJI_INLIERS, score_mode=L.SCORE_EXACT, **RELOC)
    assert got["matches"] == len(o["fi"]) and ref["max_votes"] > 20
    assert got["max_votes"] == ref["max_votes"] and got["iters"] == ref["iters"] and np.array_equal(got["masks"], ref["masks"])
    assert TG.same(ctx.download(L.XW), o["XW"]) and TG.same(ctx.download(L.XC), o["XC"])
    assert np.array_equal(ctx.features_angles(L.FEAT_FRAME), o["fb"]) and np.array_equal(ctx.features_angles(L.FEAT_MODEL), o["mb"])
    e = VC.pose_error(got["pose12"], p.pb)
    print(motion, "oriented:", got["matches"], "matches,", e, "from", VC.pose_error(p.pa, p.pb))
    assert e[0] < OC.RELOC_BOUND[0] and e[1] < OC.RELOC_BOUND[1]


# ---------------------------------------------------------------------------------------------- keyframes
def test_an_oriented_store_and_rolled_queries(gpu_ctx_factory):
    """counts, order and keyframe_match lists are keyframe_oracle's fed oriented descriptors; relocalize_keyframes picks the keyframe
    of the oracle's walk, with rpe_run's votes"""
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    ctx.features_set_descriptor(L.DESC_ORIENTED)
    kfs = [OC.keyframe(s) for s in r.shots]
    for i, (s, k) in enumerate(zip(r.shots, kfs)):
        assert s.as_model(ctx) == len(k["xy"]) and ctx.keyframe_add() == i
        assert TK.same_keyframe(ctx.keyframe(i), k)
    assert ctx.keyframes_descriptor() == L.DESC_ORIENTED
    solver = dict(method=api.M_SK_PROSAC, ls=api.LS_SHINJI_INLIERS)
    for i, q in enumerate(OC.rolled_queries(r)):
        fxy, _, fd, fb = OO.detect(q.rgba, q.V, q.N)
        q.as_frame(ctx)
        assert ctx.features_detect(L.FEAT_FRAME) == len(fxy) and np.array_equal(ctx.features_angles(L.FEAT_FRAME), fb)
        for mopt in (KO.MOPT, (64, 8, 10, True)):
            counts, order = TK.check_query(ctx, fd, kfs, mopt)
            TK.check_match(ctx, q, int(order[0]), kfs[order[0]], mopt, fxy, fd)
        counts, order = KO.query(fd, kfs)
        print(i, "counts", counts.tolist())
        if i not in (0, 3, 6):
            continue
        runs = {}

        def run(k):
            o = KO.match(fxy, fd, q.V, q.N, q.B, q.w, kfs[k])
            w3 = np.repeat(o["w"][:, None], 3, axis=1)
            ref = api.run(solver["method"], L.F32, xw=o["XW"], xc=o["XC"], bv=o["BV"], nw=o["NW"], nc=o["NC"], weights=w3, f=q.cam[0],
                          ls=solver["ls"], score_mode=L.SCORE_EXACT, **RELOC)
            runs[k] = (o, ref)
            return ref["max_votes"], ref

        win, ref = KO.walk(counts, order, KC.CANDIDATES, KC.MIN_MATCHES, run)
        assert ref is not None and counts[win] >= KC.MIN_MATCHES
        got = ctx.relocalize_keyframes(candidates=KC.CANDIDATES, min_matches=KC.MIN_MATCHES, **solver, **RELOC)
        o = runs[win][0]
        assert got["keyframe"] == win and got["matches"] == len(o["fi"]) == counts[win]
        assert got["max_votes"] == ref["max_votes"] and got["iters"] == ref["iters"] and np.array_equal(got["masks"], ref["masks"])
        assert TG.same(ctx.download(L.XW), o["XW"]) and TG.same(ctx.download(L.XC), o["XC"]) and np.array_equal(ctx.matches()[1], o["mi"])
        print(i, "keyframe", win, "votes", got["max_votes"], "error", VC.pose_error(got["pose12"], q.pose))


# ---------------------------------------------------------------------------------------------- C++
def test_oriented_reloc_cpp(tmp_path):
    """DepthFrontEnd::setDescriptor + relocalize on a rolled pair from plain C++ (tests/cpp/oriented_reloc.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "oriented_reloc")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "oriented_reloc.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "oriented_reloc: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
