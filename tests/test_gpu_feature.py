"""GPU parity of the feature stage (csrc/rpe_feature.hip) against tests/feature_oracle.py, BIT FOR BIT -- keypoints, scores, descriptors
of both sides, the match list, the five solver slots -- on every case of tests/feature_cases.py and three camera sizes; the edges
(no keypoint, one model keypoint, a cap of 1, more survivors than the cap, the cross-check, Hamming ties, the invalidation rules, every
error code); and end to end: rpe_relocalize is rpe_run fed the oracle's matches, and ICP from its pose ends where tracking would."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import feature_oracle as FE
import photo_cases as PC
import util
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def same(a, b):
    """bit for bit, every NaN where the other has one"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32))


def check_side(ctx, which, xy, sc, de):
    gxy, gsc, gde = ctx.features(which)
    assert gxy.shape == xy.shape and np.array_equal(gxy, xy), (which, gxy.shape, xy.shape)
    assert np.array_equal(gsc, sc) and np.array_equal(gde, de)


def check_pair(ctx, p, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS), mopt=(FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, False)):
    """detect both sides, match, and hold everything to the oracle; returns the oracle's dict"""
    o = p.oracle(fopt, mopt)
    p.upload(ctx)
    assert ctx.features_detect(L.FEAT_FRAME, *fopt) == len(o["fxy"])
    assert ctx.features_detect(L.FEAT_MODEL, *fopt) == len(o["mxy"])
    check_side(ctx, L.FEAT_FRAME, o["fxy"], o["fs"], o["fd"])
    check_side(ctx, L.FEAT_MODEL, o["mxy"], o["ms"], o["md"])
    m = ctx.features_match(mopt[0], (mopt[1], mopt[2]), mopt[3])
    assert m == len(o["fi"]) == ctx.n
    fi, mi, d1, d2, w = ctx.matches()
    assert np.array_equal(fi, o["fi"]) and np.array_equal(mi, o["mi"]) and np.array_equal(d1, o["d1"]) and np.array_equal(d2, o["d2"])
    assert np.array_equal(w, o["w"])
    if m:
        for slot, key in ((L.XW, "XW"), (L.XC, "XC"), (L.BV, "BV"), (L.NW, "NW"), (L.NC, "NC")):
            assert same(ctx.download(slot), o[key]), key
    return o


# ---------------------------------------------------------------------------------------------- bit for bit, every case and size
@pytest.mark.parametrize("motion", ["narrow", "wide1", "wide2"])
@pytest.mark.parametrize("cam", ["small", "half", "full"])
def test_pairs_bit_exact(gpu_ctx_factory, cam, motion):
    o = check_pair(gpu_ctx_factory(), FC.pair(cam, motion))
    assert len(o["fi"]) >= 100


@pytest.mark.parametrize("cross", [False, True])
def test_cross_check_on_and_off(gpu_ctx_factory, cross):
    p = FC.pair("half", "wide1")
    off = p.oracle()
    o = check_pair(gpu_ctx_factory(), p, mopt=(FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, cross))
    if cross:
        assert 0 < len(o["fi"]) < len(off["fi"]) and len(np.unique(o["mi"])) == len(o["mi"])   # the check removes something here


def test_model_colour_with_holes(gpu_ctx_factory):
    p = FC.Pair(FC.HALF_CAM, FC.WIDE1, holes=True)
    o = check_pair(gpu_ctx_factory(), p)
    assert len(o["mxy"]) < len(FC.pair("half", "wide1").oracle()["mxy"])
    known = p.model_rgba[..., 3] != 0
    for dx, dy in FE.RING + ((0, 0),):
        assert known[o["mxy"][:, 1] + dy, o["mxy"][:, 0] + dx].all()


def test_other_thresholds_and_ratios(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("small", "narrow")
    check_pair(ctx, p, fopt=(30, 300), mopt=(40, 9, 10, True))
    check_pair(ctx, p, fopt=(1, FE.MAX_KEYPOINTS), mopt=(256, 1, 1, False))
    check_pair(ctx, p, fopt=(255, 10), mopt=(0, 8, 10, False))


# ---------------------------------------------------------------------------------------------- edges
def test_flat_frame_has_no_keypoints_and_no_matches(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    o = check_pair(ctx, FC.flat_pair())
    assert len(o["fxy"]) == 0 and len(o["mxy"]) > 0 and len(o["fi"]) == 0 and ctx.n == 0


def test_cap_of_one_and_one_model_keypoint(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("small", "narrow")
    o = check_pair(ctx, p, fopt=(FE.THRESHOLD, 1), mopt=(256, 8, 10, False))
    assert len(o["fxy"]) == len(o["mxy"]) == 1 and (len(o["d2"]) == 0 or o["d2"][0] == 257)
    # the frame's full list against ONE model keypoint: every d2 is 257
    assert ctx.features_detect(L.FEAT_FRAME) > 100
    full = p.frame.detect()
    fi, mi, d1, d2 = FE.match(full[2], o["md"], 256, 8, 10)
    assert ctx.features_match(256, (8, 10)) == len(fi) > 0
    g = ctx.matches()
    assert np.array_equal(g[0], fi) and np.array_equal(g[1], mi) and np.array_equal(g[2], d1) and np.array_equal(g[3], d2)
    assert (g[3] == 257).all() and (g[1] == 0).all()


@pytest.mark.parametrize("cap", [FE.MAX_KEYPOINTS, 1000])
def test_more_survivors_than_the_cap(gpu_ctx_factory, cap):
    p = FC.overcap_pair()
    assert p.frame.detect(with_survivors=True)[3] > FE.MAX_KEYPOINTS
    o = check_pair(gpu_ctx_factory(), p, fopt=(FE.THRESHOLD, cap))
    assert len(o["fxy"]) == len(o["mxy"]) == cap and (o["d1"] == 0).mean() > 0.8    # the same image on both sides (the depths differ)


def test_hamming_ties_of_a_repeated_texture(gpu_ctx_factory):
    """the model's descriptors repeat with the texture, the frame's differ from them by a few bits: the copies tie at d1 = d2 > 0 and
    the lowest index wins (a ratio of 2 / 1 lets a tie through; exact duplicates, d1 = d2 = 0, never pass a ratio test)"""
    p = FC.tiled_pair()
    o = check_pair(gpu_ctx_factory(), p, mopt=(256, 2, 1, False))
    assert len(np.unique(o["md"], axis=0)) < len(o["md"]) / 2 and (o["d2"] == o["d1"]).sum() > len(o["fi"]) / 2 > 10
    check_pair(gpu_ctx_factory(), p, mopt=(256, 2, 1, True))


def test_detect_twice_gives_the_same_bits(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("half", "wide1")
    p.upload(ctx)
    ctx.features_detect(L.FEAT_FRAME)
    a = ctx.features(L.FEAT_FRAME)
    ctx.features_detect(L.FEAT_MODEL)          # the shared workspace is used in between
    ctx.features_detect(L.FEAT_FRAME)
    b = ctx.features(L.FEAT_FRAME)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) == len(p.frame.detect()[0])


def code_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except L.RpeError as e:
        return e.code
    return L.RPE_OK


def test_state_and_argument_errors(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("small", "narrow")
    assert code_of(ctx.features_detect, L.FEAT_FRAME) == L.RPE_ERR_STATE            # no frame
    assert code_of(ctx.features_detect, L.FEAT_MODEL) == L.RPE_ERR_STATE            # no model
    ctx.frame_set_depth(p.db, p.cam, dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])
    assert code_of(ctx.features_detect, L.FEAT_FRAME) == L.RPE_ERR_STATE            # depth, no colour
    ctx.frame_set_color(p.cb)
    assert code_of(ctx.features, L.FEAT_FRAME) == L.RPE_ERR_STATE                   # not detected yet
    assert ctx.features_detect(L.FEAT_FRAME) > 0
    assert code_of(ctx.features_match) == L.RPE_ERR_STATE                           # no model
    assert code_of(ctx.relocalize, api.M_SK_PROSAC) == L.RPE_ERR_STATE
    ctx.model_upload(p.model.V, p.model.N, p.cam, p.pa)
    assert code_of(ctx.features_detect, L.FEAT_MODEL) == L.RPE_ERR_STATE            # model, no colour
    ctx.model_color_upload(p.model_rgba)
    assert code_of(ctx.features_match) == L.RPE_ERR_STATE                           # model features missing
    assert code_of(ctx.matches) == L.RPE_ERR_STATE
    assert ctx.features_detect(L.FEAT_MODEL) > 0
    assert ctx.features_match() > 0
    for bad in (dict(threshold=0), dict(threshold=256), dict(max_keypoints=0), dict(max_keypoints=L.MAX_KEYPOINTS + 1)):
        assert code_of(ctx.features_detect, L.FEAT_FRAME, **bad) == L.RPE_ERR_ARG, bad
    assert code_of(ctx.features_detect, 2) == L.RPE_ERR_ARG
    for bad in (dict(max_dist=-1), dict(max_dist=257), dict(ratio=(0, 10)), dict(ratio=(8, 0)), dict(ratio=(8, 65537)), dict(cross_check=2)):
        assert code_of(ctx.features_match, **bad) == L.RPE_ERR_ARG, bad
    assert code_of(ctx.relocalize, api.M_SK_PROSAC, min_matches=3) == L.RPE_ERR_ARG
    assert code_of(ctx.relocalize, 10) == L.RPE_ERR_ARG and code_of(ctx.relocalize, -1) == L.RPE_ERR_ARG
    assert ctx.features_match() > 0                                                  # the failed calls left the features alone


def test_invalidation_rules(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = FC.pair("small", "narrow")
    p.upload(ctx)
    depth_kw = dict(dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])

    def both():
        ctx.features_detect(L.FEAT_FRAME); ctx.features_detect(L.FEAT_MODEL)
        assert ctx.features_match() > 0 and len(ctx.matches()[0]) > 0

    both()
    ctx.frame_set_color(p.cb)                               # a new frame colour: the frame's features go, the model's stay
    assert code_of(ctx.features, L.FEAT_FRAME) == L.RPE_ERR_STATE and len(ctx.features(L.FEAT_MODEL)[0]) > 0
    assert code_of(ctx.features_match) == L.RPE_ERR_STATE and code_of(ctx.matches) == L.RPE_ERR_STATE
    both()
    ctx.frame_set_depth(p.db, p.cam, **depth_kw)            # a new depth drops colour and features
    assert code_of(ctx.features, L.FEAT_FRAME) == L.RPE_ERR_STATE and code_of(ctx.features_detect, L.FEAT_FRAME) == L.RPE_ERR_STATE
    ctx.frame_set_color(p.cb)
    both()
    ctx.model_color_upload(p.model_rgba)                    # a new model colour: the model's features go, the frame's stay
    assert code_of(ctx.features, L.FEAT_MODEL) == L.RPE_ERR_STATE and len(ctx.features(L.FEAT_FRAME)[0]) > 0
    assert code_of(ctx.matches) == L.RPE_ERR_STATE
    both()
    ctx.model_upload(p.model.V, p.model.N, p.cam, p.pa)     # a new model drops its colour and features
    assert code_of(ctx.features, L.FEAT_MODEL) == L.RPE_ERR_STATE and code_of(ctx.features_detect, L.FEAT_MODEL) == L.RPE_ERR_STATE
    ctx.model_color_upload(p.model_rgba)
    both()
    ctx.features_detect(L.FEAT_FRAME)                       # a new detection drops the match list, not the other side
    assert code_of(ctx.matches) == L.RPE_ERR_STATE and ctx.features_match() > 0
    ctx.model_from_frame(p.pb)                              # frame-to-frame users: model and colour from the frame
    assert code_of(ctx.features, L.FEAT_MODEL) == L.RPE_ERR_STATE
    ctx.model_color_from_frame()
    ctx.features_detect(L.FEAT_MODEL)
    a, b = ctx.features(L.FEAT_MODEL), ctx.features(L.FEAT_FRAME)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))   # the same view on both sides
    assert ctx.features_match() == len(a[0]) and (ctx.matches()[2] == 0).all()


# ---------------------------------------------------------------------------------------------- end to end
RELOC = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, **FC.RELOC_THRE)


@pytest.mark.parametrize("method,ls", [("M_SK_PROSAC", "LS_SHINJI_INLIERS"), ("M_SHINJI_RANSAC2", "LS_NONE"), ("M_NL_SK_RANSAC", "LS_NONE")])
@pytest.mark.parametrize("motion", ["wide1", "wide2"])
def test_relocalize_is_rpe_run_on_the_oracles_matches(gpu_ctx_factory, motion, method, ls):
    ctx = gpu_ctx_factory()
    p = FC.pair("half", motion)
    o = p.oracle()
    p.upload(ctx)
    got = ctx.relocalize(getattr(api, method), ls=getattr(api, ls), **RELOC)
    w3 = np.repeat(o["w"][:, None], 3, axis=1)
    ref = api.run(getattr(api, method), L.F32, xw=o["XW"], xc=o["XC"], bv=o["BV"], nw=o["NW"], nc=o["NC"], weights=w3, f=p.cam[0],
                  ls=getattr(api, ls), score_mode=L.SCORE_EXACT, **RELOC)
    assert got["matches"] == len(o["fi"]) and ref["max_votes"] > 20
    assert got["max_votes"] == ref["max_votes"] and got["iters"] == ref["iters"] and np.array_equal(got["masks"], ref["masks"])
    assert util.rot_err(got["pose12"][:9].reshape(3, 3), ref["R"]) < util.ROT_TOL_RAD
    assert util.trans_rel_err(got["pose12"][9:], ref["t"]) < util.TRANS_REL_TOL
    # the slots keep the matches, and the pose is the frame's up to what the matches' noise allows
    assert same(ctx.download(L.XW), o["XW"]) and same(ctx.download(L.XC), o["XC"])
    e = VC.pose_error(got["pose12"], p.pb)
    print(motion, method, "relocalised to", e, "from", VC.pose_error(p.pa, p.pb))
    assert e[0] < 0.02 and e[1] < 0.05


@pytest.mark.parametrize("motion", ["wide1", "wide2"])
def test_icp_from_the_relocalised_pose_tracks(gpu_ctx_factory, motion):
    """relocalize, then the RGB-D pyramid ICP from its pose: within 2 x the oracle's recorded figure (the margin volume_cases.py /
    photo_cases.py give GPU loops whose sums round differently)"""
    ctx = gpu_ctx_factory()
    p = FC.pair("half", motion)
    levels = len(VC.TRACK_ITERS)
    ctx.frame_set_depth(p.da, p.cam, 1.0, *VC.RANGE, levels=levels)
    ctx.frame_set_color(p.ca)
    ctx.model_from_frame(p.pa)
    ctx.model_color_from_frame()
    ctx.frame_set_depth(p.db, p.cam, 1.0, *VC.RANGE, levels=levels)
    ctx.frame_set_color(p.cb)
    got = ctx.relocalize(api.M_SK_PROSAC, ls=api.LS_SHINJI_INLIERS, **RELOC)
    ctx.photo_prepare(levels)
    pose = ctx.icp_pyramid_rgbd(got["pose12"], PC.WEIGHT, VC.TRACK_ITERS, VC.TRACK_GATES, cos_thr=PC.COS_THR)[0]
    e = VC.pose_error(pose, p.pb)
    want = FC.FIGURES[("half", motion)]["icp_after_reloc"]
    print(motion, "ICP after relocalisation", e, "oracle", want)
    assert e[0] < 2 * want[0] and e[1] < 2 * want[1]


def test_relocalize_on_a_flat_frame_is_degenerate(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    FC.flat_pair().upload(ctx)
    p = np.arange(12, dtype=np.float64)
    it, m, mv = api.C.c_int(50), api.C.c_int(-1), api.C.c_int(0)
    mask = np.zeros(3 * L.MAX_KEYPOINTS, np.int16)
    rc = L.lib().rpe_relocalize(ctx._h, None, None, api.M_SK_PROSAC, 0.05, 3.0, 0.1, api.C.byref(it), 0.99, 1, 0, 12, api._p(p), api.C.byref(m),
                                api.C.byref(mv), api._p(mask))
    assert rc == L.RPE_ERR_DEGENERATE and m.value == 0 and np.array_equal(p, np.arange(12))
    assert code_of(ctx.relocalize, api.M_SK_PROSAC) == L.RPE_ERR_DEGENERATE


# ---------------------------------------------------------------------------------------------- C++
def test_feature_reloc_cpp(tmp_path):
    """DepthFrontEnd::detectFeatures / matchFeatures / relocalize from plain C++ (tests/cpp/feature_reloc.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "feature_reloc")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "feature_reloc.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "feature_reloc: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
