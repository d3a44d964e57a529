"""CPU: the numpy statement of the scale levels (tests/scale_oracle.py) against itself -- sizes, weights, centres, one level = the
stage as it was -- the figures of tests/scale_cases.py recomputed (what moving closer does to a one-level detection and what four levels
make of it, matches and relocalisation end to end in the oracles), the case conditions the GPU tests rely on, and the cross-compiled
library: exports, header, the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import feature_edge_cases as FEC
import feature_oracle as FE
import keyframe_cases as KC
import oriented_oracle as OO
import scale_cases as SC
import scale_oracle as SO
import unit_gates as UG
import volume_cases as VC
from frontend_util import SMALL_CAM
from rgbd_pose_estimation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_features_set_levels", "rpe_features_get_levels", "rpe_features_scale"}


def per_level(level):
    return [int((level == l).sum()) for l in range(SO.MAX_LEVELS)]


# ---------------------------------------------------------------------------------------------- properties of the statement
def test_sizes_and_centres():
    assert [SO.level_size(160, 120, l) for l in range(4)] == [(160, 120), (106, 80), (80, 60), (53, 40)]
    assert [SO.level_size(96, 72, l) for l in range(4)] == [(96, 72), (64, 48), (48, 36), (32, 24)]
    assert [SO.level_size(161, 121, l) for l in range(4)] == [(161, 121), (107, 80), (80, 60), (53, 40)]
    u = np.arange(200)
    assert np.array_equal(SO.centre(u, 0), u) and np.array_equal(SO.centre(u, 2), 2 * u) and np.array_equal(SO.centre(u, 3), 3 * u + 1)
    assert np.array_equal(SO.centre(u, 1), (6 * u + 1) // 4)
    for w in (33, 96, 160, 161, 641):                       # the centre of the last level pixel is a pixel of the image
        for l in range(4):
            wl = SO.level_size(w, w, l)[0]
            assert wl == 0 or SO.centre(wl - 1, l) < w
    # 0.81 times the pixels of level 0 in the three extra levels
    assert abs(sum(np.prod(SO.level_size(640, 480, l)) for l in (1, 2, 3)) / (640 * 480) - (4 / 9 + 1 / 4 + 1 / 9)) < 1e-3


def test_level_images_are_the_stated_means():
    rng = np.random.default_rng(5)
    h, w = 41, 47
    rgba = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    rgba[..., 3] = np.where(rng.random((h, w)) < 0.1, 0, 255)
    Y0, A = FE.luma(rgba).astype(np.int64), rgba[..., 3] != 0
    ims = SO.level_images(rgba, 4)
    assert np.array_equal(ims[0][0], Y0) and np.array_equal(ims[0][1], A)
    # 1 / 2: the rounded 2 x 2 mean; 1 / 3: the rounded 3 x 3 mean
    for l, q in ((2, 2), (3, 3)):
        Y, K = ims[l]
        assert Y.shape == (h // q, w // q)
        blocks = Y0[:h // q * q, :w // q * q].reshape(h // q, q, w // q, q)
        assert np.array_equal(Y, (blocks.sum((1, 3)) + q * q // 2) // (q * q))
        assert np.array_equal(K, A[:h // q * q, :w // q * q].reshape(h // q, q, w // q, q).all((1, 3)))
    # 2 / 3: per axis weights (2, 1) on sources (3 k, 3 k + 1) for u = 2 k and (1, 2) on (3 k + 1, 3 k + 2) for u = 2 k + 1
    Y, K = ims[1]
    assert Y.shape == (h * 2 // 3, w * 2 // 3)

    def taps(n):
        k, odd = np.arange(n) // 2, np.arange(n) % 2
        return 3 * k + odd, 3 * k + odd + 1, np.where(odd, 1, 2), np.where(odd, 2, 1)

    xa, xb, wxa, wxb = taps(Y.shape[1])
    ya, yb, wya, wyb = taps(Y.shape[0])
    rows = lambda img: img[ya] * wya[:, None] + img[yb] * wyb[:, None]
    tot = (rows(Y0)[:, xa] * wxa + rows(Y0)[:, xb] * wxb)
    assert np.array_equal(Y, (tot + 4) // 9)
    assert np.array_equal(K, A[ya][:, xa] & A[ya][:, xb] & A[yb][:, xa] & A[yb][:, xb])


@pytest.mark.parametrize("kind", [SO.UPRIGHT, SO.ORIENTED])
def test_one_level_is_the_stage_as_it_was(kind):
    p = SC.pair("small", "tz-1.6")
    for view in (p.frame, p.model):
        xy, sc, de, level, lxy, bins = SC.detect(view, 1, kind)
        if kind == SO.ORIENTED:
            ref = OO.detect(view.rgba, view.V, view.N)
            assert np.array_equal(bins, ref[3])
        else:
            ref = FE.detect(view.rgba, view.V, view.N)
            assert not bins.any()
        assert np.array_equal(xy, ref[0]) and np.array_equal(sc, ref[1]) and np.array_equal(de, ref[2])
        assert not level.any() and np.array_equal(lxy, xy) and xy.dtype == lxy.dtype == level.dtype == np.int32
    xy, sc, de = SC.detect(p.frame, 1, fopt=(FE.THRESHOLD, 100))[:3]
    assert all(np.array_equal(a, b) for a, b in zip((xy, sc, de), FE.detect(p.frame.rgba, p.frame.V, p.frame.N, FE.THRESHOLD, 100)))


def test_the_levels_share_one_list_and_one_cap():
    p = SC.pair("small", "tz-1.6")
    xy, sc, de, level, lxy, _ = SC.detect(p.frame, 4)
    assert per_level(level) == [291, 159, 81, 19] and (np.diff(level) >= 0).all()
    for l in range(4):
        m = level == l
        wl = SO.level_size(p.frame.w, p.frame.h, l)[0]
        assert (np.diff(lxy[m, 1].astype(np.int64) * wl + lxy[m, 0]) > 0).all()           # level pixel order inside a level
        assert np.array_equal(xy[m], np.stack([SO.centre(lxy[m, 0], l), SO.centre(lxy[m, 1], l)], 1))
    # the first levels of a longer ladder are the shorter ladder
    x3 = SC.detect(p.frame, 3)
    assert all(np.array_equal(a[level < 3], b) for a, b in zip((xy, sc, de, level, lxy), x3))
    # the cap keeps the strongest across levels, listed in the list's order
    cxy, csc, cde, clevel, clxy, _ = SC.detect(p.frame, 4, fopt=(FE.THRESHOLD, 100))
    assert len(csc) == 100 and csc.min() >= np.sort(sc)[::-1][99] and len(np.unique(clevel)) >= 3 and (np.diff(clevel) >= 0).all()
    keep = np.sort(np.lexsort((np.arange(len(sc)), -sc.astype(np.int64)))[:100])
    assert np.array_equal(cxy, xy[keep]) and np.array_equal(cde, de[keep]) and np.array_equal(clxy, lxy[keep])


# ---------------------------------------------------------------------------------------------- the figures of scale_cases.py
@pytest.mark.parametrize("cam,motion,kind", sorted(SC.FIGURES))
def test_pair_figures(oracle, cam, motion, kind):
    p = SC.pair(cam, motion)
    fig = SC.FIGURES[(cam, motion, kind)]
    near = lambda got, want: all(abs(g - w) <= 0.05 * w for g, w in zip(got, want))
    for name, levels in (("one", 1), ("four", 4)):
        o = SC.oracle(p, levels, kind)
        c = p.correct(o)
        pose, r = FC.oracle_relocalise(oracle, p, o)
        e = VC.pose_error(pose, p.pb)
        print(cam, motion, kind, levels, "levels:", len(o["fi"]), "matches", int(c.sum()), "correct, error", e, "votes", r["max_votes"],
              "iters", r["iters"])
        assert (len(o["fi"]), int(c.sum())) == fig[name]
        assert np.array_equal(o["w"], (256 - o["d1"]).astype(np.float32)) and (np.diff(o["fi"]) > 0).all()
        want = fig["reloc_" + name]
        assert not np.isfinite(e[0]) if want is None else near(e, want)
        inside = e[0] < SC.RELOC_BOUND[0] and e[1] < SC.RELOC_BOUND[1]
        if levels == 4:
            assert (r["max_votes"], r["iters"]) == (fig["votes_four"], fig["iters_four"])
            assert inside or (cam, motion, kind) not in SC.WITHIN
        elif (cam, motion, kind) in SC.LOST_AT_ONE:
            assert not inside


def test_the_bound_and_the_cases_it_holds_for():
    assert SC.RELOC_BOUND == KC.RELOC_BOUND == (5e-3, 15e-3)
    assert set(SC.WITHIN) >= {("half", m, SO.UPRIGHT) for m in ("narrow", "tz-1.0", "tz-1.6", "tz-2.1", "wide1_tz-1.6")}
    assert set(SC.WITHIN) >= {("half", "roll0.6_tz-1.6", SO.ORIENTED), ("half", "wide1_rz0.8_tz-1.6", SO.ORIENTED)}


def test_every_level_pays():
    p = SC.pair("half", "tz-1.6")
    for levels, want in SC.LADDER.items():
        o = SC.oracle(p, levels)
        assert (len(o["fi"]), int(p.correct(o).sum())) == want
    assert [SC.LADDER[n][1] for n in (2, 3, 4)] == [182, 303, 364]


# ---------------------------------------------------------------------------------------------- conditions of the GPU cases
def test_the_noise_image_exceeds_the_cap_with_a_tie_on_two_levels():
    p = SC.overcap_pair()
    for view, kept_ties in ((p.frame, 3), (p.model, 9)):
        xy, sc, de, level, lxy, _, survivors = SO.detect(view.rgba, view.V, view.N, levels=4, with_survivors=True)
        assert sum(survivors) > FE.MAX_KEYPOINTS and all(s > 0 for s in survivors) and len(sc) == FE.MAX_KEYPOINTS
        every = SO.detect(view.rgba, view.V, view.N, max_keypoints=sum(survivors), levels=4)
        T = sc.min()
        ties = per_level(every[3][every[1] == T])
        assert ties[0] > 0 and ties[1] > 0 and (sc == T).sum() == kept_ties < sum(ties), (T, ties)
        # the kept ties are the first of the list's order: level 0's before level 1's
        first = np.flatnonzero(every[1] == T)[:kept_ties]
        assert np.array_equal(every[4][first], lxy[sc == T]) and np.array_equal(every[3][first], level[sc == T])


def test_the_small_cameras_take_every_path():
    # 96 x 72: level 3 is 32 x 24 and empty, level 2 (48 x 36) has an interior of 16 x 4
    cam = FEC.camera(96, 72)
    p = FC.Pair(cam, SC.MOTIONS["tz-1.6"])
    for view in (p.frame, p.model):
        level, lxy = SC.detect(view, 4)[3:5]
        n = per_level(level)
        assert n[3] == 0 and n[2] > 0 and n[1] > 0
        at2 = lxy[level == 2]
        assert at2[:, 0].min() >= 16 and at2[:, 0].max() <= 31 and at2[:, 1].min() >= 16 and at2[:, 1].max() <= 19
    # 161 x 121: keypoints on every level, both kinds
    p = FC.Pair(FEC.camera(161, 121), SC.MOTIONS["tz-1.6"])
    for kind in (SO.UPRIGHT, SO.ORIENTED):
        o = SC.oracle(p, 4, kind)
        assert min(per_level(o["fl"])) > 0 and min(per_level(o["ml"])) > 0 and len(o["fi"]) > 20


def test_holes_leave_keypoints_only_where_every_source_is_known():
    p = FC.Pair(SMALL_CAM, SC.MOTIONS["tz-1.6"], holes=True)
    ims = SO.level_images(p.model.rgba, 4)
    share = [K.mean() for _, K in ims]
    assert share[0] > 0.9 and all(s < 0.86 for s in share[1:])                           # the [::7, ::5] pattern spreads
    xy, sc, de, level, lxy, _ = SC.detect(p.model, 4)
    assert per_level(level)[1] > 50 and per_level(level)[2] > 10
    for l, (u, v) in zip(level, lxy):
        K = ims[l][1]
        assert K[v, u] and all(K[v + dy, u + dx] for dx, dy in FE.RING)
    clean = SC.detect(SC.pair("small", "tz-1.6").model, 4)
    assert len(sc) < len(clean[1])


def test_a_hole_at_the_centre_pixel_drops_the_level_keypoint():
    holed, clean, chosen = SC.centre_hole_pair()
    assert [l for l, _, _ in chosen] == [1, 2, 3]
    a, b = SC.detect(clean.frame, 4), SC.detect(holed.frame, 4)
    had = {(int(l), int(u), int(v)) for l, (u, v) in zip(a[3], a[4])}
    has = {(int(l), int(u), int(v)) for l, (u, v) in zip(b[3], b[4])}
    assert all(k in had and k not in has for k in chosen) and len(has) > 0.9 * len(had)
    assert np.array_equal(holed.frame.rgba, clean.frame.rgba)                            # the colour is untouched: geometry alone


@pytest.mark.parametrize("oriented", [False, True])
def test_the_corner_scene_has_a_keypoint_on_the_border_of_every_level(oriented):
    scene, dots = SC.corner_scene(oriented=oriented)
    h, w = scene.cam[5], scene.cam[4]
    assert sorted({l for l, _, _ in dots}) == [0, 1, 2, 3] and len(dots) == 16
    for which in (0, 1):
        xy, sc, de, level, lxy, bins = SC.detect(scene.view(which), 4, int(oriented))
        have = {(int(l), int(u), int(v)) for l, (u, v) in zip(level, lxy)}
        found = [d in have for d in dots]
        if oriented:
            assert sum(found) >= 14 and all(n > 0 for n in SC.outside_samples(level, lxy, bins, w, h))
        else:
            assert all(found) and not bins.any()


def test_mixed_cameras_match_across_levels():
    p = FEC.MixedPair(SMALL_CAM, FC.HALF_CAM, motion=SC.MOTIONS["tz-1.6"])
    o = SC.oracle(p, 4)
    assert per_level(o["fl"]) == [291, 159, 81, 19] and per_level(o["ml"]) == [1210, 896, 514, 231]
    assert len(o["fi"]) == 196 and int(p.correct(o).sum()) == 184


# ---------------------------------------------------------------------------------------------- the cross-compiled library
def test_header_and_library_export_the_scale_entry_points():
    hdr = UG.check_entry_points(SYMS)
    flat = " ".join(hdr.replace(" *", " ").split())
    assert "Scale levels" in flat and "1 / 1, 2 / 3, 1 / 2, 1 / 3" in flat and "floor(((2 u + 1) q - p) / (2 p))" in flat
    assert "no suppression across levels" in flat and "no level above scale 1" in flat and "quantised to level-0 pixels" in flat
    assert "RPE_FEAT_FRAME = 0, RPE_FEAT_MODEL = 1, RPE_MAX_KEYPOINTS = 4096" in hdr                # the cap stays the total
    assert "typedef struct { int threshold; int max_keypoints; } rpe_feature_options;" in hdr       # the layout stays
    assert L.lib().rpe_abi_version() == 1


def test_level_arguments_are_checked_before_anything_else():
    """the argument checks need no device: a null context and a null output are refused on any machine"""
    UG.built()
    lib = L.lib()
    assert lib.rpe_features_set_levels(None, 2) == L.RPE_ERR_ARG and lib.rpe_features_get_levels(None, None) == L.RPE_ERR_ARG
    assert lib.rpe_features_scale(None, 0, None, None) == L.RPE_ERR_ARG


def test_scale_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "scale_reloc.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "scale_reloc")])
