"""CPU: the numpy statement of the feature stage (tests/feature_oracle.py) against itself -- its properties, the figures of
tests/feature_cases.py recomputed, the case conditions the GPU tests rely on, relocalisation end to end in the oracles -- and the
cross-compiled library: exports, header, the generated table, the C++ driver compiles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import feature_cases as FC
import feature_oracle as FE
import photo_cases as PC
import unit_gates as UG
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, simulator as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_features_detect", "rpe_features_download", "rpe_features_match", "rpe_matches_download", "rpe_relocalize"}
ALL_PAIRS = sorted(FC.FIGURES)
WIDE_HALF = [("half", "wide1"), ("half", "wide2")]


# ---------------------------------------------------------------------------------------------- properties of the statement
def test_identical_pair_matches_every_keypoint_to_itself():
    p = FC.pair("small", "narrow")
    xy, sc, de = p.frame.detect()
    assert len(xy) > 300
    # the box sums round many patches to the same bits only rarely: distinct descriptors match themselves at distance 0
    fi, mi, d1, d2 = FE.match(de, de, 256, 65536, 1)
    distinct = d2 > 0
    assert distinct.mean() > 0.95 and len(fi) == distinct.sum()
    assert np.array_equal(fi, mi) and (d1 == 0).all()
    fi, mi, d1, d2 = FE.match(de, de, 256, 65536, 1, cross_check=True)
    assert np.array_equal(fi, mi) and (d1 == 0).all() and len(fi) > 0.95 * len(xy)


@pytest.mark.parametrize("cam,motion", [("small", "wide1"), ("half", "narrow")])
def test_keypoints_keep_to_the_rules(cam, motion):
    p = FC.Pair(FC.CAMS[cam], FC.MOTIONS[motion], holes=True)
    for view in (p.frame, p.model):
        xy, sc, de = view.detect()
        pix = xy[:, 1].astype(np.int64) * view.w + xy[:, 0]
        assert len(pix) > 100 and (np.diff(pix) > 0).all()                       # pixel order, no duplicates
        assert (xy >= FE.BORDER).all() and (xy[:, 0] < view.w - FE.BORDER).all() and (xy[:, 1] < view.h - FE.BORDER).all()
        assert np.isfinite(view.V[pix]).all() and np.isfinite(view.N[pix]).all()
        assert (sc > 0).all() and de.shape == (len(pix), 8) and de.dtype == np.uint32
        known = view.rgba[..., 3] != 0
        for dx, dy in FE.RING + ((0, 0),):
            assert known[xy[:, 1] + dy, xy[:, 0] + dx].all()
        full = FE.scores(view.rgba, view.V, view.N)
        assert np.array_equal(full[xy[:, 1], xy[:, 0]], sc)
        for dy in (-1, 0, 1):                                                    # no survivor beside a stronger pixel
            for dx in (-1, 0, 1):
                assert (full[xy[:, 1] + dy, xy[:, 0] + dx] <= sc).all()
    assert np.isnan(p.frame.N).any(1).sum() > 100                                 # there were NaN normals to avoid


def test_the_detector_on_hand_made_patches():
    h = w = 48
    V = np.ones((h * w, 3), np.float32)
    base = np.zeros((h, w, 4), np.uint8)
    base[..., :3] = 100
    base[..., 3] = 255
    corner = base.copy()
    corner[24:, 24:, :3] = 200                                                   # a bright quadrant: its tip is a corner
    xy, sc, de = FE.detect(corner, V, V)
    assert len(xy) >= 1 and (np.abs(xy - 24) <= 2).all()
    edge = base.copy()
    edge[:, 24:, :3] = 200                                                       # a straight edge: 7 or 8 contiguous at most, no corner
    assert len(FE.detect(edge, V, V)[0]) == 0
    assert len(FE.detect(base, V, V)[0]) == 0
    unknown = corner.copy()
    unknown[21, 24, 3] = 0                                                       # one ring pixel of the tip without colour
    assert not any((x, y) == (24, 24) for x, y in FE.detect(unknown, V, V)[0])
    bad = V.copy()
    bad[:] = np.nan
    assert len(FE.detect(corner, V, bad)[0]) == 0 and len(FE.detect(corner, bad, V)[0]) == 0
    assert FE.luma(np.array([[[255, 255, 255, 255], [255, 255, 255, 0], [10, 20, 30, 1]]], np.uint8)).tolist() == [[255, 0, 18]]   # (770 + 3000 + 870 + 128) >> 8
    assert FE.box_sums(np.full((9, 9), 255, np.int32))[4, 4] == 6375 and FE.box_sums(np.full((9, 9), 255, np.int32))[0, 0] == 9 * 255


def test_the_cap_keeps_exactly_the_strongest_under_the_tie_rule():
    p = FC.overcap_pair()
    xy_all, sc_all, _, survivors = p.frame.detect(max_keypoints=1 << 30, with_survivors=True)
    assert survivors == len(xy_all) == FC.OVERCAP_SURVIVORS > FE.MAX_KEYPOINTS
    pix_all = xy_all[:, 1].astype(np.int64) * p.frame.w + xy_all[:, 0]
    ties = 0
    for cap in (FE.MAX_KEYPOINTS, 1000, 1):
        xy, sc, _ = p.frame.detect(max_keypoints=cap)
        pix = xy[:, 1].astype(np.int64) * p.frame.w + xy[:, 0]
        assert len(pix) == cap and (np.diff(pix) > 0).all()
        kept = np.isin(pix_all, pix)
        cut = sc.min()
        assert (sc_all[~kept] <= cut).all() and (sc_all[kept] >= cut).all()
        tie_kept, tie_lost = pix_all[kept & (sc_all == cut)], pix_all[~kept & (sc_all == cut)]
        assert len(tie_lost) == 0 or tie_kept.max() < tie_lost.min()             # among equals the lower pixels stay
        ties += len(tie_lost)
    assert ties > 0                                                              # the tie rule did decide something


def test_match_rules_on_hand_made_descriptors():
    z = np.zeros((1, 8), np.uint32)
    one = z.copy(); one[0, 0] = 1
    three = z.copy(); three[0, 7] = 0x80000001; three[0, 3] = 2
    model = np.concatenate([three, one, one, z])                                 # distances from z: 3 1 1 0
    fi, mi, d1, d2 = FE.match(z, model, 256, 65536, 1)
    assert (fi.tolist(), mi.tolist(), d1.tolist(), d2.tolist()) == ([0], [3], [0], [1])
    fi, mi, d1, d2 = FE.match(z, model[:3], 256, 2, 1)                           # a tie at 1: the lower index, d2 = d1
    assert (mi.tolist(), d1.tolist(), d2.tolist()) == ([1], [1], [1])
    assert len(FE.match(z, model[:3], 256, 1, 1)[0]) == 0                        # 1 * 1 < 1 * 1 fails
    assert len(FE.match(z, model[:3], 0, 2, 1)[0]) == 0                          # max_dist
    fi, mi, d1, d2 = FE.match(z, model[:1], 256, 8, 10)
    assert (d1.tolist(), d2.tolist()) == ([3], [257])                            # one model keypoint
    assert len(FE.match(z, model[:0])[0]) == 0 and len(FE.match(model[:0], z)[0]) == 0
    # cross-check: both frame keypoints pick model 0, model 0 picks the lower of its two equals
    fi, mi, _, _ = FE.match(np.concatenate([one, one]), np.concatenate([z, three]), 256, 8, 10, cross_check=True)
    assert (fi.tolist(), mi.tolist()) == ([0], [0])
    bits = np.zeros((1, 8), np.uint32); bits[0, 2] = 1 << 5                      # bit 69 lives in word 2 at bit 5
    S_ = np.zeros((64, 64), np.int32)
    a = FE.PAIRS[69]
    S_[32 + a[3], 32 + a[2]] = 9
    assert np.array_equal(FE.describe(S_, np.array([32 * 64 + 32]), 64) & bits, bits)


def test_table_header_is_what_the_generator_regenerates():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_brief_table as GB
    assert open(GB.HEADER).read() == GB.render()
    P = np.array(GB.pairs())
    assert P.shape == (256, 4) and np.abs(P).max() == 13 and (P[:, :2] != P[:, 2:]).any(1).all()
    assert len({tuple(r) for r in P.tolist()} | {tuple(r[2:] + r[:2]) for r in P.tolist()}) == 512     # no test twice, in either direction
    assert GB.PCG32(42, 54).next32() == 0xa15c02b7                              # the stream is the reference vector's (pcg32 demo, seed 42)


def test_cell_texture_has_corners_on_every_surface():
    P = np.array([[0.01, 0.02, 0.03], [0.06, 0.02, 0.03], [0.09, 0.02, 0.03], [2.7, 1.5, 5.0], [2.7 + 1e-12, 1.5 - 1e-12, 5.0]])
    c = S.cell_texture(P)
    assert c.shape == (5, 3) and (c >= 0).all() and (c <= 255).all() and np.array_equal(c, np.rint(c))
    assert np.array_equal(c[0], c[1]) and not np.array_equal(c[0], c[2])         # one cell, then the next
    assert np.array_equal(c[3], c[4])                                            # the room's walls are off the cell boundaries
    assert not np.array_equal(S.cell_texture(P, 0.05)[0], S.cell_texture(P, 0.05)[1])


# ---------------------------------------------------------------------------------------------- the figures of feature_cases.py
@pytest.mark.parametrize("cam,motion", ALL_PAIRS)
def test_pair_figures_and_case_conditions(cam, motion):
    p = FC.pair(cam, motion)
    o = p.oracle()
    ok = p.correct(o)
    fig = FC.FIGURES[(cam, motion)]
    print(cam, motion, len(o["fxy"]), len(o["mxy"]), len(o["fi"]), ok.mean())
    assert (len(o["fxy"]), len(o["mxy"])) == fig["keypoints"] and len(o["fi"]) == fig["matches"]
    assert abs(ok.mean() - fig["correct"]) < 6e-4           # the figure is recorded to three places
    assert len(o["fi"]) >= 100 and ok.mean() >= 0.5                              # what every pair used end to end must offer
    assert np.array_equal(o["w"], (256 - o["d1"]).astype(np.float32)) and (np.diff(o["fi"]) > 0).all()


def test_other_case_figures():
    o = FC.flat_pair().oracle()
    assert len(o["fxy"]) == 0 and len(o["fi"]) == 0 and len(o["mxy"]) > 100
    t = FC.tiled_pair().oracle(mopt=(256, 2, 1, False))
    assert (len(t["fxy"]), len(t["mxy"]), len(t["fi"])) == (457, 388, 451)
    assert len(np.unique(t["md"], axis=0)) == 74 and (t["d1"] == t["d2"]).sum() == 361
    hp = FC.Pair(FC.HALF_CAM, FC.WIDE1, holes=True)
    h = hp.oracle()
    assert len(h["mxy"]) < FC.FIGURES[("half", "wide1")]["keypoints"][1] and len(h["fi"]) >= 100 and hp.correct(h).mean() >= 0.5


def _near(got, want, rel=0.05):
    return all(abs(g - w) <= rel * w for g, w in zip(got, want))


@pytest.mark.parametrize("cam,motion", WIDE_HALF)
def test_relocalise_then_track(oracle, cam, motion):
    """the oracle-side solver on the oracle's matches gives a pose from which oracle RGB-D ICP ends within the order of the tracked
    pair's figure (photo_cases.PAIR_ROOM_RGBD); the same ICP from the stale pose A stays lost"""
    p = FC.pair(cam, motion)
    o = p.oracle()
    fig = FC.FIGURES[(cam, motion)]
    pose, r = FC.oracle_relocalise(oracle, p, o)
    start, reloc = VC.pose_error(p.pa, p.pb), VC.pose_error(pose, p.pb)
    after = VC.pose_error(FC.oracle_track(oracle, p, pose), p.pb)
    stale = VC.pose_error(FC.oracle_track(oracle, p, p.pa), p.pb)
    print(cam, motion, "votes", r["max_votes"], "iters", r["iters"], "start", start, "reloc", reloc, "ICP after", after, "ICP from stale", stale)
    assert (r["max_votes"], r["iters"]) == (fig["votes"], fig["iters"])
    assert _near(start, fig["start"]) and _near(reloc, fig["reloc"]) and _near(after, fig["icp_after_reloc"]) and _near(stale, fig["icp_from_stale"])
    assert after[0] < 10 * PC.PAIR_ROOM_RGBD[0] and after[1] < 10 * PC.PAIR_ROOM_RGBD[1]      # the same order as a tracked pair
    assert stale[0] > 0.5 * start[0] and stale[1] > 0.5 * start[1]                            # tracking alone does not recover
    assert reloc[0] < 0.01 * start[0] + 1e-3 and reloc[1] < 0.02 * start[1]


# ---------------------------------------------------------------------------------------------- the cross-compiled library
def test_header_and_library_export_the_feature_entry_points():
    hdr = UG.check_entry_points(SYMS)
    assert "RPE_FEAT_FRAME = 0, RPE_FEAT_MODEL = 1, RPE_MAX_KEYPOINTS = 4096" in hdr
    assert (L.FEAT_FRAME, L.FEAT_MODEL, L.MAX_KEYPOINTS) == (0, 1, FE.MAX_KEYPOINTS)
    assert L.lib().rpe_abi_version() == 1


def test_feature_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "feature_reloc.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "feature_reloc")])
