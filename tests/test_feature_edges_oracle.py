"""CPU: every figure and case condition of tests/feature_edge_cases.py recomputed with tests/feature_oracle.py, so that each GPU test
of tests/test_gpu_feature_edges.py may rely on its case doing what its name says; and a SECOND statement of the detector, plain
scalar Python written from the text of include/rgbd_pose_hip.h Part 3 without a call into feature_oracle, to which the vectorised
oracle -- written beside the kernels and the only reference the GPU is held to -- is held in every array, at the sizes where a loop
per pixel is affordable."""
import math
import os
import re

import numpy as np
import pytest

import feature_cases as FC
import feature_edge_cases as E
import feature_oracle as FE
import volume_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNCAPPED = 1 << 30


def pixels(xy, w):
    return xy[:, 1].astype(np.int64) * w + xy[:, 0]


# ---------------------------------------------------------------------------------------------- odd and mixed pairs
def check_figures(p, o, fig):
    ok = p.correct(o)
    print(len(o["fxy"]), len(o["mxy"]), len(o["fi"]), ok.mean())
    assert (len(o["fxy"]), len(o["mxy"])) == fig["keypoints"] and len(o["fi"]) == fig["matches"]
    assert abs(ok.mean() - fig["correct"]) < 6e-4           # the figure is recorded to three places
    assert len(o["fi"]) >= 100 and ok.mean() >= 0.5


@pytest.mark.parametrize("motion", sorted(E.ODD_FIGURES))
def test_odd_pair_figures_and_limit_lines(motion):
    p = E.odd_pair(motion)
    w, h = E.ODD_CAM[4:]
    assert w % 32 and h % 8 and (w * h) % 256                 # partial tiles on both axes, a chunk tail
    o = p.oracle()
    check_figures(p, o, E.ODD_FIGURES[motion])
    assert all(n > 0 for n in E.on_limit_lines(o["fxy"], w, h)), E.on_limit_lines(o["fxy"], w, h)


@pytest.mark.parametrize("name", sorted(E.MIXED))
def test_mixed_pair_figures_and_the_two_widths(name):
    p = E.mixed_pair(name)
    assert p.cam[4] != p.mcam[4] and p.cam[5] != p.mcam[5]
    o = p.oracle()
    check_figures(p, o, E.MIXED_FIGURES[name])
    # the frame is feature_cases' own, the model the odd camera's (or the other way round)
    assert np.array_equal(o["fxy"], FC.Pair(p.cam, FC.WIDE1).oracle()["fxy"])
    assert np.array_equal(o["mxy"], FC.Pair(p.mcam, FC.WIDE1).oracle()["mxy"])
    # a gather that indexed the model maps with the frame's width would change EVERY row of XW (a NaN row counts as a value)
    wrong = E.mixed_pair(name, swap_model_width=True).oracle()
    for k in ("fi", "mi", "d1", "XC", "NC", "BV"):
        assert np.array_equal(wrong[k], o[k], equal_nan=True)
    changed = (np.nan_to_num(wrong["XW"], nan=-1e9) != np.nan_to_num(o["XW"], nan=-1e9)).any(1)
    assert changed.all() and len(changed) == E.MIXED_FIGURES[name]["matches"]


# ---------------------------------------------------------------------------------------------- lattices
@pytest.mark.parametrize("size", sorted(E.LATTICE_SIZES))
def test_lattice_survivors_all_tie(size):
    s = E.lattice(size)
    w, h = E.LATTICE_SIZES[size]
    dots = E.lattice_pixels(w, h)
    assert len(dots) == E.LATTICE_SURVIVORS[size] > FE.MAX_KEYPOINTS
    for which in (0, 1):
        for t, score in E.LATTICE_SCORE.items():
            xy, sc, de, n = s.detect(which, t, UNCAPPED, with_survivors=True)
            assert n == len(dots) and np.array_equal(pixels(xy, w), dots) and (sc == score).all()
            assert score == 16 * (255 - t)
        assert len(np.unique(de, axis=0)) == 9                # first / inner / last row x column
        assert len(np.unique(s.detect(which)[2], axis=0)) == E.LATTICE_DISTINCT_DESCRIPTORS
        assert len(s.detect(which, 255)[0]) == 0              # no survivor is possible: nothing exceeds Y + 255
        for cap in E.LATTICE_CAPS:                            # the cut inside the one tie class: the first `cap` in pixel order
            xy, sc, de = s.detect(which, FE.THRESHOLD, cap)
            assert np.array_equal(pixels(xy, w), dots[:cap]) and (sc == E.LATTICE_SCORE[FE.THRESHOLD]).all()
    assert E.LATTICE_SCORE[1] == 4064 < 4096                  # the top of the score range, inside the histogram's 4096 bins


def test_two_class_lattice():
    s = E.lattice("640x480", two_class=True)
    w, h = 640, 480
    xy, sc, de, n = s.detect(0, FE.THRESHOLD, UNCAPPED, with_survivors=True)
    pix = pixels(xy, w)
    assert np.array_equal(pix, E.lattice_pixels(w, h))
    assert dict(zip(*(a.tolist() for a in np.unique(sc, return_counts=True)))) == E.TWO_CLASS
    hi, lo = pix[sc == 3888], pix[sc == 2928]
    want = {4096: np.sort(np.concatenate([hi, lo[:4096 - 2838]])), 2838: hi, 2839: np.sort(np.concatenate([hi, lo[:1]])), 1: hi[:1]}
    assert set(want) == set(E.TWO_CLASS_CAPS) and 4096 - 2838 == 1258
    for cap, keep in want.items():
        assert np.array_equal(pixels(s.detect(0, FE.THRESHOLD, cap)[0], w), keep), cap


@pytest.mark.parametrize("size", sorted(E.LATTICE_SIZES))
def test_lattice_against_itself_matches_only_the_unique_descriptors(size):
    """4096 keypoints of 6 distinct descriptors: a repeated one has d1 = d2 = 0, which passes no ratio; the two descriptors that occur
    once (the first row's first and last dot) match themselves, at any ratio"""
    de = E.lattice(size).detect(0)[2]
    assert len(de) == FE.MAX_KEYPOINTS
    d1, i1, d2 = FE.best_two(FE.hamming(de, de))
    _, first, inverse, counts = np.unique(de, axis=0, return_index=True, return_inverse=True, return_counts=True)
    once = counts[inverse.reshape(-1)] == 1
    assert (d1 == 0).all() and np.array_equal(d2 == 0, ~once) and once.sum() == 2 == E.LATTICE_MATCHES
    for ratio in ((FE.RATIO_NUM, FE.RATIO_DEN), (65536, 1)):
        fi, mi, _, _ = FE.match(de, de, FE.MAX_DIST, *ratio)
        assert np.array_equal(fi, np.flatnonzero(once)) and np.array_equal(mi, fi)


@pytest.mark.parametrize("size", sorted(E.TINY), ids=lambda s: "x".join(map(str, s)))
def test_tiny_images(size):
    s = E.lattice(size)
    for which in (0, 1):
        xy, sc, de = s.detect(which)
        assert xy.tolist() == [list(k) for k in E.TINY[size]] and xy.shape == (len(E.TINY[size]), 2)
        assert sc.shape == (len(xy),) and de.shape == (len(xy), 8) and de.dtype == np.uint32
    fi, mi, d1, d2 = FE.match(de, de, 256)
    assert (fi.tolist(), mi.tolist(), d1.tolist(), d2.tolist()) == (([0], [0], [0], [257]) if len(de) else ([], [], [], []))


# ---------------------------------------------------------------------------------------------- noise, holes, flat models
def test_noise_figures():
    p = E.noise_pair()
    w, h = E.NOISE_CAM[4:]
    assert w % 32 and w > 32 and h % 8 and (w * h) % 256
    v = p.frame
    ones = np.ones_like(v.V)
    assert FE.detect(v.rgba, ones, ones, FE.THRESHOLD, UNCAPPED, with_survivors=True)[3] == E.NOISE_SURVIVORS["finite"]
    xy, sc, de, n = v.detect(FE.THRESHOLD, UNCAPPED, with_survivors=True)
    assert n == E.NOISE_SURVIVORS["rendered"] and np.isnan(v.N).any(1).sum() == E.NOISE_NAN_NORMALS
    assert all(k > 0 for k in E.on_limit_lines(xy, w, h)), E.on_limit_lines(xy, w, h)
    V = v.V.copy()
    V[E.noise_holes()] = np.nan
    assert FE.detect(v.rgba, V, v.N, FE.THRESHOLD, UNCAPPED, with_survivors=True)[3] == E.NOISE_SURVIVORS["holed"]
    # the model: alpha = 0 holes took keypoints away, and enough stay for the caps of the M1 tails on both sides
    m = p.model.detect()
    assert len(m[0]) < len(E.noise_pair(holes=False).model.detect()[0]) and (p.model_rgba[..., 3] == 0).any()
    assert len(m[0]) == E.NOISE_MODEL_KEYPOINTS > 2 * 256 + 1 and n >= max(E.M1_FRAME_CAPS)
    assert all(k > 0 for k in E.on_limit_lines(m[0], w, h))


def test_holes_in_the_depth_remove_keypoints():
    plain, holed = E.holed_depth_scenes()
    assert (holed.depth == 0).sum() >= E.noise_holes().sum() > 0.04 * holed.depth.size
    a, b = plain.detect(0)[0], holed.detect(0)[0]
    pa, pb = set(pixels(a, plain.cam[4]).tolist()), set(pixels(b, plain.cam[4]).tolist())
    gone = sorted(pa - pb)
    assert len(gone) > 20 and len(b) < len(a)
    # every keypoint that went had a NaN vertex or normal in the holed maps: the colour alone would have kept it
    assert all(not (np.isfinite(holed.V[q]).all() and np.isfinite(holed.N[q]).all()) for q in gone)
    assert any(np.isnan(holed.V[q]).any() for q in gone)


def test_flat_models():
    o = E.flat_model_pair().oracle()
    assert len(o["fxy"]) > 100 and len(o["mxy"]) == 0 and len(o["fi"]) == 0
    o = E.both_flat_pair().oracle()
    assert len(o["fxy"]) == 0 and len(o["mxy"]) == 0 and len(o["fi"]) == 0
    for cross in (False, True):
        assert len(E.flat_model_pair().oracle(mopt=(FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, cross))["fi"]) == 0


def test_odd_wide1_relocalises_in_the_oracles(oracle):
    p = E.odd_pair("wide1")
    pose, r = FC.oracle_relocalise(oracle, p, p.oracle())
    e = VC.pose_error(pose, p.pb)
    print("votes", r["max_votes"], "iters", r["iters"], "error", e)
    fig = E.ODD_WIDE1_RELOC
    assert (r["max_votes"], r["iters"]) == (fig["votes"], fig["iters"])
    assert all(abs(g - w) <= 0.05 * w for g, w in zip(e, fig["error"]))
    assert e[0] < 0.01 and e[1] < 0.025                      # 2 x stays inside test_gpu_feature's own bound on a relocalised pose


# ---------------------------------------------------------------------------------------------- the second statement
# Plain scalar Python from include/rgbd_pose_hip.h Part 3.  Nothing below calls feature_oracle; the ring offsets are typed from the
# header's text, the pair table is read from the generated csrc/rpe_brief_table.h.
H_RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2),
          (-1, -3)]


def table_pairs():
    text = open(os.path.join(ROOT, "rgbd_pose_estimation_amd", "csrc", "rpe_brief_table.h")).read()
    rows = re.findall(r"\{\s*(-?\d+),\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\}", text)
    assert len(rows) == 256
    return [tuple(int(x) for x in r) for r in rows]


def scalar_detect(rgba, V, N, t, max_keypoints):
    """(xy, score, desc) as nested lists: the header's conventions, one pixel at a time"""
    h, w = len(rgba), len(rgba[0])

    def known(u, v):
        return 0 <= u < w and 0 <= v < h and rgba[v][u][3] != 0

    def Y(u, v):            # "0 where A = 0.  Pixels outside the image count as Y = 0, A = 0"
        if not known(u, v):
            return 0
        r, g, b, _ = rgba[v][u]
        return (77 * r + 150 * g + 29 * b + 128) >> 8

    luma = [[Y(u, v) for u in range(w)] for v in range(h)]

    def Yat(u, v):
        return luma[v][u] if 0 <= u < w and 0 <= v < h else 0

    def score(u, v):
        if u < 16 or v < 16 or u > w - 17 or v > h - 17:                        # at least 16 pixels from every edge
            return 0
        if not known(u, v) or not all(known(u + dx, v + dy) for dx, dy in H_RING):
            return 0
        if not all(math.isfinite(x) for x in V[v * w + u]) or not all(math.isfinite(x) for x in N[v * w + u]):
            return 0
        c = luma[v][u]
        ring = [luma[v + dy][u + dx] for dx, dy in H_RING]
        corner = False
        for start in range(16):                                                  # nine contiguous, cyclically
            run = [ring[(start + k) % 16] for k in range(9)]
            if all(y > c + t for y in run) or all(y < c - t for y in run):
                corner = True
                break
        return sum(max(abs(y - c) - t, 0) for y in ring) if corner else 0

    sc = [[score(u, v) for u in range(w)] for v in range(h)]

    def at(u, v):
        return sc[v][u] if 0 <= u < w and 0 <= v < h else 0

    survivors = []
    for v in range(h):
        for u in range(w):
            s = sc[v][u]
            if s <= 0:
                continue
            beats = True
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    nb = at(u + dx, v + dy)
                    lower = (v + dy) * w + (u + dx) < v * w + u                    # the neighbour has the lower index: it wins a tie
                    if nb > s or (nb == s and lower):
                        beats = False
            if beats:
                survivors.append((v * w + u, s))
    kept = sorted(sorted(survivors, key=lambda ps: (-ps[1], ps[0]))[:max_keypoints])   # the strongest, then listed in pixel order

    def box(u, v):
        return sum(Yat(u + dx, v + dy) for dy in range(-2, 3) for dx in range(-2, 3))

    pairs = table_pairs()
    xy, scores, desc = [], [], []
    for p, s in kept:
        u, v = p % w, p // w
        words = [0] * 8
        for i, (ax, ay, bx, by) in enumerate(pairs):
            if box(u + ax, v + ay) < box(u + bx, v + by):
                words[i // 32] |= 1 << (i % 32)
        xy.append([u, v]); scores.append(s); desc.append(words)
    return xy, scores, desc, len(survivors)


def hold_to_second_statement(view, t, cap):
    xy, sc, de, n = FE.detect(view.rgba, view.V, view.N, t, cap, with_survivors=True)
    sxy, ssc, sde, sn = scalar_detect(view.rgba.tolist(), view.V.tolist(), view.N.tolist(), t, cap)
    assert n == sn and xy.tolist() == sxy and sc.tolist() == ssc and de.tolist() == sde, (t, cap, n, sn, len(xy), len(sxy))
    return n, len(sxy)


@pytest.mark.parametrize("t,cap", [(1, UNCAPPED), (12, UNCAPPED), (40, UNCAPPED), (12, 1), (12, 50)])
def test_noise_with_holes_against_the_second_statement(t, cap):
    p = E.noise_pair()
    for view in (p.frame, p.model):                     # the frame: NaN normals; the model: those, and alpha = 0 holes
        n, k = hold_to_second_statement(view, t, cap)
        assert n > 100 and k == min(n, cap)
    assert np.isnan(p.frame.N).any() and (p.model_rgba[..., 3] == 0).any()


def test_holed_vertices_against_the_second_statement():
    v = E.noise_pair().frame
    V = v.V.copy()
    V[E.noise_holes()] = np.nan
    n, _ = hold_to_second_statement(FC.View(v.rgba, V, v.N, v.B, v.cam), FE.THRESHOLD, UNCAPPED)
    assert n == E.NOISE_SURVIVORS["holed"]


@pytest.mark.parametrize("size", [(33, 33), (40, 33), (32, 32), (1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_tiny_lattices_against_the_second_statement(size):
    s = E.lattice(size)
    for which in (0, 1):
        n, k = hold_to_second_statement(s.view(which), FE.THRESHOLD, FE.MAX_KEYPOINTS)
        assert n == k == len(E.TINY[size])


def test_second_statement_on_a_lattice_window():
    """a 72 x 56 lattice: 5 x 3 dots that all tie; caps inside the tie class keep the first in pixel order in both statements"""
    s = E.lattice((72, 56))
    for cap in (1, 7, 15, 16):
        n, k = hold_to_second_statement(s.view(0), 1, cap)
        assert n == 15 and k == min(cap, 15)
