"""CPU: the robust volume terms as tests/sdf_robust_oracle.py states them.  The two weights at their edges, the weighted record as the
sum of its rows, every figure of tests/sdf_robust_cases.py recomputed -- the intruder frames on the window, with colour and on the map
-- with the conditions on the cases, and the build surface: the entry points and the header's block, the resources and the kernarg
layouts of the four new round kernels, the hook, the untouched siblings, the C++ example."""
import os
import re
import subprocess

import numpy as np
import pytest

import isa_tools as T
import sdf_cases as SC
import sdf_oracle as SO
import sdf_photo_oracle as SP
import sdf_robust_cases as RC
import sdf_robust_oracle as RO
import unit_gates as UG
import volume_cases as VC
from frontend_util import SMALL_CAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENTRY_POINTS = {"rpe_sdf_set_robust", "rpe_sdf_robust", "rpe_sdf_robust_weights", "rpe_map_sdf_robust_weights"}
ROUND_KERNELS = {"icp_sdf_robust_kernel": 4, "icp_map_sdf_robust_kernel": 4, "icp_sdf_photo_robust_kernel": 8,
                 "icp_map_sdf_photo_robust_kernel": 8}                       # kinds x (with the geometric row) x workgroup sizes
SIBLINGS = {"icp_sdf_kernel": 2, "icp_sdf_photo_kernel": 4, "icp_map_sdf_kernel": 2, "icp_map_sdf_photo_kernel": 4, "sdf_rows_kernel": 1,
            "map_sdf_rows_kernel": 1, "sdf_photo_rows_kernel": 1, "map_sdf_photo_rows_kernel": 1}


# ---------------------------------------------------------------------------------------------- the rule
def test_huber_is_one_up_to_the_scale_and_k_over_s_beyond():
    k = F(0.01)
    up, down = np.nextafter(k, F(1)), np.nextafter(k, F(0))
    r = np.array([0, down, k, -k, up, -up, 0.08, -0.08, np.inf, np.nan], F)
    w = RO.huber(r, k)
    assert w.dtype == F and (w[:4] == 1).all()                                # s <= k: the edge itself has weight 1
    assert w[4] == k / up and w[4] < 1 and w[5] == w[4]
    assert w[6] == F(0.01) / F(0.08) and w[7] == w[6] and w[8] == 0 and np.isnan(w[9])


def test_tukey_is_exactly_zero_from_the_scale_on():
    k = F(0.05)
    up, down = np.nextafter(k, F(1)), np.nextafter(k, F(0))
    r = np.array([0, 0.025, -0.025, down, k, -k, up, 0.08, np.inf, np.nan], F)
    w = RO.tukey(r, k)
    assert w.dtype == F and w[0] == 1
    u = F(0.025) / k
    q = F(1.0) - u * u
    assert w[1] == q * q and w[2] == w[1] and 0 < w[3] < 1e-12               # fabsf(r) < k: just inside is tiny, not zero
    # (a NaN residual fails fabsf(r) < k: 0 by the rule itself; the plane's NaN is "no row", test_the_plane_of_weights_...)
    assert (w[4:] == 0).all() and not np.signbit(w[4:]).any()


def test_the_plane_of_weights_has_nan_where_there_is_no_row():
    r = np.array([0.0, np.nan, 0.03, -0.2], F)
    assert np.array_equal(RO.weights(RO.NONE, r, 0.0), np.array([1, np.nan, 1, 1], F), equal_nan=True)
    assert np.array_equal(RO.weights(RO.TUKEY, r, 0.0), np.array([1, np.nan, 1, 1], F), equal_nan=True)      # photo_k = 0
    assert np.array_equal(RO.weights(RO.HUBER, r, 0.1), np.array([1, np.nan, 1, 0.5], F), equal_nan=True)
    assert np.array_equal(RO.weights(RO.TUKEY, r, 0.1)[[0, 1, 3]], np.array([1, np.nan, 0], F), equal_nan=True)


def room_rows():
    dims, desc, G, vol = SC.room_volume(SMALL_CAM)
    _, V, N, _ = SC.frame_pyramid(SC.RAGGED_CAM)[1]
    return SO.rows(vol, G, V, N, SC.poses()[1], 0.15, SC.COS_THR, True)


def test_the_weighted_record_is_the_sum_of_the_weighted_rows():
    r, J, ok = room_rows()
    w = RO.weights(RO.TUKEY, r, 0.02)
    assert ((w[ok] == 0).sum() > 100) and ((w[ok] > 0).sum() > 100)
    rec, S = RO.record(r, J, ok, w)
    Jd, rd, wd = J[ok].astype(np.float64), r[ok].astype(np.float64), w[ok].astype(np.float64)
    H = (Jd * wd[:, None]).T @ Jd
    assert np.allclose(rec[:21], H[np.triu_indices(6)], rtol=1e-12) and np.allclose(rec[21:27], (Jd * wd[:, None]).T @ rd, rtol=1e-9, atol=1e-12)
    assert rec[27] == pytest.approx((wd * rd * rd).sum(), rel=1e-12)
    assert rec[28] == ok.sum()                                                # every row that passed the gates, weight 0 included
    assert (S[:28] >= np.abs(rec[:28])).all()


def test_weight_one_is_the_unweighted_record():
    r, J, ok = room_rows()
    one = RO.weights(RO.NONE, r, 0.0)
    a, Sa = RO.record(r, J, ok, one)
    b, Sb = SO.record(r, J, ok)
    assert np.array_equal(a, b) and np.array_equal(Sa, Sb)
    big = RO.weights(RO.HUBER, r, 1.0)                                        # k above the gate: every weight 1
    assert np.array_equal(big, one, equal_nan=True)
    a, Sa = RO.record(r, J, ok, one, 0.01)
    b, Sb = SP.record(r, J, ok, 0.01)
    assert np.array_equal(a, b) and np.array_equal(Sa, Sb)


# ---------------------------------------------------------------------------------------------- the figures of sdf_robust_cases
@pytest.fixture(scope="module")
def window_figures(oracle):
    return {f: {s: RC.oracle_window(oracle, f, s) for s in RC.SETTINGS} for f in RC.FRAMES}


def test_the_window_cases_figures(window_figures):
    start = VC.pose_error(RC.window_start(), RC.window_truth())
    assert start == pytest.approx((1.08e-2, 5.4e-2), rel=0.02)
    rs, cs = RC.patch_slices(RC.WINDOW_CAM, RC.PATCH)
    assert (rs, cs) == (slice(30, 100), slice(20, 80))
    rs, cs = RC.patch_slices(RC.WINDOW_CAM, RC.SMALL_PATCH)
    assert (rs.stop - rs.start, cs.stop - cs.start) == (40, 40)
    for f in RC.FRAMES:
        for s in RC.SETTINGS:
            got, want = window_figures[f][s], RC.WINDOW_ORACLE[f][s]
            print(f, "|", s, "|", "%.3g mrad / %.3g mm" % (1e3 * got[0], 1e3 * got[1]), "recorded", want)
            assert got[0] == pytest.approx(want[0], rel=0.02) and got[1] == pytest.approx(want[1], rel=0.02), (f, s, got, want)
    assert RC.WINDOW_ORACLE["clean"]["none"] == SC.CONVERGE_ORACLE["160"]    # the unweighted loop on the clean frame is sdf_cases'


def test_tukey_returns_the_tracker_to_the_clean_frames_error(window_figures):
    """THE CONDITIONS ON THE CASE, on the 8 cm / 22 % intruder: Tukey k = 50 mm ends within 2 x the clean frame's unweighted error, and
    the unweighted loop ends at least 4 x further off than Tukey"""
    clean, plain, tukey = window_figures["clean"]["none"], window_figures["intruder 8 cm"]["none"], window_figures["intruder 8 cm"]["tukey 50 mm"]
    print("clean", clean, "intruder: unweighted", plain, "tukey 50 mm", tukey, "ratios", tukey[0] / clean[0], tukey[1] / clean[1],
          plain[0] / tukey[0], plain[1] / tukey[1])
    assert tukey[0] <= 2 * clean[0] and tukey[1] <= 2 * clean[1]
    assert plain[0] >= 4 * tukey[0] and plain[1] >= 4 * tukey[1]


@pytest.mark.parametrize("which", ["colour", "map"])
def test_the_colour_and_map_cases_figures(oracle, which):
    """with colour the direction shows by far more than 2 x only with BOTH weights: the weight on the geometric rows alone does not pay on
    a wall (it ends further off than the unweighted loop), which the cases file and the README say in capitals"""
    run, table = (RC.oracle_colour, RC.COLOUR_ORACLE) if which == "colour" else (RC.oracle_map, RC.MAP_ORACLE)
    got = {i: {s: run(oracle, i, s) for s in RC.COLOUR_SETTINGS} for i in (False, True)}
    for i in (False, True):
        for s in RC.COLOUR_SETTINGS:
            print(which, "intruder" if i else "clean", "|", s, "|", got[i][s], "recorded", table[i][s])
            rel = 0.02 if got[i][s][1] < 0.1 else 0.2          # (a loop that has lost the frame ends anywhere: its figure says "lost")
            assert got[i][s][0] == pytest.approx(table[i][s][0], rel=rel) and got[i][s][1] == pytest.approx(table[i][s][1], rel=rel), (i, s)
    both, plain, geo_only = got[True]["tukey 50 mm, 25 levels"], got[True]["none"], got[True]["tukey 50 mm"]
    assert plain[0] >= 2 * both[0] and plain[1] >= 2 * both[1]                # the direction, by at least 2 x
    assert geo_only[1] > plain[1]                                             # DOES NOT PAY without photo_k
    assert got[True]["huber 10 mm, 5 levels"][1] <= 0.5 * plain[1]
    for s in RC.COLOUR_SETTINGS:                                              # on the clean frame no setting costs anything
        assert got[False][s][1] <= 1.05 * got[False]["none"][1]


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    at = hdr.index("---- Robust volume terms:")
    assert at > hdr.index("---- Map volume colour term:")
    block = " ".join(hdr[at:hdr.index("int rpe_sdf_set_robust(")].replace("\n *", " ").split())
    for what in ("OFF by default", "s = fabsf(r); w = s <= k ? 1.0f : k / s", "u = r / k; q = 1.0f - u * u; w = fabsf(r) < k ? q * q : 0.0f",
                 "weight 0 included", "photo_k = 0 leaves the photometric rows at weight 1", "RPE_ERR_DEGENERATE", "the same bits",
                 "No confidence weighting", "No scale estimation", "No Cauchy", "stay unweighted"):
        assert what in block, what
    assert "RPE_ROBUST_TUKEY = 3" in hdr and "RPE_ROBUST_CAUCHY = 2" in hdr
    for name in ("Volume term", "Volume colour term", "Map volume term", "Map volume colour term"):     # the caveat stays where it was
        assert "not weighted by voxel weight" in " ".join(hdr[hdr.index("---- %s:" % name):].split("/* ----")[0].split())
    from rgbd_pose_estimation_amd import _lib as L
    assert (L.ROBUST_NONE, L.ROBUST_HUBER, L.ROBUST_TUKEY) == (RO.NONE, RO.HUBER, RO.TUKEY) == (0, 1, 3)
    src = open(os.path.join(UG.CSRC, "rpe_map_sdf_photo.hpp")).read()          # the end of the chain of headers rpe_frontend.hip compiles
    assert src.rstrip().endswith('#include "rpe_sdf_robust.hpp"')            # behind every kernel it shares with: no new compile unit
    from rgbd_pose_estimation_amd import build as B
    assert "rpe_sdf_robust.hpp" not in B.SOURCES and "rpe_sdf_api.hip" in B.SOURCES
    text = open(os.path.join(UG.CSRC, "rpe_sdf_robust.hpp")).read()
    assert text.count("RPE_PRELOAD(") == 5                                    # one node per new kernel
    assert "huber_weight" not in text and "tukey_weight" not in text          # the rule is stated once, in its own header
    assert not any(old in new for new in list(ROUND_KERNELS) + ["sdf_robust_weights_kernel"] for old in SIBLINGS)


def frontend_kernels():
    UG.built()
    rows = {}
    for r in T.kernel_resources(UG.obj("rpe_frontend.hip")):
        rows.setdefault(r["base"], []).append(r)
    return rows


def test_the_new_kernels_are_in_their_siblings_class():
    """no scratch, no vector or scalar spill, and the waves-per-SIMD class of the sibling: at most 128 registers (four waves), and at
    most 256 (two) for the map's combined colour round, whose sibling takes 142"""
    rows = frontend_kernels()
    for base, count in ROUND_KERNELS.items():
        assert len(rows.get(base, [])) == count, (base, sorted(rows))
        for r in rows[base]:
            print(base, r["mangled"][-70:], r["vgpr"], r["lds"])
            assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, r
            two_waves = base == "icp_map_sdf_photo_robust_kernel" and re.search(r"robust_kernelILi\dELb1E", r["mangled"])
            assert r["vgpr"] <= (256 if two_waves else 128), r
    assert sum(bool(re.search(r"robust_kernelILi\dELb1E", r["mangled"])) for r in rows["icp_map_sdf_photo_robust_kernel"]) == 4
    assert len(rows.get("sdf_robust_weights_kernel", [])) == 4
    for r in rows["sdf_robust_weights_kernel"]:
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 128, r


def test_the_siblings_are_what_they_were():
    """the twelve existing kernels of the volume terms keep their instances and registers (DESIGN.md section 4 has the comparison of
    their instructions with the parent's)"""
    rows = frontend_kernels()
    for base, count in SIBLINGS.items():
        assert len(rows.get(base, [])) == count, (base, sorted(rows))
    assert [r["vgpr"] for r in rows["icp_sdf_kernel"]] == [128, 128] and [r["vgpr"] for r in rows["icp_map_sdf_kernel"]] == [120, 120]
    assert sorted(r["vgpr"] for r in rows["icp_sdf_photo_kernel"]) == [110, 110, 124, 124]
    assert sorted(r["vgpr"] for r in rows["icp_map_sdf_photo_kernel"]) == [127, 127, 142, 142]


def kernarg_layouts(tmp_path, name):
    co = T.code_object(UG.obj("rpe_frontend.hip"), str(tmp_path))
    notes = subprocess.check_output([T.READELF, "--notes", co]).decode()
    out = []
    for m in re.finditer(r"\.name:\s+(\S*%s\S*)\n" % name, notes):
        if m.group(1).endswith(".kd"):
            continue
        args = notes[notes.rfind(".args:", 0, m.start()):m.start()]
        out.append([(int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)", args)])
    return out


LAYOUTS = {
    "icp_sdf_robust_kernel": [(0, 8), (8, 8), (16, 8), (24, 8), (32, 36), (68, 16), (84, 4), (88, 48), (136, 136)],
    "icp_map_sdf_robust_kernel": [(0, 8), (8, 8), (16, 8), (24, 64), (88, 36), (124, 16), (140, 4), (144, 48), (192, 136)],
    "icp_sdf_photo_robust_kernel": [(0, 8), (8, 8), (16, 8), (24, 8), (32, 8), (40, 8), (48, 36), (84, 16), (100, 4), (104, 8), (112, 48),
                                    (160, 136)],
    "icp_map_sdf_photo_robust_kernel": [(0, 8), (8, 8), (16, 8), (24, 8), (32, 80), (112, 36), (148, 16), (164, 4), (168, 8), (176, 48),
                                        (224, 136)],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_round_kernels_find_their_late_arguments_in_the_kernarg_segment(tmp_path, name):
    """the new kernels read the reduction's argument -- and, but for the window's geometric one, the pose; the map's colour round the view
    too -- from the kernarg segment at the offsets of structs that mirror their argument lists (rpe_sdf_robust.hpp): the code object's
    metadata must hold the arguments exactly there, the scales between gates and pose"""
    UG.built()
    layouts = kernarg_layouts(tmp_path, name)
    assert len(layouts) == ROUND_KERNELS[name]
    for layout in layouts:
        assert layout[:len(LAYOUTS[name])] == LAYOUTS[name], layout
    src = open(os.path.join(UG.CSRC, "rpe_sdf_robust.hpp")).read()
    for claim in ("offsetof(SdfRobustRoundArgs, fin) == 136", "offsetof(MapSdfRobustRoundArgs, fin) == 192", "offsetof(MapSdfRobustRoundArgs, T) == 144",
                  "offsetof(SdfPhotoRobustRoundArgs, fin) == 160", "offsetof(SdfPhotoRobustRoundArgs, T) == 112",
                  "offsetof(MapSdfPhotoRobustRoundArgs, fin) == 224", "offsetof(MapSdfPhotoRobustRoundArgs, T) == 176",
                  "offsetof(MapSdfPhotoRobustRoundArgs, P) == 32"):
        assert claim in src, claim


def test_the_documents_have_the_row():
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = [ln for ln in readme.splitlines() if "rpe_sdf_set_robust" in ln and ln.lstrip().startswith("|")]
    assert len(row) == 1, len(row)
    for what in ("RPE_ROBUST_TUKEY", "DOES NOT PAY", "No confidence weighting", "no scale estimation", "no Cauchy", "unweighted",
                 "profiles/sdf_robust_time_640.json"):
        assert what in row[0], what
    assert "not weighted by voxel weight" in readme                           # the caveat stays
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "icp_map_sdf_photo_robust_kernel" in design and "profiles/sdf_robust_isa_diff.txt" in design
    assert os.path.exists(os.path.join(ROOT, "profiles", "sdf_robust_isa_diff.txt"))
    assert "sdf_set_robust" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_volume_sdf_robust_track_cpp_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_sdf_robust_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_sdf_robust_track")])
