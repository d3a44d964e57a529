"""CPU: the keyframe-graph oracle (tests/graph_oracle.py) on the drifted rooms of tests/graph_cases.py -- its recorded figures
recomputed, every keyframe's end error within keyframe_cases.RELOC_BOUND from a start far outside it -- and the library's dense solve
(rpe_graph_solve, host code: no GPU) against numpy.linalg.solve on the oracle's records."""
import numpy as np
import pytest

import graph_cases as GC
import graph_oracle as GO
import keyframe_cases as KC
from rgbd_pose_estimation_amd import _lib as L, api


@pytest.mark.parametrize("cam", ["small", "half"])
def test_the_oracles_figures_and_the_end_error(cam):
    c, fig = GC.case(cam), GC.FIGURES[cam]
    assert (len(c.edges), sum(len(e[2]) for e in c.edges)) == (fig["edges"], fig["pairs"])
    assert all(e[0] > e[1] and len(e[2]) >= GC.MIN_MATCHES for e in c.edges)
    assert [(e[0], e[1]) for e in c.edges] == sorted((e[0], e[1]) for e in c.edges)
    start = c.errors(c.poses0)
    worst = (max(e[0] for e in start), max(e[1] for e in start))
    assert worst == pytest.approx(fig["start"], rel=5e-3)
    assert worst[0] > 10 * KC.RELOC_BOUND[0] and worst[1] > 4 * KC.RELOC_BOUND[1]           # the drifted start is outside the bound
    assert sum(e[0] > KC.RELOC_BOUND[0] or e[1] > KC.RELOC_BOUND[1] for e in start) >= 6
    poses, stats = c.loop
    assert len(stats) == len(GC.GATES)
    assert all(abs(s[0] - p) <= 2 for s, p in zip(stats, fig["round_pairs"])), [s[0] for s in stats]
    end = c.errors(poses)
    print(cam, "end", end)
    for k, (e, f) in enumerate(zip(end, fig["end"])):
        assert e[0] < KC.RELOC_BOUND[0] and e[1] < KC.RELOC_BOUND[1], (k, e)
        assert e[0] == pytest.approx(f[0], rel=2e-2, abs=1e-9) and e[1] == pytest.approx(f[1], rel=2e-2, abs=1e-9), (k, e, f)
    assert np.array_equal(poses[GC.ANCHOR], c.poses0[GC.ANCHOR])


def test_wrong_edges_are_there_and_the_gate_drops_them():
    c = GC.case("small")
    frac = [GC.correct_fraction(c, e) for e in c.edges]
    bad = [f for f in frac if f <= 0.14]
    assert len(bad) == 7 and min(f for f in frac if f > 0.14) >= 0.5
    rec, _ = GO.records(c.keyframes, c.edges, c.loop[0], c.poses0, GC.GATES[-1])
    counted = rec[:, 0] / np.array([len(e[2]) for e in c.edges])
    assert all(x <= 0.2 for x, f in zip(counted, frac) if f <= 0.14) and all(x >= 0.4 for x, f in zip(counted, frac) if f >= 0.5)


def test_records_are_the_direct_sums_of_the_issues_jacobians():
    """graph_oracle.record goes the kernel's way (38 world-frame sums, then a congruence per block).  Here the same record is built
    the plain way, pair by pair, from the Jacobians as the issue states them -- dX_k/d upsilon = -R_k^T, dX_k/d omega = R_k^T [p]x,
    p = R_k X_k + t_k, the residual's row by keyframe i with the other sign -- and from a central difference of X_k under
    exp(delta) T_k, so that the reference does not share its derivation with the implementation"""
    c = GC.case("small")
    poses = [PCmoved(p, k) for k, p in enumerate(c.poses0)]
    corr = GO.corrections(poses, c.poses0)
    for e in (c.edges[0], c.edges[7], c.edges[-1]):
        j, i = e[0], e[1]
        X, Y, r, ok = GO.pair_rows(c.keyframes, e, corr, 10.0)             # a wide gate: every pair counts, wrong matches included
        assert ok.sum() == len(e[2]) >= 12
        w, _ = GO.raw_sums(X, Y, r, ok)
        rec = GO.record(w, poses[j], poses[i])
        H, g = np.zeros((12, 12)), np.zeros(12)
        for x, y, res in zip(X[ok].astype(np.float64), Y[ok].astype(np.float64), r[ok].astype(np.float64)):
            J = np.zeros((3, 12))
            for col, (p, pt, sign) in enumerate(((poses[j], x, 1.0), (poses[i], y, -1.0))):
                R, t = p[:9].reshape(3, 3), p[9:]
                J[:, 6 * col:6 * col + 3] = sign * -R.T
                J[:, 6 * col + 3:6 * col + 6] = sign * R.T @ GO.skew(R @ pt + t)
            H += J.T @ J
            g += J.T @ res
        gj, gi, Hjj, Hii, Hji = GO.unpack(rec)
        scale = np.abs(H).max()
        assert np.abs(np.concatenate([gj, gi]) - g).max() <= 1e-12 * np.abs(g).max() + 1e-13 * scale
        assert np.abs(Hjj - H[:6, :6]).max() <= 1e-12 * scale and np.abs(Hii - H[6:, 6:]).max() <= 1e-12 * scale
        assert np.abs(Hji - H[:6, 6:]).max() <= 1e-12 * scale
        assert rec[0] == ok.sum() and abs(rec[1] - (r[ok].astype(np.float64) ** 2).sum()) <= 1e-12 * rec[1]
    # the Jacobian itself against a central difference of X_k(x) = R^T (R0 x + t0 - t) under T <- exp(delta) T
    p0, p = c.poses0[3], poses[3]
    x = c.keyframes[3]["xw"][5].astype(np.float64)
    cam = p0[:9].reshape(3, 3) @ x + p0[9:]

    def world(q):
        return q[:9].reshape(3, 3).T @ (cam - q[9:])

    R, t = p[:9].reshape(3, 3), p[9:]
    J = np.concatenate([-R.T, R.T @ GO.skew(R @ world(p) + t)], 1)
    for k in range(6):
        d = np.zeros(6)
        d[k] = 1e-6
        num = (world(GO.left_update(d, p)) - world(GO.left_update(-d, p))) / 2e-6
        assert np.abs(num - J[:, k]).max() < 1e-8, k


def PCmoved(p, k):
    import photo_cases as PC
    return PC.moved(np.asarray(p), 0.004 * (k % 3 - 1), -0.003, 0.006, 0.012, 0.009 * (k % 2), -0.007)


def check_solve(K, ji, rec, fixed):
    want = GO.solve(K, ji, rec, fixed)
    got = api.graph_solve(K, ji, rec, fixed)
    assert want is not None
    scale = max(1e-12, np.abs(want).max())
    assert np.abs(got - want).max() <= 1e-9 * scale, np.abs(got - want).max() / scale
    assert not got[np.asarray(fixed, bool)].any()
    return got


def records_of(c, ids, anchor):
    """the records of the sub-graph over the keyframes `ids` (renumbered) at the drifted poses, first gate"""
    ids = list(ids)
    pos = {k: n for n, k in enumerate(ids)}
    kfs, poses = [c.keyframes[k] for k in ids], [c.poses0[k] for k in ids]
    edges = [(pos[j], pos[i], a, b) for j, i, a, b in c.edges if j in pos and i in pos]
    rec, _ = GO.records(kfs, edges, poses, poses, GC.GATES[0])
    ji = [(e[0], e[1]) for e in edges]
    return len(ids), ji, rec, GO.fixed_set(len(ids), ji, rec, anchor)


def test_graph_solve_two_keyframes():
    K, ji, rec, fixed = records_of(GC.case("small"), (0, 1), 0)
    assert fixed.tolist() == [True, False] and len(ji) == 1
    d = check_solve(K, ji, rec, fixed)
    assert np.abs(d[1]).max() > 1e-3


def test_graph_solve_eight_keyframes_anchor_three():
    K, ji, rec, fixed = records_of(GC.case("small"), range(8), 3)
    assert np.flatnonzero(fixed).tolist() == [3]
    check_solve(K, ji, rec, fixed)


def test_graph_solve_two_components_and_an_isolated_keyframe():
    c = GC.case("small")
    K, ji, rec, _ = records_of(c, range(8), 0)
    keep = [n for n, (j, i) in enumerate(ji) if {j, i} <= {0, 1, 3} or {j, i} <= {2, 5}]          # {0, 1, 3}, {2, 5}; 4, 6, 7 alone
    ji, rec = [ji[n] for n in keep], rec[keep]
    fixed = GO.fixed_set(K, ji, rec, 1)
    assert np.flatnonzero(fixed).tolist() == [1, 2, 4, 6, 7]
    d = check_solve(K, ji, rec, fixed)
    assert d[0].any() and d[3].any() and d[5].any() and not d[[4, 6, 7]].any()
    # an isolated keyframe that is NOT marked fixed has no equation and keeps delta = 0
    fixed[7] = False
    assert not check_solve(K, ji, rec, fixed)[7].any()


def test_graph_solve_refuses_a_rank_deficient_edge():
    """three collinear pairs: the rotation about their line is not determined"""
    line = np.array([[0.2, 0.1, 2.0], [0.4, 0.2, 2.5], [0.8, 0.4, 3.5]], np.float32)
    kfs = [dict(xw=line), dict(xw=line + np.float32(0.001))]
    poses = [GC.IDENTITY, GC.IDENTITY]
    edges = [(1, 0, np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32))]
    rec, _ = GO.records(kfs, edges, poses, poses, 0.1)
    assert rec[0, 0] == 3
    assert GO.solve(2, [(1, 0)], rec, [True, False]) is None
    with pytest.raises(L.RpeError) as ei:
        api.graph_solve(2, [(1, 0)], rec, [0])
    assert ei.value.code == L.RPE_ERR_DEGENERATE


def test_the_fp32_rows_are_not_fused():
    """the rows' operation order rounds every product and sum on its own (tests/graph_oracle.py rotate / transform): no kernel of the
    unit may hold an fp32 multiply-add -- the fp64 sums behind the rows may fuse, a product of two fp32 numbers is exact there"""
    import os
    import isa_tools as T
    from rgbd_pose_estimation_amd import build as B
    obj = os.path.join(os.path.dirname(B.LIB), "rpe_graph.o")
    if not os.path.exists(obj):
        B.build()
    fused = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_fma_mix", "v_mad_f32", "v_mac_f32", "v_fma_legacy", "v_dot2")
    kernels = T.disassemble(obj)
    assert len(kernels) == 4
    for name, body in kernels.items():
        assert not [i.text for i in body if i.text.startswith(fused)], name
    rows = [b for n, b in kernels.items() if "graph_rows_kernel" in n][0]
    assert sum(i.text.startswith(("v_mul_f32", "v_pk_mul_f32")) for i in rows) >= 12       # the products are there, on their own


def test_graph_cpp_driver_compiles(tmp_path):
    import os
    import subprocess
    from rgbd_pose_estimation_amd import build as B
    lib = B.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(root, "tests", "cpp", "graph_optimize.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "graph_optimize")])


def test_graph_solve_under_asan_ubsan(tmp_path):
    """tests/cpp/graph_solve_host.cpp compiled together with csrc/library.cpp (the host side) with the sanitizers, as
    tests/test_sanitizers_cpu.py builds its programs; no GPU call is made"""
    import os
    import subprocess
    from rgbd_pose_estimation_amd import build as B
    lib = B.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "rgbd_pose_estimation_amd", "include")
    exe = str(tmp_path / "graph_solve_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(root, "tests", "cpp", "graph_solve_host.cpp"),
                           os.path.join(root, "rgbd_pose_estimation_amd", "csrc", "library.cpp"),
                           "-L", os.path.dirname(lib), "-lrgbdpose_hip", "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "graph_solve_host: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_graph_solve_argument_errors():
    rec = np.zeros((1, L.GRAPH_RECORD))
    for ji in ([(2, 0)], [(1, 1)], [(-1, 0)]):
        with pytest.raises(L.RpeError) as ei:
            api.graph_solve(2, ji, rec)
        assert ei.value.code == L.RPE_ERR_ARG
    assert not api.graph_solve(3, np.zeros((0, 2), np.int32), np.zeros((0, L.GRAPH_RECORD))).any()    # no edge: nothing moves
