"""GPU parity of the keyframe graph (csrc/rpe_graph.hip, rpe_graph_api.hip, rpe_keyframes_link) against tests/graph_oracle.py: the
edges and pair lists BIT FOR BIT on every case (all-pairs, incremental, cross-check, ties, empty and one-keypoint keyframes), the fp32
rows bit for bit, the records within the rounding bound derived from the kernel's reduction, host edges of every block shape in one
graph, the optimisation held to the oracle loop, the apply step bit for bit and what relocalisation answers before and after it."""
import os
import subprocess

import numpy as np
import pytest

import feature_cases as FC
import graph_cases as GC
import graph_oracle as GO
import keyframe_cases as KC
import keyframe_oracle as KO
import photo_cases as PC
import util
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RELOC = dict(iters=FC.RELOC_ITERS, confidence=FC.RELOC_CONF, seed=FC.RELOC_SEED, **FC.RELOC_THRE)
SOLVER = dict(method=api.M_SK_PROSAC, ls=api.LS_SHINJI_INLIERS)
U = 2.0 ** -53


def same(a, b):
    """bit for bit, every NaN where the other has one"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32))


def close(p, q, tol=1e-6):
    return util.rot_err(p[:9].reshape(3, 3), q[:9].reshape(3, 3)) < tol and np.linalg.norm(p[9:] - q[9:]) < tol


def kw(mopt):
    return dict(max_dist=mopt[0], ratio=(mopt[1], mopt[2]), cross_check=mopt[3])


def code_of(fn, *a, **kwargs):
    try:
        fn(*a, **kwargs)
    except L.RpeError as e:
        return e.code
    return L.RPE_OK


def add_host(ctx, k, pose=GC.IDENTITY, w=160, h=120):
    return ctx.keyframe_add_host(k["xy"], k["desc"], k["xw"], k["nw"], pose, w, h)


def graph_of(ctx):
    return [(int(j), int(i), *ctx.graph_edge(e)) for e, (j, i, _) in enumerate(ctx.graph_edges())]


def check_graph(ctx, want):
    jic = ctx.graph_edges()
    assert [tuple(r) for r in jic.tolist()] == [(e[0], e[1], len(e[2])) for e in want]
    assert ctx.graph_info() == (len(want), sum(len(e[2]) for e in want))
    for got, e in zip(graph_of(ctx), want):
        assert np.array_equal(got[2], e[2]) and np.array_equal(got[3], e[3]), (e[0], e[1])


def put_edges(ctx, edges):
    for j, i, a, b in edges:
        ctx.graph_add_edge(j, i, a, b)


# ---------------------------------------------------------------------------------------------- links
def test_link_all_pairs_is_the_oracles_graph(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    c.fill(ctx)
    assert ctx.keyframes_link() == (GC.FIGURES["small"]["edges"], GC.FIGURES["small"]["pairs"])
    check_graph(ctx, c.edges)
    for mopt, mm in (((64, 8, 10, True), 12), ((256, 8, 10, False), 3), ((256, 8, 10, True), 40)):
        want = GO.link(c.keyframes, 0, mopt, mm)
        assert ctx.keyframes_link(0, mm, **kw(mopt))[0] == len(want) > 0
        check_graph(ctx, want)
    assert sum(len(e[2]) for e in GO.link(c.keyframes, 0, (64, 8, 10, True))) < GC.FIGURES["small"]["pairs"]   # the cross-check removes something


def test_link_keyframe_by_keyframe_gives_the_same_graph(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    for n in range(len(c.keyframes)):
        kid = c.fill(ctx, c.keyframes[n:n + 1], c.poses0[n:n + 1])[0]
        assert kid == n
        ctx.keyframes_link(first=kid)
        check_graph(ctx, [e for e in c.edges if e[0] <= n])
    # the tail rebuilt with other options, the older edges stay
    want = GO.link(c.keyframes, 5, (64, 8, 10, True), 12, c.edges)
    ctx.keyframes_link(5, cross_check=True)
    check_graph(ctx, want)
    assert ctx.keyframes_link(first=8) == (len([e for e in want if e[0] < 8]), sum(len(e[2]) for e in want))   # first = K: nothing to do
    ctx.keyframes_link()
    check_graph(ctx, c.edges)


def test_link_ties_of_a_repeated_texture(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    _, kfs, _ = KC.tiled_store()
    for k in kfs:
        add_host(ctx, k)
    for mopt in ((256, 2, 1, False), (256, 2, 1, True)):
        want = GO.link(kfs, 0, mopt, 12)
        ctx.keyframes_link(0, 12, **kw(mopt))
        check_graph(ctx, want)
        assert len(want) == 3
    a, b, d1, d2 = GO.FE.match(kfs[1]["desc"], kfs[0]["desc"], 256, 2, 1, False)
    assert (d1 == d2).any() and len(a) >= 12                                           # ties among the accepted pairs: ratio 2 / 1 lets them through


def test_link_with_empty_and_one_keypoint_keyframes(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    r = KC.room("small")
    kfs = [KC.tiny_keyframe(0, 0), r.keyframes[0], KC.tiny_keyframe(2, 1), KC.tiny_keyframe(3, 0), r.keyframes[1], KC.tiny_keyframe(5, 1),
           KC.tiny_keyframe(6, 5)]
    kfs[5]["desc"][0] = r.keyframes[1]["desc"][7]
    for k in kfs:
        add_host(ctx, k)
    for mopt, mm in (((256, 8, 10, False), 3), ((256, 8, 10, True), 3), (KO.MOPT, 3), ((256, 65536, 1, False), 5)):
        want = GO.link(kfs, 0, mopt, mm)
        ctx.keyframes_link(0, mm, **kw(mopt))
        check_graph(ctx, want)
    want = GO.link(kfs, 0, (256, 8, 10, False), 3)
    assert any(e[:2] == (4, 2) and len(e[2]) == len(kfs[4]["xy"]) for e in want)      # against ONE keypoint d2 = 257: everything passes
    assert not any(e[0] in (0, 3) or e[1] in (0, 3) for e in want)                    # an empty keyframe has no edge


def test_no_edges_is_a_state_error_for_the_optimiser(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    assert code_of(ctx.keyframes_link) == L.RPE_ERR_STATE                             # an empty store
    c.fill(ctx, upto=1)
    assert ctx.keyframes_link() == (0, 0) and len(ctx.graph_edges()) == 0            # K = 1
    assert code_of(ctx.keyframes_optimize, GC.GATES) == L.RPE_ERR_STATE
    assert code_of(ctx.graph_residuals) == L.RPE_ERR_STATE and code_of(ctx.graph_normal_eq) == L.RPE_ERR_STATE
    ctx.keyframes_clear()
    c.fill(ctx)
    most = max(len(e[2]) for e in GO.link(c.keyframes, 0, KO.MOPT, 3))
    assert ctx.keyframes_link(min_matches=most + 1) == (0, 0)
    assert code_of(ctx.keyframes_optimize, GC.GATES) == L.RPE_ERR_STATE
    assert ctx.keyframes_link(min_matches=most)[0] == 1
    ctx.keyframes_clear()                                                             # the graph goes with the store
    assert ctx.graph_info() == (0, 0)


# ---------------------------------------------------------------------------------------------- rows and records
def offset_poses(poses):
    return [PC.moved(np.asarray(p), 0.004 * (k % 3 - 1), -0.003, 0.006, 0.012, 0.009 * (k % 2), -0.007) for k, p in enumerate(poses)]


def test_rows_are_bit_exact(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    c.fill(ctx)
    ctx.keyframes_link()
    for poses in (None, c.truth, offset_poses(c.poses0)):
        for gate in (0.1, 0.03):
            want = GO.residuals(c.keyframes, c.edges, c.poses0 if poses is None else poses, c.poses0, gate)
            got = ctx.graph_residuals(poses, gate)
            assert same(got, want), (gate, np.isnan(got).sum(), np.isnan(want).sum())
            assert 0 < np.isnan(want[:, 0]).sum() < len(want)
    at_truth = GO.residuals(c.keyframes, c.edges, c.truth, c.poses0, 0.03)
    assert np.isfinite(at_truth[:, 0]).sum() > 1.1 * np.isfinite(GO.residuals(c.keyframes, c.edges, c.poses0, c.poses0, 0.03)[:, 0]).sum()


def check_records(got, rec, mag, what=""):
    """counts equal, every entry within 2^-46 x the image of the sums of magnitudes; returns the worst ratio"""
    assert np.array_equal(got[:, 0], rec[:, 0]), what
    err = np.abs(got - rec)
    bound = 128 * U * mag
    assert (err <= bound).all(), (what, (err / np.maximum(bound, 1e-300)).max())
    return float((err[mag > 0] / (U * mag[mag > 0])).max()) if (mag > 0).any() else 0.0


@pytest.mark.parametrize("cam", ["small", "half"])
def test_records_within_the_rounding_bound(gpu_ctx_factory, cam):
    """Pair counts equal; every entry within 128 * 2^-53 * S of the oracle's record, S the image of the sums of the products' magnitudes
    under the record's map with every coefficient's absolute value (graph_oracle.record(magnitude=True)).  Derived from the code
    (rpe_graph.hip graph_round_kernel, rpe_graph_api.hip graph_record): behind the fp32 rows X, Y, r every term is formed in fp64 --
    a product of two fp32 numbers is exact there, a cross-product term is the difference of two exact products (one rounding), the
    cost term three exact products and two additions --, so a sum's error is its additions': at most 16 per thread (an edge has at
    most 4096 pairs, 256 threads), 6 levels of the wave's shuffle tree and 3 additions of the four waves: 25 roundings, 27 with the
    term's own, each at most 2^-53 of the magnitudes summed.  The oracle's numpy sums add at most 20 of their own (pairwise
    summation over at most 4096 terms).  The map from the 38 sums to the record is three 6 x 6 congruences in fp64 on both sides, in
    different orders: at most 14 roundings per entry on either side, and 8 for the two roundings of each entry of R^T [t]x that enters
    twice: 27 + 20 + 2 * 14 + 8 = 83, 128 with slack."""
    ctx = gpu_ctx_factory()
    c = GC.case(cam)
    c.fill(ctx)
    ctx.keyframes_link()
    for poses in (None, offset_poses(c.poses0), c.truth):
        for gate in (0.1, 0.03):
            rec, mag = GO.records(c.keyframes, c.edges, c.poses0 if poses is None else poses, c.poses0, gate)
            got = ctx.graph_normal_eq(poses, gate)
            print(cam, "gate", gate, "worst error / (2^-53 S):", check_records(got, rec, mag))
            assert rec[:, 0].sum() > 0                                                  # some pairs count at every pose and gate
            again = ctx.graph_normal_eq(poses, gate)
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64))          # the same call, the same bits


# ---------------------------------------------------------------------------------------------- block edges
EDGE_SIZES = (1, 3, 63, 64, 65, 255, 256, 257, 4096)


def block_store():
    """six keyframes of 4096 random descriptors over the same 4096 points of a 4 m cube, each with its own 5 mm noise; half of every
    keyframe's points (another half in each) pushed 0.5 m away, some NaN; keyframe 5 sits 1 m off altogether.  Host edges of
    EDGE_SIZES pairs over the ten pairs of keyframes 0 .. 4, pairing a point with itself, and edge (5, 0) whose pairs are all gated out"""
    rng = np.random.default_rng(11)
    P = rng.uniform(-2, 2, (4096, 3))
    kfs, poses = [], []
    for k in range(6):
        kf = KC.tiny_keyframe(k, 4096, seed=9)
        x = P + rng.normal(0, 0.005, P.shape)
        x[rng.permutation(4096)[:2048]] += 0.5
        x[rng.integers(0, 4096, 40), rng.integers(0, 3, 40)] = np.nan
        if k == 5:
            x = P + 1.0
        kfs.append(dict(kf, xw=x.astype(F32)))
        poses.append(PC.moved(GC.IDENTITY, *rng.normal(0, 0.02, 3), *rng.normal(0, 0.05, 3)))
    pairs = [(j, i) for j in range(1, 5) for i in range(j)]
    edges = []
    for (j, i), n in zip(pairs, EDGE_SIZES):
        a = rng.permutation(4096)[:n].astype(np.int32) if n < 4096 else np.arange(4096, dtype=np.int32)
        edges.append((j, i, a, a.copy()))
    a = rng.permutation(4096)[:100].astype(np.int32)
    edges.append((5, 0, a, a.copy()))
    return kfs, poses, sorted(edges, key=lambda e: (e[0], e[1]))


def test_host_edges_of_every_block_shape_in_one_graph(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    kfs, poses, edges = block_store()
    for k, p in zip(kfs, poses):
        add_host(ctx, k, p)
    put_edges(ctx, reversed(edges))                                                    # any order in, (j, i) order out
    check_graph(ctx, edges)
    assert sorted(len(e[2]) for e in edges) == sorted(EDGE_SIZES + (100,))
    trial = offset_poses(poses)
    for P in (None, trial):
        at = poses if P is None else P
        assert same(ctx.graph_residuals(P, 0.1), GO.residuals(kfs, edges, at, poses, 0.1))
        rec, mag = GO.records(kfs, edges, at, poses, 0.1)
        got = ctx.graph_normal_eq(P, 0.1)
        print("worst error / (2^-53 S):", check_records(got, rec, mag))
        counted = rec[:, 0] / np.array([len(e[2]) for e in edges])
        assert all(0 < x < 1 for x, e in zip(counted, edges) if e[0] < 5 and len(e[2]) >= 63)   # about half of the pairs sit beyond the gate
        assert not got[-1].any() and edges[-1][:2] == (5, 0)                          # all gated out: a zero record
    # replacing an edge: the new pairs in its place, every other record as before
    j, i, a, b = edges[3]
    ctx.graph_add_edge(j, i, a[::-1].copy(), b[::-1].copy())
    edges[3] = (j, i, a[::-1].copy(), b[::-1].copy())
    check_graph(ctx, edges)
    rec, mag = GO.records(kfs, edges, poses, poses, 0.1)
    check_records(ctx.graph_normal_eq(None, 0.1), rec, mag)
    # an edge replaced again and again -- smaller (its old place), larger (behind the last edge), forty times at full size (the dead
    # pairs outweigh the live ones: they are compacted away) -- leaves every other edge's pairs where the graph finds them
    rng = np.random.default_rng(3)
    for n in (2, 40, 4096) + (4096,) * 40 + (7,):
        a = rng.integers(0, 4096, n).astype(np.int32)
        edges[3] = (j, i, a, a.copy())
        ctx.graph_add_edge(j, i, a, a)
    check_graph(ctx, edges)
    rec, mag = GO.records(kfs, edges, poses, poses, 0.1)
    check_records(ctx.graph_normal_eq(None, 0.1), rec, mag)
    # keyframe 5 has no counted pair: it is its own component and stays; the others move as the oracle's do
    want, wstats = GO.optimize(kfs, edges, poses, (0.1, 0.1, 0.05), 0)
    got, stats = ctx.keyframes_optimize((0.1, 0.1, 0.05), apply=False)
    assert np.array_equal(got[5], poses[5]) and np.array_equal(got[0], poses[0])
    assert all(close(p, q) for p, q in zip(got, want)) and all(abs(s[0] - w[0]) <= 2 + 1e-4 * w[0] for s, w in zip(stats, wstats)) and len(stats) == len(wstats)


# ---------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("cam", ["small", "half"])
def test_loop_matches_the_oracle_loop(gpu_ctx_factory, cam):
    """poses within 1e-6 (rad, m) of the oracle loop's and the counted pairs of every round within 2 + 1e-4 n: the rule of
    test_gpu_photo.py::test_loop_matches_the_oracle_loop; the end error of every keyframe within RELOC_BOUND"""
    ctx = gpu_ctx_factory()
    c = GC.case(cam)
    c.fill(ctx)
    ctx.keyframes_link()
    want, wstats = c.loop
    got, stats = ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=False)
    assert len(stats) == len(GC.GATES)
    for k in range(len(want)):
        assert close(got[k], want[k]), (k, got[k], want[k])
    for s, w in zip(stats, wstats):
        assert abs(s[0] - w[0]) <= 2 + 1e-4 * w[0] and abs(s[1] - w[1]) <= 1e-3 * w[1] + 1e-9 and abs(s[2] - w[2]) <= 1e-6
    end = c.errors(got)
    print(cam, "end errors", end, "oracle", GC.FIGURES[cam]["end"])
    assert all(e[0] < KC.RELOC_BOUND[0] and e[1] < KC.RELOC_BOUND[1] for e in end)
    assert np.array_equal(got[GC.ANCHOR], c.poses0[GC.ANCHOR])
    assert all(np.array_equal(ctx.keyframe(k)["pose12"], c.poses0[k]) for k in range(8))   # apply = 0: the store is what it was


def test_tol_ends_the_loop_early(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("half")
    c.fill(ctx)
    ctx.keyframes_link()
    wstats = c.loop[1]
    tol = 1e-3
    first = next(n for n, s in enumerate(wstats) if s[2] < tol)
    assert 0 < first < len(GC.GATES) - 1
    got, stats = ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, tol=tol, apply=False)
    assert len(stats) == first + 1 and stats[-1][2] < tol <= stats[-2][2]
    want, _ = GO.optimize(c.keyframes, c.edges, c.poses0, GC.GATES, GC.ANCHOR, tol)
    assert all(close(p, q) for p, q in zip(got, want))


def test_another_anchor_and_two_components(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    c.fill(ctx)
    ctx.keyframes_link()
    want, _ = GO.optimize(c.keyframes, c.edges, c.poses0, GC.GATES, 3)
    got, _ = ctx.keyframes_optimize(GC.GATES, 3, apply=False)
    assert np.array_equal(got[3], c.poses0[3]) and not np.array_equal(got[0], c.poses0[0])
    assert all(close(p, q) for p, q in zip(got, want))
    # {0, 1, 3} and {2, 5} through host edges (a caller's own lists); 4, 6 and 7 have no edge and keep their poses
    edges = [e for e in c.edges if {e[0], e[1]} <= {0, 1, 3} or {e[0], e[1]} <= {2, 5}]
    ctx.keyframes_clear()
    c.fill(ctx)
    put_edges(ctx, edges)
    check_graph(ctx, edges)
    want, wstats = GO.optimize(c.keyframes, edges, c.poses0, GC.GATES, 1)
    got, stats = ctx.keyframes_optimize(GC.GATES, 1, apply=False)
    for k in (1, 2, 4, 6, 7):
        assert np.array_equal(got[k], c.poses0[k]), k
    for k in (0, 3, 5):
        assert not np.array_equal(got[k], c.poses0[k]), k
    assert all(close(p, q) for p, q in zip(got, want)) and all(abs(s[0] - w[0]) <= 2 + 1e-4 * w[0] for s, w in zip(stats, wstats)) and len(stats) == len(wstats)


# ---------------------------------------------------------------------------------------------- apply
def relocalise(ctx, q):
    q.as_frame(ctx)
    return ctx.relocalize_keyframes(candidates=KC.CANDIDATES, min_matches=KC.MIN_MATCHES, **SOLVER, **RELOC)


def test_apply_rewrites_the_store_and_relocalisation_answers_in_the_corrected_world(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c, fig = GC.case("small"), GC.FIGURES["small"]
    queries = KC.FIGURES["small"]["queries"]
    # ONE query, chosen from the oracle alone, is held to both sides: outside RELOC_BOUND against the drifted store, inside it against
    # the corrected one.  Against the drifted store a query that keyframe k wins is answered in k's drifted world, P = Q T_k^-1 T0_k
    # (pose algebra on the oracle's poses), off by `before`; against the corrected store it is off by at most its own figure
    # (keyframe_cases) plus k's end error (graph_cases), `after`.  The query with the largest worst-case margin on both sides is taken
    def inverse(p):
        R = p[:9].reshape(3, 3)
        return np.concatenate([R.T.reshape(9), -R.T @ p[9:]])

    def ratio(e):
        return max(e[0] / KC.RELOC_BOUND[0], e[1] / KC.RELOC_BOUND[1])

    margin = []
    for n, q in enumerate(queries):
        k, Q = q["keyframe"], c.room.queries[n].pose
        before = ratio(VC.pose_error(GC.compose(Q, GC.compose(inverse(c.truth[k]), c.poses0[k])), Q))
        after = ratio((q["reloc"][0] + fig["end"][k][0], q["reloc"][1] + fig["end"][k][1]))
        margin.append(min(before, 1 / after))
    pick = int(np.argmax(margin))
    assert margin[pick] > 1.5, margin
    start = c.errors(c.poses0)
    far = int(np.argmax([e[0] for e in start]))
    q_far = next(n for n, q in enumerate(queries) if q["keyframe"] == far)
    assert start[far][0] > 5 * KC.RELOC_BOUND[0]
    c.fill(ctx)
    ctx.keyframes_link()
    for n in (pick, q_far):
        got = relocalise(ctx, c.room.queries[n])
        e = VC.pose_error(got["pose12"], c.room.queries[n].pose)
        print("drifted store: query", n, "keyframe", got["keyframe"], "error", e)
        assert got["keyframe"] == queries[n]["keyframe"] and (e[0] > KC.RELOC_BOUND[0] or e[1] > KC.RELOC_BOUND[1])
    poses, _ = ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=False)
    before = ctx.graph_residuals(poses, 0.03)
    assert all(same(ctx.keyframe(k)["xw"], c.keyframes[k]["xw"]) for k in range(8))
    applied, _ = ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=True)
    assert np.array_equal(applied, poses)
    want = GO.apply(c.keyframes, poses, c.poses0)
    for k in range(8):
        g = ctx.keyframe(k)
        assert np.array_equal(g["pose12"], poses[k]), k
        assert same(g["xw"], want[k]["xw"]) and same(g["nw"], want[k]["nw"]), k
        assert np.array_equal(g["desc"], c.keyframes[k]["desc"]) and np.array_equal(g["xy"], c.keyframes[k]["xy"])
    assert same(ctx.keyframe(0)["xw"], c.keyframes[0]["xw"])                          # the anchor's points did not move
    check_graph(ctx, c.edges)                                                         # edges are indices: still valid
    assert same(ctx.graph_residuals(None, 0.03), before) and same(ctx.graph_residuals(poses, 0.03), before)
    # the corrected points sit where the true ones do
    d = np.linalg.norm(ctx.keyframe(far)["xw"].astype(np.float64) - c.true_keyframes[far]["xw"], axis=1)
    d0 = np.linalg.norm(c.keyframes[far]["xw"].astype(np.float64) - c.true_keyframes[far]["xw"], axis=1)
    assert 4 * np.median(d) < np.median(d0) and np.median(d0) > 0.1
    got = relocalise(ctx, c.room.queries[pick])
    e = VC.pose_error(got["pose12"], c.room.queries[pick].pose)
    print("corrected store: query", pick, "keyframe", got["keyframe"], "error", e)
    assert got["keyframe"] == queries[pick]["keyframe"] and e[0] < KC.RELOC_BOUND[0] and e[1] < KC.RELOC_BOUND[1]
    # the query of the keyframe that had drifted furthest: the oracle's figures do not promise the bound for it (its own figure plus
    # the keyframe's end error pass it), so its error is held to that sum, the query's figure with the margin 2 that
    # test_gpu_keyframes.py gives the GPU's relocalisation against the oracle's
    got = relocalise(ctx, c.room.queries[q_far])
    e = VC.pose_error(got["pose12"], c.room.queries[q_far].pose)
    print("corrected store: query", q_far, "keyframe", got["keyframe"], "error", e)
    assert e[0] < 2 * queries[q_far]["reloc"][0] + fig["end"][far][0] and e[1] < 2 * queries[q_far]["reloc"][1] + fig["end"][far][1]


# ---------------------------------------------------------------------------------------------- errors
def test_state_and_argument_errors(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    c = GC.case("small")
    c.fill(ctx, upto=3)
    n = [len(k["xy"]) for k in c.keyframes[:3]]
    one = np.zeros(1, np.int32)
    for bad in (dict(first=-1), dict(first=4), dict(min_matches=2), dict(min_matches=L.MAX_KEYPOINTS + 1), dict(max_dist=257), dict(ratio=(0, 1)),
                dict(cross_check=2)):
        assert code_of(ctx.keyframes_link, **bad) == L.RPE_ERR_ARG, bad
    for j, i in ((0, 0), (0, 1), (3, 0), (1, -1)):
        assert code_of(ctx.graph_add_edge, j, i, one, one) == L.RPE_ERR_ARG, (j, i)
    assert code_of(ctx.graph_add_edge, 2, 1, [n[2]], [0]) == L.RPE_ERR_ARG and code_of(ctx.graph_add_edge, 2, 1, [0], [n[1]]) == L.RPE_ERR_ARG
    assert code_of(ctx.graph_add_edge, 2, 1, [-1], [0]) == L.RPE_ERR_ARG
    assert code_of(ctx.graph_add_edge, 2, 1, np.zeros(0, np.int32), np.zeros(0, np.int32)) == L.RPE_ERR_ARG
    assert code_of(ctx.graph_add_edge, 2, 1, np.zeros(L.MAX_KEYPOINTS + 1, np.int32), np.zeros(L.MAX_KEYPOINTS + 1, np.int32)) == L.RPE_ERR_ARG
    assert ctx.graph_info() == (0, 0) and code_of(ctx.keyframes_optimize, GC.GATES) == L.RPE_ERR_STATE
    assert code_of(ctx.graph_edge, 0) == L.RPE_ERR_ARG
    ctx.keyframes_link()
    assert ctx.graph_info()[0] == 3
    assert code_of(ctx.keyframes_optimize, GC.GATES, 3) == L.RPE_ERR_ARG and code_of(ctx.keyframes_optimize, GC.GATES, -1) == L.RPE_ERR_ARG
    assert code_of(ctx.keyframes_optimize, ()) == L.RPE_ERR_ARG and code_of(ctx.keyframes_optimize, (0.1, -1.0)) == L.RPE_ERR_ARG
    assert code_of(ctx.keyframes_optimize, GC.GATES, 0, -1.0) == L.RPE_ERR_ARG
    assert code_of(ctx.graph_residuals, None, -1.0) == L.RPE_ERR_ARG and code_of(ctx.graph_normal_eq, None, float("nan")) == L.RPE_ERR_ARG
    bad = np.array(c.poses0[:3])
    bad[1, 4] = np.nan
    assert code_of(ctx.graph_residuals, bad) == L.RPE_ERR_ARG
    assert code_of(ctx.graph_edge, 3) == L.RPE_ERR_ARG and code_of(ctx.graph_edge, -1) == L.RPE_ERR_ARG
    # a rank-deficient graph: three collinear pairs hold no rotation about their line; nothing is changed
    ctx.keyframes_clear()
    line = np.array([[0.2, 0.1, 2.0], [0.4, 0.2, 2.5], [0.8, 0.4, 3.5]], F32)
    for k in range(2):
        add_host(ctx, dict(KC.tiny_keyframe(k, 3), xw=line + F32(0.001 * k)))
    ctx.graph_add_edge(1, 0, [0, 1, 2], [0, 1, 2])
    assert ctx.graph_normal_eq()[0, 0] == 3
    assert code_of(ctx.keyframes_optimize, GC.GATES) == L.RPE_ERR_DEGENERATE
    assert np.array_equal(ctx.keyframe(1)["pose12"], GC.IDENTITY) and same(ctx.keyframe(1)["xw"], line + F32(0.001))


# ---------------------------------------------------------------------------------------------- C++
def test_graph_optimize_cpp(tmp_path):
    """DepthFrontEnd::linkKeyframes / optimizeKeyframes from plain C++ (tests/cpp/graph_optimize.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "graph_optimize")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "graph_optimize.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "graph_optimize: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
