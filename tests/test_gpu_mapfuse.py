"""GPU: the map fuse (csrc/rpe_mapfuse.hpp, rpe_mapfuse_api.hip) held BIT FOR BIT -- window, colour window and every archived brick, as
words -- to tests/mapfuse_oracle.py and, independent of the oracle, to the existing kernel: rpe_volume_fuse_keyframes of a second
context that holds the dense virtual volume of the box, split back into window and bricks.  The small scene of tests/mapfuse_cases.py:
a window of 3 x 2 x 2 bricks, boxes of at most 6 x 4 x 4, three keyframes of 48 x 36 and 40 x 30 pixels."""
import numpy as np
import pytest

import archive_oracle as AO
import mapfuse_cases as C
import mapfuse_oracle as MF
import mapmesh_cases as MC
import mapmesh_oracle as MM
import shift_oracle as SO
from rgbd_pose_estimation_amd import _lib as L
from test_gpu_rebuild import code_of

pytestmark = pytest.mark.gpu
U16 = np.uint16
ALL = [0, 1, 2]


def last_error():
    return L.lib().rpe_last_error().decode()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def rig(gpu_ctx_factory):
    """(ctx, ref): two contexts whose stores hold the three keyframes with depth and colour attached"""
    ctx, ref = gpu_ctx_factory(), gpu_ctx_factory()
    assert C.fill_store(ctx) == ALL and C.fill_store(ref) == ALL
    return ctx, ref


def walked(ctx, colour=True, capacity=96):
    """mapfuse_cases' short walk on the device: content in the window, 13 held bricks around it, total (8, 8, -8)"""
    m = MC.Map(ctx, C.DIMS, C.KW, capacity=capacity).fill(MC.sphere((10.2, 7.7, 8.4), 9.3), [(8, 0, 0), (0, 8, -8)], colour=colour)
    assert len(m.store) == 13 and tuple(m.total) == (8, 8, -8)
    return m


def snapshot(ctx):
    colour = ctx.volume_color_download().view(U16) if code_of(ctx.volume_color_download) == L.RPE_OK else None
    return (ctx.volume_download().view(np.uint32), colour, ctx.volume_archive_download(), ctx.volume_archive_info())


def unchanged(a, b):
    flat = lambda s: [s[0], s[1], *s[2]]
    return a[3] == b[3] and all((x is None and y is None) or (x is not None and y is not None and same(x, y)) for x, y in zip(flat(a), flat(b)))


def differ(a, b):
    """how many rows (voxels) of two arrays of equal layout differ, and the first few of them: the assertion's message"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return a.shape, a.dtype, b.shape, b.dtype
    bad = np.nonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(-1, a.shape[-1] * a.dtype.itemsize).any(1))[0]
    return len(bad), bad[:6], a.reshape(-1, a.shape[-1])[bad[:3]], b.reshape(-1, b.shape[-1])[bad[:3]]


def agree(ctx, m, what):
    """the context holds the model's map, bit for bit"""
    got = ctx.volume_download()
    assert same(got, m.window), (what, "window", differ(got, m.window))
    if m.cwindow is None:
        assert code_of(ctx.volume_color_download) == L.RPE_ERR_STATE, what
    else:
        got = ctx.volume_color_download().view(U16)
        assert same(got, m.cwindow), (what, "colour window", differ(got, m.cwindow))
    coords, tsdf, colour = ctx.volume_archive_download()
    wc, wt, wcol = AO.download(m.store)
    assert ctx.volume_archive_info()["held"] == len(m.store) and np.array_equal(coords, wc), (what, len(coords), len(wc))
    assert same(tsdf, wt), (what, "held tsdf", differ(tsdf, wt))
    colour = np.zeros_like(wcol) if colour is None else colour.view(U16)
    assert same(colour, wcol), (what, "held colour", differ(colour, wcol))


def reference(ref, m, box, ids, poses, clear, color, cull=True):
    """the existing kernel's answer: the dense box in a second context, rpe_volume_fuse_keyframes there, split back into the map"""
    vol, cvol = m.dense(box)
    G = MM.geometry(m.kw, box)
    ref.volume_init(G.dim, **dict(m.kw, origin=tuple(SO.origin_after(m.kw["origin"], m.kw["voxel_size"], box[0]))))
    ref.volume_upload(vol)
    if m.has_colour():
        ref.volume_color_upload(cvol.view(np.float16))
    ref.volume_fuse_keyframes(ids, poses, clear=clear, color=color, cull=cull)
    out = ref.volume_download()
    cout = ref.volume_color_download().view(U16) if (color or (m.has_colour() and not clear)) else None
    cwindow = np.zeros(m.window.shape[:3] + (4,), U16) if (color and m.cwindow is None) else m.cwindow
    return MF.split(out, cout, box, m.window, cwindow, m.total, m.store)


def run(rig, m, ids=ALL, poses=None, clear=True, color=False, cull=True, box=None, what=""):
    """the call on the context, the oracle on the model, the second context's answer; all three agree.  Returns the call's stats"""
    ctx, ref = rig
    bx = m.bounds() if box is None else box
    w, cw, store = reference(ref, m, bx, ids, poses, clear, color, cull)
    stats = ctx.volume_map_fuse_keyframes(ids, poses, clear=clear, color=color, cull=cull, box=box)
    want = C.fuse(m, ids, poses, clear, color, bx)
    assert same(w, m.window) and ((cw is None and m.cwindow is None) or same(cw, m.cwindow)), (what, "the second context and the oracle")
    agree(ctx, m, what)
    assert set(store) == set(m.store) and all(same(store[k][0], m.store[k][0]) and same(store[k][1], m.store[k][1]) for k in store), what
    print(what, stats, want)
    assert all(stats[k] == want[k] for k in want), (what, stats, want)
    return stats


# ---------------------------------------------------------------------------------------------- 1. CLEAR and accumulate
@pytest.mark.parametrize("color", (False, True), ids=("tsdf", "colour"))
def test_clear_on_an_empty_archive(rig, color):
    m = MC.Map(rig[0], C.DIMS, C.KW, capacity=96)
    stats = run(rig, m, clear=True, color=color, box=C.BOX, what="clear, nothing held")
    assert stats["bricks"] == 96 and stats["released"] == 0 and stats["archived"] == len(m.store) > 40
    assert stats["written"] == 12 + stats["archived"] and (m.window[..., 1] > 0).sum() > 1000
    assert (m.cwindow is not None and (m.cwindow[..., 3] != 0).sum() > 500) if color else m.cwindow is None
    # again on what it left: CLEAR starts from zeros, so the same map
    before = snapshot(rig[0])
    rig[0].volume_map_fuse_keyframes(ALL, clear=True, color=color, box=C.BOX)
    assert unchanged(before, snapshot(rig[0]))


@pytest.mark.parametrize("map_colour,color", ((True, False), (True, True), (False, True), (False, False)),
                         ids=("coloured-map-tsdf", "coloured-map-colour", "plain-map-colour", "plain-map-tsdf"))
def test_accumulate_onto_a_walked_map(rig, map_colour, color):
    m = walked(rig[0], map_colour)
    held = {k: (t.copy(), c.copy()) for k, (t, c) in m.store.items()}
    stats = run(rig, m, clear=False, color=color, box=C.BOX, what="accumulate")
    assert stats["released"] == 0 and stats["archived"] > 10 and 0 < stats["written"] < 96 and set(held) <= set(m.store)
    assert any(not same(m.store[k][0], held[k][0]) for k in held)                        # a held brick took observations
    # ... and a second time, onto weights that now sit at the clamp
    run(rig, m, ids=[2, 0], clear=False, color=color, box=C.BOX, what="accumulate again")
    assert (m.window[..., 1] == C.KW["max_weight"]).any()


def test_clear_without_color_zeroes_the_colour_and_releases_unseen_bricks(rig):
    m = walked(rig[0], True)
    assert m.cwindow.any() and any(c.any() for _, c in m.store.values())
    stats = run(rig, m, ids=[1], clear=True, color=False, what="clear, colour exists")
    assert stats["released"] >= 5 and rig[0].volume_archive_info()["held"] == 13 + stats["archived"] - stats["released"]
    assert m.cwindow is not None and not m.cwindow.any() and all(not c.any() for _, c in m.store.values())


def test_a_held_brick_nobody_sees_keeps_its_bits(rig):
    m = walked(rig[0], True)
    held = {k: (t.copy(), c.copy()) for k, (t, c) in m.store.items()}
    run(rig, m, ids=[1], clear=False, color=True, what="accumulate, one view")
    kept = [k for k in held if same(m.store[k][0], held[k][0]) and same(m.store[k][1], held[k][1])]
    assert len(kept) >= 5 and len(kept) < len(held)


# ---------------------------------------------------------------------------------------------- 2. boxes
@pytest.mark.parametrize("clear", (True, False), ids=("clear", "accumulate"))
def test_boxes_that_cut_and_miss_the_window(rig, clear):
    ctx = rig[0]
    for name, box in (("cuts", (np.array([-8, -8, -8]), np.array([16, 16, 8]))), ("misses", (np.array([-8, -8, -8]), np.array([8, 24, 24])))):
        m = walked(ctx, True)
        w0, c0, s0 = m.window.copy(), m.cwindow.copy(), dict(m.store)
        run(rig, m, clear=clear, color=True, box=box, what=name)
        # outside the box nothing moved
        inside = np.zeros(m.window.shape[:3], bool)
        MM._paste(inside, np.ones(tuple(int(x) for x in (box[1] - box[0])[::-1]), bool), box[0], *m.extent())
        assert same(m.window[~inside], w0[~inside]) and same(m.cwindow[~inside], c0[~inside]) and (name == "misses") == (not inside.any())
        out = [k for k in s0 if not all(box[0][a] <= 8 * k[a] < box[1][a] for a in range(3))]
        assert out and all(same(m.store[k][0], s0[k][0]) for k in out)


@pytest.mark.parametrize("color", (False, True), ids=("tsdf", "colour"))
def test_the_windows_extent_is_the_window_fuse_of_the_same_context(rig, color):
    ctx = rig[0]
    m = walked(ctx, True)
    ctx.volume_fuse_keyframes(ALL, clear=True, color=color)
    want = ctx.volume_download()
    cwant = ctx.volume_color_download() if color else None
    m = walked(ctx, True)
    stats = run(rig, m, clear=True, color=color, box=m.extent(), what="the window's extent")
    assert same(ctx.volume_download(), want) and stats == dict(bricks=12, written=12, archived=0, released=0)
    assert cwant is None or same(ctx.volume_color_download(), cwant)


# ---------------------------------------------------------------------------------------------- 3. the list
def test_the_cull_changes_no_bit_and_poses_default_to_the_stores(rig):
    ctx = rig[0]
    moved = [C.pose_at((0.0, 0.1, -0.1), 0.0, 0.05, 0.0), C.pose_at((0.7, 0.0, 0.1), 0.0, 0.2, 0.02)]
    got = []
    for cull in (True, False):
        m = walked(ctx, True)
        run(rig, m, ids=[1, 0], poses=moved, clear=False, color=True, cull=cull, box=C.BOX, what=f"cull {cull}")
        got.append(snapshot(ctx))
    assert unchanged(*got)
    m = walked(ctx, True)
    run(rig, m, ids=[1, 0], poses=None, clear=False, color=True, box=C.BOX, what="the store's poses")
    assert not unchanged(got[0], snapshot(ctx))                                           # the given poses were used above


@pytest.mark.parametrize("count", (129, 256))
def test_long_lists_reach_the_second_cull_entry_per_thread(rig, count):
    """2 x 2 x 2 bricks, one of them the window's; ids repeated: entries 128 .. 255 are the cull's second trip and the whole keep[]"""
    ids = (ALL * 86)[:count]
    box = (np.array([16, 8, 8]), np.array([32, 24, 24]))
    for cull in (True, False):
        m = MC.Map(rig[0], C.DIMS, C.KW, capacity=8)
        stats = run(rig, m, ids=ids, clear=False, color=True, cull=cull, box=box, what=f"{count} entries, cull {cull}")
        assert stats["bricks"] == 8 and stats["archived"] >= 3 and (m.window[..., 1] == 4).any()


# ---------------------------------------------------------------------------------------------- 4. capacity
def test_capacity_is_checked_before_anything_is_written(rig):
    ctx = rig[0]
    probe = MC.Map(None, C.DIMS, C.KW)
    need = C.fuse(probe, ALL, None, True, True, C.BOX)["archived"]
    m = MC.Map(ctx, C.DIMS, C.KW, capacity=need - 1)
    m.upload(*MC.sphere((10.2, 7.7, 8.4), 9.3)(m.total, m.dims))
    before = snapshot(ctx)
    for clear in (True, False):
        assert code_of(ctx.volume_map_fuse_keyframes, ALL, None, clear, True, True, C.BOX) == L.RPE_ERR_STATE
        assert "free slots" in last_error() and str(need) in last_error()
        assert unchanged(before, snapshot(ctx))
    ctx.volume_archive(need)
    stats = run(rig, m, clear=True, color=True, box=C.BOX, what="after growing the pool")
    assert stats["archived"] == need and ctx.volume_archive_info() == dict(held=need, capacity=need)
    # a full pool: CLEAR's releases count as free slots, accumulation has none
    m = walked(ctx, True, capacity=13)
    before = snapshot(ctx)
    assert code_of(ctx.volume_map_fuse_keyframes, [1], None, False, False) == L.RPE_ERR_STATE and unchanged(before, snapshot(ctx))
    stats = run(rig, m, ids=[1], clear=True, color=False, what="a full pool, clear")
    assert stats["released"] >= stats["archived"] > 0


# ---------------------------------------------------------------------------------------------- 5. the shift
def test_a_shift_brings_the_rebuilt_bricks_into_the_window_and_back(rig):
    ctx = rig[0]
    m = MC.Map(ctx, C.DIMS, C.KW, capacity=128)
    run(rig, m, clear=True, color=True, box=C.BOX, what="before the shifts")
    held = len(m.store)
    for d in ((8, 8, 0), (-8, -8, 0), (-8, 0, -8), (8, 0, 8)):
        m.shift(d)
        agree(ctx, m, f"shift {d}")
    assert len(m.store) == held and (m.window[..., 1] > 0).any()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    raw = L.lib().rpe_volume_map_fuse_keyframes
    one, lo, hi, st = np.zeros(1, np.int32), np.zeros(3, np.int64), np.full(3, 8, np.int64), np.zeros(4, np.int64)
    call = lambda **kw: code_of(ctx.volume_map_fuse_keyframes, **kw)
    assert call() == L.RPE_ERR_STATE                                                     # no volume
    ctx.volume_init((20, 16, 16), **C.KW)
    assert call() == L.RPE_ERR_STATE                                                     # a dim that is no multiple of 8
    ctx.volume_init(C.DIMS, **C.KW)
    assert call() == L.RPE_ERR_STATE and call(ids=[0]) == L.RPE_ERR_ARG                  # an empty store; no such keyframe
    rng = np.random.default_rng(1)
    for k in C.keyframes()[:2]:
        ctx.keyframe_add_host(rng.integers(4, 20, (4, 2)), rng.integers(0, 99, (4, 8)), rng.normal(0, 1, (4, 3)), np.tile([0, 0, 1.0], (4, 1)),
                              k["pose"], k["cam"][4], k["cam"][5])
    assert call() == L.RPE_ERR_STATE and call(ids=[0]) == L.RPE_ERR_STATE                # nothing attached
    k = C.keyframes()[0]
    ctx.keyframe_attach(0, k["z"].reshape(36, 48), None, k["cam"])
    before = ctx.volume_download()
    assert call(ids=[0, 1]) == L.RPE_ERR_STATE and call(ids=[0], color=True) == L.RPE_ERR_STATE   # no depth; no colour
    assert call(ids=[2]) == L.RPE_ERR_ARG and call(ids=[-1]) == L.RPE_ERR_ARG and call(ids=[0] * 257) == L.RPE_ERR_ARG
    assert raw(ctx._h, one.ctypes.data, 0, None, 1, None, None, None) == L.RPE_ERR_ARG   # count 0 with a list
    assert raw(ctx._h, one.ctypes.data, 1, None, 8, None, None, None) == L.RPE_ERR_ARG   # an unknown flag
    assert raw(ctx._h, one.ctypes.data, 1, None, 1, lo.ctypes.data, None, None) == L.RPE_ERR_ARG   # lo without hi
    assert raw(None, one.ctypes.data, 1, None, 1, None, None, None) == L.RPE_ERR_ARG
    for box in ((lo + [4, 0, 0], hi), (lo, lo), (hi, lo), (lo, lo + [8, 8, (1 << 20) + 8])):
        assert call(ids=[0], box=box) == L.RPE_ERR_ARG, box
    assert call(ids=[0], box=(lo, lo + [8 * 512, 8 * 512, 8 * 128])) == L.RPE_ERR_ARG and "2^24" in last_error()   # 2^25 bricks
    assert call(ids=[0], box=(lo - 8, hi)) == L.RPE_ERR_STATE and "archive is off" in last_error()
    assert same(ctx.volume_download(), before)
    # the archive off, the box inside the window: the window fuse
    assert raw(ctx._h, one.ctypes.data, 1, None, 1, None, None, st.ctypes.data) == L.RPE_OK and list(st) == [12, 12, 0, 0]
    got = ctx.volume_download()
    ctx.volume_fuse_keyframes([0], clear=True)
    assert same(got, ctx.volume_download()) and (got[..., 1] > 0).any()
    # the last mesh goes with CLEAR, as after rpe_volume_fuse_keyframes, and stays without
    V, N, T = ctx.volume_mesh(1.0)
    v, n, t = np.zeros_like(V), np.zeros_like(N), np.zeros_like(T)
    download = lambda: L.lib().rpe_volume_mesh_download(ctx._h, v.ctypes.data, n.ctypes.data, t.ctypes.data)
    ctx.volume_map_fuse_keyframes([0], clear=False)
    assert len(T) > 50 and download() == L.RPE_OK and same(v, V)
    ctx.volume_map_fuse_keyframes([0], clear=True)
    assert download() == L.RPE_ERR_STATE


# ---------------------------------------------------------------------------------------------- 7. the use case
def test_the_walk_rebuilt_at_corrected_poses(gpu_ctx_factory):
    """tests/mapfuse_cases.py through the API: the archive's walk fused at drifted poses with every other frame a keyframe, the map
    meshed as fused, rebuilt at the corrected and at the true poses, and by today's route; the oracle's figures, and the claim"""
    import archive_cases as AC
    import shift_cases as SC
    ctx = gpu_ctx_factory()
    ctx.volume_init(AC.DIMS, **SC.desc())
    ctx.volume_archive(C.CAPACITY)
    P, at, ids, rng = C.walk_poses("drifted"), C.keyframe_positions(), [], np.random.default_rng(5)
    for n in range(len(AC.PATH)):
        if n:
            sh = ctx.volume_follow(P[n], SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(P[n])
        if n in at:
            ids.append(ctx.keyframe_add_host(rng.integers(4, 60, (4, 2)), rng.integers(0, 99, (4, 8)), rng.normal(0, 1, (4, 3)),
                                             np.tile([0, 0, 1.0], (4, 1)), P[n], AC.CAM[4], AC.CAM[5]))
            ctx.keyframe_attach_frame(ids[-1])
    box = ctx.volume_map_bounds()
    assert (tuple(box[0]), tuple(box[1])) == C.USE_BOX and ctx.volume_archive_info()["held"] == C.USE_HELD
    f = {}
    V, _, T = ctx.volume_map_mesh(C.WMIN)
    f["drifted"] = C.figures(V, T)
    for name in ("corrected", "truth"):
        Q = C.walk_poses(name)
        stats = ctx.volume_map_fuse_keyframes(ids, [Q[n] for n in at], clear=True, box=box)
        if name == "corrected":
            assert (stats["archived"], stats["released"]) == (C.USE_ARCHIVED, C.USE_RELEASED), stats
        assert ctx.volume_archive_info()["held"] == C.USE_HELD_REBUILT
        V, _, T = ctx.volume_map_mesh(C.WMIN, box)
        f[name] = C.figures(V, T)
    Q = C.walk_poses("corrected")
    ctx.volume_fuse_keyframes(ids, [Q[n] for n in at], clear=True)
    ctx.volume_archive_clear()
    V, _, T = ctx.volume_map_mesh(C.WMIN)
    f["today"] = C.figures(V, T)
    print(f)
    assert all(C.same_figures(f[k], C.FIGURES[k]) for k in C.FIGURES), f
    C.claim(f)
