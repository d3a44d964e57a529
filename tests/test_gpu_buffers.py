"""GPU: device buffers that grow, are reused and shrink on ONE context (csrc/rpe_devbuf.hpp behind every host unit).  The oracle tests
run each feature on a context of one size; here a context changes size under them -- 64 x 48 -> 96 x 64 -> 64 x 48, volume 32^3 ->
48^3 -> 32^3 -- and the keyframe store, the graph's pair arrays, the model maps and the solver's arrays grow past their first
allocation.  Every result is compared BIT FOR BIT with what a fresh context gives at the same size, or with the bytes that went in."""
import numpy as np
import pytest

from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
F32 = np.float32
EYE = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
SMALL, LARGE = (64, 48, 32), (96, 64, 48)          # width, height, voxels per volume side


def scene(w, h):
    """a wavy wall in front of the camera with a few holes, and a blocky random texture (corners for the detector)"""
    cam = (0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0, w, h)
    v, u = np.mgrid[0:h, 0:w]
    depth = (1.3 + 0.2 * np.sin(u / 9.0) + 0.15 * np.cos(v / 7.0)).astype(F32)
    depth[h // 3, w // 4:w // 4 + 3] = 0.0
    rng = np.random.default_rng(w * 1000 + h)
    blocks = rng.integers(0, 256, ((h + 5) // 6, (w + 5) // 6, 3)).astype(np.uint8)
    rgb = np.ascontiguousarray(np.kron(blocks, np.ones((6, 6, 1), np.uint8))[:h, :w])
    return cam, depth, rgb


def front_end(ctx, size):
    """every Part 3 stage once at `size`; {name: bytes} of everything it leaves on the device"""
    w, h, dim = size
    cam, depth, rgb = scene(w, h)
    out = {}

    def keep(name, a):
        out[name] = (np.asarray(a).shape, np.ascontiguousarray(a).tobytes())

    ctx.frame_set_filter(1)
    ctx.frame_set_depth(depth, cam, dmin=0.1, dmax=5.0, levels=2)
    ctx.frame_set_color(rgb)
    for level in (0, 1):
        for which in (L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_DEPTH):
            keep(f"frame {which} level {level}", ctx.frame_download(which, level))
    keep("frame colour", ctx.frame_color())
    voxel = 2.4 / dim
    ctx.volume_init((dim, dim, dim), voxel, (-1.2, -1.2, 0.2), 3 * voxel)
    ctx.volume_integrate_color(EYE)
    keep("volume", ctx.volume_download())
    keep("colour volume", ctx.volume_color_download().view(np.uint16))
    ctx.volume_raycast(EYE, cam, 0.1, 4.0, levels=2)
    keep("model colour", ctx.model_color())
    for level in (0, 1):
        for which in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL):
            keep(f"model {which} level {level}", ctx.frame_download(which, level))
    V, N, T = ctx.volume_mesh(1.0)
    keep("mesh vertices", V); keep("mesh normals", N); keep("mesh triangles", T)
    keep("mesh colours", ctx.volume_mesh_colors())
    ctx.photo_prepare(2)
    for level in (0, 1):
        for which in (L.PHOTO_FRAME, L.PHOTO_MODEL):
            keep(f"photo {which} level {level}", ctx.photo_download(which, level))
    counts = [ctx.features_detect(L.FEAT_FRAME), ctx.features_detect(L.FEAT_MODEL)]
    for which in (L.FEAT_FRAME, L.FEAT_MODEL):
        for name, a in zip(("xy", "score", "desc"), ctx.features(which)):
            keep(f"features {which} {name}", a)
    m = ctx.features_match()
    for name, a in zip(("frame", "model", "d1", "d2", "weight"), ctx.matches()):
        keep(f"matches {name}", a)
    for slot in (L.XW, L.XC, L.BV, L.NW, L.NC):
        keep(f"slot {slot}", ctx.download(slot) if m else np.zeros(0, F32))
    print(f"front end {w} x {h}, {dim}^3: {counts[0]} / {counts[1]} keypoints, {m} matches, {len(V)} vertices, {len(T)} triangles")
    assert min(counts) > 0 and len(V) > 0 and len(T) > 0          # the stages had something to work on
    return out


def differing(a, b):
    return [k for k in a if a[k] != b.get(k)] + [k for k in b if k not in a]


def keyframes(count):
    """`count` synthetic keyframes of 4096 keypoints inside a 64 x 48 image"""
    rng = np.random.default_rng(7)
    k = L.MAX_KEYPOINTS
    out = []
    for i in range(count):
        xy = np.stack([rng.integers(0, 64, k), rng.integers(0, 48, k)], axis=1).astype(np.int32)
        desc = rng.integers(0, 2 ** 32, (k, 8), dtype=np.uint64).astype(np.uint32)
        xw, nw = rng.normal(0, 1, (k, 3)).astype(F32), rng.normal(0, 1, (k, 3)).astype(F32)
        pose = EYE.copy(); pose[9:] = (0.01 * i, 0.0, 0.0)
        out.append(dict(xy=xy, desc=desc, xw=xw, nw=nw, pose12=pose))
    return out


def same_keyframe(got, kf):
    return all(got[n].tobytes() == kf[n].tobytes() for n in ("xy", "desc", "xw", "nw", "pose12")) and (got["width"], got["height"]) == (64, 48)


def add_keyframe(ctx, kf):
    return ctx.keyframe_add_host(kf["xy"], kf["desc"], kf["xw"], kf["nw"], kf["pose12"], 64, 48)


def test_buffers_grow_shrink_and_are_reused_on_one_context(gpu_ctx_factory):
    from rgbd_pose_estimation_amd import api
    ctx, fresh_small, fresh_large = api.Context(0), gpu_ctx_factory(), gpu_ctx_factory()
    # ---- 1. the front end at 64 x 48 / 32^3, grown to 96 x 64 / 48^3, back at 64 x 48 / 32^3 (every buffer now larger than needed)
    ref_small, ref_large = front_end(fresh_small, SMALL), front_end(fresh_large, LARGE)
    assert differing(front_end(ctx, SMALL), ref_small) == []
    assert differing(front_end(ctx, LARGE), ref_large) == []
    assert differing(front_end(ctx, SMALL), ref_small) == []

    # ---- 4. the model maps grown from 1 to 3 levels: fresh_small's two-level maps (3840 pixels) must grow for three levels (4032) and
    # keep level 0 on the way; ctx's maps still have the large frame's room and stay where they are
    level0 = [fresh_small.frame_download(w, 0).tobytes() for w in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL)]
    fresh_small.model_build_pyramid(3)
    ctx.model_build_pyramid(3)
    assert [fresh_small.frame_download(w, 0).tobytes() for w in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL)] == level0
    for level in (0, 1, 2):
        for which in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL):
            assert fresh_small.frame_download(which, level).tobytes() == ctx.frame_download(which, level).tobytes(), (which, level)

    # ---- 2. nine keyframes of 4096 keypoints: the ninth forces the store's first doubling past 32768 keypoints; the query's rows
    # grow from 8 to 16 with it.  fresh_small takes all nine before its first query
    kfs = keyframes(9)
    for kf in kfs[:8]:
        add_keyframe(ctx, kf)
    counts8, order8 = ctx.keyframes_query()
    assert add_keyframe(ctx, kfs[8]) == 8
    for i in (0, 7, 8):
        assert same_keyframe(ctx.keyframe(i), kfs[i]), i                      # the bytes that went in
    for kf in kfs:
        add_keyframe(fresh_small, kf)
    counts9, order9 = ctx.keyframes_query()
    ref_counts, ref_order = fresh_small.keyframes_query()
    assert np.array_equal(counts9, ref_counts) and np.array_equal(order9, ref_order) and np.array_equal(counts9[:8], counts8)
    assert ctx.keyframe_match(8) == fresh_small.keyframe_match(8) == counts9[8]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.matches(), fresh_small.matches()))

    # ---- 3. edges of 4096 pairs until the pair arrays double (65536 pairs hold sixteen): the first edge is then unchanged
    rng = np.random.default_rng(11)
    pairs = [(j, i) for j in range(1, 9) for i in range(j)][:18]
    edges = {ji: (rng.integers(0, 4096, 4096).astype(np.int32), rng.integers(0, 4096, 4096).astype(np.int32)) for ji in pairs}
    for n, (j, i) in enumerate(pairs):
        ctx.graph_add_edge(j, i, *edges[(j, i)])
        a, b = ctx.graph_edge(0)
        assert np.array_equal(a, edges[pairs[0]][0]) and np.array_equal(b, edges[pairs[0]][1]), n
    assert ctx.graph_info() == (18, 18 * 4096)
    for n, ji in enumerate(sorted(pairs)):
        a, b = ctx.graph_edge(n)
        assert np.array_equal(a, edges[ji][0]) and np.array_equal(b, edges[ji][1]), ji

    # ---- 5. the solver's arrays, masks and weights at n = 1000, 5000, 0 and 1000 again: the same record, exactly
    def record(c, n, seed):
        r = np.random.default_rng(seed)
        xw = r.normal(0, 1, (n, 3)).astype(F32)
        c.load(L.F32, xw=xw, xc=xw + r.normal(0, 0.01, (n, 3)).astype(F32))
        for mod in (L.MOD_23, L.MOD_33, L.MOD_NN):
            c.upload_mask(mod, (r.uniform(0, 1, n) < 0.8).astype(np.int16))
            c.upload_weight(mod, r.uniform(0.5, 1.5, n).astype(F32))
        return c.normal_eq(L.RES_P2P, EYE, L.USE_MASK | L.USE_WEIGHT)[0]

    def empty_problem(c):                                                      # nothing to copy, and still a mask and a weight
        c.set_problem(0)
        for mod in (L.MOD_23, L.MOD_33, L.MOD_NN):
            c.upload_mask(mod, np.zeros(4, np.int16)[:0])
            c.upload_weight(mod, np.zeros(4, F32)[:0])

    first = record(ctx, 1000, 21)
    assert first[28] > 0                                                       # the masked, weighted pairs counted
    record(ctx, 5000, 22)
    empty_problem(ctx)
    assert record(ctx, 1000, 21).tobytes() == first.tobytes()

    # ---- the context goes, with everything it grew; the next one works
    ctx.close()
    again = api.Context(0)
    try:
        empty_problem(again)                                                   # (its first masks and weights: zero bytes asked)
        assert record(again, 1000, 21).tobytes() == first.tobytes()
        assert differing(front_end(again, SMALL), ref_small) == []
    finally:
        again.close()
