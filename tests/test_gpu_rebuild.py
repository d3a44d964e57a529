"""GPU: keyframe attachments and rpe_volume_fuse_keyframes (csrc/rpe_rebuild.hip, rpe_rebuild_api.hip, the attachment calls of
rpe_keyframe_api.hip).  The fuse is held BIT FOR BIT to two references at once: the frame-by-frame route of a second context
(volume_init + as_frame + volume_integrate[_color] per keyframe, code that exists without this feature) and tests/rebuild_oracle.py
-- over awkward volumes, lists of every length, the weight clamp, repeated ids, an uploaded start without CLEAR, the cull on and off,
mixed cameras and the caller's poses -- and the loop closure is followed end to end into the rebuilt map.  `same` is bit for bit;
colour volumes are compared as uint16."""
import os
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import graph_cases as GC
import keyframe_cases as KC
import rebuild_cases as RC
import rebuild_oracle as RO
import volume_cases as VC
import volume_oracle as VO
from rgbd_pose_estimation_amd import _lib as L

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


def same16(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16))


def code_of(fn, *a, **kwargs):
    try:
        fn(*a, **kwargs)
    except L.RpeError as e:
        return e.code
    return L.RPE_OK


def colour_of(ctx):
    return ctx.volume_color_download().view(np.uint16)


def sequential(seq, dims, kw, pairs, color, start=None):
    """the route that exists without the feature: clear (or the uploaded start), then one frame at a time"""
    seq.volume_init(dims, **kw)
    if start is not None:
        seq.volume_upload(start[0])
        if start[1] is not None:
            seq.volume_color_upload(start[1].view(np.float16))
    for shot, pose in pairs:
        shot.as_frame(seq)
        (seq.volume_integrate_color if color else seq.volume_integrate)(pose)
    has_colour = color or (start is not None and start[1] is not None)
    return seq.volume_download(), colour_of(seq) if has_colour else None


def random_start(G, seed):
    """a volume and a colour volume of arbitrary content: any tsdf, weights 0 .. W, colours 0 .. 255, a few NaNs of several payloads"""
    rng = np.random.default_rng(seed)
    d0, d1, d2 = G.dim
    vol = np.empty((d2, d1, d0, 2), F32)
    vol[..., 0] = rng.normal(0, 0.7, (d2, d1, d0))
    vol[..., 1] = rng.integers(0, int(G.W) + 1, (d2, d1, d0))
    flat = vol.reshape(-1).view(np.uint32)
    n = flat.size
    flat[rng.integers(0, n, 40)] = np.uint32(0x7fc00000)
    flat[rng.integers(0, n, 10)] = np.uint32(0xffc01234)
    flat[rng.integers(0, n, 10)] = np.uint32(0x80000000)
    cvol = np.empty((d2, d1, d0, 4), np.uint16)
    cvol[..., :3] = CO.h(rng.uniform(0, 255, (d2, d1, d0, 3)))
    cvol[..., 3] = CO.h(rng.integers(0, int(G.W) + 1, (d2, d1, d0)).astype(F32))
    cflat = cvol.reshape(-1)
    cflat[rng.integers(0, cflat.size, 40)] = np.uint16(0x7e00)
    cflat[rng.integers(0, cflat.size, 10)] = np.uint16(0x7e01)
    return vol, cvol


@pytest.fixture(scope="module")
def rig(gpu_ctx_factory):
    """(ctx, seq, case): a context whose store holds the eight drifted `small` keyframes with their shots attached through
    attach_frame, and the second context of the frame-by-frame route"""
    ctx, seq, c = gpu_ctx_factory(), gpu_ctx_factory(), RC.case()
    ids = c.fill(ctx)
    for i, s in zip(ids, RC.shots()):
        s.as_frame(ctx)
        ctx.keyframe_attach_frame(i)
    return ctx, seq, c


# ---------------------------------------------------------------------------------------------- 1. attachments
def test_attachment_round_trip(gpu_ctx_factory):
    ctx, c = gpu_ctx_factory(), RC.case()
    shots = RC.shots()
    c.fill(ctx, upto=3)
    assert ctx.keyframe_attachment(0) == dict(z=None, rgba=None, cam=None)
    assert code_of(ctx.keyframe_attach_frame, 0) == L.RPE_ERR_STATE                       # no frame yet
    shots[0].as_frame(ctx)
    ctx.keyframe_attach_frame(0)
    a = ctx.keyframe_attachment(0)
    zmap = ctx.frame_download(L.MAP_VERTEX)[:, 2]
    assert same(a["z"].reshape(-1), zmap) and same(zmap, shots[0].V[:, 2]) and (~np.isnan(zmap)).any()
    assert np.array_equal(a["rgba"], ctx.frame_color()) and np.array_equal(a["rgba"], shots[0].rgba)
    assert a["cam"] == tuple(float(x) for x in RC.CAM[:4]) + tuple(RC.CAM[4:])
    assert ctx.keyframe_attachment(1)["z"] is None                                        # the others carry nothing
    # a frame without colour attaches its depth alone
    ctx.frame_set_depth(shots[1].depth, RC.CAM, dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])
    ctx.keyframe_attach_frame(1)
    b = ctx.keyframe_attachment(1)
    assert b["rgba"] is None and same(b["z"].reshape(-1), shots[1].V[:, 2])
    # with the depth filter on, the plane is the filtered z
    ctx.frame_set_filter()
    shots[2].as_frame(ctx)
    ctx.keyframe_attach_frame(2)
    ctx.frame_set_filter(0)
    f = ctx.keyframe_attachment(2)["z"].reshape(-1)
    assert same(f, ctx.frame_download(L.MAP_VERTEX)[:, 2]) and not same(f, shots[2].V[:, 2])
    # host arrays: the bits are taken as given, NaN payloads and a negative zero included
    z = np.random.default_rng(3).uniform(0.5, 4, (RC.CAM[5], RC.CAM[4])).astype(F32)
    zb = z.reshape(-1).view(np.uint32)
    zb[:4] = (0x7fc00000, 0xffc01234, 0x80000000, 0x7f800000)
    rgba = np.random.default_rng(4).integers(0, 256, (RC.CAM[5], RC.CAM[4], 4)).astype(np.uint8)
    cam = (150.25, 149.5, 80.125, 59.75, RC.CAM[4], RC.CAM[5])
    ctx.keyframe_attach(2, z, rgba, cam)                                                  # replaces the filtered frame
    g = ctx.keyframe_attachment(2)
    assert np.array_equal(g["z"].view(np.uint32), z.view(np.uint32)) and np.array_equal(g["rgba"], rgba) and g["cam"] == cam
    ctx.keyframe_attach(2, z, None, cam)                                                  # ... and again, without colour
    assert ctx.keyframe_attachment(2)["rgba"] is None
    # wrong size, bad ids
    assert code_of(ctx.keyframe_attach, 0, np.zeros((60, 80), F32), None, (100, 100, 40, 30, 80, 60)) == L.RPE_ERR_ARG
    ctx.frame_set_depth(np.ones((60, 80), F32), (100, 100, 40, 30, 80, 60))
    assert code_of(ctx.keyframe_attach_frame, 0) == L.RPE_ERR_ARG
    for bad in (-1, 3):
        assert code_of(ctx.keyframe_attach_frame, bad) == L.RPE_ERR_ARG and code_of(ctx.keyframe_attach, bad, z, None, RC.CAM) == L.RPE_ERR_ARG
        assert code_of(ctx.keyframe_attachment, bad) == L.RPE_ERR_ARG
    assert code_of(ctx.keyframe_attach, 0, z, None, (0.0, 100, 40, 30, RC.CAM[4], RC.CAM[5])) == L.RPE_ERR_ARG
    assert same(ctx.keyframe_attachment(0)["z"], a["z"])                                  # the refused calls changed nothing
    # the download's own state errors
    out = np.empty(RC.CAM[4] * RC.CAM[5] * 4, np.uint8)
    assert L.lib().rpe_keyframe_attachment_download(ctx._h, 1, None, out.ctypes.data) == L.RPE_ERR_STATE   # depth but no colour
    # clearing the store drops the attachments: a new keyframe 0 carries nothing
    ctx.keyframes_clear()
    c.fill(ctx, upto=1)
    assert ctx.keyframe_attachment(0) == dict(z=None, rgba=None, cam=None)
    assert code_of(ctx.volume_fuse_keyframes) == L.RPE_ERR_STATE


def test_attachments_leave_the_graph_and_the_query_alone(gpu_ctx_factory):
    """link, optimize, query and relocalisation give the same bits with and without attachments"""
    plain, ctx, c = gpu_ctx_factory(), gpu_ctx_factory(), RC.case()
    q = c.room.queries[0]
    out = []
    for x, attach in ((plain, False), (ctx, True)):
        c.fill(x)
        if attach:
            for i, s in enumerate(RC.shots()):
                x.keyframe_attach(i, s.V[:, 2], s.rgba, s.cam)
        link = x.keyframes_link()
        poses, stats = x.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=True)
        q.as_frame(x)
        x.features_detect()
        counts, order = x.keyframes_query()
        out.append((link, poses, stats, counts, order, x.keyframe(5)["xw"]))
    a, b = out
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and same(a[5], b[5])


# ---------------------------------------------------------------------------------------------- 2. fuse = the sequential route
def check_fuse(rig, G, dims, kw, ids, poses=None, cull=True):
    """fuse(clear) of the rig's keyframes `ids`, depth only and with colour, against both references; returns the oracle's volumes"""
    ctx, seq, c = rig
    shots = RC.shots()
    at = [c.poses0[i] for i in ids] if poses is None else poses
    es = RC.entries(at, ids)
    ctx.volume_init(dims, **kw)
    out = None
    for color in (False, True):
        ctx.volume_fuse_keyframes(ids, poses, clear=True, color=color, cull=cull)
        got = ctx.volume_download()
        want, cwant = RO.fuse(None, None, G, es, RO.CLEAR | (RO.COLOR if color else 0))
        svol, scol = sequential(seq, dims, kw, [(shots[i], p) for i, p in zip(ids, at)], color)
        assert same(got, want) and same(got, svol), (ids, color)
        if color:
            gc = colour_of(ctx)
            assert same16(gc, cwant) and same16(gc, scol), ids
            out = want, cwant
    return out


@pytest.mark.parametrize("lst", list(RC.LISTS))
@pytest.mark.parametrize("volume", list(RC.VOLUMES))
def test_fuse_equals_the_sequential_route_and_the_oracle(rig, volume, lst):
    dims, s, o = RC.VOLUMES[volume]
    G, kw = RC.geometry(dims, s, o)
    want, cwant = check_fuse(rig, G, dims, kw, RC.LISTS[lst])
    assert (want[..., 1] > 0).any() and (cwant[..., 3] != 0).any()                      # something was fused, and coloured
    if volume != "two":
        assert (want[..., 1] == 0).any()                                                  # ... and something was left alone


def test_fuse_the_room_once(rig):
    G, dims, kw = RC.room()
    want, cwant = check_fuse(rig, G, dims, kw, RC.LISTS["all"])
    assert (want[..., 1] > 1).sum() > 10000 and (cwant[..., 3] != 0).sum() > 10000
    assert same(want, RC.fused("drifted"))                                                # the map of the figures, at the drifted poses


def test_the_weight_clamp_makes_the_order_matter(rig):
    ctx, seq, c = rig
    dims, s, o = RC.VOLUMES["odd"]
    G, kw = RC.geometry(dims, s, o, max_weight=3)
    ids = list(RC.LISTS["all"])
    fwd, _ = check_fuse(rig, G, dims, kw, ids)
    rev, _ = check_fuse(rig, G, dims, kw, ids[::-1])                                     # the reversed list = the reversed sequential route
    assert (fwd[..., 1] == 3).sum() > 100
    assert not same(fwd, rev)                                                             # ... and not the forward one


def test_a_repeated_id_and_the_default_list(rig, gpu_ctx_factory):
    dims, s, o = RC.VOLUMES["odd"]
    G, kw = RC.geometry(dims, s, o)
    once, _ = check_fuse(rig, G, dims, kw, [4, 1])
    twice, _ = check_fuse(rig, G, dims, kw, [4, 1, 4, 4])
    assert not same(once, twice)
    # ids = None: every keyframe with depth, by id -- keyframe 1 of this store has none
    ctx, c, shots = gpu_ctx_factory(), RC.case(), RC.shots()
    c.fill(ctx, upto=3)
    for i in (2, 0):
        ctx.keyframe_attach(i, shots[i].V[:, 2], shots[i].rgba, shots[i].cam)
    ctx.volume_init(dims, **kw)
    ctx.volume_fuse_keyframes(color=True)
    want, cwant = RO.fuse(None, None, G, RC.entries([c.poses0[0], c.poses0[2]], (0, 2)), RO.CLEAR | RO.COLOR)
    assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant)
    assert code_of(ctx.volume_fuse_keyframes, [0, 1, 2]) == L.RPE_ERR_STATE               # listed, but without depth


# ---------------------------------------------------------------------------------------------- 3. without CLEAR
def test_without_clear_the_uploaded_volume_is_the_start(rig):
    ctx, seq, c = rig
    shots = RC.shots()
    dims, s, o = RC.VOLUMES["odd"]
    G, kw = RC.geometry(dims, s, o, max_weight=5)
    start = random_start(G, 21)
    ids = RC.LISTS["three"]
    es = RC.entries([c.poses0[i] for i in ids], ids)
    pairs = [(shots[i], c.poses0[i]) for i in ids]
    for color in (True, False):
        ctx.volume_init(dims, **kw)
        ctx.volume_upload(start[0])
        ctx.volume_color_upload(start[1].view(np.float16))
        ctx.volume_fuse_keyframes(ids, clear=False, color=color)
        got, gcol = ctx.volume_download(), colour_of(ctx)
        want, cwant = RO.fuse(start[0], start[1], G, es, RO.COLOR if color else 0)
        svol, scol = sequential(seq, dims, kw, pairs, color, start)
        assert same(got, want) and same(got, svol), color
        assert same16(gcol, cwant) and same16(gcol, scol), color
        # what no keyframe updates keeps its uploaded bits, NaN payloads and all
        up = np.zeros(G.dim[::-1], bool)
        band = np.zeros(G.dim[::-1], bool)
        v, cv = start
        for e in es:
            v, cv, b = CO.integrate(v, cv, G, RO.as_map(e["z"]), e["rgba"], e["cam"], e["pose"], with_band=True)
            up |= VO.integrate(G.empty(), G, RO.as_map(e["z"]), e["cam"], e["pose"], with_mask=True)[1]
            band |= b
        assert 0 < up.sum() < up.size and 0 < band.sum() < up.sum()
        assert np.array_equal(got.view(np.uint32)[~up], start[0].view(np.uint32)[~up])
        assert np.array_equal(gcol[~band] if color else gcol, start[1][~band] if color else start[1])
    # without a colour volume, COLOR without CLEAR makes one, cleared, as the first colour integrate does
    ctx.volume_init(dims, **kw)
    ctx.volume_upload(start[0])
    ctx.volume_fuse_keyframes(ids, clear=False, color=True)
    want, cwant = RO.fuse(start[0], None, G, es, RO.COLOR)
    assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant)


# ---------------------------------------------------------------------------------------------- 4. the cull
def test_culling_changes_no_bit(rig, gpu_ctx_factory):
    ctx, seq, c = rig
    dims, s, o = RC.WIDE
    G, kw = RC.geometry(dims, s, o)
    ids = [0, 1, 2, 3]
    for poses in (None, RC.rolled_poses()):
        at = [c.poses0[i] for i in ids] if poses is None else poses
        want, cwant = RO.fuse(None, None, G, RC.entries(at, ids), RO.CLEAR | RO.COLOR)
        assert 0.3 < (want[..., 1] == 0).mean() < 1                                       # much of the volume is seen by nobody
        ctx.volume_init(dims, **kw)
        for cull in (True, False):
            ctx.volume_fuse_keyframes(ids, poses, clear=True, color=True, cull=cull)
            assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant), cull
        # ... nor without CLEAR, where a culled brick is not even loaded
        start = random_start(G, 5)
        want, cwant = RO.fuse(start[0], start[1], G, RC.entries(at, ids), RO.COLOR)
        for cull in (True, False):
            ctx.volume_upload(start[0])
            ctx.volume_color_upload(start[1].view(np.float16))
            ctx.volume_fuse_keyframes(ids, poses, clear=False, color=True, cull=cull)
            assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant), cull
    # a keyframe that sees none of the volume leaves an uploaded volume untouched, among others it changes nothing
    own, shots = gpu_ctx_factory(), RC.shots()
    c.fill(own, upto=2)
    for i in range(2):
        own.keyframe_attach(i, shots[i].V[:, 2], shots[i].rgba, shots[i].cam)
    start = random_start(G, 6)
    own.volume_init(dims, **kw)
    for cull in (True, False):
        own.volume_upload(start[0])
        own.volume_color_upload(start[1].view(np.float16))
        own.volume_fuse_keyframes([1], [RC.BLIND], clear=False, color=True, cull=cull)
        assert np.array_equal(own.volume_download().view(np.uint32), start[0].view(np.uint32)) and same16(colour_of(own), start[1])
    want, _ = RO.fuse(None, None, G, RC.entries([c.poses0[0]], [0]), RO.CLEAR)
    own.volume_fuse_keyframes([1, 0, 1], [RC.BLIND, c.poses0[0], RC.BLIND])
    assert same(own.volume_download(), want)
    own.volume_fuse_keyframes([1], [RC.BLIND])                                            # CLEAR and nothing seen: the cleared volume
    assert not own.volume_download().view(np.uint32).any()


# ---------------------------------------------------------------------------------------------- 5. mixed cameras, caller's poses
def test_two_cameras_in_one_list_at_the_callers_poses(gpu_ctx_factory):
    ctx, c = gpu_ctx_factory(), RC.case()
    store = KC.two_camera_store()[:4]
    holes = {}
    for i, (s, k) in enumerate(store):
        assert ctx.keyframe_add_host(k["xy"], k["desc"], k["xw"], k["nw"], c.poses0[i], s.w, s.h) == i
        holes[i] = s.V[:, 2].copy()
        holes[i][1000 * (i + 1):3000 * (i + 1)] = np.nan                                  # the closed room has no invalid depth: some here
        ctx.keyframe_attach(i, holes[i], s.rgba, s.cam)
    assert store[0][0].cam != store[1][0].cam
    dims, sz, o = RC.VOLUMES["odd"]
    G, kw = RC.geometry(dims, sz, o)
    ids = [3, 0, 1, 2]
    truth = [store[i][0].pose for i in ids]
    es = [dict(RC.entry(store[i][0], p), z=holes[i]) for i, p in zip(ids, truth)]
    ctx.volume_init(dims, **kw)
    ctx.volume_fuse_keyframes(ids, truth, color=True)
    want, cwant = RO.fuse(None, None, G, es, RO.CLEAR | RO.COLOR)
    assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant)
    assert all(np.array_equal(ctx.keyframe(i)["pose12"], c.poses0[i]) for i in range(4))  # the store's own poses are what they were
    ctx.volume_fuse_keyframes(ids, color=True)                                            # ... and what poses=None fuses at
    stored, _ = RO.fuse(None, None, G, [dict(RC.entry(store[i][0], c.poses0[i]), z=holes[i]) for i in ids], RO.CLEAR | RO.COLOR)
    assert same(ctx.volume_download(), stored) and not same(stored, want)


# ---------------------------------------------------------------------------------------------- 6. state
def test_state_rules_and_error_codes(gpu_ctx_factory):
    ctx, c, shots = gpu_ctx_factory(), RC.case(), RC.shots()
    dims, s, o = RC.VOLUMES["flat"]
    G, kw = RC.geometry(dims, s, o)
    c.fill(ctx, upto=3)
    for i in range(2):
        ctx.keyframe_attach(i, shots[i].V[:, 2], shots[i].rgba if i == 0 else None, shots[i].cam)
    assert code_of(ctx.volume_fuse_keyframes, [0]) == L.RPE_ERR_STATE                      # no volume
    ctx.volume_init(dims, **kw)
    assert code_of(ctx.volume_fuse_keyframes, [2]) == L.RPE_ERR_STATE                      # no depth
    assert code_of(ctx.volume_fuse_keyframes, [0, 1], color=True) == L.RPE_ERR_STATE       # keyframe 1 has no colour
    assert code_of(ctx.volume_fuse_keyframes, color=True) == L.RPE_ERR_STATE               # ... nor in the default list
    assert code_of(ctx.volume_fuse_keyframes, [3]) == L.RPE_ERR_ARG and code_of(ctx.volume_fuse_keyframes, [-1]) == L.RPE_ERR_ARG
    assert code_of(ctx.volume_fuse_keyframes, []) == L.RPE_ERR_ARG
    assert code_of(ctx.volume_fuse_keyframes, [0] * (L.MAX_KEYFRAMES + 1)) == L.RPE_ERR_ARG
    one = np.zeros(1, np.int32)
    assert L.lib().rpe_volume_fuse_keyframes(ctx._h, one.ctypes.data, 1, None, 8) == L.RPE_ERR_ARG   # an unknown flag bit
    assert L.lib().rpe_volume_fuse_keyframes(ctx._h, one.ctypes.data, 1, None, -1) == L.RPE_ERR_ARG
    assert not ctx.volume_download().any()                                                # the refused calls fused nothing
    ctx.volume_fuse_keyframes([0] * L.MAX_KEYFRAMES)                                      # the longest list there is
    want = G.empty()
    e = RC.entry(shots[0], c.poses0[0])
    for _ in range(L.MAX_KEYFRAMES):
        want = VO.integrate(want, G, RO.as_map(e["z"]), e["cam"], e["pose"])
    assert same(ctx.volume_download(), want)
    # the colour volume: made by CLEAR | COLOR with untouched voxels zero, dropped by CLEAR alone, as by volume_init
    ctx.volume_fuse_keyframes([0], color=True)
    want, cwant = RO.fuse(None, None, G, [e], RO.CLEAR | RO.COLOR)
    got = colour_of(ctx)
    assert same16(got, cwant) and not got[cwant[..., 3] == 0].any() and (cwant[..., 3] == 0).any()
    ctx.volume_fuse_keyframes([0, 1])
    assert code_of(ctx.volume_color_download) == L.RPE_ERR_STATE
    # the mesh: kept by a fuse without CLEAR, dropped by one with
    ctx.volume_fuse_keyframes([0], color=True)
    V, N, T = ctx.volume_mesh()
    assert len(T) > 0
    ctx.volume_fuse_keyframes([1], clear=False)
    again, tri = np.empty_like(V), np.empty_like(T)
    assert L.lib().rpe_volume_mesh_download(ctx._h, again.ctypes.data, None, tri.ctypes.data) == L.RPE_OK and same(again, V)
    assert len(ctx.volume_mesh_colors()) == len(V)
    ctx.volume_fuse_keyframes([0])
    assert L.lib().rpe_volume_mesh_download(ctx._h, again.ctypes.data, None, tri.ctypes.data) == L.RPE_ERR_STATE
    # the current frame and the model are not touched
    shots[2].as_frame(ctx)
    before = ctx.frame_download(L.MAP_VERTEX)
    ctx.volume_fuse_keyframes([0, 1])
    assert same(ctx.frame_download(L.MAP_VERTEX), before) and np.array_equal(ctx.frame_color(), shots[2].rgba)


# ---------------------------------------------------------------------------------------------- 7. the loop closes the map
def test_the_loop_closes_the_map(gpu_ctx_factory):
    ctx, c, shots = gpu_ctx_factory(), RC.case(), RC.shots()
    ids = c.fill(ctx)
    for i, s in zip(ids, shots):
        s.as_frame(ctx)
        ctx.keyframe_attach_frame(i)
    ctx.keyframes_link()
    ctx.keyframes_optimize(GC.GATES, GC.ANCHOR, apply=True)
    poses = [ctx.keyframe(i)["pose12"] for i in ids]
    assert all(VC.pose_error(p, q)[0] < 1e-6 and VC.pose_error(p, q)[1] < 1e-6 for p, q in zip(poses, c.loop[0]))
    G, dims, kw = RC.room()
    ctx.volume_init(dims, **kw)
    ctx.volume_fuse_keyframes(color=True)
    want, cwant = RO.fuse(None, None, G, RC.entries(poses), RO.CLEAR | RO.COLOR)
    assert same(ctx.volume_download(), want) and same16(colour_of(ctx), cwant)
    # the held-out view of the rebuilt map: the oracle's raycast of the same bits, and the CPU's figures for the optimised poses (the
    # GPU's poses are within 1e-6 rad / m of the oracle loop's, four orders below the figures)
    ctx.volume_raycast(VC.held_out_pose(), RC.CAM, *VC.RAY)
    MV = ctx.frame_download(L.MAP_MODEL_VERTEX)
    assert same(MV, VO.raycast(want, G, RC.CAM, VC.held_out_pose(), *VC.RAY)[0])
    hits, med, p90 = RC.held_out_figures(MV)
    fig, bad = RC.FIGURES["optimised"], RC.FIGURES["drifted"]
    print("rebuilt map:", (hits, med, p90), "CPU:", fig)
    assert abs(hits - fig[0]) <= 10 and med == pytest.approx(fig[1], rel=2e-2) and p90 == pytest.approx(fig[2], rel=2e-2)
    assert 5 * med < bad[1] and 4 * p90 < bad[2]
    V, N, T = ctx.volume_mesh()
    assert len(T) > 10000 and len(ctx.volume_mesh_colors()) == len(V)


def test_volume_rebuild_cpp(tmp_path):
    """DepthFrontEnd::attachFrame / fuseKeyframes from plain C++ (tests/cpp/volume_rebuild.cpp): attach, optimise, fuse, mesh"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_rebuild")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_rebuild.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "volume_rebuild: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
