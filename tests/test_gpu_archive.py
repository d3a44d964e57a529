"""GPU: the volume archive (csrc/rpe_archive.hip, rpe_archive_api.hip, the hook in rpe_shift_api.hip) held BIT FOR BIT to
tests/archive_oracle.py: round trips over small windows with every kind of shift, with and without a colour volume, over arbitrary
content and over bricks whose only non-zero word is a -0, a colour half-word or a tsdf of weight 0; a random walk with uploads and
integrates in between; the capacity rules; preconditions and lifetimes; the archive off; and the use case of tests/archive_cases.py
-- a walk out and back whose return leg finds the map it left."""
import numpy as np
import pytest

import archive_cases as AC
import archive_oracle as AO
import rebuild_cases as RC
import shift_cases as SC
import shift_oracle as SO
import volume_cases as VC
from frontend_util import SMALL_CAM
from rgbd_pose_estimation_amd import _lib as L
from test_gpu_rebuild import code_of, random_start, same16

pytestmark = pytest.mark.gpu
F32 = np.float32
WINDOWS = [(8, 8, 8), (16, 8, 8), (24, 16, 8), (16, 16, 16), (32, 24, 16)]
PLANTS = ("negative zero", "weight zero", "colour half-word")


def bits(a, b):
    """bit for bit, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def all_bricks(dims):
    return AO.bricks_in([((0, 0, 0), AO.bricks_of(dims))])


def plant(vol, cvol, b, kind):
    """brick b becomes all zero but for ONE word"""
    AO._cut(vol, b)[...] = 0
    AO._cut(cvol, b)[...] = 0
    if kind == "negative zero":
        AO._cut(vol.view(np.uint32), b)[7, 7, 7, 0] = 0x80000000          # a -0 tsdf in the brick's last voxel
    elif kind == "weight zero":
        AO._cut(vol, b)[2, 5, 3, 0] = 0.375                               # a tsdf whose weight is 0
    else:
        AO._cut(cvol, b)[0, 0, 0, 2] = 0x3c00                              # one colour half-word in its first voxel


def contents(dims, colour, seed):
    """[(volume, colour volume)]: random_start with a random third of the bricks zeroed and the planted bricks among those; windows with
    fewer than three zeroed bricks get the plants that are left one by one, each alone in an empty window"""
    G, _ = RC.geometry(dims, 0.03, (-0.7, 0.3, 1.1), max_weight=16)
    rng = np.random.default_rng(seed)
    vol, cvol = random_start(G, seed)
    bricks = all_bricks(dims)
    zeroed = [bricks[i] for i in rng.permutation(len(bricks))[:len(bricks) // 3]]
    for b in zeroed:
        AO._cut(vol, b)[...] = 0
        AO._cut(cvol, b)[...] = 0
    kinds = [k for k in PLANTS if colour or k != "colour half-word"]
    for b, k in zip(zeroed, list(kinds)):
        plant(vol, cvol, b, k)
        kinds.remove(k)
    out = [(vol, cvol)]
    for k in kinds:
        v, c = np.zeros_like(vol), np.zeros_like(cvol)
        plant(v, c, bricks[-1], k)
        out.append((v, c))
    return out


def shifts_for(dims):
    out = [(8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8), (8, -8, 16)]
    for a in range(3):
        for m in (dims[a], dims[a] + 8):
            d = [0, 0, 0]
            d[a] = m if a != 1 else -m
            out.append(tuple(d))
    return out + [tuple(dims)]


def init(ctx, dims, origin=(-0.7, 0.3, 1.1), voxel=0.03):
    G, kw = RC.geometry(dims, voxel, origin, max_weight=16)
    ctx.volume_init(dims, **kw)
    return G, kw


def archive_equals(ctx, store):
    """archive_info and archive_download against the store model"""
    coords, tsdf, col = ctx.volume_archive_download()
    oc, ot, ocol = AO.download(store)
    col = np.zeros(ocol.shape, np.uint16) if col is None else col
    return ctx.volume_archive_info()["held"] == len(store) and coords.dtype == np.int64 and np.array_equal(coords, oc) and bits(tsdf, ot) \
        and same16(col, ocol)


def window_equals(ctx, vol, cvol, total):
    return bits(ctx.volume_download(), vol) and (cvol is None or same16(ctx.volume_color_download(), cvol)) \
        and np.array_equal(ctx.volume_geometry()["total_shift"], total)


# ---------------------------------------------------------------------------------------------- 1. round trips
@pytest.mark.parametrize("colour", (False, True), ids=("tsdf", "colour"))
@pytest.mark.parametrize("dims", WINDOWS, ids=lambda d: "x".join(map(str, d)))
def test_round_trips(gpu_ctx_factory, dims, colour):
    ctx = gpu_ctx_factory()
    init(ctx, dims)
    for n, (vol, cvol) in enumerate(contents(dims, colour, sum(dims) + colour)):
        cvol = cvol if colour else None
        ctx.volume_upload(vol)
        if colour:
            ctx.volume_color_upload(cvol.view(np.float16))
        ctx.volume_archive(len(all_bricks(dims)))
        for d in shifts_for(dims):
            store = {}
            a, ca, tot = AO.shift(vol, cvol, (0, 0, 0), d, store)
            ctx.volume_shift(d)
            assert window_equals(ctx, a, ca, tot) and archive_equals(ctx, store), (n, d)
            back = tuple(-x for x in d)
            b, cb, tot = AO.shift(a, ca, tot, back, store)
            ctx.volume_shift(back)
            assert store == {} and bits(b, vol) and window_equals(ctx, vol, cvol, (0, 0, 0)), (n, d)
            assert ctx.volume_archive_info() == dict(held=0, capacity=len(all_bricks(dims))), (n, d)
    if not colour:                                                   # none comes into being
        assert code_of(ctx.volume_color_download) == L.RPE_ERR_STATE


# ---------------------------------------------------------------------------------------------- 2. a random walk
def test_a_random_walk(gpu_ctx_factory):
    """only data movement is compared: before every shift the oracle is handed the GPU's own window"""
    ctx = gpu_ctx_factory()
    dims = (24, 16, 8)
    G, kw = init(ctx, dims, origin=(-1.3, -0.9, 4.5), voxel=0.11)    # across the room's back wall (z = 5)
    vol, cvol = random_start(G, 21)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    ctx.volume_archive(4096)
    pose = VC.view(0)
    ctx.frame_set_depth(VC.depth_at(pose, SMALL_CAM), SMALL_CAM, 1.0, *VC.RANGE)
    rng = np.random.default_rng(22)
    total, store, peak, fused, returned = (0, 0, 0), {}, 0, 0, 0
    for step in range(30):
        if step % 4 == 0:                                            # new evidence between shifts
            before = ctx.volume_download()
            ctx.volume_integrate(pose)
            fused += not bits(before, ctx.volume_download())
        elif step % 7 == 3:
            ctx.volume_upload(random_start(G, 100 + step)[0])
        vol, cvol = ctx.volume_download(), ctx.volume_color_download().view(np.uint16)
        to = rng.integers(-2, 3, 3)                                  # the window wanders over 5 x 5 x 5 bricks: it comes back often
        d = tuple(int(8 * x - t) for x, t in zip(to, total))
        held = set(store)
        vol, cvol, total = AO.shift(vol, cvol, total, d, store)
        returned += len(held - set(store))
        ctx.volume_shift(d)
        peak = max(peak, len(store))
        assert window_equals(ctx, vol, cvol, total), (step, d)
        assert ctx.volume_archive_info()["held"] == len(store), (step, d)
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store)
    assert fused >= 1 and peak >= 12 and returned >= 30, (fused, peak, returned)


# ---------------------------------------------------------------------------------------------- 3. capacity
def test_capacity(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    dims = (24, 16, 8)                                               # 3 x 2 x 1 bricks, every one non-zero
    G, kw = init(ctx, dims)
    vol, cvol = random_start(G, 31)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    ctx.volume_archive(3)
    assert ctx.volume_archive_info() == dict(held=0, capacity=3)
    store = {}
    vol, cvol, total = AO.shift(vol, cvol, (0, 0, 0), (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))                                      # two bricks leave: one slot is left
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and len(store) == 2
    ctx.volume_upload(vol + 1)                                       # the entering slab is no longer zero
    vol = vol + 1
    geometry = ctx.volume_geometry()
    with pytest.raises(L.RpeError) as e:
        ctx.volume_shift((8, 0, 0))
    assert e.value.code == L.RPE_ERR_STATE and " 2 free slots" in str(e.value) and "has 1 " in str(e.value), str(e.value)
    after = ctx.volume_geometry()
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and np.array_equal(geometry["origin"], after["origin"])
    assert ctx.volume_archive_info() == dict(held=2, capacity=3)
    # a shift that frees slots by what enters still needs free slots BEFORE: (-8) brings two back and pushes two out
    assert code_of(ctx.volume_shift, (-8, 0, 0)) == L.RPE_ERR_STATE and window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store)
    # below held: RPE_ERR_ARG; growing keeps the content and the same shift then succeeds
    assert code_of(ctx.volume_archive, 1) == L.RPE_ERR_ARG and code_of(ctx.volume_archive, -1) == L.RPE_ERR_ARG
    ctx.volume_archive(8)
    assert ctx.volume_archive_info() == dict(held=2, capacity=8) and archive_equals(ctx, store) and window_equals(ctx, vol, cvol, total)
    ctx.volume_archive(2)                                            # between held and the capacity: nothing changes
    assert ctx.volume_archive_info() == dict(held=2, capacity=8)
    vol, cvol, total = AO.shift(vol, cvol, total, (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and len(store) == 4
    vol, cvol, total = AO.shift(vol, cvol, total, (-16, 0, 0), store)
    ctx.volume_shift((-16, 0, 0))                                    # four return; of the four that leave two are all zero
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and len(store) == 2 and total == (0, 0, 0)
    # clear: nothing held, the pool stays; what would have returned does not
    ctx.volume_archive_clear()
    assert ctx.volume_archive_info() == dict(held=0, capacity=8) and archive_equals(ctx, {})
    store = {}
    vol, cvol, total = AO.shift(vol, cvol, total, (16, 0, 0), store)
    ctx.volume_shift((16, 0, 0))
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and not vol[:, :, 8:].any()
    # capacity 0 switches it off: the next shift behaves as without an archive, odd shifts included
    ctx.volume_archive(0)
    assert ctx.volume_archive_info() == dict(held=0, capacity=0) and archive_equals(ctx, {})
    for d in ((-16, 0, 0), (3, -1, 2)):
        ctx.volume_shift(d)
        vol, cvol = SO.shift(vol, cvol, d)
        total = tuple(t + x for t, x in zip(total, d))
        assert window_equals(ctx, vol, cvol, total), d
    assert not vol[:, :, :13].any()                                  # nothing came back


# ---------------------------------------------------------------------------------------------- 4. preconditions and lifetimes
def test_preconditions_and_lifetimes(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    assert code_of(ctx.volume_archive, 4) == L.RPE_ERR_STATE         # no volume
    assert ctx.volume_archive_info() == dict(held=0, capacity=0)
    ctx.volume_archive(0).volume_archive_clear()                     # off stays off
    init(ctx, (20, 16, 8))
    assert code_of(ctx.volume_archive, 4) == L.RPE_ERR_STATE         # a dim that is no multiple of 8
    dims = (24, 16, 8)
    G, kw = init(ctx, dims)
    ctx.volume_shift((4, 0, 0))
    assert code_of(ctx.volume_archive, 4) == L.RPE_ERR_STATE and ctx.volume_archive_info() == dict(held=0, capacity=0)   # the total
    ctx.volume_shift((4, 0, 0))
    ctx.volume_archive(16)                                           # total (8, 0, 0)
    vol, cvol = random_start(G, 41)
    ctx.volume_upload(vol)
    total = (8, 0, 0)
    for d in ((4, 0, 0), (8, 0, -1), (0, 12, 0)):                    # a shift that is no multiple of 8: RPE_ERR_ARG, nothing changed
        assert code_of(ctx.volume_shift, d) == L.RPE_ERR_ARG and window_equals(ctx, vol, None, total) and archive_equals(ctx, {}), d
    ctx.volume_shift((0, 0, 0))                                      # a zero shift changes nothing
    assert window_equals(ctx, vol, None, total) and archive_equals(ctx, {})
    # a colour volume that comes into being after bricks were archived: those restore zero colour, later ones their colour
    store = {}
    vol, _, total = AO.shift(vol, None, total, (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))
    assert archive_equals(ctx, store) and len(store) == 2 and ctx.volume_archive_download()[2] is None
    cvol = cvol.copy()
    ctx.volume_color_upload(cvol.view(np.float16))
    vol, cvol, total = AO.shift(vol, cvol, total, (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and len(store) == 4
    col = ctx.volume_archive_download()[2].view(np.uint16)
    assert not col[[0, 2]].any() and col[[1, 3]].any()               # sorted (bz, by, bx): bx = 1 left first, without colour
    vol, cvol, total = AO.shift(vol, cvol, total, (-16, 0, 0), store)
    ctx.volume_shift((-16, 0, 0))
    assert window_equals(ctx, vol, cvol, total) and archive_equals(ctx, store) and len(store) == 2   # colour alone keeps a brick
    assert not cvol[:, :, :8].any() and cvol[:, :, 8:16].any() and vol[:, :, :8].any()
    # volume_init drops the archive: nothing is held, nothing returns, and it is off
    ctx.volume_shift((8, 0, 0))
    assert ctx.volume_archive_info()["held"] > 0
    init(ctx, dims)
    assert ctx.volume_archive_info() == dict(held=0, capacity=0)
    ctx.volume_shift((-8, 0, 0)).volume_shift((5, 0, 0))             # off: any shift, and the window stays empty
    assert not ctx.volume_download().view(np.uint32).any()


def test_a_rebuild_does_not_touch_the_archive_and_a_window_without_colour_archives_zero_colour(gpu_ctx_factory):
    """rpe_volume_fuse_keyframes leaves the archive alone; with RPE_FUSE_CLEAR and without RPE_FUSE_COLOR it drops the colour volume,
    and a brick that then leaves into a slot that has held colour restores all-zero colour"""
    ctx, c = gpu_ctx_factory(), RC.case()
    for i, s in zip(c.fill(ctx), RC.shots()):
        s.as_frame(ctx)
        ctx.keyframe_attach_frame(i)
    dims, (_, voxel, origin) = (40, 32, 24), RC.VOLUMES["odd"]
    G, kw = init(ctx, dims, origin, voxel)
    vol, cvol = random_start(G, 51)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    ctx.volume_archive(32)
    store = {}
    a, ca, total = AO.shift(vol, cvol, (0, 0, 0), (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))
    assert window_equals(ctx, a, ca, total) and archive_equals(ctx, store) and len(store) == 12
    ctx.volume_fuse_keyframes(list(RC.LISTS["three"]), clear=True, color=False)
    assert archive_equals(ctx, store) and code_of(ctx.volume_color_download) == L.RPE_ERR_STATE
    rebuilt = ctx.volume_download()
    assert (rebuilt[..., 1] > 0).sum() > 1000
    # back: the archived slab returns (its tsdf; the window has no colour), the rebuilt window's last slab leaves into free slots
    b, _, total = AO.shift(rebuilt, None, total, (-8, 0, 0), store)
    ctx.volume_shift((-8, 0, 0))
    assert window_equals(ctx, b, None, total) and archive_equals(ctx, store) and bits(b[:, :, :8], vol[:, :, :8])
    # out again: the slab leaves into the slots that held its colour, now with zero colour
    b2, _, total = AO.shift(b, None, total, (8, 0, 0), store)
    ctx.volume_shift((8, 0, 0))
    assert window_equals(ctx, b2, None, total) and archive_equals(ctx, store)
    held = ctx.volume_archive_info()["held"]
    assert held >= 12 and ctx.volume_archive_download()[2] is None
    ctx.volume_archive_clear()
    ctx.volume_shift((-8, 0, 0))
    assert not ctx.volume_download()[:, :, :8].view(np.uint32).any()


# ---------------------------------------------------------------------------------------------- 5. the archive off
def test_archive_off_is_the_plain_shift(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    dims = (24, 16, 8)
    G, kw = init(ctx, dims)
    vol, cvol = random_start(G, 61)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    total = np.zeros(3, np.int64)
    for d in shifts_for(dims)[:8] + [(-8, 0, 0), (3, -2, 1), (24, 0, 0), (-24, 0, 0)]:
        ctx.volume_shift(d)
        vol, cvol = SO.shift(vol, cvol, d)
        total += d
        assert window_equals(ctx, vol, cvol, total), d
        assert ctx.volume_archive_info() == dict(held=0, capacity=0)
        ctx.volume_upload(vol + 1)
        vol = vol + 1
    assert ctx.volume_archive_download()[0].shape == (0, 3)


# ---------------------------------------------------------------------------------------------- 6. the use case
@pytest.mark.parametrize("archive", (True, False), ids=("archive", "plain"))
def test_the_walk_out_and_back(gpu_ctx_factory, archive):
    """tests/archive_cases.py through the API: the oracle's hit counts on the return leg and its final window, bit for bit"""
    ctx = gpu_ctx_factory()
    ctx.volume_init(AC.DIMS, **SC.desc())
    if archive:
        ctx.volume_archive(AC.CAPACITY)
    got, peak, moved = [], 0, np.zeros(3, np.int64)
    for n in range(len(AC.PATH)):
        p = AC.pose(n)
        if n:
            sh = ctx.volume_follow(p, SC.LOOK_AHEAD, AC.GRANULE)
            if sh.any():
                ctx.volume_shift(sh)
                moved += sh
                peak = max(peak, ctx.volume_archive_info()["held"])
            if n in AC.RETURN:
                ctx.volume_raycast(p, AC.CAM, *SC.RAY)
                h, m = AC.hits(ctx.frame_download(L.MAP_MODEL_VERTEX), n)
                got.append(h)
                assert m == AC.PIXELS
        ctx.frame_set_depth(AC.depth(n), AC.CAM, 1.0, *SC.RANGE)
        ctx.volume_integrate(p)
    vol = ctx.volume_download()
    want, digest = (AC.HITS_ARCHIVE, AC.DIGEST_ARCHIVE) if archive else (AC.HITS_PLAIN, AC.DIGEST_PLAIN)
    print(f"{'archive' if archive else 'plain'}: hits on the return leg {got}; peak {peak} bricks; mean weight {vol[..., 1].mean():.4f}; "
          f"the window ends at {tuple(moved)}")
    assert got == want, (got, want)
    assert AC.digest(vol) == digest
    assert peak == (AC.PEAK_HELD if archive else 0)
    if archive:                                                      # one slot fewer and the walk does not fit
        assert ctx.volume_archive_info()["capacity"] == AC.PEAK_IN_FLIGHT
    assert got[-1] >= AC.GAIN_LIMIT * AC.HITS_PLAIN[-1] if archive else got[-1] == AC.HITS_PLAIN[-1]
