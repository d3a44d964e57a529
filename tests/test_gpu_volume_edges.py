"""GPU parity of the TSDF volume and the mesh at their edges and at full size, against tests/volume_oracle.py and tests/mesh_oracle.py
(bit for bit unless noted): integrate's lane tails, integrate into uploaded volumes of awkward bits, every tie of
tests/volume_edge_cases.py on integrate and raycast, 640 x 480 and 641 x 479 frames on a 256^3 volume, the mesh scan past one chunk per
lane, a volume of more than 2^29 voxels checked window by window, and the refusal of a mesh of 2^31 or more vertices at 1024^3."""
import ctypes as C
import resource
import time

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
import volume_cases as VC
import volume_edge_cases as E
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12
from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
f32 = np.float32


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def maps(ctx):
    return ctx.frame_download(L.MAP_MODEL_VERTEX), ctx.frame_download(L.MAP_MODEL_NORMAL)


def assert_mesh(got, want):
    V, N, T = got
    Vo, No, To = want
    assert same(V, Vo) and same(N, No) and np.array_equal(T, To) and T.dtype == np.int32, (len(V), len(Vo), len(T), len(To))


def report(name, t0):
    rss = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20
    print(f"{name}: {time.perf_counter() - t0:.1f} s, peak RSS {rss:.2f} GiB")


# ---------------------------------------------------------------------------------------------------------------- integrate
def integrate_checked(ctx, G, before, depth, cam, p, rng, scale=1.0):
    """one frame into the context's volume (holding `before`); the result against the oracle under the rule of
    volume_edge_cases.integrate_matches; returns the downloaded volume and the oracle's mask"""
    ctx.frame_set_depth(depth, cam, scale, *rng)
    ctx.volume_integrate(p)
    got = ctx.volume_download()
    want, ok = VO.integrate(before, G, FO.frame_maps(depth, cam, scale, *rng)[0], cam, p, with_mask=True)
    assert E.integrate_matches(got, before, want, ok) == 0
    return got, ok


@pytest.mark.parametrize("start", ["zero", "awkward"])
@pytest.mark.parametrize("dims", E.TAIL_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_integrate_lane_tails(gpu_ctx_factory, dims, start):
    ctx = gpu_ctx_factory()
    G, desc, depth, p = E.tail_scene(dims)
    ctx.volume_init(dims, **desc)
    vol = G.empty() if start == "zero" else E.awkward(G, 7, int(G.W))
    ctx.volume_upload(vol)
    got, ok = integrate_checked(ctx, G, vol, depth, E.TAIL_CAM, p, E.TAIL_RANGE)
    assert ok.any() and not ok.all()
    if start == "zero":
        assert same(got, VO.integrate(vol, G, FO.frame_maps(depth, E.TAIL_CAM, 1.0, *E.TAIL_RANGE)[0], E.TAIL_CAM, p))
    # a second frame from another pose into the result
    p2 = pose12(np.eye(3), np.array([0.01, -0.02, 1.45]))
    integrate_checked(ctx, G, got, depth[::-1].copy(), E.TAIL_CAM, p2, E.TAIL_RANGE)


@pytest.mark.parametrize("max_weight", [1, 16])
def test_integrate_into_uploaded_awkward_volumes(gpu_ctx_factory, max_weight):
    """NaNs (quiet, signalling, payloads), +-Inf, -0, denormals; weights negative, -1, >= W, NaN: skipped voxels keep their bits, the
    unchanged half of a 16-byte pair included; updated voxels are the oracle's (NaN results compare as NaN)"""
    ctx = gpu_ctx_factory()
    dims = (37, 29, 43)
    G, desc, depth, p = E.tail_scene(dims, max_weight=max_weight, seed=1)
    ctx.volume_init(dims, **desc)
    vol = E.awkward(G, 11, max_weight)
    ctx.volume_upload(vol)
    got, ok = integrate_checked(ctx, G, vol, depth, E.TAIL_CAM, p, E.TAIL_RANGE)
    w = vol[..., 1]
    for kind in (np.isnan(w), w == -1, w >= max_weight, w < -1, np.isnan(vol[..., 0])):
        assert (ok & kind).sum() > 10 and (~ok & kind).sum() > 10
    assert np.all(got[..., 1][ok & np.isnan(w)] == G.W)                 # fminf: a NaN weight becomes W
    pairs = ok.reshape(-1)[: ok.size - ok.size % 2].reshape(-1, 2)
    assert (pairs[:, 0] != pairs[:, 1]).sum() > 10
    integrate_checked(ctx, G, got, depth, E.TAIL_CAM, p, E.TAIL_RANGE)


# ---------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("max_weight", [16, 1])
def test_integrate_ties(gpu_ctx_factory, max_weight):
    ctx = gpu_ctx_factory()
    G, desc, depth = E.integrate_ties(max_weight)
    ctx.volume_init(G.dim, **desc)
    got, _ = integrate_checked(ctx, G, G.empty(), depth, E.TIE_CAM, E.IDENTITY, E.TIE_RANGE)
    for name, ((i, j, k), want) in E.INTEGRATE_TIES.items():
        assert tuple(float(x) for x in got[k, j, i]) == ((0.0, 0.0) if want is None else want), name
    assert same(got, VO.integrate(G.empty(), G, FO.frame_maps(depth, E.TIE_CAM, 1.0, *E.TIE_RANGE)[0], E.TIE_CAM, E.IDENTITY))
    got2, _ = integrate_checked(ctx, G, got, depth, E.TIE_CAM, E.IDENTITY, E.TIE_RANGE)
    # and the raycast of the tie volume
    ctx.volume_raycast(E.IDENTITY, E.TIE_CAM, 0.125, 3.0)
    MV, MN = VO.raycast(got2, G, E.TIE_CAM, E.IDENTITY, 0.125, 3.0)
    gv, gn = maps(ctx)
    assert same(gv, MV) and same(gn, MN) and (~np.isnan(MV).any(1)).sum() > 10


@pytest.mark.parametrize("name", sorted(E.raycast_ties()))
def test_raycast_ties(gpu_ctx_factory, name):
    ctx = gpu_ctx_factory()
    G, vol, desc, cam, dmin, dmax, _ = E.raycast_ties()[name]
    ctx.volume_init(G.dim, **desc)
    ctx.volume_upload(vol)
    ctx.volume_raycast(E.IDENTITY, cam, dmin, dmax)
    MV, MN = VO.raycast(vol, G, cam, E.IDENTITY, dmin, dmax)
    gv, gn = maps(ctx)
    assert same(gv, MV) and same(gn, MN), name
    # the tie volume integrated by a frame of its own camera: integrate into an uploaded volume with exact samples
    depth = np.full((cam[5], cam[4]), 0.6, f32)
    integrate_checked(ctx, G, vol, depth, cam, E.IDENTITY, (0.05, 5.0, 10.0))


# ---------------------------------------------------------------------------------------------------------------- full size
REF_CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)
ODD_BIG_CAM = (590.5, 583.25, 321.3, 238.7, 641, 479)


@pytest.mark.parametrize("cam", [REF_CAM, ODD_BIG_CAM], ids=["640x480", "641x479"])
def test_full_size_frames_on_a_256_cube(gpu_ctx_factory, cam):
    """a u16 frame with holes in 0.2 mm units (depth_scale 0.0002) integrated into a 256^3 volume over the room, then raycast"""
    t0 = time.perf_counter()
    ctx = gpu_ctx_factory()
    s = 0.027
    G, desc = MC.geometry((256, 256, 256), s, (-2.8, -1.9, -1.6), trunc=3 * s, max_weight=64)
    ctx.volume_init(G.dim, **desc)
    rng = np.random.default_rng(4)
    vol = G.empty()
    for k in (0, 1):
        d = VC.depth_at(VC.view(k), cam, 0.002, rng).astype(np.float64)
        d16 = np.clip(np.round(d / 0.0002), 0, 65535).astype(np.uint16)
        d16.reshape(-1)[rng.integers(0, d16.size, d16.size // 20)] = 0
        vol, ok = integrate_checked(ctx, G, vol, d16, cam, VC.view(k), VC.RANGE, scale=0.0002)
        assert ok.sum() > 10 ** 5, ok.sum()
    ctx.volume_raycast(VC.held_out_pose(), cam, *VC.RAY)
    MV, MN = VO.raycast(vol, G, cam, VC.held_out_pose(), *VC.RAY)
    gv, gn = maps(ctx)
    assert same(gv, MV) and same(gn, MN)
    assert (~np.isnan(MV).any(1)).mean() > 0.7, (~np.isnan(MV).any(1)).mean()
    report(f"full size {cam[4]}x{cam[5]}", t0)


# ---------------------------------------------------------------------------------------------------------------- mesh chunks
def chunk_case(name):
    if name == "chunks_1024":
        return E.gyroid((256, 256, 64), seed=1)
    if name == "chunks_1025":
        return E.gyroid((256, 164, 100), seed=2)
    if name == "chunks_1031_odd":
        return E.gyroid((251, 251, 67), 7.0, seed=3)
    if name == "chunks_4096_sparse":
        return E.sparse_256()
    raise KeyError(name)


def vertex_chunks(V, G):
    """the chunk of each vertex's owner voxel: its coordinates along the two other axes are voxel centres (up to fp32 rounding), along
    the edge's axis it lies in [i + 0.5, i + 1.5] voxel units (the owner's index i, but for t within 1e-3 of 1)"""
    g = (V.astype(np.float64) - G.o.astype(np.float64)) / float(G.s) - 0.5
    r = np.round(g)
    g = np.where(np.abs(g - r) < 1e-3, r, np.floor(g)).astype(np.int64)
    flat = (g[:, 2] * G.dim[1] + g[:, 1]) * G.dim[0] + g[:, 0]
    return flat // E.CHUNK


@pytest.mark.parametrize("name", ["chunks_1024", "chunks_1025", "chunks_1031_odd", "chunks_4096_sparse"])
def test_mesh_chunk_counts(gpu_ctx_factory, name):
    t0 = time.perf_counter()
    ctx = gpu_ctx_factory()
    G, vol, desc = chunk_case(name)
    ctx.volume_init(G.dim, **desc)
    ctx.volume_upload(vol)
    got = ctx.volume_mesh(1.0)
    assert_mesh(got, MO.mesh(vol, G, 1.0))
    V, _, T = got
    nchunks = -(-int(np.prod(G.dim)) // E.CHUNK)
    ch = vertex_chunks(V, G)
    assert ch.min() == 0 and ch.max() == nchunks - 1, (ch.min(), ch.max(), nchunks)
    tc = ch[T]
    assert ((tc[:, 0] != tc[:, 1]) | (tc[:, 1] != tc[:, 2])).sum() > 10        # triangles across chunk boundaries
    report(name, t0)


def test_mesh_of_the_room_at_25mm_2089_chunks(gpu_ctx_factory):
    t0 = time.perf_counter()
    ctx = gpu_ctx_factory()
    dims, desc = VC.room_geometry(0.025, 64)
    assert dims == (228, 140, 268)
    ctx.volume_init(dims, **desc)
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    want = G.empty()
    for k in (0, 1):
        d = VC.depth_at(VC.view(k), SMALL_CAM)
        ctx.frame_set_depth(d, SMALL_CAM, 1.0, *VC.RANGE)
        ctx.volume_integrate(VC.view(k))
        want = VO.integrate(want, G, FO.frame_maps(d, SMALL_CAM, 1.0, *VC.RANGE)[0], SMALL_CAM, VC.view(k))
    assert same(ctx.volume_download(), want)
    got = ctx.volume_mesh(1.0)
    assert_mesh(got, MO.mesh(want, G, 1.0))
    assert len(got[2]) > 10000
    report("room at 25 mm", t0)


# ---------------------------------------------------------------------------------------------------------------- large volume
def large_frame(zc, depth=0.1):
    """a 640 x 480 camera (f = 30) at (4, 4, zc) looking along +z at a plane `depth` in front of it: the voxels it can update have
    camera z in (0, depth + tr], so slabs more than a few voxels away are skipped"""
    cam = (30.0, 30.0, 319.5, 239.5, 640, 480)
    d = np.full((480, 640), depth, f32)
    d[::5, ::3] = 0
    return cam, d, pose12(np.eye(3), np.array([-4.0, -4.0, -zc]))


def test_large_volume_windows(gpu_ctx_factory):
    """1024 x 1024 x 544 voxels (more than 2^29, byte offsets past 2^31 and 2^32): analytic content in windows straddling k = 256,
    k = 512 and in the last slabs, weight 0 elsewhere.  The mesh against the windowed oracle, a raycast into each window, and one
    frame per window integrated and compared slab range by slab range (every voxel outside it bitwise unchanged)."""
    t0 = time.perf_counter()
    ctx = gpu_ctx_factory()
    G, desc = E.large_geometry()
    d0, d1, d2 = G.dim
    ctx.volume_init(G.dim, **desc)
    vol = np.zeros((d2, d1, d0, 2), f32)
    windows = []
    for n, (k0, k1) in enumerate(E.LARGE_WINDOWS):
        vol[k0:k1] = E.large_window(G, k0, k1, n)
        windows.append((k0, vol[k0:k1]))
    ctx.volume_upload(vol)
    # the mesh, window by window
    V, N, T = ctx.volume_mesh(1.0)
    id0, parts = 0, []
    for k0, slab in windows:
        parts.append(MO.mesh(slab, G, 1.0, k0, id0))
        id0 += len(parts[-1][0])
        assert len(parts[-1][0]) > 10 ** 5
    assert len(V) == id0
    assert same(V, np.concatenate([p[0] for p in parts])) and same(N, np.concatenate([p[1] for p in parts]))
    assert np.array_equal(T, np.concatenate([p[2] for p in parts]))
    del V, N, T, parts
    # a raycast into each window from 0.5 m in front of it, rays through the window and out of its far side
    cam = (40.0, 40.0, 79.5, 59.5, 160, 120)
    for k0, k1 in E.LARGE_WINDOWS:
        zc = k0 * float(G.s) - 0.5
        p = pose12(np.eye(3), np.array([-4.0, -4.0, -zc]))
        rng = (0.45, 0.5 + (k1 - k0 + 8) * float(G.s))
        ctx.volume_raycast(p, cam, *rng)
        MV, MN = VO.raycast(windows, G, cam, p, *rng)
        gv, gn = maps(ctx)
        assert same(gv, MV) and same(gn, MN), (k0, k1)
        assert (~np.isnan(MV).any(1)).mean() > 0.5
    # integrate: one frame near each window; the oracle over the slabs the frame can reach, the rest unchanged
    before = vol
    del vol, windows
    for zc, (a, b) in ((256 * float(G.s) - 0.06, (240, 272)), (512 * float(G.s) - 0.06, (496, 528)), (4.19, (528, 544))):
        cam, depth, p = large_frame(zc)
        ctx.frame_set_depth(depth, cam, 1.0, 0.01, 10.0, 0.1)
        ctx.volume_integrate(p)
        got = ctx.volume_download()
        want, ok = VO.integrate(before[a:b], G, FO.frame_maps(depth, cam, 1.0, 0.01, 10.0, 0.1)[0], cam, p, a, with_mask=True)
        assert ok.sum() > 10 ** 4 and not ok[0].any() and (b == d2 or not ok[-1].any())
        assert E.integrate_matches(got[a:b], before[a:b], want, ok) == 0, (a, b)
        for lo in range(0, d2, 32):
            hi = min(d2, lo + 32)
            keep = [(x, y) for x, y in ((lo, min(hi, a)), (max(lo, b), hi)) if x < y]
            for x, y in keep:
                assert np.array_equal(got[x:y].view(np.uint32), before[x:y].view(np.uint32)), (x, y)
        del before
        before = got
    report("large volume 1024x1024x544", t0)


# ---------------------------------------------------------------------------------------------------------------- maximum volume
def test_max_volume_checkerboard_refuses_the_mesh(gpu_ctx_factory):
    """1024^3 checkerboard: 3 * 1023 * 1024^2 = 3 218 079 744 vertices, more than int32 ids hold: RPE_ERR_ARG with that count, no mesh
    left behind; the same context then re-inits to smaller dims and extracts bit-exact"""
    t0 = time.perf_counter()
    ctx = gpu_ctx_factory()
    dims = (1024, 1024, 1024)
    ctx.volume_init(dims, voxel_size=0.01, origin=(0.0, 0.0, 0.0), trunc=0.03, max_weight=4)
    vol = E.checkerboard(dims)
    ctx.volume_upload(vol)
    del vol
    nv, _ = E.checkerboard_counts(dims)
    assert nv == 3218079744
    with pytest.raises(L.RpeError) as e:
        ctx.volume_mesh(1.0)
    assert e.value.code == L.RPE_ERR_ARG and f"{nv} vertices" in str(e.value), str(e.value)
    buf = np.zeros(64, f32)
    lib = L.lib()
    assert lib.rpe_volume_mesh_download(ctx._h, buf.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p)) == L.RPE_ERR_STATE
    for case in (MC.sphere, lambda: MC.noise((41, 33, 30), 3)):
        G, v, desc = case()
        ctx.volume_init(G.dim, **desc)
        ctx.volume_upload(v)
        assert_mesh(ctx.volume_mesh(1.0), MO.mesh(v, G, 1.0))
    small = (6, 5, 4)
    G, desc = MC.geometry(small, 0.1, (0, 0, 0))
    ctx.volume_init(small, **desc)
    ctx.volume_upload(E.checkerboard(small))
    V, _, T = ctx.volume_mesh(1.0)
    assert (len(V), len(T)) == E.checkerboard_counts(small)
    report("max volume 1024^3", t0)
