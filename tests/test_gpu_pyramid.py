"""GPU parity of the coarse-to-fine pyramids (F1p / F2p of csrc/rpe_frontend.hip, rpe_icp_pyramid) against tests/pyramid_oracle.py.
Maps of every level are BIT-EXACT; the pyramid ICP returns the same bits as the chained single-level calls it stands for, and one
level of it is rpe_icp."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyramid_oracle as PO
from frontend_util import FO, SMALL_CAM, oracle_icp, pose12, rot, two_views
from rgbd_pose_estimation_amd import _lib as L, api, simulator as S
from util import rot_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_CAM = S.DEFAULT_CAMERA
ODD_CAM = (100.0, 90.0, 18.3, 11.1, 37, 23)
RANGE = (0.1, 10.0, 0.1)   # dmin, dmax, max_jump
MOTION = (0.02, -0.015, 0.01, 0.03, -0.02, 0.025)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def max_levels(cam):
    return max(l for l in range(1, L.MAX_LEVELS + 1) if cam[4] >> (l - 1) >= 1 and cam[5] >> (l - 1) >= 1)


def set_pyramid(ctx, depth, cam, scale, levels, rng=RANGE):
    """rpe_frame_set_depth_pyramid at any level count (Context.frame_set_depth takes levels = 1 to rpe_frame_set_depth)."""
    d = np.ascontiguousarray(depth)
    kind = L.DEPTH_U16 if d.dtype == np.uint16 else L.DEPTH_F32
    k = ctx._camera(cam)
    L.check(L.lib().rpe_frame_set_depth_pyramid(ctx._h, d.ctypes.data_as(C.c_void_p), kind, C.byref(k), scale, *rng, levels))
    ctx._pixels = cam[4] * cam[5]


def holes(depth, rng, frac=0.03):
    d = depth.copy()
    idx = rng.integers(0, d.size, int(frac * d.size))
    d.reshape(-1)[idx] = 0
    return d


@pytest.mark.parametrize("cam,u16", [(SMALL_CAM, False), (SMALL_CAM, True), (FULL_CAM, True), (FULL_CAM, False), (ODD_CAM, False), (ODD_CAM, True)])
def test_frame_pyramid_bit_exact(gpu_ctx_factory, cam, u16):
    rng = np.random.default_rng(11)
    depth = holes(S.render_depth(rot(0.05, -0.1, 0.02), np.array([0.1, -0.05, 0.2]), cam, noise_sigma=0.004, rng=rng, as_u16=u16), rng)
    scale = 0.001 if u16 else 1.0
    ctx = gpu_ctx_factory()
    ref = gpu_ctx_factory().frame_set_depth(depth, cam, scale, *RANGE)    # the single-level front end
    V0 = [ref.frame_download(m) for m in (L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING)]
    for levels in range(1, max_levels(cam) + 1):
        set_pyramid(ctx, depth, cam, scale, levels)
        want = PO.frame_pyramid(depth, cam, scale, *RANGE, levels)
        for l, (z, V, N, B) in enumerate(want):
            assert same(ctx.frame_download(L.MAP_DEPTH, l), z.reshape(-1)), (levels, l)
            assert same(ctx.frame_download(L.MAP_VERTEX, l), V), (levels, l)
            assert same(ctx.frame_download(L.MAP_NORMAL, l), N), (levels, l)
            assert same(ctx.frame_download(L.MAP_BEARING, l), B), (levels, l)
            assert ctx.frame_camera(l) == PO.level_camera(cam, l)
        for m, ref_map in zip((L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING), V0):
            assert same(ctx.frame_download(m), ref_map)
        if cam[4] >= 160 and levels >= 2:
            assert 0.2 < (~np.isnan(want[1][2]).any(1)).mean() < 1.0
    with pytest.raises(L.RpeError) as e:
        ctx.frame_download(L.MAP_DEPTH, max_levels(cam))
    assert e.value.code == L.RPE_ERR_ARG


@pytest.mark.parametrize("cam", [SMALL_CAM, FULL_CAM, ODD_CAM])
def test_model_pyramid_bit_exact(gpu_ctx_factory, cam):
    (RA, tA, dA), _ = two_views(cam)
    pA = pose12(RA, tA)
    levels = min(max_levels(cam), 4)
    ctx = gpu_ctx_factory()
    set_pyramid(ctx, dA, cam, 1.0, levels)
    ctx.model_from_frame(pA)
    frame = PO.frame_pyramid(dA, cam, 1.0, *RANGE, levels)
    for l, (z, V, N, B) in enumerate(frame):
        MV, MN = FO.to_world(V, N, pA)
        assert same(ctx.frame_download(L.MAP_MODEL_VERTEX, l), MV), l
        assert same(ctx.frame_download(L.MAP_MODEL_NORMAL, l), MN), l
        assert ctx.frame_camera(l, model=True) == PO.level_camera(cam, l)
    MV0, MN0 = FO.to_world(frame[0][1], frame[0][2], pA)
    up = gpu_ctx_factory()
    up.model_upload(MV0, MN0, cam, pA)
    with pytest.raises(L.RpeError):
        up.frame_download(L.MAP_MODEL_VERTEX, 1)       # an upload is one level until the pyramid is built
    up.model_build_pyramid(levels)
    for l, (MV, MN) in enumerate(PO.model_pyramid(MV0, MN0, cam, levels)):
        assert same(up.frame_download(L.MAP_MODEL_VERTEX, l), MV), l
        assert same(up.frame_download(L.MAP_MODEL_NORMAL, l), MN), l
        assert up.frame_camera(l, model=True) == PO.level_camera(cam, l)


FORMS = {"host": dict(device_resident=False, fused=False), "fused": dict(device_resident=False, fused=True),
         "device": dict(device_resident=True, fused=False), "device_fused": dict(device_resident=True, fused=True)}


def load_pyramid_pair(ctx, cam, levels, motion=MOTION, noise=0.002, seed=0):
    (RA, tA, dA), (RB, tB, dB) = two_views(cam, motion, noise=noise, seed=seed)
    pA, pB = pose12(RA, tA), pose12(RB, tB)
    if levels == 1:
        ctx.frame_set_depth(dA, cam, 1.0, *RANGE)
        ctx.model_from_frame(pA)
        ctx.frame_set_depth(dB, cam, 1.0, *RANGE)
    else:
        set_pyramid(ctx, dA, cam, 1.0, levels)
        ctx.model_from_frame(pA)
        set_pyramid(ctx, dB, cam, 1.0, levels)
    return dA, dB, pA, pB


@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_one_level_is_icp(gpu_ctx_factory, form):
    ctx = gpu_ctx_factory()
    _, _, pA, pB = load_pyramid_pair(ctx, FULL_CAM, 1)
    a = ctx.icp(pA, L.RES_P2PLANE, 8, 1e-7, 0.15, 0.8, **FORMS[form])
    slots = [ctx.download(s) for s in range(5)]
    b = ctx.icp_pyramid(pA, (8,), (0.15,), L.RES_P2PLANE, 1e-7, 0.8, **FORMS[form])
    assert np.array_equal(a[0], b[0]) and (a[1],) == b[1] and a[2:] == b[2:], (a, b)
    for s in range(5):
        assert same(ctx.download(s), slots[s]), s
    assert ctx.n == FULL_CAM[4] * FULL_CAM[5]


@contextlib.contextmanager
def fresh_context():
    c = api.Context(0)
    try:
        yield c
    finally:
        c.close()


def chained_icp(load_model, zB, cam, pose, iters, thr, form, tol=1e-7):
    """What a caller does without rpe_icp_pyramid: per level (coarse to fine) a fresh context holding the level's model
    (load_model(ctx, level)) and the level's metric depth uploaded as a frame of the level camera; rpe_icp with that level's rounds
    and gate; a level of 0 rounds is skipped.  Returns what icp_pyramid returns."""
    p, its, rest = np.array(pose, np.float64), [0] * len(iters), None
    for l in reversed(range(len(iters))):
        if iters[l] == 0:
            continue
        with fresh_context() as c:
            load_model(c, l)
            c.frame_set_depth(zB[l], PO.level_camera(cam, l), 1.0, *RANGE)
            p, its[l], *rest = c.icp(p, L.RES_P2PLANE, iters[l], tol, thr[l], 0.8, **FORMS[form])
    return (p, tuple(its), *rest)


def model_of_frames(zA, cam, pA):
    def load(c, l):
        c.frame_set_depth(zA[l], PO.level_camera(cam, l), 1.0, *RANGE)
        c.model_from_frame(pA)
    return load


def assert_same_run(got, want):
    """bit for bit: pose, rounds per level, and the last level's step, cost and pairs"""
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2:] == want[2:], (got, want)


CHAINS = {"L3": ((4, 3, 3), (0.15, 0.2, 0.3)),
          "L4_one_round_level": ((4, 3, 1, 3), (0.15, 0.2, 0.3, 0.4)),
          "L4_no_round_level": ((4, 0, 3, 2), (0.15, 0.2, 0.3, 0.4))}


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_is_the_chained_single_level_run(gpu_ctx_factory, form, chain):
    """Every form, up to RPE_MAX_LEVELS levels, levels of 1 round (the per-round path even in the resident forms) and of none: the
    pyramid returns the bits of the chained single-level runs."""
    iters, thr = CHAINS[chain]
    levels = len(iters)
    ctx = gpu_ctx_factory()
    dA, dB, pA, pB = load_pyramid_pair(ctx, FULL_CAM, levels)
    got = ctx.icp_pyramid(pA, iters, thr, L.RES_P2PLANE, 1e-7, 0.8, **FORMS[form])
    zA, zB = PO.depth_pyramid(dA, 1.0, *RANGE, levels), PO.depth_pyramid(dB, 1.0, *RANGE, levels)
    assert_same_run(got, chained_icp(model_of_frames(zA, FULL_CAM, pA), zB, FULL_CAM, pA, iters, thr, form))


@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_stops_early_at_a_coarse_level(gpu_ctx_factory, form):
    """tol ends coarse levels before their rounds run out; every level's round count is the chained runs' count."""
    iters, thr, tol = (10, 12, 12, 12), (0.15, 0.2, 0.3, 0.4), 1e-4
    ctx = gpu_ctx_factory()
    dA, dB, pA, pB = load_pyramid_pair(ctx, FULL_CAM, 4)
    got = ctx.icp_pyramid(pA, iters, thr, L.RES_P2PLANE, tol, 0.8, **FORMS[form])
    zA, zB = PO.depth_pyramid(dA, 1.0, *RANGE, 4), PO.depth_pyramid(dB, 1.0, *RANGE, 4)
    want = chained_icp(model_of_frames(zA, FULL_CAM, pA), zB, FULL_CAM, pA, iters, thr, form, tol)
    assert_same_run(got, want)
    assert any(0 < got[1][l] < iters[l] for l in (1, 2, 3)), got[1]


# the model's principal point differs from the frame's: each level must associate through the model's own level camera
MODEL_CAMS = {"same": FULL_CAM, "shifted": (FULL_CAM[0], FULL_CAM[1], FULL_CAM[2] + 3.5, FULL_CAM[3] - 2.25, FULL_CAM[4], FULL_CAM[5])}


def uploaded_pair(mcam):
    """frame B of the full camera; the model: the world maps of view A seen by mcam (level 0, as a caller uploads it)."""
    (RA, tA, _), (RB, tB, dB) = two_views(FULL_CAM, MOTION, noise=0.002, seed=0)
    dA = S.render_depth(RA, tA, mcam, noise_sigma=0.002, rng=np.random.default_rng(7))
    V, N, _ = FO.frame_maps(dA, mcam, 1.0, *RANGE)
    pA = pose12(RA, tA)
    MV0, MN0 = FO.to_world(V, N, pA)
    return dB, pA, MV0, MN0


@pytest.mark.parametrize("model_cam", list(MODEL_CAMS))
@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_on_an_uploaded_model(gpu_ctx_factory, form, model_cam):
    """rpe_model_upload + rpe_model_build_pyramid, then the pyramid ICP: the bits of the chained runs whose models are uploaded
    levels of PO.model_pyramid with their level cameras."""
    iters, thr, levels = (4, 3, 1, 3), (0.15, 0.2, 0.3, 0.4), 4
    mcam = MODEL_CAMS[model_cam]
    dB, pA, MV0, MN0 = uploaded_pair(mcam)
    ctx = gpu_ctx_factory()
    ctx.model_upload(MV0, MN0, mcam, pA)
    ctx.model_build_pyramid(levels)
    set_pyramid(ctx, dB, FULL_CAM, 1.0, levels)
    got = ctx.icp_pyramid(pA, iters, thr, L.RES_P2PLANE, 1e-7, 0.8, **FORMS[form])
    model = PO.model_pyramid(MV0, MN0, mcam, levels)

    def load(c, l):
        c.model_upload(*model[l], PO.level_camera(mcam, l), pA)
    assert_same_run(got, chained_icp(load, PO.depth_pyramid(dB, 1.0, *RANGE, levels), FULL_CAM, pA, iters, thr, form))


@pytest.mark.parametrize("model_cam", list(MODEL_CAMS))
def test_icp_pyramid_on_an_uploaded_model_matches_the_oracle_loop(gpu_ctx_factory, oracle, model_cam):
    iters, thr, levels = (4, 3, 1, 3), (0.15, 0.2, 0.3, 0.4), 4
    mcam = MODEL_CAMS[model_cam]
    dB, pA, MV0, MN0 = uploaded_pair(mcam)
    ctx = gpu_ctx_factory()
    ctx.model_upload(MV0, MN0, mcam, pA)
    ctx.model_build_pyramid(levels)
    set_pyramid(ctx, dB, FULL_CAM, 1.0, levels)
    got = ctx.icp_pyramid(pA, iters, thr, L.RES_P2PLANE, 0.0, 0.8)
    B, model = PO.frame_pyramid(dB, FULL_CAM, 1.0, *RANGE, levels), PO.model_pyramid(MV0, MN0, mcam, levels)
    p = pA
    for l in reversed(range(levels)):
        p, _ = oracle_icp(oracle, B[l][1], B[l][2], B[l][3], *model[l], PO.level_camera(mcam, l), p, pA, L.RES_P2PLANE, iters[l], thr[l],
                          0.8)
    assert got[1] == iters
    assert rot_err(got[0][:9].reshape(3, 3), p[:9].reshape(3, 3)) < 1e-6 and np.linalg.norm(got[0][9:] - p[9:]) < 1e-6


SMALL_PYR_CAM = (91.4, 91.4, 49.5, 37.5, 100, 76)     # level 2 is 25 x 19: 475 pixels, n % 4 = 3


def pyramid_icp_run(ctx, cam, levels, upload, form):
    """frame and model pyramids of one scene on ctx (the model from frame A, or uploaded and resized), then rpe_icp_pyramid; returns
    the result and every level's frame and model maps."""
    (RA, tA, dA), (RB, tB, dB) = two_views(cam, MOTION, noise=0.002, seed=levels)
    pA = pose12(RA, tA)
    if upload:
        V, N, _ = FO.frame_maps(dA, cam, 1.0, *RANGE)
        ctx.model_upload(*FO.to_world(V, N, pA), cam, pA)
        ctx.model_build_pyramid(levels)
    else:
        set_pyramid(ctx, dA, cam, 1.0, levels)
        ctx.model_from_frame(pA)
    set_pyramid(ctx, dB, cam, 1.0, levels)
    got = ctx.icp_pyramid(pA, (4, 3, 1, 3)[:levels], (0.15, 0.2, 0.3, 0.4)[:levels], L.RES_P2PLANE, 1e-7, 0.8, **FORMS[form])
    maps = [ctx.frame_download(m, l) for l in range(levels)
            for m in (L.MAP_DEPTH, L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING, L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL)]
    return got, maps


@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_context_reuse_across_cameras(gpu_ctx_factory, form):
    """One context: L = 4 at 640 x 480, then L = 3 at 100 x 76 with an uploaded model, then the first run again.  The level buffers
    only grow, so each run must not see the offsets, padding or contents another camera left: every result is a fresh context's."""
    ctx = gpu_ctx_factory()
    for cam, levels, upload in ((FULL_CAM, 4, False), (SMALL_PYR_CAM, 3, True), (FULL_CAM, 4, False)):
        got, maps = pyramid_icp_run(ctx, cam, levels, upload, form)
        with fresh_context() as c:
            want, want_maps = pyramid_icp_run(c, cam, levels, upload, form)
        assert_same_run(got, want)
        assert all(same(a, b) for a, b in zip(maps, want_maps)), (cam, levels)


def test_icp_pyramid_matches_the_oracle_loop(gpu_ctx_factory, oracle):
    iters, thr = (4, 3, 3), (0.15, 0.2, 0.3)
    ctx = gpu_ctx_factory()
    dA, dB, pA, pB = load_pyramid_pair(ctx, FULL_CAM, 3)
    got = ctx.icp_pyramid(pA, iters, thr, L.RES_P2PLANE, 0.0, 0.8)
    A, B = PO.frame_pyramid(dA, FULL_CAM, 1.0, *RANGE, 3), PO.frame_pyramid(dB, FULL_CAM, 1.0, *RANGE, 3)
    p = pA
    for l in (2, 1, 0):
        MV, MN = FO.to_world(A[l][1], A[l][2], pA)
        p, _ = oracle_icp(oracle, B[l][1], B[l][2], B[l][3], MV, MN, PO.level_camera(FULL_CAM, l), p, pA, L.RES_P2PLANE, iters[l], thr[l], 0.8)
    assert got[1] == iters
    assert rot_err(got[0][:9].reshape(3, 3), p[:9].reshape(3, 3)) < 1e-6 and np.linalg.norm(got[0][9:] - p[9:]) < 1e-6


@pytest.mark.parametrize("form", list(FORMS))
def test_icp_pyramid_recovers_a_large_motion(gpu_ctx_factory, form):
    """6 x the tests' default motion (9.4 deg, 26 cm): the 3-level pyramid with per-level gates converges to the true pose."""
    ctx = gpu_ctx_factory()
    _, _, pA, pB = load_pyramid_pair(ctx, FULL_CAM, 3, motion=tuple(6 * m for m in MOTION), noise=0.002, seed=1)
    p, its, step, cost, pairs = ctx.icp_pyramid(pA, (3, 3, 10), (0.15, 0.2, 0.3), L.RES_P2PLANE, 1e-6, 0.8, **FORMS[form])
    assert rot_err(p[:9].reshape(3, 3), pB[:9].reshape(3, 3)) < 1e-4 and np.linalg.norm(p[9:] - pB[9:]) < 1e-3, (its, step)
    assert pairs > 0.3 * FULL_CAM[4] * FULL_CAM[5]


def test_icp_pyramid_errors(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    _, _, pA, _ = load_pyramid_pair(ctx, SMALL_CAM, 2)
    with pytest.raises(L.RpeError) as e:
        ctx.icp_pyramid(pA, (3, 3, 3))                     # the frame has 2 levels
    assert e.value.code == L.RPE_ERR_STATE and "frame" in str(e.value)
    with pytest.raises(L.RpeError) as e:
        ctx.icp_pyramid(pA, (3,) * 5)                      # more than RPE_MAX_LEVELS
    assert e.value.code == L.RPE_ERR_ARG
    with pytest.raises(L.RpeError) as e:
        ctx.icp_pyramid(pA, (0, 3))                        # no round at level 0
    assert e.value.code == L.RPE_ERR_ARG
    assert ctx.icp_pyramid(pA, (3, 0))[1] == (3, 0)        # a coarse level may have none
    (RA, tA, dA), _ = two_views(SMALL_CAM)
    ctx.model_upload(ctx.frame_download(L.MAP_MODEL_VERTEX), ctx.frame_download(L.MAP_MODEL_NORMAL), SMALL_CAM, pA)
    with pytest.raises(L.RpeError) as e:
        ctx.icp_pyramid(pA, (3, 3))                        # the model has 1 level
    assert e.value.code == L.RPE_ERR_STATE and "model" in str(e.value)
    with pytest.raises(L.RpeError) as e:                  # level 2 of a 3 x 3 camera has no pixel
        set_pyramid(ctx, np.full((3, 3), 2.0, np.float32), (50.0, 50.0, 1.0, 1.0, 3, 3), 1.0, 3)
    assert e.value.code == L.RPE_ERR_ARG
    with pytest.raises(L.RpeError) as e:
        ctx.model_build_pyramid(5)
    assert e.value.code == L.RPE_ERR_ARG
    ctx.frame_set_depth(dA, SMALL_CAM, 1.0, *RANGE)       # rpe_frame_set_depth: one level, no metric depth
    with pytest.raises(L.RpeError) as e:
        ctx.frame_download(L.MAP_DEPTH, 0)
    assert e.value.code == L.RPE_ERR_STATE
    with pytest.raises(L.RpeError) as e:
        L.check(L.lib().rpe_frame_download(ctx._h, L.MAP_DEPTH, np.empty(SMALL_CAM[4] * SMALL_CAM[5], np.float32).ctypes.data_as(C.c_void_p)))
    assert e.value.code == L.RPE_ERR_ARG


def test_icp_pyramid_cpp(tmp_path):
    """DepthFrontEnd::icpPyramid from plain C++ (tests/cpp/pyramid_icp.cpp)."""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "pyramid_icp")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "pyramid_icp.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    assert r.returncode == 0 and "pyramid_icp: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("entry", ["icp_pyramid", "icp_pyramid_rgbd", "icp_pyramid_sdf"])
def test_pyramid_entries_refuse_in_their_own_order(gpu_ctx_factory, entry):
    """Which error a doubly wrong call gets is each entry point's own order of checks: rpe_icp_pyramid asks for frame and model (STATE)
    before it looks at the levels (ARG); the RGB-D and the volume form look at options and levels (ARG) before what is prepared
    (STATE).  No call here gets as far as a launch."""
    P0 = pose12(np.eye(3), np.zeros(3))

    def refused(ctx, **kw):
        with pytest.raises(L.RpeError) as e:
            getattr(ctx, entry)(P0, **kw)
        return e.value

    fresh = gpu_ctx_factory()                                  # no frame AND bad levels
    first = L.RPE_ERR_STATE if entry == "icp_pyramid" else L.RPE_ERR_ARG
    assert refused(fresh, iters=(0, 3)).code == first          # a finest level without rounds
    assert refused(fresh, iters=()).code == first              # no level at all
    cam = (20.0, 20.0, 7.5, 5.5, 16, 12)
    ctx = gpu_ctx_factory().frame_set_depth(np.full((12, 16), 1.0, np.float32), cam)
    ctx.model_from_frame(P0)
    if entry == "icp_pyramid_sdf":
        ctx.volume_init((8, 8, 8), 0.25, (-1.0, -1.0, 0.0), 0.5)
    assert refused(ctx, iters=(3,), dist_thr=(-0.1,)).code == L.RPE_ERR_ARG
    e = refused(ctx, iters=(3, 3))                             # one level is there (the RGB-D form: none prepared), two are asked
    assert e.code == L.RPE_ERR_STATE and "2 asked" in str(e)
