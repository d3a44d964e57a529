"""GPU parity of the colour volume (C1-C3 of csrc/rpe_color.hip) against tests/color_oracle.py: the colour integrate leaves the tsdf
bits of the plain integrate, the colour volume, the model colour and the mesh colours are BIT-EXACT with the oracle, the state rules of
the header hold, the fused textured room comes back within the oracle's own error, and the C++ driver equals the Python path."""
import os
import subprocess

import numpy as np
import pytest

import color_cases as CC
import color_oracle as CO
import mesh_oracle as MO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12, rot
from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = VC.RANGE
FULL_CAM = (585.0, 585.0, 320.0, 240.0, 640, 480)
ODD_CAM = (585.0, 585.0, 320.5, 239.5, 641, 479)
OUTSIDE = pose12(rot(0.1, 0.25, 0.0), np.array([0.3, 0.1, 3.2]))   # camera centre behind the volume, looking in


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def geometry(ctx, dims, voxel_size, origin, trunc, max_weight):
    ctx.volume_init(dims, voxel_size=voxel_size, origin=origin, trunc=trunc, max_weight=max_weight)
    return VO.Geometry(dims, voxel_size, origin, trunc, max_weight)


def room(ctx, voxel_size=0.05, max_weight=64):
    dims, desc = VC.room_geometry(voxel_size, max_weight)
    ctx.volume_init(dims, **desc)
    return VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])


def holes(a, rng, frac=0.05):
    a = a.copy()
    a.reshape(-1)[rng.integers(0, a.size, int(frac * a.size))] = 0
    return a


def set_frame(ctx, p, cam, depth=None, rgb=None, scale=1.0, order="rgb"):
    """set depth (rendered unless given) and colour (rendered unless given) of pose p; returns (V, rgba) for the oracle"""
    d = VC.depth_at(p, cam) if depth is None else depth
    c = CC.rgb_at(p, cam) if rgb is None else rgb
    ctx.frame_set_depth(d, cam, scale, *RANGE)
    ctx.frame_set_color(c if order == "rgb" else np.ascontiguousarray(c[..., ::-1]), order)
    return FO.frame_maps(d, cam, scale, *RANGE)[0], CO.frame_rgba(c)


# ---------------------------------------------------------------------------------------------- depth bits unchanged
@pytest.mark.parametrize("cam", [FULL_CAM, ODD_CAM], ids=["640x480", "641x479"])
@pytest.mark.parametrize("kind", ["f32", "u16_holes"])
def test_integrate_color_leaves_the_tsdf_bits_of_integrate(gpu_ctx_factory, cam, kind):
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    G = room(a)
    room(b)
    rng = np.random.default_rng(7)
    want_c = CO.empty(G)
    want_v = G.empty()
    for k in (0, 2):
        p = VC.view(k)
        if kind == "f32":
            d, scale = VC.depth_at(p, cam), 1.0
        else:
            d, scale = holes(VC.depth_at(p, cam, 0.003, rng, as_u16=True), rng), 0.001
        a.frame_set_depth(d, cam, scale, *RANGE)
        a.volume_integrate(p)
        V, rgba = set_frame(b, p, cam, d, scale=scale)
        b.volume_integrate_color(p)
        want_v, want_c = CO.integrate(want_v, want_c, G, V, rgba, cam, p)
    va, vb = a.volume_download(), b.volume_download()
    assert np.array_equal(bits(va), bits(vb))
    assert np.array_equal(bits(vb), bits(want_v))
    assert np.array_equal(bits(b.volume_color_download()), want_c)
    assert (want_c[..., 3] > 0).sum() > 10000


def test_tracking_loop_gives_the_same_poses_with_integrate_color(gpu_ctx_factory):
    cam = VC.HALF_CAM
    depths = VC.track_depths(cam)
    levels = len(VC.TRACK_ITERS)
    runs = []
    for colour in (False, True):
        ctx = gpu_ctx_factory()
        dims, desc = VC.room_geometry(VC.TRACK_VOXEL)
        ctx.volume_init(dims, **desc)
        est = [VC.track_pose(0)]

        def fuse(p, f):
            if colour:
                ctx.frame_set_color(CC.rgb_at(VC.track_pose(f), cam))
                ctx.volume_integrate_color(p)
            else:
                ctx.volume_integrate(p)
        ctx.frame_set_depth(depths[0], cam, 1.0, *RANGE, levels=levels)
        fuse(est[0], 0)
        for f in range(1, VC.TRACK_FRAMES):
            ctx.frame_set_depth(depths[f], cam, 1.0, *RANGE, levels=levels)
            ctx.volume_raycast(est[-1], cam, *VC.RAY, levels=levels)
            p = ctx.icp_pyramid(est[-1], VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)[0]
            fuse(p, f)
            est.append(p)
        runs.append((np.array(est), ctx.volume_download()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1]))


# ---------------------------------------------------------------------------------------------- colour volume bit-exact
def _random_colour_volume(G, rng, special=False):
    """random colour bits: plain values and weights, or (special) NaN, +-Inf, -0, subnormals, odd and negative weights among them"""
    d0, d1, d2 = G.dim
    c = CO.h(rng.uniform(-20, 300, (d2, d1, d0, 4)).astype(np.float32))
    c[..., 3] = CO.h(rng.choice(np.array([0, 0, 1, 2, 3, 17, 63, 64, 2046, 2047, 2048], np.float32), (d2, d1, d0)))
    if special:
        pool = np.array([0x7E00, 0x7E01, 0xFFFF, 0x7D00, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0x0003, 0x83FF, 0x03FF, 0x7BFF, 0xFBFF,
                         0xBC00, 0xC000, 0x4100, 0x3C01], np.uint16)          # NaNs, Infs, -0, subnormals, max, -1, -2, 2.5, 1 + ulp
        m = rng.random(c.shape) < 0.3
        c[m] = rng.choice(pool, int(m.sum()))
    return c


LANE_TAILS = {"nvox%4=0": (4, 3, 5), "nvox%4=1": (5, 3, 7), "nvox%4=2": (5, 3, 6), "nvox%4=3": (7, 3, 3), "2x2x2": (2, 2, 2)}


@pytest.mark.parametrize("name", list(LANE_TAILS))
def test_colour_volume_lane_tails(gpu_ctx_factory, name):
    """tiny volumes on the back wall, with a truncation so wide that almost every voxel is updated and in the band"""
    ctx = gpu_ctx_factory()
    dims = LANE_TAILS[name]
    G = geometry(ctx, dims, 0.2, (-0.4, -0.3, 4.4), 2.0, 64)
    rng = np.random.default_rng(len(name))
    c0 = _random_colour_volume(G, rng)
    ctx.volume_color_upload(c0.view(np.float16))
    vol, cvol = G.empty(), c0
    for k in (0, 1, 3):
        p = VC.view(k)
        V, rgba = set_frame(ctx, p, SMALL_CAM)
        ctx.volume_integrate_color(p)
        vol, cvol, band = CO.integrate(vol, cvol, G, V, rgba, SMALL_CAM, p, with_band=True)
        assert np.array_equal(bits(ctx.volume_color_download()), cvol), (name, k)
        assert np.array_equal(bits(ctx.volume_download()), bits(vol)), (name, k)
    assert band.reshape(-1)[-1], name                          # the last voxel (the lane tail) is updated and in the band


@pytest.mark.parametrize("max_weight", [1, 64, 5000])
def test_colour_volume_bit_exact_at_max_weights(gpu_ctx_factory, max_weight):
    ctx = gpu_ctx_factory()
    G = room(ctx, 0.05, max_weight)
    rng = np.random.default_rng(max_weight)
    c0 = _random_colour_volume(G, rng)
    ctx.volume_color_upload(c0.view(np.float16))
    vol, cvol = G.empty(), c0
    for k in (0, 1, 2, 1):
        p = VC.view(k)
        V, rgba = set_frame(ctx, p, SMALL_CAM)
        ctx.volume_integrate_color(p)
        vol, cvol = CO.integrate(vol, cvol, G, V, rgba, SMALL_CAM, p)
    got = bits(ctx.volume_color_download())
    assert np.array_equal(got, cvol)
    assert np.array_equal(bits(ctx.volume_download()), bits(vol))
    w = CO.f32(got[..., 3])
    changed = got[..., 3] != c0[..., 3]
    assert changed.sum() > 10000
    if max_weight == 5000:
        assert w.max() == 2048 and (w[changed] == 2048).sum() > 100     # 2046 / 2047 -> 2048, and 2049 rounds back to 2048
    else:
        assert np.all(w[changed] <= max_weight) and (w[changed] == max_weight).sum() > 10000


def test_bgr_equals_rgb_of_the_swapped_image(gpu_ctx_factory):
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    room(a)
    room(b)
    for k in (0, 2):
        p = VC.view(k)
        set_frame(a, p, SMALL_CAM, order="rgb")
        set_frame(b, p, SMALL_CAM, order="bgr")
        assert np.array_equal(a.frame_color(), b.frame_color())
        a.volume_integrate_color(p)
        b.volume_integrate_color(p)
    c = CC.rgb_at(VC.view(2), SMALL_CAM)
    assert np.array_equal(a.frame_color().reshape(-1, 4), CO.frame_rgba(c))
    assert np.array_equal(bits(a.volume_color_download()), bits(b.volume_color_download()))


@pytest.mark.parametrize("seed", [0, 1])
def test_uploaded_special_colour_volumes(gpu_ctx_factory, seed):
    ctx = gpu_ctx_factory()
    G = room(ctx, 0.05, 64)
    rng = np.random.default_rng(100 + seed)
    c0 = _random_colour_volume(G, rng, special=True)
    ctx.volume_color_upload(c0.view(np.float16))
    assert np.array_equal(bits(ctx.volume_color_download()), c0)              # the upload keeps every bit
    p = VC.view(seed)
    V, rgba = set_frame(ctx, p, SMALL_CAM)
    ctx.volume_integrate_color(p)
    _, cvol, band = CO.integrate(G.empty(), c0, G, V, rgba, SMALL_CAM, p, with_band=True)
    assert np.array_equal(bits(ctx.volume_color_download()), cvol)
    assert np.isnan(cvol[band].view(np.float16)).sum() > 100
    # the colour field over those bits, at the raycast's model vertices
    ctx.volume_raycast(p, SMALL_CAM, *VC.RAY)
    MV = ctx.frame_download(L.MAP_MODEL_VERTEX)
    assert np.array_equal(ctx.model_color().reshape(-1, 4), CO.sample(cvol, G, MV))


def test_camera_outside_the_volume(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G = room(ctx)
    vol, cvol = G.empty(), CO.empty(G)
    for p in (OUTSIDE, VC.view(1)):
        V, rgba = set_frame(ctx, p, SMALL_CAM)
        ctx.volume_integrate_color(p)
        vol, cvol = CO.integrate(vol, cvol, G, V, rgba, SMALL_CAM, p)
    assert np.array_equal(bits(ctx.volume_color_download()), cvol)
    ctx.volume_raycast(OUTSIDE, SMALL_CAM, *VC.RAY)
    MV = ctx.frame_download(L.MAP_MODEL_VERTEX)
    MC = ctx.model_color().reshape(-1, 4)
    assert np.array_equal(MC, CO.sample(cvol, G, MV)) and (MC[:, 3] == 255).sum() > 100


def test_colour_bytes_past_2_to_the_31(gpu_ctx_factory):
    """1024 x 1024 x 288 voxels: 2.4 GB of colour, the back wall at k ~ 272 (byte offsets above 2^31), checked by z-slab windows"""
    ctx = gpu_ctx_factory()
    dims = (1024, 1024, 288)
    G = geometry(ctx, dims, 0.01, (-5.12, -5.12, 2.28), 0.03, 64)
    cam = SMALL_CAM
    p = VC.view(0)
    V, rgba = set_frame(ctx, p, cam)
    ctx.volume_integrate_color(p)
    cv = bits(ctx.volume_color_download())
    assert cv.nbytes > 2 ** 31
    vol = ctx.volume_download()
    checked = 0
    for k0, k1 in ((0, 16), (136, 152), (256, 272), (272, 288)):
        wv, wc = CO.integrate(np.zeros((k1 - k0, 1024, 1024, 2), np.float32), np.zeros((k1 - k0, 1024, 1024, 4), np.uint16), G, V, rgba,
                              cam, p, k0)
        assert np.array_equal(cv[k0:k1], wc), (k0, k1)
        assert np.array_equal(bits(vol[k0:k1]), bits(wv)), (k0, k1)
        if k0 >= 256:
            checked += int((wc[..., 3] > 0).sum())
    assert checked > 10000                                      # colour stored beyond 2^31 bytes


# ---------------------------------------------------------------------------------------------- state rules
def _state(e):
    return isinstance(e.value, L.RpeError) and e.value.code == L.RPE_ERR_STATE


def test_state_rules(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    lib, h = L.lib(), ctx._h
    G = room(ctx)
    p = VC.view(0)
    buf = np.zeros(64, np.uint8)
    # no frame: set_color and integrate_color refuse
    with pytest.raises(L.RpeError) as e:
        ctx.frame_set_color(CC.rgb_at(p, SMALL_CAM))
    assert _state(e)
    # no colour volume yet: download, sample, mesh colours refuse
    with pytest.raises(L.RpeError) as e:
        ctx.volume_color_download()
    assert _state(e)
    # a frame, no frame colour
    ctx.frame_set_depth(VC.depth_at(p, SMALL_CAM), SMALL_CAM, 1.0, *RANGE)
    with pytest.raises(L.RpeError) as e:
        ctx.volume_integrate_color(p)
    assert _state(e) and "colour" in str(e.value)
    with pytest.raises(L.RpeError) as e:
        ctx.frame_color()
    assert _state(e)
    # set_depth after set_color drops the frame colour (both forms)
    for levels in (1, 2):
        ctx.frame_set_color(CC.rgb_at(p, SMALL_CAM))
        assert ctx.frame_color().shape == (SMALL_CAM[5], SMALL_CAM[4], 4)
        ctx.frame_set_depth(VC.depth_at(p, SMALL_CAM), SMALL_CAM, 1.0, *RANGE, levels=levels)
        with pytest.raises(L.RpeError) as e:
            ctx.volume_integrate_color(p)
        assert _state(e)
    # bad arguments
    assert lib.rpe_frame_set_color(h, buf.ctypes.data, 2) == L.RPE_ERR_ARG
    assert lib.rpe_color_download(h, 2, buf.ctypes.data) == L.RPE_ERR_ARG
    with pytest.raises(ValueError):
        ctx.frame_set_color(np.zeros((3, 3, 3), np.uint8))
    # the plain integrate never touches the colour volume
    V, rgba = set_frame(ctx, p, SMALL_CAM)
    ctx.volume_integrate_color(p)
    c1 = bits(ctx.volume_color_download()).copy()
    assert (c1[..., 3] > 0).sum() > 1000
    ctx.volume_integrate(VC.view(1))
    ctx.frame_set_depth(VC.depth_at(VC.view(2), SMALL_CAM), SMALL_CAM, 1.0, *RANGE)
    ctx.volume_integrate(VC.view(2))
    assert np.array_equal(bits(ctx.volume_color_download()), c1)
    # no model yet
    with pytest.raises(L.RpeError) as e:
        ctx.model_color()
    assert _state(e)
    # model colour: a new raycast, an upload or a model from the frame drops it
    ctx.volume_raycast(p, SMALL_CAM, *VC.RAY)
    mc = ctx.model_color()
    assert (mc[..., 3] == 255).sum() > 1000
    assert lib.rpe_color_download(h, L.COLOR_MODEL, mc.ctypes.data) == L.RPE_OK
    MV, MN = ctx.frame_download(L.MAP_MODEL_VERTEX), ctx.frame_download(L.MAP_MODEL_NORMAL)
    for replace in (lambda: ctx.volume_raycast(p, SMALL_CAM, *VC.RAY), lambda: ctx.model_upload(MV, MN, SMALL_CAM, p),
                    lambda: ctx.model_from_frame(p)):
        assert lib.rpe_model_sample_color(h) == L.RPE_OK
        replace()
        assert lib.rpe_color_download(h, L.COLOR_MODEL, mc.ctypes.data) == L.RPE_ERR_STATE
    # the model pyramid keeps level 0 and its colour
    assert lib.rpe_model_sample_color(h) == L.RPE_OK
    ctx.model_build_pyramid(2)
    assert lib.rpe_color_download(h, L.COLOR_MODEL, mc.ctypes.data) == L.RPE_OK
    # mesh colours before any mesh
    with pytest.raises(L.RpeError) as e:
        ctx.volume_mesh_colors()
    assert _state(e)
    assert lib.rpe_volume_mesh_colors(h, buf.ctypes.data) == L.RPE_ERR_STATE
    # volume_init drops the colour volume and the mesh; a colour upload brings a colour volume back
    ctx.volume_mesh()
    assert len(ctx.volume_mesh_colors()) > 0
    room(ctx)
    for call in (ctx.volume_color_download, ctx.volume_mesh_colors):
        with pytest.raises(L.RpeError) as e:
            call()
        assert _state(e)
    assert lib.rpe_model_sample_color(h) == L.RPE_ERR_STATE
    ctx.volume_mesh()
    with pytest.raises(L.RpeError) as e:
        ctx.volume_mesh_colors()                                 # a mesh, no colour volume
    assert _state(e)
    ctx.volume_color_upload(c1.view(np.float16))
    assert np.array_equal(bits(ctx.volume_color_download()), c1)
    # after a re-init the first colour integrate starts from zeros
    room(ctx)
    V, rgba = set_frame(ctx, p, SMALL_CAM)
    ctx.volume_integrate_color(p)
    assert np.array_equal(bits(ctx.volume_color_download()), CO.integrate(G.empty(), CO.empty(G), G, V, rgba, SMALL_CAM, p)[1])
    # an empty mesh gives 0 colours
    ctx.volume_init((8, 8, 8), voxel_size=0.05, origin=(0, 0, 0), trunc=0.15, max_weight=8)
    ctx.volume_color_upload(np.zeros((8, 8, 8, 4), np.float16))
    V_, _, T_ = ctx.volume_mesh()
    assert len(V_) == 0 and len(T_) == 0
    assert ctx.volume_mesh_colors().shape == (0, 4)
    assert lib.rpe_volume_mesh_colors(h, None) == L.RPE_OK


# ---------------------------------------------------------------------------------------------- model colour and mesh colours
def fused_colour_room(ctx, cam=SMALL_CAM, views=(0, 1, 2), voxel_size=0.05):
    G = room(ctx, voxel_size)
    vol, cvol = G.empty(), CO.empty(G)
    for k in views:
        p = VC.view(k)
        V, rgba = set_frame(ctx, p, cam)
        ctx.volume_integrate_color(p)
        vol, cvol = CO.integrate(vol, cvol, G, V, rgba, cam, p)
    return G, vol, cvol


def test_model_colour_after_a_raycast(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G, vol, cvol = fused_colour_room(ctx)
    assert np.array_equal(bits(ctx.volume_color_download()), cvol)
    for p, cam in ((VC.view(1), SMALL_CAM), (VC.held_out_pose(), VC.HALF_CAM)):
        ctx.volume_raycast(p, cam, *VC.RAY)
        MV = ctx.frame_download(L.MAP_MODEL_VERTEX)
        assert np.array_equal(bits(MV), bits(VO.raycast(vol, G, cam, p, *VC.RAY)[0]))
        MC = ctx.model_color()
        want = CO.sample(cvol, G, MV)
        assert MC.shape == (cam[5], cam[4], 4) and np.array_equal(MC.reshape(-1, 4), want)
        assert (want[:, 3] == 255).mean() > 0.7 and np.all(want[want[:, 3] == 0] == 0)


def _awkward_points(G, rng, n):
    """NaN points, points outside the volume, on voxel centres, in the last cell and on its far faces, and random ones"""
    d = np.array(G.dim)
    centres = lambda idx: (G.o + (idx.astype(np.float32) + np.float32(0.5)) * G.s).astype(np.float32)  # noqa: E731
    P = [np.full((5, 3), np.nan, np.float32), np.array([[0, np.nan, 0], [np.inf, 0, 0], [-np.inf, 0, 0]], np.float32),
         (G.o - np.float32(1.0)).reshape(1, 3).astype(np.float32), (G.o + d * G.s + 1).reshape(1, 3).astype(np.float32),
         centres(rng.integers(0, d, (200, 3))), centres(d - 2 + rng.random((100, 3)).astype(np.float32)),
         centres(np.tile(d - 2, (3, 1))), centres(np.tile(d - 1, (3, 1))), centres(np.zeros((3, 3), int)),
         (G.o + rng.random((n, 3)).astype(np.float32) * d * G.s).astype(np.float32)]
    return np.concatenate(P).astype(np.float32)


def test_model_colour_of_uploaded_awkward_points(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G, vol, cvol = fused_colour_room(ctx)
    rng = np.random.default_rng(11)
    cam = SMALL_CAM
    n = cam[4] * cam[5]
    P = _awkward_points(G, rng, n)[:n]
    P = np.concatenate([P, np.full((n - len(P), 3), np.nan, np.float32)]) if len(P) < n else P
    ctx.model_upload(P, np.zeros_like(P), cam, VC.view(0))
    MC = ctx.model_color().reshape(-1, 4)
    want = CO.sample(cvol, G, P)
    assert np.array_equal(MC, want)
    assert np.all((MC[:, 3] == 0) == (want[:, 3] == 0)) and np.all(MC[np.isnan(P).any(1)] == 0)
    assert (want[:, 3] == 255).sum() > 50 and (want[:, 3] == 0).sum() > 50
    # model_from_frame leaves world-frame vertices too
    set_frame(ctx, VC.view(1), cam)
    ctx.model_from_frame(VC.view(1))
    assert np.array_equal(ctx.model_color().reshape(-1, 4), CO.sample(cvol, G, ctx.frame_download(L.MAP_MODEL_VERTEX)))


def test_mesh_colours_equal_the_oracle_and_the_model_colour_at_the_same_points(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G, vol, cvol = fused_colour_room(ctx)
    V, N, T = ctx.volume_mesh()
    assert np.array_equal(bits(V), bits(MO.mesh(vol, G)[0]))
    VCl = ctx.volume_mesh_colors()
    assert VCl.shape == (len(V), 4) and np.array_equal(VCl, CO.sample(cvol, G, V))
    assert (VCl[:, 3] == 255).mean() > 0.8
    # the same points uploaded as a model give the same colours
    cam = (100.0, 100.0, 50.0, 50.0, 128, (len(V) + 127) // 128)
    n = cam[4] * cam[5]
    P = np.concatenate([V, np.full((n - len(V), 3), np.nan, np.float32)])
    ctx.model_upload(P, np.zeros_like(P), cam, VC.view(0))
    assert np.array_equal(ctx.model_color().reshape(-1, 4)[:len(V)], VCl)


def test_colour_accuracy_of_the_fused_textured_room(gpu_ctx_factory):
    cam = VC.HALF_CAM
    ctx = gpu_ctx_factory()
    dims, desc = VC.room_geometry(VC.ACC_VOXEL)
    ctx.volume_init(dims, **desc)
    for k in VC.ACC_VIEWS:
        set_frame(ctx, VC.view(k), cam)
        ctx.volume_integrate_color(VC.view(k))
    ctx.volume_raycast(VC.held_out_pose(), cam, *VC.RAY)
    med, p95, cover = CC.color_errors(ctx.model_color(), ctx.frame_download(L.MAP_MODEL_VERTEX))
    print(f"colour accuracy: median {med}, p95 {p95}, coverage {cover:.4f}")
    assert np.all(med <= CC.ACC_MEDIAN) and np.all(p95 <= CC.ACC_P95) and cover >= CC.ACC_COVERAGE, (med, p95, cover)


# ---------------------------------------------------------------------------------------------- C++
def test_volume_color_cpp_equals_the_python_path(tmp_path, gpu_ctx_factory):
    """DepthFrontEnd::setColor / integrateColor / modelColor / meshColors from plain C++ (tests/cpp/volume_color.cpp), replayed here"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_color")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_color.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    assert r.returncode == 0 and "volume_color: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    cam = (292.5, 292.5, 160.0, 120.0, 320, 240)
    rng_ = (0.1, 10.0, 0.1)
    poses = np.fromfile(out / "poses.bin", np.float64).reshape(3, 12)
    ctx = gpu_ctx_factory()
    ctx.volume_init((90, 72, 120), voxel_size=0.04, origin=(-1.7, -1.4, -0.5), trunc=0.12, max_weight=64)
    for f in range(3):
        d = np.fromfile(out / f"depth{f}.bin", np.float32).reshape(240, 320)
        rgb = np.fromfile(out / f"rgb{f}.bin", np.uint8).reshape(240, 320, 3)
        ctx.frame_set_depth(d, cam, 1.0, *rng_)
        ctx.frame_set_color(rgb)
        ctx.volume_integrate_color(poses[f])
    assert np.array_equal(bits(ctx.volume_color_download()).reshape(-1), np.fromfile(out / "color_volume.bin", np.uint16))
    ctx.volume_raycast(poses[1], cam, *rng_[:2])
    assert np.array_equal(ctx.model_color().reshape(-1), np.fromfile(out / "model_color.bin", np.uint8))
    V, _, _ = ctx.volume_mesh()
    assert np.array_equal(bits(V).reshape(-1), np.fromfile(out / "mesh_vertices.bin", np.float32).view(np.uint32))
    assert np.array_equal(ctx.volume_mesh_colors().reshape(-1), np.fromfile(out / "mesh_colors.bin", np.uint8))
