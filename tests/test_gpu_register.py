"""GPU parity of colour registration (R1 / R2 of csrc/rpe_register.hip, rpe_frame_register_color) against tests/register_oracle.py, BIT
FOR BIT: the frame colour of every case equals the oracle's on the vertex map the device holds, over the smallest shapes that reach
each branch; the count, the state and argument rules of the header hold; A = 0 keeps a pixel out of the colour volume (through the
colour integrate and through the keyframe fuse) and out of the photometric maps; the fused textured room seen through the rig comes
back within the oracle's own error; and the C++ driver equals the Python path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import color_cases as CC
import color_oracle as CO
import feature_oracle as FE
import oriented_oracle as OO
import register_cases as RC
import register_oracle as RO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import pose12, rot
from rgbd_pose_estimation_amd import _lib as L
from rgbd_pose_estimation_amd import simulator as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = VC.RANGE
DIST = RC.DIST
# a wide baseline (0.3 m) and a small turn: at these few pixels the spheres of the room still hide wall behind them
WIDE = pose12(rot(0.02, -0.05, 0.01), np.array([-0.3, 0.02, 0.01]))


def cam_of(w, h, scale=1.0):
    """the reference camera's field of view at w x h pixels (scale > 1: a longer lens)"""
    f = 585.0 * w / 640.0 * scale
    return (f, f, w / 2.0, h / 2.0, w, h)


def image_of(p, rig, seed=None):
    """the rig's colour image at depth pose p; with a seed, noise on top so that neighbouring pixels differ by many levels"""
    img = RC.color_image(p, rig)
    if seed is not None:
        rng = np.random.default_rng(seed)
        img = np.clip(img.astype(np.int64) + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    return img


def crig(ctx, rig):
    return ctx.color_rig(rig.cam, rig.dist, rig.pose12, rig.r2_max, rig.cell, rig.occl_tol, rig.occl_tol_z2)


def register(ctx, img, rig, order="rgb"):
    """one call with a count and one without: (frame colour (n, 4), count), the second call's bits equal the first's"""
    arg = img if order == "rgb" else np.ascontiguousarray(img[..., ::-1])
    known = ctx.frame_register_color(arg, crig(ctx, rig), order, want_known=True)
    a = ctx.frame_color().reshape(-1, 4).copy()
    assert ctx.frame_register_color(arg, crig(ctx, rig), order) is ctx
    assert np.array_equal(ctx.frame_color().reshape(-1, 4), a)
    return a, known


def check(ctx, img, rig, order="rgb", min_known=1, hidden=None):
    """the device's frame colour against the oracle on the device's own vertex map; returns the oracle's (rgba, projection, visible)"""
    got, known = register(ctx, img, rig, order)
    V = ctx.frame_download(L.MAP_VERTEX)
    want, P, vis = RO.register(V, img, rig, with_info=True)
    assert np.array_equal(got, want), (int((got != want).any(1).sum()), len(want))
    assert known == int((want[:, 3] == 255).sum()) == int(vis.sum()) and known >= min_known
    assert np.all(want[~vis] == 0)
    if hidden is not None:
        assert (P["ok"] & ~vis).sum() >= hidden, int((P["ok"] & ~vis).sum())
    return want, P, vis


def set_depth(ctx, p, dcam, kind="f32", levels=1, holes=0.0, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "u16":
        d, scale = VC.depth_at(p, dcam, 0.002, rng, as_u16=True), 0.001
    else:
        d, scale = VC.depth_at(p, dcam), 1.0
    if holes:
        d = d.copy()
        d.reshape(-1)[rng.integers(0, d.size, int(holes * d.size))] = 0
    ctx.frame_set_depth(d, dcam, scale, *RANGE, levels=levels)
    return d


# ---------------------------------------------------------------------------------------------- shapes and branches
SHAPES = {
    "37x29_into_53x41_cell3": (cam_of(37, 29), cam_of(53, 41, 1.1), 3),        # partial last cells, sizes off every block multiple
    "64x48_into_40x30": (cam_of(64, 48), cam_of(40, 30, 1.05), 2),             # a colour camera smaller than the depth camera
    "cell1": (cam_of(64, 48), cam_of(96, 72, 1.1), 1),
    "cell16": (cam_of(64, 48), cam_of(96, 72, 1.1), 16),
    "cell0": (cam_of(64, 48), cam_of(96, 72, 1.1), 0),
}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_frame_colour_bit_exact(gpu_ctx_factory, name, order):
    dcam, ccam, cell = SHAPES[name]
    ctx = gpu_ctx_factory()
    rig = RO.Rig(ccam, DIST, tuple(WIDE), 0.0, cell)
    for k in (0, 2):
        p = VC.view(k)
        set_depth(ctx, p, dcam)
        want, P, vis = check(ctx, image_of(p, rig, seed=k), rig, order, min_known=250,
                             hidden=0 if cell in (0, 16) else 5)
        if cell == 0:
            assert np.array_equal(vis, P["ok"])
        if cell == 16:
            assert (P["ok"] & ~vis).sum() > 100                      # cells that coarse hide plenty


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("form", ["plain", "pyramid", "filtered"])
def test_depth_kinds_pyramid_and_filtered_frames(gpu_ctx_factory, kind, form):
    dcam, ccam = cam_of(64, 48), cam_of(80, 60, 1.1)
    ctx = gpu_ctx_factory()
    if form == "filtered":
        ctx.frame_set_filter()
    rig = RO.Rig(ccam, DIST, tuple(WIDE), 0.0, 2)
    p = VC.view(1)
    set_depth(ctx, p, dcam, kind, levels=3 if form == "pyramid" else 1, holes=0.05, seed=3)       # holes: invalid pixels among them
    V = ctx.frame_download(L.MAP_VERTEX)
    assert 50 < np.isnan(V).any(1).sum() < 0.2 * len(V)
    want, P, vis = check(ctx, image_of(p, rig, seed=1), rig, min_known=1500, hidden=5)
    assert np.all(want[np.isnan(V).any(1)] == 0)


def test_thousands_of_minima_on_four_words(gpu_ctx_factory):
    """64 x 48 depth into an 8 x 6 colour camera with cell 4: a 2 x 2 grid, every pixel's minimum lands on one of four words; on a flat
    wall head-on many of them are equal"""
    dcam, ccam = cam_of(64, 48), cam_of(8, 6)
    ctx = gpu_ctx_factory()
    rig = RO.Rig(ccam, (0, 0, 0, 0, 0), RO.I12, 0.0, 4, 0.02, 0.01)
    ctx.frame_set_depth(np.full((48, 64), 2.5, np.float32), dcam, 1.0, *RANGE)
    img = np.random.default_rng(0).integers(0, 256, (6, 8, 3)).astype(np.uint8)
    want, P, vis = check(ctx, img, rig, min_known=1500)
    assert P["ok"].sum() > 1500 and len(np.unique(P["z"][P["ok"]].view(np.uint32))) < 10
    assert np.array_equal(vis, P["ok"])                                  # a wall hides nothing of itself
    # the room through the same four words: the spheres hide wall
    p = VC.view(0)
    set_depth(ctx, p, dcam)
    rig2 = RO.Rig(ccam, (0, 0, 0, 0, 0), tuple(WIDE), 0.0, 4, 0.02, 0.01)
    check(ctx, image_of(p, rig2), rig2, min_known=20, hidden=100)


def test_rig_turned_past_the_frame_and_an_r2_limit(gpu_ctx_factory):
    dcam, ccam = cam_of(64, 48), cam_of(80, 60)
    ctx = gpu_ctx_factory()
    p = VC.view(0)
    set_depth(ctx, p, dcam)
    V = ctx.frame_download(L.MAP_VERTEX)
    # a wide colour camera in the middle of the room, turned by 34 degrees: a third of the frame lies behind it
    turned = RO.Rig(cam_of(80, 60, 0.6), DIST, tuple(pose12(rot(0.0, 0.6, 0.0), np.array([0.1, 0.0, -2.5]))), 0.0, 2)
    want, P, vis = check(ctx, image_of(p, turned, seed=2), turned, min_known=50)
    R, t = np.asarray(turned.pose12[:9], np.float32), np.asarray(turned.pose12[9:], np.float32)
    kz = ((R[6] * V[:, 0] + R[7] * V[:, 1]) + R[8] * V[:, 2]) + t[2]
    assert (kz <= 0).sum() > 200 and np.all(want[kz <= 0] == 0)
    # an r2 limit that cuts the corners
    cut = RO.Rig(ccam, DIST, tuple(RC.RIG_POSE), 0.3, 2)
    full = RO.Rig(ccam, DIST, tuple(RC.RIG_POSE), 0.0, 2)
    a, _, _ = check(ctx, image_of(p, cut, seed=2), cut, min_known=500)
    b, _, _ = check(ctx, image_of(p, full, seed=2), full, min_known=500)
    lost = (b[:, 3] == 255) & (a[:, 3] == 0)
    assert lost.sum() > 100 and lost.reshape(48, 64)[1, 1] and not lost.reshape(48, 64)[20:28, 28:36].any()


def test_all_invalid_depth_and_regrown_buffers(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    dcam, ccam = cam_of(64, 48), cam_of(80, 60)
    rig = RO.Rig(ccam, DIST, tuple(WIDE), 0.0, 2)
    ctx.frame_set_depth(np.zeros((48, 64), np.float32), dcam, 1.0, *RANGE)
    img = image_of(VC.view(0), rig)
    got, known = register(ctx, img, rig)
    assert known == 0 and np.all(got == 0) and got.shape == (64 * 48, 4)
    # larger on both sides, then smaller on both sides (the z-buffer of the earlier call must not show), then larger again
    for (dw, dh), (cw, ch), cell, k in (((96, 72), (120, 90), 2, 0), ((37, 29), (53, 41), 3, 1), ((96, 72), (128, 96), 1, 2)):
        d2, c2 = cam_of(dw, dh), cam_of(cw, ch, 1.1)
        r2 = RO.Rig(c2, DIST, tuple(WIDE), 0.0, cell)
        p = VC.view(k)
        set_depth(ctx, p, d2)
        check(ctx, image_of(p, r2, seed=k), r2, min_known=250, hidden=5)


# ---------------------------------------------------------------------------------------------- state and argument rules
def test_errors_leave_the_frame_colour_and_a_new_depth_drops_it(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    lib, h = L.lib(), ctx._h
    dcam, ccam = cam_of(64, 48), cam_of(80, 60)
    rig = RO.Rig(ccam, DIST, tuple(WIDE), 0.0, 2)
    p = VC.view(0)
    img = image_of(p, rig)
    ptr = img.ctypes.data_as(C.c_void_p)
    good = crig(ctx, rig)
    assert lib.rpe_frame_register_color(h, ptr, L.COLOR_RGB8, C.byref(good), None) == L.RPE_ERR_STATE          # no frame yet
    set_depth(ctx, p, dcam)
    with pytest.raises(L.RpeError) as e:
        ctx.frame_color()
    assert e.value.code == L.RPE_ERR_STATE
    before, _ = register(ctx, img, rig)
    assert (before[:, 3] == 255).sum() > 1000

    def bad(**kw):
        r = crig(ctx, rig)
        for k, v in kw.items():
            if k in ("width", "height", "fx", "fy", "cx"):
                setattr(r.cam, k, v)
            elif k == "dist":
                r.dist[v[0]] = v[1]
            elif k == "pose":
                r.pose12[v[0]] = v[1]
            else:
                setattr(r, k, v)
        return r

    nan, inf = float("nan"), float("inf")
    rigs = [bad(cell=-1), bad(cell=17), bad(width=1), bad(height=1), bad(width=0), bad(fx=0.0), bad(fx=-5.0), bad(fy=nan), bad(fx=inf),
            bad(cx=nan), bad(dist=(0, nan)), bad(dist=(4, inf)), bad(pose=(3, nan)), bad(pose=(11, -inf)), bad(occl_tol=-0.01),
            bad(occl_tol_z2=-1.0), bad(occl_tol=nan), bad(occl_tol_z2=inf), bad(r2_max=-0.5), bad(r2_max=nan)]
    known = C.c_int64(-7)
    for r in rigs:
        assert lib.rpe_frame_register_color(h, ptr, L.COLOR_RGB8, C.byref(r), C.byref(known)) == L.RPE_ERR_ARG
    assert lib.rpe_frame_register_color(h, ptr, 2, C.byref(good), None) == L.RPE_ERR_ARG
    assert lib.rpe_frame_register_color(h, None, L.COLOR_RGB8, C.byref(good), None) == L.RPE_ERR_ARG
    assert lib.rpe_frame_register_color(h, ptr, L.COLOR_RGB8, None, None) == L.RPE_ERR_ARG
    assert known.value == -7 and np.array_equal(ctx.frame_color().reshape(-1, 4), before)
    with pytest.raises(ValueError):
        ctx.frame_register_color(img[:-1], good)
    with pytest.raises(ValueError):
        ctx.frame_register_color(img, good, "gbr")
    # the limits themselves are fine
    for r in (bad(cell=16), bad(cell=0), bad(occl_tol=0.0, occl_tol_z2=0.0)):
        assert lib.rpe_frame_register_color(h, ptr, L.COLOR_RGB8, C.byref(r), None) == L.RPE_OK
    # a new depth drops the colour, as it drops rpe_frame_set_color's (both forms); rpe_frame_set_color replaces it and back
    for levels in (1, 2):
        register(ctx, img, rig)
        set_depth(ctx, p, dcam, levels=levels)
        with pytest.raises(L.RpeError) as e:
            ctx.frame_color()
        assert e.value.code == L.RPE_ERR_STATE
    plain = S.render_rgb(p[:9].reshape(3, 3), p[9:], dcam)
    ctx.frame_set_color(plain)
    assert np.array_equal(ctx.frame_color().reshape(-1, 4), CO.frame_rgba(plain))
    after, _ = register(ctx, img, rig)
    assert np.array_equal(after, before)


# ---------------------------------------------------------------------------------------------- A = 0 means no colour
GATE_DIMS, GATE_VOXEL, GATE_ORIGIN = (23, 18, 16), 0.25, (-2.9, -2.2, 1.2)      # 6 624 voxels over the far half of the room


def _gate_scene(ctx, k=0, size=(64, 48)):
    dcam, ccam = cam_of(*size), cam_of(size[0] * 5 // 4, size[1] * 5 // 4)
    rig = RO.Rig(ccam, DIST, tuple(pose12(rot(0.0, 0.5, 0.0), np.array([-0.3, 0.0, 0.1]))), 0.0, 2)   # turned: a third of the frame has no colour
    p = VC.view(k)
    set_depth(ctx, p, dcam)
    img = image_of(p, rig, seed=4)
    rgba, _ = register(ctx, img, rig)
    V = ctx.frame_download(L.MAP_VERTEX)
    assert np.array_equal(rgba, RO.register(V, img, rig))
    none = rgba[:, 3] == 0
    assert 0.2 * len(none) < none.sum() < 0.8 * len(none)
    return dcam, p, V, rgba


def _gate_geometry(ctx):
    ctx.volume_init(GATE_DIMS, voxel_size=GATE_VOXEL, origin=GATE_ORIGIN, trunc=3 * GATE_VOXEL, max_weight=64)
    return VO.Geometry(GATE_DIMS, GATE_VOXEL, GATE_ORIGIN, 3 * GATE_VOXEL, 64)


def test_alpha_gate_in_the_colour_integrate(gpu_ctx_factory):
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    G = _gate_geometry(a)
    _gate_geometry(b)
    vol, cvol, ungated = G.empty(), CO.empty(G), CO.empty(G)
    for k in (0, 2):
        dcam, p, V, rgba = _gate_scene(a, k)
        a.volume_integrate_color(p)
        set_depth(b, p, dcam)
        b.volume_integrate(p)
        ungated = CO.integrate(vol, ungated, G, V, rgba, dcam, p)[1]
        vol, cvol = RO.integrate(vol, cvol, G, V, rgba, dcam, p)
    assert np.array_equal(a.volume_color_download().view(np.uint16), cvol)
    va = a.volume_download()
    assert np.array_equal(va.view(np.uint32), b.volume_download().view(np.uint32))          # the tsdf bits of the plain integrate
    assert np.array_equal(va.view(np.uint32), vol.view(np.uint32))
    has, would = cvol[..., 3] > 0, ungated[..., 3] > 0
    assert has.sum() > 300 and (would & ~has).sum() > 100 and not (has & ~would).any()      # the gate kept voxels out


def test_alpha_gate_in_the_keyframe_fuse(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G = _gate_geometry(ctx)
    vol, cvol = G.empty(), CO.empty(G)
    ids, poses = [], []
    for k in (0, 2):
        dcam, p, V, rgba = _gate_scene(ctx, k)
        kp = np.array([[5, 5], [20, 9], [40, 30], [60, 40]], np.int32)
        i = ctx.keyframe_add_host(kp, np.zeros((4, 8), np.uint32) + k, np.ones((4, 3), np.float32), np.tile([0, 0, 1], (4, 1)).astype(np.float32),
                                  p, dcam[4], dcam[5])
        ctx.keyframe_attach_frame(i)
        att = ctx.keyframe_attachment(i)
        assert np.array_equal(att["rgba"].reshape(-1, 4), rgba) and (att["rgba"][..., 3] == 0).sum() > 500    # the alpha travels
        ids.append(i)
        poses.append(p)
        vol, cvol = RO.integrate(vol, cvol, G, V, rgba, dcam, p)
    for cull in (True, False):
        ctx.volume_fuse_keyframes(ids, poses, clear=True, color=True, cull=cull)
        assert np.array_equal(ctx.volume_color_download().view(np.uint16), cvol), cull
        assert np.array_equal(ctx.volume_download().view(np.uint32), vol.view(np.uint32)), cull
    # without CLEAR on top of what is there: the same chain again
    ctx.volume_fuse_keyframes(ids[:1], poses[:1], clear=False, color=True)
    _, p0, V0, rgba0 = _gate_scene(gpu_ctx_factory(), 0)
    vol2, cvol2 = RO.integrate(vol, cvol, G, V0, rgba0, cam_of(64, 48), p0)
    assert np.array_equal(ctx.volume_color_download().view(np.uint16), cvol2)
    assert np.array_equal(ctx.volume_download().view(np.uint32), vol2.view(np.uint32))


def test_photo_intensity_is_nan_exactly_where_alpha_is_zero(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    dcam, p, V, rgba = _gate_scene(ctx)
    ctx.model_from_frame(p)
    ctx.model_color_from_frame()
    ctx.photo_prepare(1)
    I = ctx.photo_download(L.PHOTO_FRAME, 0).reshape(-1)
    assert np.array_equal(np.isnan(I), rgba[:, 3] == 0)
    c = rgba[:, :3].astype(np.float32)
    want = (np.float32(0.299) * c[:, 0] + np.float32(0.587) * c[:, 1]) + np.float32(0.114) * c[:, 2]
    m = rgba[:, 3] == 255
    assert np.array_equal(I[m].view(np.uint32), want[m].view(np.uint32))


@pytest.mark.parametrize("kind", ["upright", "oriented"])
def test_detector_finds_nothing_where_alpha_is_zero(gpu_ctx_factory, kind):
    """rpe_features_detect on a frame coloured through the rig, bit for bit the feature oracles on the registered RGBA: a pixel with
    A = 0 has luma 0, is no keypoint and spoils every ring it lies on, so the uncoloured part of the frame yields nothing"""
    ctx = gpu_ctx_factory()
    dcam, p, V, rgba = _gate_scene(ctx, size=(128, 96))
    w, h = dcam[4], dcam[5]
    N = ctx.frame_download(L.MAP_NORMAL)
    img = rgba.reshape(h, w, 4)
    ctx.features_set_descriptor(L.DESC_ORIENTED if kind == "oriented" else L.DESC_UPRIGHT)
    if kind == "oriented":
        xy, sc, de, bins = OO.detect(img, V, N)
    else:
        xy, sc, de = FE.detect(img, V, N)
    assert ctx.features_detect(L.FEAT_FRAME) == len(xy) and len(xy) > 30
    gxy, gsc, gde = ctx.features(L.FEAT_FRAME)
    assert np.array_equal(gxy, xy) and np.array_equal(gsc, sc) and np.array_equal(gde, de)
    if kind == "oriented":
        assert np.array_equal(ctx.features_angles(L.FEAT_FRAME), bins)
    # no keypoint without a colour, none whose ring touches a pixel without one
    A = img[..., 3] != 0
    assert A[gxy[:, 1], gxy[:, 0]].all()
    for dx, dy in FE.RING:
        assert A[gxy[:, 1] + dy, gxy[:, 0] + dx].all()
    # the gate is what keeps them out: the same bytes with A = 255 everywhere give keypoints on and beside the uncoloured part
    opaque = img.copy()
    opaque[..., 3] = 255
    oxy = FE.detect(opaque, V, N)[0]
    ring_ok = np.all([A[oxy[:, 1] + dy, oxy[:, 0] + dx] for dx, dy in FE.RING], 0)
    assert (~ring_ok).sum() > 0 and len(oxy) > len(xy)


# ---------------------------------------------------------------------------------------------- end to end
def test_colour_accuracy_of_the_room_fused_through_the_rig(gpu_ctx_factory):
    """color_cases' accuracy case with every view's colour taken through the rig: the figures of register_cases.py"""
    cam = RC.DEPTH_CAM
    ctx = gpu_ctx_factory()
    dims, desc = VC.room_geometry(VC.ACC_VOXEL)
    ctx.volume_init(dims, **desc)
    rig = crig(ctx, RC.ROOM_RIG)
    for p, d, img in RC.accuracy_frames():
        ctx.frame_set_depth(d, cam, 1.0, *RANGE)
        ctx.frame_register_color(img, rig)
        ctx.volume_integrate_color(p)
    ctx.volume_raycast(VC.held_out_pose(), cam, *VC.RAY)
    med, p95, cover = CC.color_errors(ctx.model_color(), ctx.frame_download(L.MAP_MODEL_VERTEX))
    print(f"colour accuracy through the rig: median {med}, p95 {p95}, coverage {cover:.4f}")
    assert np.all(med <= RC.ACC_MEDIAN) and np.all(p95 <= RC.ACC_P95) and cover >= RC.ACC_COVERAGE, (med, p95, cover)
    # and the room pair's two conditions, on the device's output
    p, d, img = RC.accuracy_frames()[0]
    ctx.frame_set_depth(d, cam, 1.0, *RANGE)
    known = ctx.frame_register_color(img, rig, want_known=True)
    got = ctx.frame_color().reshape(-1, 4)
    V = ctx.frame_download(L.MAP_VERTEX)
    want, P, _ = RO.register(V, img, RC.ROOM_RIG, with_info=True)
    assert np.array_equal(got, want) and known == (want[:, 3] == 255).sum()
    vis = RC.truly_visible(V, p)
    coloured, inimg = got[:, 3] == 255, P["ok"]
    occl = inimg & ~vis
    assert occl.sum() > 300 and (occl & coloured).sum() <= RC.MAX_OCCLUDED_COLOURED * occl.sum()
    assert (inimg & vis & ~coloured).sum() <= RC.MAX_VISIBLE_DROPPED * (inimg & vis).sum()


# ---------------------------------------------------------------------------------------------- C++
def test_register_color_cpp_equals_the_python_path(tmp_path, gpu_ctx_factory):
    """DepthFrontEnd::registerColor / integrateColor from plain C++ (tests/cpp/register_color.cpp), replayed here"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "register_color")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "register_color.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    assert r.returncode == 0 and "register_color: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    cam = (292.5, 292.5, 160.0, 120.0, 320, 240)
    rig = RO.Rig((365.0, 365.0, 200.0, 150.0, 400, 300), (-0.1, 0, 0, 0, 0), (1, 0, 0, 0, 1, 0, 0, 0, 1, -0.05, 0, 0), 0.0, 2, 0.02, 0.01)
    d = np.fromfile(out / "depth.bin", np.float32).reshape(240, 320)
    img = np.fromfile(out / "rgb.bin", np.uint8).reshape(300, 400, 3)
    ctx = gpu_ctx_factory()
    ctx.volume_init((90, 72, 120), voxel_size=0.04, origin=(-1.7, -1.4, -0.5), trunc=0.12, max_weight=64)
    ctx.frame_set_depth(d, cam, 1.0, 0.1, 10.0, 0.1)
    ctx.frame_register_color(img, crig(ctx, rig))
    got = ctx.frame_color().reshape(-1)
    assert np.array_equal(got, np.fromfile(out / "rgba.bin", np.uint8))
    assert np.array_equal(got.reshape(-1, 4), RO.register(ctx.frame_download(L.MAP_VERTEX), img, rig))
    ctx.volume_integrate_color(RO.I12)
    assert np.array_equal(ctx.volume_color_download().view(np.uint16).reshape(-1), np.fromfile(out / "color_volume.bin", np.uint16))
