"""GPU parity of the TSDF volume (V1 / V2 of csrc/rpe_volume.hip) against tests/volume_oracle.py: integrate and raycast are BIT-EXACT;
the raycast model is interchangeable with the same maps uploaded; fused frames raycast to the rendered depth; a 10-frame frame-to-model
tracking loop (set_depth_pyramid -> raycast -> model pyramid -> icp_pyramid -> integrate) stays on the true path."""
import os
import subprocess
import time

import numpy as np
import pytest

import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM, pose12, rot
from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = VC.RANGE
ODD_CAM = (151.0, 139.0, 70.3, 49.6, 133, 97)     # another camera than the frames': odd size, unequal focal lengths, shifted centre


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def volume_pair(ctx, voxel_size=0.05, max_weight=64):
    dims, desc = VC.room_geometry(voxel_size, max_weight)
    ctx.volume_init(dims, **desc)
    return VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])


def holes(depth, rng, frac=0.05):
    d = depth.copy()
    d.reshape(-1)[rng.integers(0, d.size, int(frac * d.size))] = 0
    return d


def frames(case):
    """[(depth, pose, scale)] of an integrate case"""
    rng = np.random.default_rng(3)
    if case == "one":
        return [(VC.depth_at(VC.view(0), SMALL_CAM), VC.view(0), 1.0)]
    if case == "three_poses":
        return [(VC.depth_at(VC.view(k), SMALL_CAM), VC.view(k), 1.0) for k in (0, 2, 3)]
    if case == "u16_noise_holes":
        return [(holes(VC.depth_at(VC.view(k), SMALL_CAM, 0.004, rng, as_u16=True), rng), VC.view(k), 0.001) for k in (0, 1)]
    if case == "four_at_max_weight_2":
        return [(VC.depth_at(VC.view(k), SMALL_CAM, 0.003, rng), VC.view(k), 1.0) for k in (0, 1, 0, 2)]
    raise KeyError(case)


@pytest.mark.parametrize("case", ["one", "three_poses", "u16_noise_holes", "four_at_max_weight_2"])
@pytest.mark.parametrize("pyramid", [False, True])
def test_integrate_bit_exact(gpu_ctx_factory, case, pyramid):
    ctx = gpu_ctx_factory()
    G = volume_pair(ctx, max_weight=2 if case == "four_at_max_weight_2" else 64)
    assert same(ctx.volume_download(), G.empty())
    want = G.empty()
    for depth, p, scale in frames(case):
        ctx.frame_set_depth(depth, SMALL_CAM, scale, *RANGE, levels=3 if pyramid else 1)
        ctx.volume_integrate(p)
        V = FO.frame_maps(depth, SMALL_CAM, scale, *RANGE)[0]
        want = VO.integrate(want, G, V, SMALL_CAM, p)
        assert same(ctx.volume_download(), want), case
    w = want[..., 1]
    assert 0.02 < (w > 0).mean() < 0.6
    if case == "four_at_max_weight_2":
        assert w.max() == np.float32(2) and (w == 2).sum() > 1000


def fused_room(ctx, cam=SMALL_CAM, views=(0, 1, 2)):
    G = volume_pair(ctx)
    want = G.empty()
    for k in views:
        d = VC.depth_at(VC.view(k), cam)
        ctx.frame_set_depth(d, cam, 1.0, *RANGE)
        ctx.volume_integrate(VC.view(k))
        want = VO.integrate(want, G, FO.frame_maps(d, cam, 1.0, *RANGE)[0], cam, VC.view(k))
    return G, want


OUTSIDE = pose12(rot(0.1, 0.25, 0.0), np.array([0.3, 0.1, 3.2]))   # camera centre ~(-1.0, -0.4, -3.1): behind the volume, looking in


@pytest.mark.parametrize("where", ["fused_view", "between_views", "outside_looking_in", "odd_camera"])
def test_raycast_bit_exact(gpu_ctx_factory, where):
    ctx = gpu_ctx_factory()
    G, vol = fused_room(ctx)
    assert same(ctx.volume_download(), vol)
    cam, p = SMALL_CAM, VC.view(1)
    if where == "between_views":
        p = VC.held_out_pose()
    elif where == "outside_looking_in":
        p = OUTSIDE
        C0 = -p[:9].reshape(3, 3).T @ p[9:]
        assert C0[2] < G.o[2]
    elif where == "odd_camera":
        cam, p = ODD_CAM, VC.view(2)
    ctx.volume_raycast(p, cam, *VC.RAY)
    MV, MN = VO.raycast(vol, G, cam, p, *VC.RAY)
    assert same(ctx.frame_download(L.MAP_MODEL_VERTEX), MV), where
    assert same(ctx.frame_download(L.MAP_MODEL_NORMAL), MN), where
    hit = ~np.isnan(MV).any(1)
    assert hit.mean() > (0.1 if where == "outside_looking_in" else 0.8), hit.mean()
    good = ~np.isnan(MN).any(1)
    assert good.mean() > 0.5 * hit.mean()
    # the normals point towards the camera
    C0 = -p[:9].reshape(3, 3).T @ p[9:]
    facing = np.einsum("ij,ij->i", MN[good].astype(np.float64), C0 - MV[good].astype(np.float64))
    assert (facing > 0).mean() > 0.98
    assert ctx.frame_camera(0, model=True) == tuple(float(x) if i < 4 else int(x) for i, x in enumerate(cam))


def test_raycast_of_an_empty_volume_is_all_nan(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    volume_pair(ctx)
    ctx.volume_raycast(VC.view(0), SMALL_CAM, *VC.RAY)
    assert np.isnan(ctx.frame_download(L.MAP_MODEL_VERTEX)).all() and np.isnan(ctx.frame_download(L.MAP_MODEL_NORMAL)).all()


@pytest.mark.parametrize("form", ["host", "fused", "device_fused"])
def test_raycast_model_is_interchangeable_with_an_upload(gpu_ctx_factory, form):
    forms = {"host": dict(device_resident=False, fused=False), "fused": dict(device_resident=False, fused=True),
             "device_fused": dict(device_resident=True, fused=True)}[form]
    cam = VC.HALF_CAM
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    fused_room(a, cam)
    pm = VC.view(1)
    a.volume_raycast(pm, cam, *VC.RAY, levels=3)
    MV, MN = a.frame_download(L.MAP_MODEL_VERTEX), a.frame_download(L.MAP_MODEL_NORMAL)
    b.model_upload(MV, MN, cam, pm).model_build_pyramid(3)
    for l in range(3):
        for m in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL):
            assert same(a.frame_download(m, l), b.frame_download(m, l)), (l, m)
        assert a.frame_camera(l, model=True) == b.frame_camera(l, model=True)
    d = VC.depth_at(VC.held_out_pose(), cam, 0.002, np.random.default_rng(1))
    for ctx in (a, b):
        ctx.frame_set_depth(d, cam, 1.0, *RANGE, levels=3)
    ra = a.icp_pyramid(pm, (5, 3, 3), (0.1, 0.15, 0.2), L.RES_P2PLANE, 0.0, 0.8, **forms)
    rb = b.icp_pyramid(pm, (5, 3, 3), (0.1, 0.15, 0.2), L.RES_P2PLANE, 0.0, 0.8, **forms)
    assert np.array_equal(ra[0], rb[0]) and ra[1:] == rb[1:]


def test_raycast_accuracy_against_the_rendered_depth(gpu_ctx_factory):
    cam = VC.HALF_CAM
    ctx = gpu_ctx_factory()
    dims, desc = VC.room_geometry(VC.ACC_VOXEL)
    ctx.volume_init(dims, **desc)
    for k in VC.ACC_VIEWS:
        ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, *RANGE)
        ctx.volume_integrate(VC.view(k))
    ctx.volume_raycast(VC.held_out_pose(), cam, *VC.RAY)
    med, p95, cover = VC.hit_depth_errors(ctx.frame_download(L.MAP_MODEL_VERTEX), VC.held_out_pose(), cam)
    print(f"raycast accuracy: median {med:.2e} m, p95 {p95:.2e} m, coverage {cover:.4f}")
    assert med < VC.ACC_MEDIAN and p95 < VC.ACC_P95 and cover > VC.ACC_COVERAGE, (med, p95, cover)


def test_tracking_loop_frame_to_model(gpu_ctx_factory):
    cam = VC.HALF_CAM
    depths = VC.track_depths(cam)
    levels = len(VC.TRACK_ITERS)
    ctx = gpu_ctx_factory()
    dims, desc = VC.room_geometry(VC.TRACK_VOXEL)
    ctx.volume_init(dims, **desc)
    est = [VC.track_pose(0)]
    ctx.frame_set_depth(depths[0], cam, 1.0, *RANGE, levels=levels)
    ctx.volume_integrate(est[0])
    stages = {"set_depth": 0.0, "raycast": 0.0, "icp": 0.0, "integrate": 0.0}
    for f in range(1, VC.TRACK_FRAMES):
        t0 = time.perf_counter()
        ctx.frame_set_depth(depths[f], cam, 1.0, *RANGE, levels=levels)
        t1 = time.perf_counter()
        ctx.volume_raycast(est[-1], cam, *VC.RAY, levels=levels)
        t2 = time.perf_counter()
        p = ctx.icp_pyramid(est[-1], VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)[0]
        t3 = time.perf_counter()
        ctx.volume_integrate(p)
        ctx.synchronize()
        t4 = time.perf_counter()
        for k, dt in zip(stages, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            stages[k] += dt
        est.append(p)
    errs = [VC.pose_error(e, VC.track_pose(f)) for f, e in enumerate(est)]
    # the same path frame to frame (model_from_frame of the previous frame at its estimate), for comparison only
    f2f = [VC.track_pose(0)]
    ctx.frame_set_depth(depths[0], cam, 1.0, *RANGE, levels=levels)
    ctx.model_from_frame(f2f[0])
    for f in range(1, VC.TRACK_FRAMES):
        ctx.frame_set_depth(depths[f], cam, 1.0, *RANGE, levels=levels)
        f2f.append(ctx.icp_pyramid(f2f[-1], VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)[0])
        ctx.model_from_frame(f2f[-1])
    drift = VC.pose_error(f2f[-1], VC.track_pose(VC.TRACK_FRAMES - 1))
    n = VC.TRACK_FRAMES - 1
    print(f"tracking: frame-to-model final error {errs[-1][0]:.2e} rad {errs[-1][1]:.2e} m; frame-to-frame {drift[0]:.2e} rad "
          f"{drift[1]:.2e} m; host ms per frame " + " ".join(f"{k} {1e3 * v / n:.3f}" for k, v in stages.items()))
    assert max(e[0] for e in errs) < VC.TRACK_ROT and max(e[1] for e in errs) < VC.TRACK_POS, errs


def test_frame_maps_survive_raycast_and_integrate(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    volume_pair(ctx)
    ctx.frame_set_depth(VC.depth_at(VC.view(0), SMALL_CAM), SMALL_CAM, 1.0, *RANGE, levels=3)
    before = [[ctx.frame_download(m, l) for m in (L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING, L.MAP_DEPTH)] for l in range(3)]
    ctx.volume_integrate(VC.view(0))
    ctx.volume_raycast(VC.view(1), ODD_CAM, *VC.RAY, levels=2)
    ctx.volume_integrate(VC.view(1))
    after = [[ctx.frame_download(m, l) for m in (L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING, L.MAP_DEPTH)] for l in range(3)]
    assert all(same(a, b) for la, lb in zip(before, after) for a, b in zip(la, lb))
    assert ctx.frame_camera(0) == SMALL_CAM and ctx.frame_camera(0, model=True)[4:] == ODD_CAM[4:]


def test_volume_errors_and_reinit(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    p = VC.view(0)
    for call in (lambda: ctx.volume_integrate(p), lambda: ctx.volume_raycast(p, SMALL_CAM, *VC.RAY)):
        with pytest.raises(L.RpeError) as e:
            call()
        assert e.value.code == L.RPE_ERR_STATE and "volume" in str(e.value)
    with pytest.raises(L.RpeError) as e:
        ctx.volume_download()
    assert e.value.code in (L.RPE_ERR_STATE, L.RPE_ERR_ARG)
    good = dict(voxel_size=0.05, origin=(0, 0, 0), trunc=0.15, max_weight=8)
    for dims, kw in [((1, 8, 8), {}), ((8, 8, 1025), {}), ((8, 8, 8), dict(voxel_size=0.0)), ((8, 8, 8), dict(voxel_size=float("nan"))),
                     ((8, 8, 8), dict(trunc=-1.0)), ((8, 8, 8), dict(max_weight=0)), ((8, 8, 8), dict(origin=(0, float("inf"), 0))),
                     ((8, 8, 8), dict(voxel_size=1e-50))]:
        with pytest.raises(L.RpeError) as e:
            ctx.volume_init(dims, **dict(good, **kw))
        assert e.value.code == L.RPE_ERR_ARG and "rpe_volume_init" in str(e.value), (dims, kw)
    ctx.volume_init((8, 8, 8), **good)
    with pytest.raises(L.RpeError) as e:
        ctx.volume_integrate(p)                                      # a volume, no frame
    assert e.value.code == L.RPE_ERR_STATE and "frame" in str(e.value)
    for cam, lo, hi in [((0.0, 100.0, 10.0, 10.0, 20, 20), 0.1, 5.0), ((100.0, 100.0, 10.0, 10.0, 0, 20), 0.1, 5.0),
                        (SMALL_CAM, 5.0, 1.0), (SMALL_CAM, -0.1, 5.0), (SMALL_CAM, 0.1, float("inf")), (SMALL_CAM, 0.1, 1e6)]:
        with pytest.raises(L.RpeError) as e:
            ctx.volume_raycast(p, cam, lo, hi)
        assert e.value.code == L.RPE_ERR_ARG, (cam, lo, hi)
    # re-initialising with other dims on the same context: smaller, then larger than the first allocation
    for voxel in (0.1, 0.05):
        G = volume_pair(ctx, voxel)
        assert same(ctx.volume_download(), G.empty())
        d = VC.depth_at(p, SMALL_CAM)
        ctx.frame_set_depth(d, SMALL_CAM, 1.0, *RANGE)
        ctx.volume_integrate(p)
        assert same(ctx.volume_download(), VO.integrate(G.empty(), G, FO.frame_maps(d, SMALL_CAM, 1.0, *RANGE)[0], SMALL_CAM, p))


def test_volume_track_cpp(tmp_path):
    """DepthFrontEnd::initVolume / integrate / raycast from plain C++ (tests/cpp/volume_track.cpp)."""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_track")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    assert r.returncode == 0 and "volume_track: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
