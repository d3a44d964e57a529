"""GPU parity of the depth filter (F0 of csrc/rpe_filter.hip behind rpe_frame_set_filter) against tests/filter_oracle.py: the maps of
rpe_frame_set_depth and of every level of rpe_frame_set_depth_pyramid are BIT-EXACT with the numpy statement, at sizes around the
kernel's 32 x 32 tile, for both raw types; the setting's state; and a short tracking run on a depth sensor's frames."""
import os
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import filter_oracle as FLO
import volume_cases as VC
from frontend_util import FO, SMALL_CAM
from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = (L.MAP_VERTEX, L.MAP_NORMAL, L.MAP_BEARING)
# 7 x 5: the window is wider than the image at radius 4.  37 x 29: odd, no row a multiple of 4, less than a tile (32) high; fx != fy and
# an off-centre principal point.  65 x 33: one pixel past a tile edge both ways.  160 x 120: rows of whole float4s, 5 x 4 tiles.
SIZES = {(7, 5): FC.CENTRED_CAM(7, 5), (37, 29): FC.ODD_CAM(37, 29), (65, 33): FC.CENTRED_CAM(65, 33), (160, 120): SMALL_CAM}
CASES = [(wh, r) for wh in SIZES for r in (1, 4)] + [((160, 120), 3)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def levels_of(cam):
    return min(3, max(l for l in range(1, L.MAX_LEVELS + 1) if cam[4] >> (l - 1) >= 1 and cam[5] >> (l - 1) >= 1))


def filt_of(radius):
    return (radius, 0.5 + 0.5 * radius, 0.01, 0.02)


def contents(wh, u16):
    """[(name, raw image, scale)] for one size: holes of every kind, a step on the first tile boundary (or mid-image), sensor noise"""
    w, h = wh
    out = [("holes", *FC.holes(w, h, 3, u16)), ("step", *FC.step(w, h, 4, u16, column=min(32, w // 2), row=min(32, (2 * h) // 3))),
           ("noise", *FC.as_type(FC.noisy_surface(w, h, 6), u16))]
    if wh == (160, 120):
        out.append(("room", *FC.room(SMALL_CAM, u16=u16)))
    return out


def check_frame(ctx, img, cam, scale, rng, filt, what):
    """both entry points against the statement: every map of every level"""
    levels = levels_of(cam)
    ctx.frame_set_depth(img, cam, scale, *rng, levels=1)
    for m, want in zip(MAPS, FLO.frame_maps(img, cam, scale, *rng, filt)):
        assert same(ctx.frame_download(m), want), (what, "set_depth", m)
    if levels < 2:
        return
    ctx.frame_set_depth(img, cam, scale, *rng, levels=levels)
    for l, (z, V, N, B) in enumerate(FLO.frame_pyramid(img, cam, scale, *rng, levels, filt)):
        assert same(ctx.frame_download(L.MAP_DEPTH, l), z.reshape(-1)), (what, "depth", l)
        for m, want in zip(MAPS, (V, N, B)):
            assert same(ctx.frame_download(m, l), want), (what, l, m)


@pytest.mark.parametrize("u16", [True, False], ids=["u16", "f32"])
@pytest.mark.parametrize("wh,radius", CASES, ids=[f"{w}x{h}-r{r}" for (w, h), r in CASES])
def test_filtered_frames_bit_exact(gpu_ctx_factory, wh, radius, u16):
    cam, filt = SIZES[wh], filt_of(radius)
    ctx = gpu_ctx_factory()
    ctx.frame_set_filter(*filt)
    assert ctx.frame_filter() == filt
    for name, img, scale in contents(wh, u16):
        rng = VC.RANGE if name == "room" else FC.RANGE
        check_frame(ctx, img, cam, scale, rng, filt, name)
        if name == "noise":   # the filter did something: the filtered depth is not the metric depth
            assert not same(FLO.filtered_depth(img, scale, *rng[:2], filt), FLO.PO.metric_depth(img, scale, *rng[:2]))


@pytest.mark.parametrize("wh", [(37, 29), (160, 120)])
def test_every_valid_neighbour_counts_under_a_large_constant_cut(gpu_ctx_factory, wh):
    filt = (4, 2.5, 50.0, 0.0)
    ctx = gpu_ctx_factory()
    ctx.frame_set_filter(*filt)
    for u16 in (True, False):
        img, scale = FC.holes(*wh, 9, u16)
        check_frame(ctx, img, SIZES[wh], scale, FC.RANGE, filt, ("large cut", u16))


@pytest.mark.parametrize("wh", [(7, 5), (65, 33)])
def test_an_all_invalid_image_gives_nan_maps_and_no_error(gpu_ctx_factory, wh):
    cam, filt = SIZES[wh], filt_of(4)
    ctx = gpu_ctx_factory()
    ctx.frame_set_filter(*filt)
    w, h = wh
    for img, scale in ((np.zeros((h, w), np.uint16), 0.001), (np.full((h, w), np.nan, np.float32), 1.0), (np.full((h, w), 9.5, np.float32), 1.0)):
        check_frame(ctx, img, cam, scale, FC.RANGE, filt, "all invalid")
        assert np.isnan(ctx.frame_download(L.MAP_VERTEX)).all() and np.isnan(ctx.frame_download(L.MAP_NORMAL)).all()
        assert not np.isnan(ctx.frame_download(L.MAP_BEARING)).any()


def downloads(ctx, levels):
    return [ctx.frame_download(m, l) for l in range(levels) for m in MAPS + ((L.MAP_DEPTH,) if levels > 1 else ())]


def test_filter_set_and_cleared_gives_the_bits_of_a_context_that_never_had_it(gpu_ctx_factory):
    img, scale = FC.room(SMALL_CAM)
    fresh, ctx, other = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    assert ctx.frame_filter() == (0, 0.0, 0.0, 0.0)                         # off by default
    for levels in (1, 3):
        fresh.frame_set_depth(img, SMALL_CAM, scale, *VC.RANGE, levels=levels)
        want = downloads(fresh, levels)
        ctx.frame_set_filter()                                              # the Python defaults
        assert ctx.frame_filter() == FC.DEFAULT_FILTER
        ctx.frame_set_depth(img, SMALL_CAM, scale, *VC.RANGE, levels=levels)
        filtered = downloads(ctx, levels)
        assert not same(filtered[0], want[0])
        other.frame_set_depth(img, SMALL_CAM, scale, *VC.RANGE, levels=levels)   # a second context without the filter is unaffected
        assert all(same(a, b) for a, b in zip(downloads(other, levels), want))
        ctx.frame_set_filter(0)
        assert ctx.frame_filter() == (0, 0.0, 0.0, 0.0)
        assert all(same(a, b) for a, b in zip(downloads(ctx, levels), filtered))   # the setting does not touch the current frame
        ctx.frame_set_depth(img, SMALL_CAM, scale, *VC.RANGE, levels=levels)
        assert all(same(a, b) for a, b in zip(downloads(ctx, levels), want))
    L.check(L.lib().rpe_frame_set_filter(ctx._h, None))                     # NULL = off
    assert ctx.frame_filter()[0] == 0


def test_a_change_of_radius_and_size_between_frames(gpu_ctx_factory):
    """the filtered buffer is made on first use, regrown for a larger frame and reused for a smaller one; the table follows the radius"""
    ctx = gpu_ctx_factory()
    for wh, radius, u16 in (((37, 29), 4, True), ((160, 120), 1, False), ((65, 33), 3, True), ((160, 120), 4, True), ((7, 5), 2, False)):
        filt = filt_of(radius)
        ctx.frame_set_filter(*filt)
        img, scale = FC.holes(*wh, 12, u16)
        check_frame(ctx, img, SIZES[wh], scale, FC.RANGE, filt, (wh, radius))


def test_argument_errors_leave_the_setting_alone(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    good = (2, 1.5, 0.02, 0.005)
    ctx.frame_set_filter(*good)
    nan, inf = float("nan"), float("inf")
    bad = [(-1, 2.0, 0.01, 0.02), (L.FILTER_MAX_RADIUS + 1, 2.0, 0.01, 0.02), (3, 0.0, 0.01, 0.02), (3, -1.0, 0.01, 0.02), (3, nan, 0.01, 0.02),
           (3, inf, 0.01, 0.02), (3, 2.0, 0.0, 0.02), (3, 2.0, -0.01, 0.02), (3, 2.0, nan, 0.02), (3, 2.0, inf, 0.02), (3, 2.0, 0.01, -1e-9),
           (3, 2.0, 0.01, nan), (3, 2.0, 0.01, inf)]
    for f in bad:
        with pytest.raises(L.RpeError) as e:
            ctx.frame_set_filter(*f)
        assert e.value.code == L.RPE_ERR_ARG, f
        assert ctx.frame_filter() == good, f
    assert L.lib().rpe_frame_get_filter(ctx._h, None) == L.RPE_ERR_ARG
    ctx.frame_set_filter(3, 2.0, 0.01, 0.0)                                 # depth_cut_z2 = 0 is a constant cut, not an error
    assert ctx.frame_filter() == (3, 2.0, 0.01, 0.0)
    for r in range(1, L.FILTER_MAX_RADIUS + 1):
        ctx.frame_set_filter(r)
        assert ctx.frame_filter()[0] == r


def test_the_worth_of_it_on_the_device(gpu_ctx_factory):
    """filter_cases' figures from the device's maps: they are the oracle's bits"""
    cam = VC.HALF_CAM
    d = FC.sensor_frame(FC.WORTH_FRAME, cam)
    Nt = FO.frame_maps(FC.true_frame(FC.WORTH_FRAME, cam), cam, 1.0, *VC.RANGE)[1]
    ctx = gpu_ctx_factory()
    ctx.frame_set_depth(d, cam, FC.U16_SCALE, *VC.RANGE)
    raw = FC.normal_angles(ctx.frame_download(L.MAP_NORMAL), Nt)
    ctx.frame_set_filter()
    ctx.frame_set_depth(d, cam, FC.U16_SCALE, *VC.RANGE)
    fil = FC.normal_angles(ctx.frame_download(L.MAP_NORMAL), Nt)
    print("raw", raw, "filtered", fil)
    assert fil[0] <= raw[0] / 3 and fil[1] >= raw[1]
    assert abs(raw[0] - FC.WORTH_RAW_DEG) < 0.05 and raw[1] == FC.WORTH_RAW_NORMALS
    assert abs(fil[0] - FC.WORTH_FILTERED_DEG) < 0.05 and fil[1] == FC.WORTH_FILTERED_NORMALS


def test_tracking_run_on_sensor_frames(gpu_ctx_factory):
    """set_depth_pyramid -> raycast -> model pyramid -> icp_pyramid -> integrate over the first three sensor frames, filter on: within
    twice the oracle loop's recorded errors (the ICP sums round differently), and pairing far more pixels than the raw frames do"""
    cam, levels = VC.HALF_CAM, len(VC.TRACK_ITERS)
    dims, desc = VC.room_geometry(VC.TRACK_VOXEL)
    pairs = {}
    for name, filt in (("filtered", FC.TRACK_FILTER), ("raw", None)):
        ctx = gpu_ctx_factory()
        if filt:
            ctx.frame_set_filter(*filt)
        ctx.volume_init(dims, **desc)
        est = [VC.track_pose(0)]
        ctx.frame_set_depth(FC.sensor_frame(0, cam), cam, FC.U16_SCALE, *VC.RANGE, levels=levels)
        ctx.volume_integrate(est[0])
        pairs[name] = []
        for f in range(1, FC.GPU_LOOP_FRAMES):
            ctx.frame_set_depth(FC.sensor_frame(f, cam), cam, FC.U16_SCALE, *VC.RANGE, levels=levels)
            ctx.volume_raycast(est[-1], cam, *VC.RAY, levels=levels)
            r = ctx.icp_pyramid(est[-1], VC.TRACK_ITERS, VC.TRACK_GATES, L.RES_P2PLANE, 1e-6, 0.8)
            pairs[name].append(int(r[-1]))
            ctx.volume_integrate(r[0])
            est.append(r[0])
        errs = [VC.pose_error(e, VC.track_pose(f)) for f, e in enumerate(est)]
        print(name, "pairs", pairs[name], "errors", errs)
        if filt:
            assert max(e[0] for e in errs) <= FC.GPU_LOOP_ROT and max(e[1] for e in errs) <= FC.GPU_LOOP_POS, errs
    assert all(f >= 2 * r for f, r in zip(pairs["filtered"], pairs["raw"])), pairs


def test_depth_filter_cpp(tmp_path):
    """DepthFrontEnd::setDepthFilter / depthFilter from plain C++ (tests/cpp/depth_filter.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "depth_filter")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "depth_filter.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "depth_filter: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
