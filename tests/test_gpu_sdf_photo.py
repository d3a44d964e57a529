"""GPU parity of the volume colour term (sdf_photo_rows_kernel, icp_sdf_photo_kernel of csrc/rpe_sdf_photo.hpp) against
tests/sdf_photo_oracle.py: the per-pixel rows are BIT-EXACT with the oracle at every level (NaN for NaN) on volumes that exercise every
gate, the sums are within their rounding bound, one round of rpe_icp_sdf_rgbd is the oracle's step, the wall -- a scene the volume term
alone loses -- and the room are tracked with no raycast and no model, the calls' own intensity pyramid follows the frame, and the state
rules of the header hold."""
import ctypes as C_
import os
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import photo_cases as PC
import sdf_cases as SC
import sdf_oracle as SO
import sdf_photo_cases as C
import sdf_photo_oracle as SP
import volume_cases as VC
from frontend_util import SMALL_CAM
from rgbd_pose_estimation_amd import _lib as L, api
from test_gpu_clean_first import _ctx
from test_gpu_photo import close, raises, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = VC.RANGE
CAMS = [SMALL_CAM, SC.RAGGED_CAM]
CAM_IDS = ["160x120", "161x119"]
BOUND = 8 * 2.0 ** -24
# The frame's colour goes through frame_register_color with the depth camera's own intrinsics, the identity pose and a limit on
# x^2 + y^2: the only way to a frame colour with A = 0 at pixels that have a vertex (the corners of the image here, 4 % of it, in place
# of a random 1 %: frame_set_color gives A = 255 everywhere).  The oracle is fed the RGBA the device holds.
R2_MAX = 0.40


def volumes():
    """the room fused with colour; spoiled (NaN tsdf, lost colour weights, NaN / Inf colour bits); the spoiled room cropped to a slab"""
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    svol, scvol = SC.spoiled(vol), C.spoiled_color(cvol)
    cd, cdesc, cG, cvol3 = SC.cropped(dims, desc, svol)
    return {"room": (dims, desc, G, vol, cvol), "spoiled": (dims, desc, G, svol, scvol), "crop": (cd, cdesc, cG, cvol3, C.cropped_color(scvol))}


def set_frame(ctx, cam, depth, rgb, levels=C.LEVELS, a0=True):
    """depth (with its holes) and colour set; returns [(V, N, If)] per level as the oracle sees the frame the device holds"""
    ctx.frame_set_depth(depth, cam, 1.0, *RANGE, levels=levels)
    if a0:
        ctx.frame_register_color(rgb, api.Context.color_rig(cam, r2_max=R2_MAX, cell=0))
    else:
        ctx.frame_set_color(rgb)
    rgba = ctx.frame_color().reshape(-1, 4)
    return C.frame_levels(cam, depth, rgba)[:levels], rgba


def load(ctx, cam, volume, levels=C.LEVELS):
    dims, desc, G, vol, cvol = volume
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(np.ascontiguousarray(cvol).view(np.float16))
    return set_frame(ctx, cam, SC.frame_depth(cam), C.rgb_at(VC.held_out_pose(), cam), levels)[0]


# ---------------------------------------------------------------------------------------------- rows bit-exact, every gate exercised
@pytest.mark.parametrize("cam", CAMS, ids=CAM_IDS)
@pytest.mark.parametrize("which", ["room", "spoiled", "crop"])
def test_rows_are_bit_exact_at_every_level(gpu_ctx_factory, which, cam):
    ctx = gpu_ctx_factory()
    volume = volumes()[which]
    _, _, G, vol, cvol = volume
    lv = load(ctx, cam, volume)
    rejected = {k: 0 for k in ("finite", "intensity", "cell", "edge", "known", "band", "nan_tsdf", "distance", "colour", "not_finite_rows")}
    for pi, pose in enumerate(SC.poses()):
        for l in range(C.LEVELS):
            gate = VC.TRACK_GATES[l]
            V, N, If = lv[l]
            st = {}
            r, J, ok = SP.rows(vol, cvol, G, V, If, pose, gate, st)
            got = ctx.sdf_photo_rows(pose, l, gate)
            assert got.shape == (7, len(V))
            assert same(got[0], r) and same(got[1:].T, J), (which, pi, l, np.isnan(got[0]).sum(), np.isnan(r).sum())
            if pi == 0 and which == "room":      # the coverage condition: no passing on an empty answer
                assert ok.sum() / len(V) >= C.COVER - 0.05, (l, ok.sum() / len(V))   # (the corners' A = 0 cost 4 %)
            # which gate turned pixels away, each counted only among the pixels that every earlier gate let through
            a = st["finite"]
            b = a & st["intensity"]
            c = b & st["cell"]
            d = c & st["known"]
            e = d & st["band"]
            f = e & st["distance"]
            rejected["finite"] += int((~a).sum())
            rejected["intensity"] += int((a & ~st["intensity"]).sum())
            rejected["cell"] += int((b & ~st["cell"]).sum())
            rejected["edge"] += int(max((c & (st["i0"][ax] == G.dim[ax] - 2)).sum() for ax in range(3)))
            rejected["known"] += int((c & ~st["known"]).sum())
            rejected["band"] += int((d & ~st["band"] & ~st["nan_tsdf"]).sum())
            rejected["nan_tsdf"] += int((d & st["nan_tsdf"]).sum())
            rejected["distance"] += int((e & ~st["distance"]).sum())
            rejected["colour"] += int((f & ~st["colour"]).sum())
            rejected["not_finite_rows"] += int((ok & ~np.isfinite(r)).sum())
    print(which, cam[4], "rejected by", rejected)
    need = set(rejected) - ({"nan_tsdf", "colour", "not_finite_rows"} if which == "room" else set())     # (the room is uploaded clean)
    assert all(rejected[k] > 0 for k in need), rejected


# ---------------------------------------------------------------------------------------------- the record
def check_record(got, rec, S, entries, what):
    err = np.abs(got[entries] - rec[entries])
    ratio = float((err / (2.0 ** -24 * S[entries])).max())
    assert (err <= BOUND * S[entries]).all(), (what, err / (2.0 ** -24 * S[entries]))
    return ratio


@pytest.mark.parametrize("cam", CAMS, ids=CAM_IDS)
def test_records_within_the_rounding_bound(gpu_ctx_factory, cam):
    """row counts equal; every entry within 8 * 2^-24 * S of the fp64 sum of the exact products of the fp32 rows, S the sum of the
    products' magnitudes.  The kernel widens each fp32 row and adds its products with fp64 fused multiply-adds -- a product of two
    floats is exact in fp64 -- so what a sum carries is fp64 accumulation error, orders below the bound (the worst ratio is printed).
    The combined round's H and g are not handed out by any entry point: the round is held through its two costs and counts here and
    through the step it takes (test_one_round_is_the_oracles_step)."""
    ctx = gpu_ctx_factory()
    volume = volumes()["crop"]
    _, _, G, vol, cvol = volume
    lv = load(ctx, cam, volume)
    # the spoiled colours make sums that are not finite, on the GPU exactly as in the oracle: the same entries
    pose = SC.poses()[0]
    V, N, If = lv[0]
    rec, _ = SP.record(*SP.rows(vol, cvol, G, V, If, pose, 0.1), C.WEIGHT)
    got = ctx.sdf_photo_normal_eq(pose, 0, 0.1, C.WEIGHT)
    assert got[28] == rec[28] > 0 and not np.isfinite(rec[:28]).any() and np.array_equal(np.isfinite(got[:28]), np.isfinite(rec[:28]))
    # ... so the bound is checked with the colour bits mended (weights still lost, tsdf still NaN)
    mended = np.where(np.isfinite(CO.f32(cvol)), cvol, CO.h(np.float32(128))).astype(np.uint16)
    ctx.volume_color_upload(mended.view(np.float16))
    worst = 0.0
    for pose in SC.poses()[:2]:
        for l in range(C.LEVELS):
            gate = VC.TRACK_GATES[l]
            V, N, If = lv[l]
            pho = SP.rows(vol, mended, G, V, If, pose, gate)
            rec, S = SP.record(*pho, C.WEIGHT)
            got = ctx.sdf_photo_normal_eq(pose, l, gate, C.WEIGHT)
            assert got[28] == rec[28] > 0.15 * len(V)
            worst = max(worst, check_record(got, rec, S, slice(0, 28), ("photo", l)))
            assert got[29] == 16 * 2.0 ** -24 and got[30] == 0 and got[31] == 0
            if l > 0:
                continue
            for use_normals in (True, False):      # the combined round, through rpe_icp_sdf_rgbd's own figures
                crec, cS = SP.combined(SO.rows(vol, G, V, N, pose, gate, SC.COS_THR, use_normals), pho, C.WEIGHT)
                p, it, step, cost, m, pcost, pm = ctx.icp_sdf_rgbd(pose, C.WEIGHT, 1, 0.0, gate, SC.COS_THR, use_normals)
                assert (m, pm) == (int(crec[28]), int(crec[30])) and m > 0.15 * len(V)
                worst = max(worst, check_record(np.array([cost, pcost]), crec[[27, 29]], cS[[27, 29]], slice(0, 2), ("costs", use_normals)))
    print("worst error / (2^-24 S):", worst)


# ---------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("cam", CAMS, ids=CAM_IDS)
def test_one_round_is_the_oracles_step(gpu_ctx_factory, oracle, cam):
    ctx = gpu_ctx_factory()
    volume = volumes()["room"]
    _, _, G, vol, cvol = volume
    lv = load(ctx, cam, volume)
    start = SC.poses()[1]
    V, N, If = lv[0]
    for use_normals in (True, False):
        po, hist = SP.icp_sdf_rgbd(oracle, vol, cvol, G, V, N, If, start, 1, 0.1, SC.TRACK_COS, C.WEIGHT, use_normals)
        p, it, step, cost, m, pcost, pm = ctx.icp_sdf_rgbd(start, C.WEIGHT, 1, 0.0, 0.1, SC.TRACK_COS, use_normals)
        assert it == 1 and close(p, po, 1e-6), (p, po)
        assert (m, pm) == hist[-1][:2] and abs(step - hist[-1][2]) < 1e-6 and step > 1e-3 and cost > 0 and pcost > 0
        # ... and the step put together from the two terms' own records
        ne = ctx.sdf_normal_eq(start, 0, 0.1, SC.TRACK_COS, use_normals)
        pe = ctx.sdf_photo_normal_eq(start, 0, 0.1, C.WEIGHT)
        ne[:27] += pe[:27]
        assert close(p, api.gn_apply(api.gn_solve(ne), start), 1e-6) and m == int(ne[28]) and pm == int(pe[28])
    # a few rounds, and the pyramid form, against the oracle's
    po, hist = SP.icp_sdf_rgbd(oracle, vol, cvol, G, V, N, If, start, 6, 0.1, SC.TRACK_COS, C.WEIGHT)
    p, it, step, cost, m, pcost, pm = ctx.icp_sdf_rgbd(start, C.WEIGHT, 6, 0.0, 0.1, SC.TRACK_COS)
    assert it == 6 and close(p, po, 1e-5), (p, po)
    frame_pyr = [(None, V_, N_, None) for V_, N_, _ in lv]
    po, hist = SP.icp_pyramid_sdf_rgbd(oracle, vol, cvol, G, frame_pyr, [x[2] for x in lv], start, VC.TRACK_ITERS, VC.TRACK_GATES, SC.TRACK_COS,
                                       C.WEIGHT)
    p, its, step, cost, m, pcost, pm = ctx.icp_pyramid_sdf_rgbd(start, C.WEIGHT, VC.TRACK_ITERS, VC.TRACK_GATES, 0.0, SC.TRACK_COS)
    assert its == VC.TRACK_ITERS and close(p, po, 1e-5), (p, po)
    assert abs(m - hist[-1][0]) <= 2 + 1e-4 * hist[-1][0] and abs(pm - hist[-1][1]) <= 2 + 1e-4 * hist[-1][1]


def gpu_loop(ctx, poses, frames, geometry, cam=VC.HALF_CAM):
    """sdf_photo_cases.oracle_loop on the GPU: no raycast, no model, no photo_prepare"""
    dims, desc = geometry
    ctx.volume_init(dims, **desc)

    def frame(f):
        ctx.frame_set_depth(frames[f][0], cam, 1.0, *RANGE, levels=C.LEVELS)
        ctx.frame_set_color(frames[f][1])
    frame(0)
    ctx.volume_integrate_color(poses[0])
    est, errs, rows = [poses[0]], [], []
    for f in range(1, len(poses)):
        frame(f)
        p, its, step, cost, m, pcost, pm = ctx.icp_pyramid_sdf_rgbd(est[-1], C.WEIGHT, VC.TRACK_ITERS, VC.TRACK_GATES, 0.0, C.COS_THR)
        ctx.volume_integrate_color(p)
        est.append(p)
        errs.append(VC.pose_error(p, poses[f]))
        rows.append((m, pm))
    return errs, rows


def test_wall_tracking_loop(gpu_ctx_factory):
    poses, frames, geometry = C.loop_scene("wall")
    ctx = gpu_ctx_factory()
    errs, rows = gpu_loop(ctx, poses, frames, geometry)
    lim = C.wall_limit()
    print("wall loop with the colour term:", errs, "rows", rows, "oracle worst", C.WALL_LOOP_RGBD, "the volume term alone", C.WALL_LOOP_SDF)
    assert len(errs) == PC.WALL_FRAMES - 1 and all(e[0] <= lim[0] and e[1] <= lim[1] for e in errs), (errs, lim)
    assert all(C.WALL_ROWS[0][0] <= g <= C.WALL_ROWS[0][1] and C.WALL_ROWS[1][0] <= p <= C.WALL_ROWS[1][1] for g, p in rows), rows
    raises(L.RPE_ERR_STATE, ctx.associate, poses[-1])          # there never was a model


def test_room_tracking_loop(gpu_ctx_factory):
    poses, frames, geometry = C.loop_scene("room")
    errs, rows = gpu_loop(gpu_ctx_factory(), poses, frames, geometry)
    lim = C.room_limit()
    print("room loop with the colour term:", errs, "rows", rows, "oracle worst", C.ROOM_LOOP_RGBD, "the volume term alone", C.ROOM_LOOP_SDF)
    assert len(errs) == VC.TRACK_FRAMES - 1 and all(e[0] <= lim[0] and e[1] <= lim[1] for e in errs), (errs, lim)
    assert all(C.ROOM_ROWS[0][0] <= g <= C.ROOM_ROWS[0][1] and C.ROOM_ROWS[1][0] <= p <= C.ROOM_ROWS[1][1] for g, p in rows), rows


# ---------------------------------------------------------------------------------------------- the calls' own intensity pyramid
def test_the_intensity_pyramid_follows_the_frame(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    cam = SC.RAGGED_CAM
    volume = volumes()["room"]
    _, _, G, vol, cvol = volume
    lv = load(ctx, cam, volume)
    pose = SC.poses()[1]

    def check(lv):
        out = []
        for l in range(C.LEVELS):
            V, N, If = lv[l]
            r, J, ok = SP.rows(vol, cvol, G, V, If, pose, 0.15)
            got = ctx.sdf_photo_rows(pose, l, 0.15)
            assert same(got[0], r) and same(got[1:].T, J) and ok.sum() > 0.5 * len(V), l
            out.append(got)
        return out
    first = check(lv)
    again = check(lv)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, again))      # twice: identical bits
    a = ctx.sdf_photo_normal_eq(pose, 1, 0.15, C.WEIGHT)
    assert np.array_equal(a, ctx.sdf_photo_normal_eq(pose, 1, 0.15, C.WEIGHT))
    # a new colour on the same depth: the pyramid is rebuilt, the rows change accordingly
    other = C.rgb_at(VC.view(1), cam)
    ctx.frame_set_color(other)
    lv2 = C.frame_levels(cam, SC.frame_depth(cam), CO.frame_rgba(other))
    second = check(lv2)
    assert not any(same(a[0], b[0]) for a, b in zip(first, second))
    # a new depth drops the colour (RPE_ERR_STATE until there is one again), and the pyramid follows the new frame
    depth = SC.frame_depth(cam, VC.view(1))
    ctx.frame_set_depth(depth, cam, 1.0, *RANGE, levels=C.LEVELS)
    raises(L.RPE_ERR_STATE, ctx.sdf_photo_rows, pose)
    ctx.frame_set_color(other)
    third = check(C.frame_levels(cam, depth, CO.frame_rgba(other)))
    assert not any(same(a[0], b[0]) for a, b in zip(second, third))
    # fewer levels than before: the old pyramid is not mistaken for the new frame's
    ctx.frame_set_depth(depth, cam, 1.0, *RANGE, levels=2)
    ctx.frame_set_color(C.rgb_at(VC.held_out_pose(), cam))
    lv4 = C.frame_levels(cam, depth, CO.frame_rgba(C.rgb_at(VC.held_out_pose(), cam)))
    V, N, If = lv4[1]
    r, J, ok = SP.rows(vol, cvol, G, V, If, pose, 0.15)
    got = ctx.sdf_photo_rows(pose, 1, 0.15)
    assert same(got[0], r) and same(got[1:].T, J)
    raises(L.RPE_ERR_STATE, ctx.sdf_photo_rows, pose, 2)


# ---------------------------------------------------------------------------------------------- state rules
def raw_icp(ctx, pose, weight, device_resident=0, max_iter=2, dist_thr=0.1, kind=L.RES_P2PLANE, fused=1):
    p = np.array(pose, np.float64).copy()
    o = L.RpeIcpOptions(kind, max_iter, 0.0, dist_thr, 0.8, 1, device_resident, fused)
    rc = L.lib().rpe_icp_sdf_rgbd(ctx._h, C_.byref(o), weight, p.ctypes.data_as(C_.c_void_p), None, None, None, None, None, None)
    return rc, p


def test_state_and_argument_rules(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    cam = SMALL_CAM
    held = VC.held_out_pose()
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    calls = (lambda: ctx.sdf_photo_rows(held), lambda: ctx.sdf_photo_normal_eq(held), lambda: ctx.icp_sdf_rgbd(held),
             lambda: ctx.icp_pyramid_sdf_rgbd(held, C.WEIGHT, (2, 2)))
    for call in calls:
        raises(L.RPE_ERR_STATE, call)                                        # nothing there
    ctx.frame_set_depth(SC.frame_depth(cam), cam, 1.0, *RANGE, levels=2)
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    for call in calls:
        raises(L.RPE_ERR_STATE, call)                                        # no frame colour
    ctx.frame_set_color(C.rgb_at(held, cam))
    for call in calls:
        call()
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    for call in calls:
        raises(L.RPE_ERR_STATE, call)                                        # a volume without a colour volume
    ctx.icp_sdf(held)                                                        # (the volume term itself runs)
    ctx.volume_color_upload(cvol.view(np.float16))
    ctx.sdf_photo_rows(held, 1)
    raises(L.RPE_ERR_STATE, ctx.sdf_photo_rows, held, 2)                    # the frame has 2 levels
    raises(L.RPE_ERR_STATE, ctx.sdf_photo_normal_eq, held, 2)
    raises(L.RPE_ERR_STATE, ctx.icp_pyramid_sdf_rgbd, held, C.WEIGHT, (2, 2, 2))
    other = gpu_ctx_factory()
    other.volume_init(dims, **desc)
    other.volume_upload(vol)
    other.volume_color_upload(cvol.view(np.float16))
    raises(L.RPE_ERR_STATE, other.icp_sdf_rgbd, held)                       # both volumes, no frame
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        assert raw_icp(ctx, held, bad)[0] == L.RPE_ERR_ARG
        raises(L.RPE_ERR_ARG, ctx.sdf_photo_normal_eq, held, 0, 0.1, bad)
        raises(L.RPE_ERR_ARG, ctx.icp_pyramid_sdf_rgbd, held, bad, (2, 2))
    assert raw_icp(ctx, held, C.WEIGHT, device_resident=1)[0] == L.RPE_ERR_ARG
    assert raw_icp(ctx, held, C.WEIGHT, max_iter=0)[0] == L.RPE_ERR_ARG
    assert raw_icp(ctx, held, C.WEIGHT, dist_thr=-1.0)[0] == L.RPE_ERR_ARG
    raises(L.RPE_ERR_ARG, ctx.sdf_photo_rows, held, 0, float("nan"))
    raises(L.RPE_ERR_ARG, ctx.sdf_photo_rows, held, -1)
    raises(L.RPE_ERR_ARG, ctx.icp_pyramid_sdf_rgbd, held, C.WEIGHT, (0, 2))  # level 0 needs a round
    raises(L.RPE_ERR_ARG, ctx.icp_pyramid_sdf_rgbd, held, C.WEIGHT, (2, 2), (0.1, -0.1))
    a = raw_icp(ctx, held, C.WEIGHT)                                         # kind and fused are not consulted
    for kind, fused in ((L.RES_P2P, 0), (77, 0)):
        b = raw_icp(ctx, held, C.WEIGHT, kind=kind, fused=fused)
        assert a[0] == b[0] == L.RPE_OK and np.array_equal(a[1], b[1])
    # a round with a failed solve: empty volumes give no row at all
    ctx.volume_init(dims, **desc)
    ctx.volume_color_upload(np.zeros_like(cvol).view(np.float16))
    with pytest.raises(L.RpeError) as e:
        ctx.icp_sdf_rgbd(held)
    assert e.value.code == L.RPE_ERR_DEGENERATE
    assert ctx.sdf_photo_normal_eq(held)[28] == 0 and np.isnan(ctx.sdf_photo_rows(held)).all()


def test_the_term_touches_nothing_else(gpu_ctx_factory):
    """the model maps, the model colour, the prepared photometric maps, an rpe_icp result, the solver slots, both volumes and sdf_rows'
    output are bit-identical before and after the four calls"""
    ctx = gpu_ctx_factory()
    cam = SMALL_CAM
    pa, da, ca, pb, db, cb = PC.pair(None, cam)
    dims, desc, G, vol, cvol = C.room_volume(SMALL_CAM)
    ctx.volume_init(dims, **desc)
    ctx.volume_upload(vol)
    ctx.volume_color_upload(cvol.view(np.float16))
    ctx.frame_set_depth(da, cam, 1.0, *RANGE, levels=3)
    ctx.frame_set_color(ca)
    ctx.model_from_frame(pa)
    ctx.model_color_from_frame()
    ctx.frame_set_depth(db, cam, 1.0, *RANGE, levels=3)
    ctx.frame_set_color(cb)
    ctx.photo_prepare(3)

    def snapshot():
        maps = [ctx.frame_download(w, l) for w in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL) for l in range(3)]
        photo = [ctx.photo_download(w, l) for w in (L.PHOTO_FRAME, L.PHOTO_MODEL) for l in range(3)]
        colour = ctx.model_color_map()
        vols = ctx.volume_download(), ctx.volume_color_download()
        rows = [ctx.sdf_rows(pa, l) for l in range(3)]
        icp = ctx.icp(pa, L.RES_P2PLANE, 5, 0.0, 0.1, 0.8, fused=True)
        pairs = ctx.associate(pa, 0.1, 0.8, True)
        slots = [ctx.download(k) for k in (L.XW, L.XC, L.NC)]
        return maps, photo, colour, vols, rows, icp, pairs, slots
    before = snapshot()
    ctx.associate(pa, 0.1, 0.8, True)
    ctx.sdf_photo_rows(pa, 1)
    ctx.sdf_photo_normal_eq(pa, 2)
    ctx.icp_sdf_rgbd(pa, C.WEIGHT, 3)
    ctx.icp_pyramid_sdf_rgbd(pa, C.WEIGHT, (2, 2, 2))
    slots = [ctx.download(k) for k in (L.XW, L.XC, L.NC)]
    assert all(same(x, y) for x, y in zip(slots, before[7]))              # the solver slots still hold the pairs
    ctx.photo_rows(pa, 2)                                                  # the prepared maps survived
    after = snapshot()
    assert all(same(x, y) for x, y in zip(before[0], after[0])) and all(same(x, y) for x, y in zip(before[1], after[1]))
    assert np.array_equal(before[2], after[2])
    assert same(before[3][0], after[3][0]) and np.array_equal(before[3][1].view(np.uint16), after[3][1].view(np.uint16))
    assert np.array_equal(before[3][1].view(np.uint16), np.asarray(cvol))
    assert all(same(x, y) for x, y in zip(before[4], after[4]))
    assert np.array_equal(before[5][0], after[5][0]) and before[5][1:] == after[5][1:] and before[6] == after[6]
    assert all(same(x, y) for x, y in zip(before[7], after[7]))


# ---------------------------------------------------------------------------------------------- full size
def test_one_full_size_round():
    """640 x 480 against a 128^3 volume with colour, in 64 workgroups of 512 threads: ten trips of the grid-stride loop in the
    512-thread instances.  One round of each kernel: the counts and the bound only"""
    cam = SC.FULL_CAM
    ctx = _ctx({"RPE_BLOCK": "512", "RPE_MAX_BLOCKS": "64"})
    try:
        dims, desc = (128, 128, 128), dict(voxel_size=0.05, origin=(-2.8, -1.9, -1.6), trunc=0.15, max_weight=64)
        ctx.volume_init(dims, **desc)
        for k in VC.ACC_VIEWS[:2]:
            ctx.frame_set_depth(VC.depth_at(VC.view(k), cam), cam, 1.0, *RANGE, levels=1)
            ctx.frame_set_color(C.rgb_at(VC.view(k), cam))
            ctx.volume_integrate_color(VC.view(k))
        import volume_oracle as VO
        G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
        vol, cvol = ctx.volume_download(), ctx.volume_color_download().view(np.uint16)
        held = VC.held_out_pose()
        (V, N, If), = set_frame(ctx, cam, SC.frame_depth(cam), C.rgb_at(held, cam), 1)[0]
        pose = SC.poses()[1]
        pho = SP.rows(vol, cvol, G, V, If, pose, 0.1)
        geo = SO.rows(vol, G, V, N, pose, 0.1, SC.COS_THR, True)
        rec, S = SP.record(*pho, C.WEIGHT)
        got = ctx.sdf_photo_normal_eq(pose, 0, 0.1, C.WEIGHT)
        assert got[28] == rec[28] > 0.25 * len(V)          # (the floors: no passing on an empty answer; two views fused, an offset pose)
        ratio = check_record(got, rec, S, slice(0, 28), "photo")
        crec, cS = SP.combined(geo, pho, C.WEIGHT)
        p, it, step, cost, m, pcost, pm = ctx.icp_sdf_rgbd(pose, C.WEIGHT, 1, 0.0, 0.1, SC.COS_THR)
        assert (m, pm) == (int(crec[28]), int(crec[30])) and m > 0.15 * len(V)
        ratio = max(ratio, check_record(np.array([cost, pcost]), crec[[27, 29]], cS[[27, 29]], slice(0, 2), "costs"))
        print("rows", m, pm, "worst error / (2^-24 S):", ratio)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- C++
def test_volume_sdf_color_track_cpp_runs(tmp_path):
    """DepthFrontEnd::icpVolumeColor / icpPyramidVolumeColor / volumeColorResiduals from plain C++ (tests/cpp/volume_sdf_color_track.cpp)"""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_sdf_color_track")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_sdf_color_track.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    assert r.returncode == 0 and "volume_sdf_color_track: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
