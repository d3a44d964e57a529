"""GPU: the ORDER in which the sixteen calls of the volume terms look at what they are given (csrc/rpe_sdf_api.hip): rows, normal equations,
loop and coarse-to-fine loop of the volume term and of the volume colour term, on the window and on the map.  Every call here has two
things wrong, and the status says which one was looked at first:
  rows and normal equations   arguments, then the context's state, then the box
  loops                       options (the weight included), then max_iter or the pyramid's arguments, then lo / hi pairing, then the
                              context's state, then the box
  the context's state         frame, frame colour, volume, colour volume, levels
The calls go straight to the C ABI: nothing of api.py stands between the test and the checks.  A 16^3 volume with colour, a 40 x 30
frame of 2 levels; the field is constant, so the few calls that get past every check have no row to sum."""
import ctypes as C

import numpy as np
import pytest

from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 19.5, 14.5, 40, 30)
POSE = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
ITERS = np.array([2, 1], np.int32)
NAN = float("nan")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def calls(ctx, level=0, weight=0.01, device_resident=0, lo=None, hi=None):
    """{name: (kind, colour, map, status)} of all sixteen calls on the context; lo / hi go to the map calls alone"""
    lib, h, p = L.lib(), ctx._h, ptr(POSE.copy())
    rows, rec = np.zeros((7, 40 * 30), np.float32), np.zeros(32, np.float64)
    o = C.byref(L.RpeIcpOptions(L.RES_P2PLANE, 2, 0.0, 0.1, 0.9, 1, device_resident, 1))
    out = {}
    for is_map, box in ((False, ()), (True, (ptr(lo), ptr(hi)))):
        m = "map_" if is_map else ""
        none4, none6 = (None,) * 4, (None,) * 6
        out[f"rpe_{m}sdf_rows"] = ("rows", False, is_map, getattr(lib, f"rpe_{m}sdf_rows")(h, level, p, 0.1, 0.9, 1, *box, ptr(rows)))
        out[f"rpe_{m}sdf_normal_eq"] = ("normal_eq", False, is_map, getattr(lib, f"rpe_{m}sdf_normal_eq")(h, level, p, 0.1, 0.9, 1, *box, ptr(rec)))
        out[f"rpe_icp_{m}sdf"] = ("loop", False, is_map, getattr(lib, f"rpe_icp_{m}sdf")(h, o, *box, p, *none4))
        out[f"rpe_icp_pyramid_{m}sdf"] = ("pyramid", False, is_map, getattr(lib, f"rpe_icp_pyramid_{m}sdf")(h, o, 2, ptr(ITERS), None, *box, p, *none4))
        out[f"rpe_{m}sdf_photo_rows"] = ("rows", True, is_map, getattr(lib, f"rpe_{m}sdf_photo_rows")(h, level, p, 0.1, *box, ptr(rows)))
        out[f"rpe_{m}sdf_photo_normal_eq"] = ("normal_eq", True, is_map,
                                              getattr(lib, f"rpe_{m}sdf_photo_normal_eq")(h, level, p, 0.1, weight, *box, ptr(rec)))
        out[f"rpe_icp_{m}sdf_rgbd"] = ("loop", True, is_map, getattr(lib, f"rpe_icp_{m}sdf_rgbd")(h, o, weight, *box, p, *none6))
        out[f"rpe_icp_pyramid_{m}sdf_rgbd"] = ("pyramid", True, is_map,
                                               getattr(lib, f"rpe_icp_pyramid_{m}sdf_rgbd")(h, o, weight, 2, ptr(ITERS), None, *box, p, *none6))
    assert len(out) == 16
    return out


def statuses(got, pick=lambda kind, colour, is_map: True):
    return {name: rc for name, (kind, colour, is_map, rc) in got.items() if pick(kind, colour, is_map)}


def ran(rc):
    """a loop that got past every check: what it then returns is the data's business (a field without a gradient gives a system that
    the solve refuses, RPE_ERR_DEGENERATE)"""
    return rc in (0, -5)


def volume_with_colour(ctx):
    ctx.volume_init((16, 16, 16), 0.05, (-0.4, -0.4, 0.2), 0.15)
    vol = np.zeros((16, 16, 16, 2), np.float32)
    vol[..., 0], vol[..., 1] = 0.5, 1.0
    ctx.volume_upload(vol)
    ctx.volume_color_upload(np.full((16, 16, 16, 4), 1.0, np.float16))


def test_what_each_of_the_sixteen_calls_looks_at_first(gpu_ctx_factory):
    misaligned = np.array([1, 0, 0], np.int64), np.array([9, 8, 8], np.int64)
    aligned_lo = np.array([0, 0, 0], np.int64)

    # ---- a volume with colour, no frame
    a = gpu_ctx_factory()
    volume_with_colour(a)
    # the state in front of the box: no frame is RPE_ERR_STATE (-4), not the box's RPE_ERR_ARG
    got = statuses(calls(a, lo=misaligned[0], hi=misaligned[1]))
    assert len(got) == 16 and set(got.values()) == {-4}, got
    # the weight in front of the state: RPE_ERR_ARG (-3) from the four colour loops and the two photometric normal equations
    got = calls(a, weight=NAN)
    weighted = statuses(got, lambda kind, colour, is_map: colour and kind != "rows")
    assert len(weighted) == 6 and set(weighted.values()) == {-3}, weighted
    rest = statuses(got, lambda kind, colour, is_map: not (colour and kind != "rows"))
    assert len(rest) == 10 and set(rest.values()) == {-4}, rest
    # the options in front of the state: device_resident = 1 is RPE_ERR_ARG from the eight loops
    got = calls(a, device_resident=1)
    loops = statuses(got, lambda kind, colour, is_map: kind in ("loop", "pyramid"))
    assert len(loops) == 8 and set(loops.values()) == {-3}, loops
    rest = statuses(got, lambda kind, colour, is_map: kind not in ("loop", "pyramid"))
    assert len(rest) == 8 and set(rest.values()) == {-4}, rest

    # ---- a frame of 2 levels without colour, no volume
    b = gpu_ctx_factory()
    b.frame_set_depth(np.full((30, 40), 1.0, np.float32), CAM, 1.0, 0.1, 5.0, levels=2)
    # the arguments in front of the state: level = -1 is RPE_ERR_ARG from the eight rows and normal-equation calls
    got = calls(b, level=-1)
    levelled = statuses(got, lambda kind, colour, is_map: kind in ("rows", "normal_eq"))
    assert len(levelled) == 8 and set(levelled.values()) == {-3}, levelled
    rest = statuses(got, lambda kind, colour, is_map: kind not in ("rows", "normal_eq"))
    assert len(rest) == 8 and set(rest.values()) == {-4}, rest                      # the loops take no level: no volume, no frame colour

    # ---- the same frame, still without colour, and the volume with colour
    volume_with_colour(b)
    # lo without hi in front of the state, in all four kinds of call on the map, both terms
    got = calls(b, lo=aligned_lo, hi=None)
    on_map = statuses(got, lambda kind, colour, is_map: is_map)
    assert len(on_map) == 8 and set(on_map.values()) == {-3}, on_map
    window = statuses(got, lambda kind, colour, is_map: not is_map)
    assert {n: rc for n, rc in window.items() if "photo" in n or "rgbd" in n} == {
        "rpe_sdf_photo_rows": -4, "rpe_sdf_photo_normal_eq": -4, "rpe_icp_sdf_rgbd": -4, "rpe_icp_pyramid_sdf_rgbd": -4}, window
    assert window["rpe_sdf_rows"] == 0 and window["rpe_sdf_normal_eq"] == 0 and ran(window["rpe_icp_sdf"]) and ran(window["rpe_icp_pyramid_sdf"])

    # ---- everything there: the box is looked at last, and is RPE_ERR_ARG
    b.frame_set_color(np.full((30, 40, 3), 128, np.uint8))
    got = calls(b, lo=misaligned[0], hi=misaligned[1])
    on_map = statuses(got, lambda kind, colour, is_map: is_map)
    assert len(on_map) == 8 and set(on_map.values()) == {-3}, on_map
    window = statuses(got, lambda kind, colour, is_map: not is_map)
    assert len(window) == 8 and all(rc == 0 if "icp" not in n else ran(rc) for n, rc in window.items()), window
    # three levels asked of a frame of two: the last of the state rules, in front of the box
    three = np.array([1, 1, 1], np.int32)
    o = C.byref(L.RpeIcpOptions(L.RES_P2PLANE, 2, 0.0, 0.1, 0.9, 1, 0, 1))
    assert L.lib().rpe_icp_pyramid_map_sdf_rgbd(b._h, o, 0.01, 3, ptr(three), None, ptr(misaligned[0]), ptr(misaligned[1]), ptr(POSE.copy()),
                                                *(None,) * 6) == -4
    assert L.lib().rpe_map_sdf_rows(b._h, 2, ptr(POSE.copy()), 0.1, 0.9, 1, ptr(misaligned[0]), ptr(misaligned[1]),
                                    ptr(np.zeros((7, 1200), np.float32))) == -4
