"""CPU: the numpy statement of the depth filter (tests/filter_oracle.py) against itself -- constant images, NaN centres, steps, the
window's bounds, the spatial table -- the figures of tests/filter_cases.py recomputed (what a depth sensor's noise does to the frame's
normals and to the tracking loop, and what the filter makes of it), and the cross-compiled library: exports, header, argument errors,
the unit the kernel lives in, the C++ driver."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import filter_oracle as FLO
import isa_tools as T
import pyramid_oracle as PO
import unit_gates as UG
import volume_cases as VC
from rgbd_pose_estimation_amd import _lib as L, simulator as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_frame_set_filter", "rpe_frame_get_filter"}
F = np.float32
FILTERS = [(1, 0.8, 0.01, 0.02), (3, 2.0, 0.01, 0.02), (4, 2.5, 0.0072, 0.0114), (4, 3.0, 0.05, 0.0)]


# ---------------------------------------------------------------------------------------------- properties of the statement
@pytest.mark.parametrize("radius,sigma", [(1, 0.8), (2, 1.5), (3, 2.0), (4, 2.5)])
def test_spatial_weights_are_symmetric_with_one_at_the_centre(radius, sigma):
    ws = FLO.spatial_weights(radius, sigma)
    assert ws.dtype == F and ws.shape == (2 * radius + 1, 2 * radius + 1)
    assert ws[radius, radius] == F(1.0)
    assert np.array_equal(ws, ws.T) and np.array_equal(ws, ws[::-1]) and np.array_equal(ws, ws[:, ::-1])
    assert (ws > 0).all() and (ws <= 1).all() and ws[radius, radius + 1] < 1 and ws[0, 0] == ws.min()
    assert ws[0, 1] == F(math.exp(-float(radius * radius + (radius - 1) ** 2) / (2 * sigma * sigma)))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("value", [0.5, 1.0, 2.0, 4.0])
def test_a_constant_image_comes_back_bit_identical(filt, value):
    """x = 0 at every tap, so wgt = ws and out = (sum ws c) / (sum ws).  For c a power of two every product ws * c and every partial sum
    of num is the exact c-fold of den's, and the quotient is c itself: bit-identical.  (Any other c: the next test.)"""
    m = np.full((13, 17), value, F)
    assert np.array_equal(FLO.bilateral(m, *filt), m)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("value", [0.777, 2.713, 6.25])
def test_a_constant_image_of_any_value_comes_back_to_rounding(filt, value):
    """A constant that is no power of two rounds in every product ws * c, so num is not the exact c-fold of den and the quotient can
    miss c by a few ulp (2.713 at radius 1 gives 2.7130003): n taps are n products, n additions in each sum and a division, each
    within 2^-24 relative."""
    m = np.full((13, 17), value, F)
    n = (2 * filt[0] + 1) ** 2
    assert np.abs(FLO.bilateral(m, *filt).astype(np.float64) - float(F(value))).max() <= (3 * n + 1) * 2.0 ** -24 * value


@pytest.mark.parametrize("filt", FILTERS)
def test_nan_centres_stay_nan_and_valid_centres_stay_valid(filt):
    img, scale = FC.holes(37, 29, 3, u16=False)
    m = PO.metric_depth(img, scale, *FC.RANGE[:2])
    out = FLO.bilateral(m, *filt)
    assert np.isnan(m).sum() > 100 and (~np.isnan(m)).sum() > 100
    assert np.array_equal(np.isnan(out), np.isnan(m))
    lonely = np.full((9, 9), np.nan, F)                  # a valid pixel without any valid neighbour is its own mean
    lonely[4, 4] = 2.5
    assert np.array_equal(FLO.bilateral(lonely, *filt), lonely, equal_nan=True)


@pytest.mark.parametrize("filt", FILTERS)
def test_a_step_larger_than_the_cut_does_not_bleed(filt):
    """each side of the step is filtered exactly as if the other side were invalid"""
    img, scale = FC.step(37, 29, 4, u16=True, column=18, row=20)
    m = PO.metric_depth(img, scale, *FC.RANGE[:2])
    near, mid, far = m < 2.0, (m >= 2.0) & (m < 3.0), m >= 3.0
    assert near.sum() > 100 and mid.sum() > 100 and far.sum() > 100
    out = FLO.bilateral(m, *filt)
    for side in (near, mid, far):
        alone = FLO.bilateral(np.where(side, m, F(np.nan)).astype(F), *filt)
        assert np.array_equal(out[side], alone[side])
    assert not np.array_equal(out, m)                      # ... and within a side it does smooth


@pytest.mark.parametrize("filt", FILTERS)
def test_the_output_lies_within_the_windows_range(filt):
    """a weighted mean of the counted neighbours: within the window's min and max to 1 ulp"""
    rng = np.random.default_rng(8)
    m = PO.metric_depth(FC.as_type(FC.noisy_surface(41, 23, 8), False)[0], 1.0, *FC.RANGE[:2])
    m[rng.random(m.shape) < 0.05] = np.nan
    out = FLO.bilateral(m, *filt)
    r = filt[0]
    pad = np.pad(m, r, constant_values=np.nan)
    win = np.stack([pad[r + dy:r + dy + m.shape[0], r + dx:r + dx + m.shape[1]] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    ok = ~np.isnan(m)
    lo, hi = np.fmin.reduce(win, 0), np.fmax.reduce(win, 0)           # NaN members are passed over
    assert (out[ok] >= np.nextafter(lo[ok], F(-np.inf))).all() and (out[ok] <= np.nextafter(hi[ok], F(np.inf))).all()
    assert (out[ok] != m[ok]).mean() > 0.9


def test_every_valid_neighbour_counts_under_a_large_constant_cut():
    """depth_cut_z2 = 0 and a cut far above the image's spread: the filter tends to the spatial Gaussian mean"""
    m = PO.metric_depth(FC.as_type(FC.noisy_surface(31, 19, 2), False)[0], 1.0, *FC.RANGE[:2])
    out = FLO.bilateral(m, 2, 1.5, 1e4, 0.0)
    ws = FLO.spatial_weights(2, 1.5).astype(np.float64)
    pad = np.pad(m.astype(np.float64), 2, mode="constant", constant_values=np.nan)
    ref = np.zeros(m.shape)
    den = np.zeros(m.shape)
    for dy in range(5):
        for dx in range(5):
            d = pad[dy:dy + m.shape[0], dx:dx + m.shape[1]]
            ref += np.where(np.isnan(d), 0, ws[dy, dx] * np.nan_to_num(d))
            den += np.where(np.isnan(d), 0, ws[dy, dx])
    # x = (dz / 1e4)^2 < 2^-25: 1 - x is 1 in fp32 and the range weight drops out.  49 ... here 25 fp32 additions in each sum, a
    # product per term and one division: within 28 * 2^-24 of values below 4.3 m
    assert np.abs(out - ref / den).max() < 28 * 2.0 ** -24 * 4.3


def test_sensor_depth_follows_the_noise_law():
    p = VC.track_pose(3)
    R, t = p[:9].reshape(3, 3), p[9:]
    truth = S.render_depth(R, t, VC.HALF_CAM).astype(np.float64)
    d = S.sensor_depth(R, t, VC.HALF_CAM, np.random.default_rng(1))
    assert d.dtype == np.uint16 and d.shape == truth.shape and np.array_equal(d == 0, truth == 0)
    df = S.sensor_depth(R, t, VC.HALF_CAM, np.random.default_rng(1), as_u16=False)
    assert df.dtype == F and np.array_equal(np.rint(df.astype(np.float64) * 1000).astype(np.uint16), d)   # the same millimetres
    err = d.astype(np.float64) * 1e-3 - truth
    for lo, hi in ((2.0, 2.5), (3.0, 3.5), (4.5, 5.0)):
        band = (truth > lo) & (truth < hi)
        want = float(np.sqrt(np.mean(S.sensor_depth_sigma(truth[band]) ** 2)))
        assert band.sum() > 3000 and abs(err[band].std() / want - 1) < 0.05, (lo, err[band].std(), want)


# ---------------------------------------------------------------------------------------------- the figures of filter_cases.py
def test_the_worth_of_it():
    """the sensor's frame at track_pose(3): the filtered normals are at most a third as far from the noiseless ones as the raw depth's,
    over at least as many pixels"""
    (raw_deg, raw_n), (fil_deg, fil_n), true_n = FC.oracle_worth()
    print(f"raw {raw_deg:.2f} deg over {raw_n} normals, filtered {fil_deg:.2f} deg over {fil_n}, noiseless {true_n}")
    assert fil_deg <= raw_deg / 3
    assert fil_n >= raw_n
    assert abs(raw_deg - FC.WORTH_RAW_DEG) < 0.05 and raw_n == FC.WORTH_RAW_NORMALS
    assert abs(fil_deg - FC.WORTH_FILTERED_DEG) < 0.05 and fil_n == FC.WORTH_FILTERED_NORMALS


@pytest.fixture(scope="module")
def loops(oracle):
    return FC.oracle_tracking_sensor(oracle, None), FC.oracle_tracking_sensor(oracle, FC.TRACK_FILTER)


def test_the_loop(loops):
    """six frames of the oracle's tracking loop on the sensor's depth: with the filter, level 0 pairs at least twice as many pixels on
    every frame and the worst rotation error is no larger"""
    (raw_est, raw_pairs), (fil_est, fil_pairs) = loops
    raw_rot, raw_pos = FC.loop_errors(raw_est)
    fil_rot, fil_pos = FC.loop_errors(fil_est)
    print("raw", raw_pairs, raw_rot, raw_pos, "filtered", fil_pairs, fil_rot, fil_pos)
    assert len(raw_pairs) == len(fil_pairs) == FC.LOOP_FRAMES - 1
    assert all(f >= 2 * r for f, r in zip(fil_pairs, raw_pairs))
    assert fil_rot <= raw_rot
    assert tuple(raw_pairs) == FC.LOOP_RAW_PAIRS and tuple(fil_pairs) == FC.LOOP_FILTERED_PAIRS
    assert abs(raw_rot - FC.LOOP_RAW_ROT) < 2e-5 and abs(raw_pos - FC.LOOP_RAW_POS) < 2e-5
    assert abs(fil_rot - FC.LOOP_FILTERED_ROT) < 2e-5 and abs(fil_pos - FC.LOOP_FILTERED_POS) < 2e-5
    # the GPU run's bound covers the frames it tracks
    errs = [VC.pose_error(fil_est[f], VC.track_pose(f)) for f in range(1, FC.GPU_LOOP_FRAMES)]
    assert max(e[0] for e in errs) <= FC.GPU_LOOP_ROT / 2 and max(e[1] for e in errs) <= FC.GPU_LOOP_POS / 2


def test_gpu_cases_have_what_they_claim():
    """the conditions tests/test_gpu_filter.py relies on: holes of every kind, a step on a tile edge, partial range weights"""
    for u16 in (True, False):
        img, scale = FC.holes(65, 33, 3, u16)
        m = PO.metric_depth(img, scale, *FC.RANGE[:2])
        assert np.isnan(m[:8, :21]).all() and np.isnan(m[16:27, 32:43]).all() and np.isnan(m[-1]).all()   # border, 11 x 11, last row
        raw = img.astype(np.float64) * scale
        assert ((raw > 0) & (raw <= FC.RANGE[0])).any() and (raw >= FC.RANGE[1]).any()
        assert u16 or np.isnan(img).sum() > 30
    img, scale = FC.step(65, 33, 4, True, column=32, row=32)
    m = PO.metric_depth(img, scale, *FC.RANGE[:2])
    assert (m[:32, :32] < 2).all() and (m[:32, 32:] > 2).all() and (m[32:] > 3).all()
    m = PO.metric_depth(*FC.room(), *VC.RANGE[:2])
    out = FLO.bilateral(m, *FC.DEFAULT_FILTER)
    assert (out != m)[~np.isnan(m)].mean() > 0.99


# ---------------------------------------------------------------------------------------------- the cross-compiled library
def test_header_and_library_export_the_filter_entry_points():
    hdr = UG.check_entry_points(SYMS)
    assert "typedef struct { int radius; double sigma_space, depth_cut, depth_cut_z2; } rpe_depth_filter;" in hdr
    assert "RPE_FILTER_MAX_RADIUS = 4" in hdr and L.FILTER_MAX_RADIUS == FLO.MAX_RADIUS == 4
    assert "out of scope" in hdr.split("Depth filter")[1].split("TSDF volume")[0]       # raw fusion beside filtered tracking
    assert L.lib().rpe_abi_version() == 1
    assert C.sizeof(L.RpeDepthFilter) == 32


def test_filter_arguments_are_checked_before_anything_else():
    """the argument checks need no device: a null context and a null output are refused on any machine"""
    UG.built()
    f = L.RpeDepthFilter(3, 2.0, 0.01, 0.02)
    assert L.lib().rpe_frame_set_filter(None, C.byref(f)) == L.RPE_ERR_ARG
    assert L.lib().rpe_frame_get_filter(None, C.byref(f)) == L.RPE_ERR_ARG


def test_filter_unit_holds_the_filter_alone_and_does_not_spill():
    """the unit's design: the filter's two instances in a unit of their own, none in the front end's.  Its spills, scratch, LDS and registers
    are its entry in tests/unit_gates.py"""
    UG.built()
    names = sorted(r["name"].rsplit("::", 1)[1] for r in T.kernel_resources(UG.obj("rpe_filter.hip")))
    assert names == ["depth_filter_kernel<float>", "depth_filter_kernel<unsigned short>"], names      # one kernel, both raw depth types
    frontend = T.kernel_bases(UG.obj("rpe_frontend.hip"))
    assert sum(frontend.values()) >= 7 and not any("filter" in b for b in frontend), frontend


def test_filter_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "depth_filter.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "depth_filter")])
