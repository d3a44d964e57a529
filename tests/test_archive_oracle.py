"""CPU: the volume archive as tests/archive_oracle.py states it.  The store model's own properties -- a round trip is the identity, a
brick is never both in the window and in the store, one non-zero word keeps a brick and none does not, two shifts are not one shift
of their sum, the leaving boxes are the leaving bricks; the figures of tests/archive_cases.py recomputed; and the build surface:
exported symbols, the header, registers of the new kernel unit, the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import archive_cases as AC
import archive_oracle as AO
import shift_oracle as SO
import unit_gates as UG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"rpe_volume_archive", "rpe_volume_archive_info", "rpe_volume_archive_download", "rpe_volume_archive_clear"}
ENTRY_POINTS = SYMS | {"rpe_volume_shift"}
DIMS = (24, 16, 8)


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def content(dims, seed):
    """a window and a colour window of arbitrary bits, a third of the bricks all zero"""
    rng = np.random.default_rng(seed)
    d0, d1, d2 = dims
    vol = rng.integers(0, 1 << 32, (d2, d1, d0, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    cvol = rng.integers(0, 1 << 16, (d2, d1, d0, 4)).astype(np.uint16)
    for b in AO.bricks_in([((0, 0, 0), AO.bricks_of(dims))]):
        if rng.integers(0, 3) == 0:
            AO._cut(vol, b)[...] = 0
            AO._cut(cvol, b)[...] = 0
    return vol, cvol


SHIFTS = [(8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8), (8, -8, 16), (24, 0, 0), (0, 24, 0), (32, 0, 0), (24, 16, 8),
          (-16, 8, 0)]


# ---------------------------------------------------------------------------------------------- the store model
@pytest.mark.parametrize("colour", (False, True), ids=("tsdf", "colour"))
def test_a_round_trip_is_the_identity(colour):
    vol, cvol = content(DIMS, 1)
    cvol = cvol if colour else None
    for d in SHIFTS:
        store = {}
        a, ca, tot = AO.shift(vol, cvol, (0, 0, 0), d, store)
        assert tot == d and not AO.covered(tot, DIMS) & set(store)
        # without the archive the same shift: the window agrees (nothing returns from an empty store)
        assert bits(a, SO.shift(vol, cvol, d)[0])
        b, cb, tot = AO.shift(a, ca, tot, tuple(-x for x in d), store)
        assert tot == (0, 0, 0) and store == {} and bits(b, vol) and (not colour or np.array_equal(cb, cvol)), d
    # a shift of zero touches nothing
    store = {}
    a, _, tot = AO.shift(vol, cvol, (8, 0, -8), (0, 0, 0), store)
    assert a is vol and tot == (8, 0, -8) and store == {}


def test_a_brick_is_never_both_in_the_window_and_in_the_store():
    rng = np.random.default_rng(2)
    vol, cvol = content(DIMS, 3)
    total, store, seen = (0, 0, 0), {}, 0
    for _ in range(40):
        d = tuple(int(8 * x) for x in rng.integers(-2, 3, 3))
        vol, cvol, total = AO.shift(vol, cvol, total, d, store)
        assert not AO.covered(total, DIMS) & set(store)
        seen = max(seen, len(store))
        # new evidence on the way: a brick that was empty may come back non-zero, a returned one may be changed
        vol = vol.copy()
        vol.view(np.uint32)[tuple(rng.integers(0, s) for s in vol.shape)] ^= np.uint32(1 << int(rng.integers(0, 32)))
    assert seen > 6
    coords, tsdf, colour = AO.download(store)
    order = [(int(c[2]), int(c[1]), int(c[0])) for c in coords]
    assert order == sorted(order) and tsdf.shape == (len(store), 8, 8, 8, 2) and colour.shape == (len(store), 8, 8, 8, 4)
    for c, t, cc in zip(coords, tsdf, colour):
        assert bits(store[tuple(int(x) for x in c)][0], t) and np.array_equal(store[tuple(int(x) for x in c)][1], cc)


def test_one_word_keeps_a_brick_and_none_does_not():
    d0, d1, d2 = DIMS
    plant = {"negative zero tsdf in the last voxel": lambda v, c: v.view(np.uint32).__setitem__((7, 7, 7, 0), 0x80000000),
             "one colour half-word in the first voxel": lambda v, c: c.__setitem__((0, 0, 0, 1), 0x3c00),
             "a tsdf of weight 0": lambda v, c: v.__setitem__((3, 4, 5, 0), 0.25),
             "nothing": lambda v, c: None}
    for name, put in plant.items():
        vol, cvol = np.zeros((d2, d1, d0, 2), np.float32), np.zeros((d2, d1, d0, 4), np.uint16)
        put(vol, cvol)
        store = {}
        a, ca, tot = AO.shift(vol, cvol, (0, 0, 0), (8, 0, 0), store)
        assert not a.view(np.uint32).any() and not ca.any()
        assert set(store) == (set() if name == "nothing" else {(0, 0, 0)}), name
        b, cb, _ = AO.shift(a, ca, tot, (-8, 0, 0), store)
        assert bits(b, vol) and np.array_equal(cb, cvol) and store == {}, name
    # without a colour window the colour word has nowhere to be: the brick restores all-zero colour
    vol = np.zeros((d2, d1, d0, 2), np.float32)
    vol[0, 0, 0, 1] = 2.0
    store = {}
    a, _, tot = AO.shift(vol, None, (0, 0, 0), (8, 0, 0), store)
    assert not store[(0, 0, 0)][1].any()
    b, cb, _ = AO.shift(a, np.zeros((d2, d1, d0, 4), np.uint16), tot, (-8, 0, 0), store)
    assert bits(b, vol) and not cb.any()


def test_two_shifts_are_not_one_shift_of_their_sum():
    vol, cvol = content(DIMS, 4)
    s1, s2 = {}, {}
    a, ca, ta = AO.shift(*AO.shift(vol, cvol, (0, 0, 0), (8, 0, 0), s1), (-8, 8, 0), s1)
    b, cb, tb = AO.shift(vol, cvol, (0, 0, 0), (0, 8, 0), s2)
    assert ta == tb == (0, 8, 0)
    # WITH the archive they are the same map: what left on the way came back
    assert bits(a, b) and np.array_equal(ca, cb) and set(s1) == set(s2)
    # without it the detour has lost a slab
    plain = SO.shift(*SO.shift(vol, cvol, (8, 0, 0)), (-8, 8, 0))[0]
    assert not bits(plain, b)
    # and two steps archive more on the way than one: the peak differs
    s3 = {}
    AO.shift(vol, cvol, (0, 0, 0), (8, 0, 0), s3)
    assert set(s3) - set(s2)


def test_leaving_boxes_are_the_leaving_bricks():
    for dims in ((24, 16, 8), (8, 8, 8), (32, 24, 16)):
        nb = AO.bricks_of(dims)
        for d in SHIFTS + [(0, 0, 0), (-40, 8, 0)]:
            s = [x // 8 for x in d]
            boxes = AO.leaving_boxes(nb, s)
            got = AO.bricks_in(boxes)
            want = {(x, y, z) for z in range(nb[2]) for y in range(nb[1]) for x in range(nb[0])
                    if not all(0 <= v - sv < n for v, sv, n in zip((x, y, z), s, nb))}
            assert len(boxes) <= 3 and len(got) == len(set(got)) and set(got) == want, (dims, d)
            # what enters is what would leave on the way back, and is as many
            assert len(AO.entering_bricks(dims, d)) == len(got)


# ---------------------------------------------------------------------------------------------- the use case
@pytest.fixture(scope="module")
def walks():
    return AC.oracle_walk(True), AC.oracle_walk(False)


def test_the_use_case_figures(walks):
    on, off = walks
    print(on["hits"], off["hits"], on["peak"], on["mean_weight"], off["mean_weight"])
    assert on["hits"] == AC.HITS_ARCHIVE and off["hits"] == AC.HITS_PLAIN and set(on["pixels"] + off["pixels"]) == {AC.PIXELS}
    assert on["digest"] == AC.DIGEST_ARCHIVE and off["digest"] == AC.DIGEST_PLAIN
    assert on["mean_weight"] == pytest.approx(AC.MEAN_WEIGHT_ARCHIVE, abs=1e-3) and off["mean_weight"] == pytest.approx(AC.MEAN_WEIGHT_PLAIN, abs=1e-3)
    assert on["total"] == off["total"] and len(on["hits"]) == len(AC.RETURN) == 12 and AC.PATH[-1] == 0


def test_the_conditions_on_the_case(walks):
    on, off = walks
    # the last return frame is the start pose: with the archive at least 1.5 x the hits without
    assert on["hits"][-1] >= AC.GAIN_LIMIT * off["hits"][-1], (on["hits"][-1], off["hits"][-1])
    assert on["peak"] == AC.PEAK_HELD <= AC.PEAK_LIMIT == 512 and on["in_flight"] == AC.PEAK_IN_FLIGHT == AC.CAPACITY
    assert not bits(on["window"], off["window"])
    assert np.mean(on["hits"]) > np.mean(off["hits"]) and all(a >= b for a, b in zip(on["hits"], off["hits"]))


# ---------------------------------------------------------------------------------------------- build surface
def test_header_and_library_export_the_archive_entry_points():
    hdr = UG.check_entry_points(ENTRY_POINTS)
    assert "Volume archive" in hdr and hdr.index("Volume archive: what leaves") > hdr.index("Moving volume: the window")


def test_archive_cpp_driver_compiles(tmp_path):
    lib = UG.built()
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_archive.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(tmp_path / "volume_archive")])
