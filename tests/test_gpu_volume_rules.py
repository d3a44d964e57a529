"""GPU: the volume's shared device rules (csrc/rpe_volume_field.hpp) probed DIRECTLY, rule by rule, and the two fuse kernels run on the
cull's own case set.  tests/cpp/volume_rules_probe.hip includes the header, is compiled once per module with the options build.py
gives the library's kernel units, and runs once per rule as a fresh process over a table of cases; every comparison is exact:

  cull, brick   box_can_update = tests/cull_oracle.py on every case of tests/cull_cases.py, in both kernels' forms of the box; the
                count of voxels voxel_project accepts = tests/volume_oracle.py integrate's mask; no case with a voxel and no entry
  half          h2f on all 65 536 patterns; f2h on every binary16 value, every midpoint and its neighbours, the subnormals, the
                overflow threshold, zeros, Infs and NaN payloads, against tests/color_oracle.py h
  blend         random bits and the special patterns of tests/test_gpu_color.py at W = 1, 64, 5000 against color_oracle.blend
  quantise      every k + 0.5, k = -1 .. 255, with its fp32 neighbours; NaN, Infs
  cell          on, one ulp below and one ulp above every cell boundary of a 3 x 2 x 2 volume and of one at a far origin, the dim - 2
                limit and points outside included, against volume_oracle.cell
  brick_word    every source s from two slots beyond the capacity to one brick beyond the window, every corner (x, y, z), against
                Python's integers (the 1024^3 window and the 2^24-slot pool are sampled: every s of their first and last rows, a
                prime stride between)

What the cull's part proves is stated in tests/test_cull_oracle.py: on this case set the variants no_fabs, centre_behind and zh_for_zl
cull needed bricks, so a device rule of any of those forms fails here; the margins of the rule are not something these cases tell
apart.  Then volume_fuse_keyframes and volume_map_fuse_keyframes take the fixed families and the random scenes that hold a one-voxel
brick through the public calls, bit for bit against tests/rebuild_oracle.py and tests/mapfuse_oracle.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import color_oracle as CO
import cull_cases as CC
import cull_oracle as CU
import mapfuse_oracle as MF
import mapmesh_cases as MC
import rebuild_oracle as RO
import volume_oracle as VO
from rgbd_pose_estimation_amd import build as B
from test_gpu_mapfuse import agree
from test_gpu_rebuild import colour_of, random_start, same, same16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, I32 = np.float32, np.uint32, np.int32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """run(rule, table) -> the raw output bytes: the probe compiled once, as the library's kernel units are, one fresh process per call"""
    d = tmp_path_factory.mktemp("volume_rules")
    exe = str(d / "volume_rules_probe")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, *B.HIP_FLAGS, "-I", B.CSRC, os.path.join(ROOT, "tests", "cpp", "volume_rules_probe.hip"), "-o", exe])

    def run(rule, table):
        fin, fout = str(d / f"{rule}.in"), str(d / f"{rule}.out")
        np.ascontiguousarray(table).tofile(fin)
        r = subprocess.run([exe, rule, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (rule, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        return np.fromfile(fout, np.uint8)

    return run


def bits(a):
    return np.ascontiguousarray(a, F).view(U32)


# ---------------------------------------------------------------------------------------------- 1. cull, brick
def test_brick_counts_and_decisions_equal_the_statement(probe):
    _, T, _, n = CC.case_set()
    out = probe("brick", T).view(I32).reshape(-1, 3)
    assert len(out) == len(T)
    count, rebuild, as_map = out[:, 0], out[:, 1] != 0, out[:, 2] != 0
    print("cases", len(T), "voxel counts differ:", (count != n).sum(), "kept", rebuild.sum(), as_map.sum())
    assert np.array_equal(count, n)                                                       # voxel_project at the pixel edges, bit for bit
    assert np.array_equal(rebuild, CU.decide(T, "rebuild")) and np.array_equal(as_map, CU.decide(T, "map"))
    cubes = (T["n"] == 8).all(1)
    assert not ((count > 0) & ~rebuild).any() and not ((count > 0) & ~as_map & cubes).any()
    assert ((count == 1) & cubes).sum() >= 100 and (~rebuild).sum() > len(T) // 2         # the edge is there, and the cull does cull


def test_cull_on_boxes_as_given(probe):
    """box_can_update on lo / hi handed in: the case set's boxes in both forms, then boxes no kernel forms -- a point, lo above hi, NaN
    and Inf corners -- where the rule is still the statement's"""
    _, T, _, _ = CC.case_set()
    T = T[::3]
    rng = np.random.default_rng(7)
    boxes = [CU.brick_box(T, "rebuild"), CU.brick_box(T, "map")]
    lo, hi = (x.copy() for x in boxes[0])
    boxes.append((lo, lo))
    boxes.append((hi, lo))
    for bad in (np.nan, np.inf, -np.inf):
        a, b = lo.copy(), hi.copy()
        a[np.arange(len(a)), rng.integers(0, 3, len(a))] = bad
        b[np.arange(len(b)), rng.integers(0, 3, len(b))] = bad
        boxes += [(a, hi), (lo, b)]
    rec = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3)] + [(k, CC.BRICK[k]) for k in ("fx", "fy", "cx", "cy", "w", "h", "R", "t")])
    assert rec.itemsize == 96
    want, tables = [], []
    for lo, hi in boxes:
        C = np.zeros(len(T), rec)
        C["lo"], C["hi"] = lo, hi
        for k in rec.names[2:]:
            C[k] = T[k]
        tables.append(C)
        want.append(CU.box_can_update(lo, hi, (T["fx"], T["fy"], T["cx"], T["cy"], T["w"], T["h"]), T["R"], T["t"]))
    got = probe("cull", np.concatenate(tables)).view(I32) != 0
    want = np.concatenate(want)
    assert len(got) == len(want) and np.array_equal(got, want) and 0 < want.sum() < len(want)


# ---------------------------------------------------------------------------------------------- 2. half
def f2h_inputs():
    """fp32 bit patterns: every binary16 value; every midpoint of two adjacent binary16 values (the overflow threshold 65520 among them)
    with its fp32 neighbours, both signs; fp32 values below the smallest binary16 subnormal and fp32 subnormals; zeros, Infs, NaNs"""
    every = CO.f32(np.arange(65536, dtype=np.uint16))
    every = every[~np.isnan(every)]
    pos = np.concatenate([CO.f32(np.arange(0x7C00, dtype=np.uint16)).astype(np.float64), [65536.0]])   # 0 .. 65504, then 2^16
    mid = ((pos[:-1] + pos[1:]) / 2).astype(F)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2) and mid[-1] == 65520.0   # exact in fp32
    mids = np.concatenate([np.nextafter(mid, F(-np.inf)), mid, np.nextafter(mid, F(np.inf))])
    tiny = np.array([2.0 ** -25, 2.0 ** -26, 2.0 ** -24, 2.0 ** -14, 2.0 ** -15, 1.5 * 2.0 ** -25, 2.0 ** -126, 2.0 ** -149, 1e-30, 65519.996, 65536.0, 1e30, 3.4e38], np.float64).astype(F)
    tiny = np.concatenate([tiny, np.nextafter(tiny, F(0)), np.nextafter(tiny, F(np.inf))])
    vals = np.concatenate([every, mids, -mids, tiny, -tiny, np.array([0.0, -0.0, np.inf, -np.inf], F)])
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC01234, 0x7FFFFFFF, 0xFF800001, 0x7FA00000, 0xFFFFFFFF, 0x7FC00001], U32)
    return np.concatenate([bits(vals), nans])


def test_half_conversions_on_every_pattern_and_every_tie(probe):
    x = f2h_inputs()
    out = probe("half", x).view(U32)
    assert len(out) == 65536 + len(x)
    got = out[:65536].view(F)
    want = np.arange(65536, dtype=np.uint16).view(np.float16).astype(F)
    nan = np.isnan(want)
    assert nan.sum() == 2046 and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
    h = out[65536:]
    want = CO.h(x.view(F)).astype(U32)
    bad = np.nonzero(h != want)[0]
    assert len(bad) == 0, (len(bad), [hex(int(v)) for v in x[bad[:5]]], h[bad[:5]], want[bad[:5]])
    assert (h[np.isnan(x.view(F))] == 0x7E00).all() and len(x) > 3 * 65536
    assert len(np.unique(h)) == 65536 - 2046 + 1                                          # every binary16 value and the one NaN come out


# ---------------------------------------------------------------------------------------------- 3. blend, quantise
SPECIAL16 = np.array([0x7E00, 0x7E01, 0xFFFF, 0x7D00, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0x0003, 0x83FF, 0x03FF, 0x7BFF, 0xFBFF,
                      0xBC00, 0xC000, 0x4100, 0x3C01], np.uint16)                         # tests/test_gpu_color.py's pool


def test_blend_on_random_bits_and_special_patterns(probe):
    rng = np.random.default_rng(11)
    n = 60000
    ch = rng.integers(0, 1 << 16, (n, 4)).astype(np.uint16)                               # r, g, b, wc: any bits
    plain = CO.h(rng.uniform(0, 255, (n, 4)).astype(F))                                   # ... colours and weights as a volume holds them
    plain[:, 3] = CO.h(rng.choice(np.array([0, 1, 2, 3, 17, 63, 64, 2046, 2047, 2048, 4999, 5000], F), n))
    ch[n // 3:] = plain[n // 3:]
    m = rng.random(ch.shape) < 0.25
    ch[m] = rng.choice(SPECIAL16, int(m.sum()))
    o = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    rec = np.dtype([("rg", "<u4"), ("bw", "<u4"), ("o", "<u4"), ("W", "<f4")])
    tables, want = [], []
    for W in (1.0, 64.0, 5000.0):
        C = np.zeros(n, rec)
        C["rg"], C["bw"] = ch[:, 0].astype(U32) | ch[:, 1].astype(U32) << 16, ch[:, 2].astype(U32) | ch[:, 3].astype(U32) << 16
        C["o"], C["W"] = o, W
        tables.append(C)
        obs = np.stack([o & 0xFF, (o >> 8) & 0xFF, (o >> 16) & 0xFF], -1).astype(F)
        nc, nw = CO.blend(CO.f32(ch[:, :3]), CO.f32(ch[:, 3]), obs, F(W))
        nc, nw = nc.astype(U32), nw.astype(U32)
        want.append(np.stack([nc[:, 0] | nc[:, 1] << 16, nc[:, 2] | nw << 16], -1))
    got = probe("blend", np.concatenate(tables)).view(U32).reshape(-1, 2)
    want = np.concatenate(want)
    bad = np.nonzero((got != want).any(1))[0]
    assert len(got) == len(want) and len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert len(np.unique(want[:, 1] >> 16)) > 20                                          # the clamp, NaN weights and plain ones all occur


def test_quantise_at_every_tie(probe):
    k = np.arange(-1, 256).astype(F) + F(0.5)
    x = np.concatenate([np.nextafter(k, F(-np.inf)), k, np.nextafter(k, F(np.inf)), np.arange(-2, 258).astype(F),
                        np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 254.99998, 255.00002], F)])
    # a quiet NaN with a payload too; no signalling one: arithmetic (the lerp chain before q) never yields it, and numpy's fmax does not
    # follow fmaxf on it
    x = np.concatenate([x, np.array([0xFFC01234, 0x7FC00001], U32).view(F)])
    got = probe("quantise", x).view(U32)
    assert np.array_equal(got, CO.quantise(x).astype(U32)) and got.max() == 255 and got[np.isnan(x)].max() == 0


# ---------------------------------------------------------------------------------------------- 4. cell
def boundary_points(G):
    """per axis the coordinates o + (m + 0.5) s of every cell boundary, m = -2 .. dim + 1 (formed in fp32 and in double: the double's
    rounding may fall an ulp away), each with its fp32 neighbours; all combinations over the three axes"""
    axes = []
    for a in range(3):
        m = np.arange(-2, G.dim[a] + 2)
        b = np.concatenate([G.o[a] + (m.astype(F) + F(0.5)) * G.s, (np.float64(G.o[a]) + (m + 0.5) * np.float64(G.s)).astype(F)])
        inner = np.concatenate([G.o[a] + (m.astype(F) + F(fr)) * G.s for fr in (0.75, 1.0, 1.25)])   # and points inside every cell
        axes.append(np.unique(np.concatenate([np.nextafter(b, F(-np.inf)), b, np.nextafter(b, F(np.inf)), inner])))
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], -1).astype(F)


def test_cell_on_and_beside_every_boundary(probe):
    rec = np.dtype([("dim", "<i4", 3), ("o", "<f4", 3), ("s", "<f4"), ("tr", "<f4"), ("W", "<f4"), ("p", "<f4", 3)])
    out = np.dtype([("known", "<i4"), ("i0", "<i4", 3), ("a", "<f4", 3)])
    tables, wants = [], []
    for dims, s, o in (((3, 2, 2), 0.05, (-0.6, -0.4, 1.0)), ((3, 2, 2), 0.005, (987.3, -654.1, 321.7)), ((2, 2, 2), 0.37, (0.0, 0.0, 0.0))):
        G = VO.Geometry(dims, s, o, 3 * s, 64)
        X = boundary_points(G)
        X = np.concatenate([X, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 1e30, 1e30]], F) + G.o])
        C = np.zeros(len(X), rec)
        C["dim"], C["o"], C["s"], C["tr"], C["W"], C["p"] = G.dim, G.o, G.s, G.tr, G.W, X
        tables.append(C)
        wants.append(VO.cell(G, X))
    got = probe("cell", np.concatenate(tables)).view(out)
    at = 0
    for C, (ok, i0, a) in zip(tables, wants):
        g = got[at:at + len(C)]
        at += len(C)
        assert np.array_equal(g["known"] != 0, ok) and 200 < ok.sum() < len(C)
        for ax in range(3):
            assert np.array_equal(g["i0"][ok, ax], i0[ax][ok].astype(I32)) and np.array_equal(bits(g["a"][ok, ax]), bits(a[ax][ok]))
            assert set(np.unique(i0[ax][ok])) == set(range(C["dim"][0][ax] - 1))          # every cell up to dim - 2, and none beyond
        assert not g["i0"][~ok].any() and not bits(g["a"][~ok]).any()
    assert at == len(got)


# ---------------------------------------------------------------------------------------------- 5. brick_word
def word_cases():
    """(view (nb0, nb1, nb2, capacity), s): every s of the small views; the first and last two x-rows and a prime stride of the big ones"""
    out = []
    for nb, cap in (((3, 2, 2), 5), ((1, 1, 1), 0), ((2, 1, 3), 1), ((127, 3, 5), 40), ((128, 128, 2), 7)):
        out.append((nb, cap, np.arange(~cap - 1, nb[0] * nb[1] * nb[2] + 1)))
    for nb, cap in (((128, 128, 128), 1 << 24), ((1, 128, 128), 1 << 12), ((128, 1, 1), 3)):
        n = nb[0] * nb[1] * nb[2]
        s = np.concatenate([np.arange(-300, min(n, 300)), np.arange(max(n - 300, 0), n + 2), np.arange(0, n, 1021),
                            np.arange(~cap - 1, ~cap + 300), -np.arange(1, cap + 2, 1021), [np.iinfo(I32).max, np.iinfo(I32).min]])
        out.append((nb, cap, np.unique(s)))
    return out


def test_brick_word_over_every_source_and_corner(probe):
    rec = np.dtype([("wnb", "<i4", 3), ("wdim0", "<i4"), ("wdim1", "<i4"), ("capacity", "<i4"), ("s", "<i4"), ("xyz", "<i4", 3)])
    res = np.dtype([("ok", "<i4"), ("pooled", "<i4"), ("w", "<i8")])
    corners = np.array([(x, y, z) for z in (0, 7) for y in (0, 7) for x in (0, 7)], np.int64)
    tables, want = [], []
    for nb, cap, s in word_cases():
        s = np.repeat(np.asarray(s, np.int64), 8)
        xyz = np.tile(corners, (len(s) // 8, 1))
        C = np.zeros(len(s), rec)
        C["wnb"], C["wdim0"], C["wdim1"], C["capacity"], C["s"], C["xyz"] = nb, 8 * nb[0], 8 * nb[1], cap, s, xyz
        tables.append(C)
        x, y, z = xyz.T                                                                   # from here on Python-width (int64) integers
        pooled = s < 0
        slot = -s - 1
        bx, by, bz = s % nb[0], (s // nb[0]) % nb[1], s // (nb[0] * nb[1])
        ok = np.where(pooled, slot < cap, s < nb[0] * nb[1] * nb[2])
        w = np.where(pooled, slot * 1024 + 2 * ((z * 8 + y) * 8 + x), 2 * (((bz * 8 + z) * 8 * nb[1] + by * 8 + y) * 8 * nb[0] + bx * 8 + x))
        W = np.zeros(len(s), res)
        W["ok"], W["pooled"], W["w"] = ok, pooled, np.where(ok, w, 0)
        want.append(W)
    got = probe("brick_word", np.concatenate(tables)).view(res)
    want = np.concatenate(want)
    bad = np.nonzero(got != want)[0]
    assert len(got) == len(want) and len(bad) == 0, (len(bad), np.concatenate(tables)[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert want["w"][want["pooled"] == 0].max() == 2 * (1024 ** 3 - 1) and (want["w"][want["pooled"] != 0] > 1 << 33).any()   # past 32 bits on either path
    assert 0 < (want["ok"] == 0).sum() < len(want) // 2


# ---------------------------------------------------------------------------------------------- 6. the two fuse kernels on the cases
RANDOM = {"random-one-voxel/rebuild": CC.REBUILD, "random-one-voxel/map": CC.MAP}
FAMILIES = [s["name"] for s in CC.families() if min(s["dims"]) >= 2] + list(RANDOM)         # volume_init takes dims >= 2
MAP_FAMILIES = [s["name"] for s in CC.families() if s["brick"] == CC.MAP] + ["random-one-voxel/map"]


def api_scenes(family):
    """the scenes of a family: the fixed one of that name, or the first 24 random scenes of a brick shape that hold a brick with
    exactly one updating voxel"""
    if family not in RANDOM:
        return [s for s in CC.families() if s["name"] == family]
    scenes, _, at, n = CC.case_set()
    one = [scenes[int(i)] for i in np.unique(at[n == 1][:, 0]) if i >= len(CC.families())]
    return [s for s in one if s["brick"] == RANDOM[family] and min(s["dims"]) >= 2][:24]


def planes(sc, cam, pose, seed):
    """the entry's two depth planes and its colours: "far" = one valid value beyond every volume; "holes" = ripples about the depth of
    the volume's middle with a fifth of the pixels invalid"""
    w, h = cam[4], cam[5]
    rng = np.random.default_rng(seed)
    mid = np.asarray(sc["o"]) + 0.5 * np.asarray(sc["dims"]) * sc["s"]
    with np.errstate(invalid="ignore"):
        z0 = float(pose[6:9] @ mid + pose[11])
    z0 = z0 if np.isfinite(z0) and z0 > 0.1 * sc["s"] else max(sc["dims"]) * sc["s"]
    holes = (z0 * (1 + 0.3 * rng.uniform(-1, 1, (h, w)))).astype(F)
    holes[rng.random((h, w)) < 0.2] = np.nan
    rgba = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    rgba[..., 3] = 255
    return dict(far=np.full((h, w), CU.FAR, F), holes=holes), rgba


def attach(ctx, sc, seed):
    """the scene's entries into a cleared store, each as two keyframes (its far plane, its plane with holes), at its own camera:
    {plane: (ids, oracle entries)}"""
    ctx.keyframes_clear()
    rng = np.random.default_rng(3)
    out = dict(far=([], []), holes=([], []))
    for n, (cam, pose) in enumerate(sc["entries"]):
        zs, rgba = planes(sc, cam, pose, seed + n)
        for name, z in zs.items():
            i = ctx.keyframe_add_host(np.zeros((4, 2), I32), rng.integers(0, 99, (4, 8)), rng.normal(0, 1, (4, 3)), np.tile([0, 0, 1.0], (4, 1)),
                                      pose, cam[4], cam[5])
            ctx.keyframe_attach(i, z, rgba, cam)
            out[name][0].append(i)
            out[name][1].append(dict(z=z.reshape(-1), rgba=rgba.reshape(-1, 4), cam=cam, pose=pose))
    return out


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.mark.parametrize("family", FAMILIES)
def test_volume_fuse_keyframes_on_the_cull_cases(ctx, family):
    """cull on and off, CLEAR and accumulation onto a random uploaded volume, with colour, both planes: the bits of rebuild_oracle.fuse"""
    group = api_scenes(family)
    assert len(group) == (24 if family in RANDOM else 1)
    updated = 0
    for sc in group:
        G = CC.geometry(sc)
        att = attach(ctx, sc, 100)
        ctx.volume_init(sc["dims"], **CC.kw(sc))
        start = random_start(G, 9)
        for plane, clear, color in (("far", True, True), ("holes", True, True), ("holes", False, True), ("far", False, False)):
            ids, es = att[plane]
            flags = (RO.CLEAR if clear else 0) | (RO.COLOR if color else 0)
            want, cwant = RO.fuse(None if clear else start[0], None if clear else start[1], G, es, flags)
            updated += int((want[..., 1] != (0 if clear else start[0][..., 1])).sum())
            for cull in (True, False):
                if not clear:
                    ctx.volume_upload(start[0])
                    ctx.volume_color_upload(start[1].view(np.float16))
                ctx.volume_fuse_keyframes(ids, clear=clear, color=color, cull=cull)
                assert same(ctx.volume_download(), want), (sc["name"], plane, clear, color, cull)
                assert same16(colour_of(ctx), cwant if cwant is not None else start[1]), (sc["name"], plane, clear, color, cull)
    assert updated > 0 or family.startswith("nonfinite")


def map_fuse(ctx, m, ids, es, clear, color, cull, box):
    """the call on the context and mapfuse_oracle.fuse on the model; returns (the call's stats, the oracle's)"""
    stats = ctx.volume_map_fuse_keyframes(ids, clear=clear, color=color, cull=cull, box=box)
    held = set(m.store)
    flags = (MF.CLEAR if clear else 0) | (MF.COLOR if color else 0)
    m.window, m.cwindow, m.store, want = MF.fuse(m.window, m.cwindow, m.total, m.store, box, m.kw, es, flags)
    m.colour_plane = m.colour_plane or (color and bool(m.store)) or (m.cwindow is not None and bool(set(m.store) - held))
    return stats, want


@pytest.mark.parametrize("family", MAP_FAMILIES)
def test_volume_map_fuse_keyframes_on_the_cull_cases(ctx, family):
    """the scene's volume as a box of 8 x 8 x 8-voxel bricks whose first brick is the window and whose others live in the archive: CLEAR
    over the far planes, then accumulation of the planes with holes, cull on and off -- window, held bricks and stats are
    mapfuse_oracle.fuse's, and under CLEAR every brick some entry updates in exactly one voxel is held (or non-zero in the window)"""
    singles = 0
    for sc in api_scenes(family):
        nb = CC.bricks_per_axis(sc)
        box = (np.zeros(3, np.int64), np.array(sc["dims"], np.int64))
        att = attach(ctx, sc, 200)
        assert np.array_equal(bits(MF.MM.geometry(CC.kw(sc), box).o), bits(CC.geometry(sc).o))     # the box's virtual volume IS the scene's volume
        one = np.zeros(nb[0] * nb[1] * nb[2], bool)
        for cam, pose in sc["entries"]:
            one |= CU.brick_counts(CU.updated(CC.geometry(sc), cam, pose), sc["brick"]) == 1
        for cull in (True, False):
            m = MC.Map(ctx, (8, 8, 8), CC.kw(sc), capacity=nb[0] * nb[1] * nb[2])
            stats, want = map_fuse(ctx, m, *att["far"], True, True, cull, box)
            agree(ctx, m, (sc["name"], "clear", cull))
            assert all(stats[k] == want[k] for k in want) and stats["written"] == 1 + stats["archived"], (sc["name"], cull, stats, want)
            for b in np.nonzero(one)[0]:
                key = (int(b % nb[0]), int((b // nb[0]) % nb[1]), int(b // (nb[0] * nb[1])))
                assert key in m.store or (key == (0, 0, 0) and m.window.any()), (sc["name"], cull, key)
            stats, want = map_fuse(ctx, m, *att["holes"], False, True, cull, box)
            agree(ctx, m, (sc["name"], "accumulate", cull))
            assert all(stats[k] == want[k] for k in want), (sc["name"], cull, stats, want)
        singles += int(one.sum())
    assert singles > 0 or not family.startswith(("edges", "random"))
