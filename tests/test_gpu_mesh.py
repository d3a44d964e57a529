"""GPU parity of the mesh extraction (M1-M5 of csrc/rpe_mesh.hip) against tests/mesh_oracle.py: vertices, normals and triangles are
BIT-EXACT on uploaded analytic fields, a slab with unknown regions, seeded noise (exact zeros, ambiguous faces, NaN / Inf tsdf,
negative weights), odd dims, several min_weight values and the room fused by integrate; upload / download round-trips the bits;
extraction is repeatable and follows the volume; the error paths; the C++ driver."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
import volume_cases as VC
import volume_oracle as VO
from frontend_util import FO, SMALL_CAM
from rgbd_pose_estimation_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def uploaded(ctx, case):
    G, vol, desc = case
    ctx.volume_init(G.dim, **desc)
    ctx.volume_upload(vol)
    return G, vol


def assert_parity(ctx, G, vol, min_weight):
    V, N, T = ctx.volume_mesh(min_weight)
    Vo, No, To = MO.mesh(vol, G, min_weight)
    assert same(V, Vo) and same(N, No) and np.array_equal(T, To) and T.dtype == np.int32, (len(V), len(Vo), len(T), len(To))
    return V, N, T


CASES = {"sphere": MC.sphere, "torus": MC.torus, "slab": MC.slab, "noise": MC.noise,
         "noise_2x3x5": lambda: MC.noise((2, 3, 5), 4), "noise_37x19x23": lambda: MC.noise((37, 19, 23), 5)}


@pytest.mark.parametrize("name, weights", [("sphere", (1.0,)), ("torus", (1.0, 0.25)), ("slab", (0.5, 1.0, 2.0, 3.0, 3.5)),
                                           ("noise", (0.5, 1.0, 2.0)), ("noise_2x3x5", (0.5, 1.0)), ("noise_37x19x23", (0.5, 1.0, 2.0))])
def test_mesh_bit_exact_on_uploaded_volumes(gpu_ctx_factory, name, weights):
    ctx = gpu_ctx_factory()
    G, vol = uploaded(ctx, CASES[name]())
    for w in weights:
        V, N, T = assert_parity(ctx, G, vol, w)
        if name in ("sphere", "torus") and w == 1.0:
            _, cnt, _ = MC.mesh_edges(T)
            assert np.all(cnt == 2) and MC.euler(V, T) == (2 if name == "sphere" else 0)
        if name.startswith("noise") and len(T):
            assert np.all((T[:, 0] != T[:, 1]) & (T[:, 1] != T[:, 2]) & (T[:, 0] != T[:, 2]))
            assert np.array_equal(np.unique(T), np.arange(len(V)))


def test_upload_download_round_trips_bits(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G, vol, desc = MC.noise((37, 19, 23), 9)
    bits = vol.view(np.uint32).copy()
    bits[0, 0, :5, 0] = [0x7fc00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000]   # NaN payloads, -0, a denormal, Inf
    vol = bits.view(np.float32)
    ctx.volume_init(G.dim, **desc)
    ctx.volume_upload(vol)
    assert np.array_equal(ctx.volume_download().view(np.uint32), bits)
    with pytest.raises(ValueError):
        ctx.volume_upload(vol[:-1])


def test_two_extractions_are_identical_and_follow_the_volume(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    G, vol = uploaded(ctx, MC.noise((31, 29, 27), 2))
    a = ctx.volume_mesh(1.0)
    b = ctx.volume_mesh(1.0)
    assert all(same(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))
    # a smaller mesh, then the larger again from the grown buffers
    assert_parity(ctx, G, vol, 2.0)
    assert_parity(ctx, G, vol, 0.5)
    # a re-init with smaller, then larger dims
    for case in (MC.sphere, lambda: MC.noise((41, 33, 30), 3)):
        G, vol = uploaded(ctx, case())
        assert_parity(ctx, G, vol, 1.0)


def fused_room(ctx, views=(0, 1, 2)):
    dims, desc = VC.room_geometry(0.05, 64)
    ctx.volume_init(dims, **desc)
    G = VO.Geometry(dims, desc["voxel_size"], desc["origin"], desc["trunc"], desc["max_weight"])
    want = G.empty()
    for k in views:
        d = VC.depth_at(VC.view(k), SMALL_CAM)
        ctx.frame_set_depth(d, SMALL_CAM, 1.0, *VC.RANGE)
        ctx.volume_integrate(VC.view(k))
        want = VO.integrate(want, G, FO.frame_maps(d, SMALL_CAM, 1.0, *VC.RANGE)[0], SMALL_CAM, VC.view(k))
    return G, want


def test_mesh_of_the_fused_room(gpu_ctx_factory):
    """the real pipeline: frames fused by integrate, then extracted; re-extracted after another integrate"""
    ctx = gpu_ctx_factory()
    G, want = fused_room(ctx, (0, 1))
    assert same(ctx.volume_download(), want)
    V, N, T = assert_parity(ctx, G, want, 1.0)
    assert len(T) > 10000
    assert_parity(ctx, G, want, 2.0)
    # the room's surfaces face the cameras: most faces point towards the first camera centre
    p = VC.view(0)
    C0 = -p[:9].reshape(3, 3).T @ p[9:]
    fn = MC.face_normals(V, T)
    assert (np.einsum("ij,ij->i", fn, C0 - V[T].mean(1).astype(np.float64)) > 0).mean() > 0.9
    d = VC.depth_at(VC.view(2), SMALL_CAM)
    ctx.frame_set_depth(d, SMALL_CAM, 1.0, *VC.RANGE)
    ctx.volume_integrate(VC.view(2))
    want = VO.integrate(want, G, FO.frame_maps(d, SMALL_CAM, 1.0, *VC.RANGE)[0], SMALL_CAM, VC.view(2))
    V2, _, T2 = assert_parity(ctx, G, want, 1.0)
    assert len(T2) > len(T)


def test_mesh_errors(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    lib = L.lib()
    import ctypes as C
    nv, nt = C.c_int64(0), C.c_int64(0)
    buf = np.zeros(64, np.float32)
    # no volume
    for rc in (lib.rpe_volume_mesh(ctx._h, 1.0, C.byref(nv), C.byref(nt)),
               lib.rpe_volume_mesh_download(ctx._h, buf.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p)),
               lib.rpe_volume_upload(ctx._h, buf.ctypes.data_as(C.c_void_p))):
        assert rc == L.RPE_ERR_STATE
    G, vol = uploaded(ctx, MC.sphere())
    # a volume but no extraction yet
    assert lib.rpe_volume_mesh_download(ctx._h, buf.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p)) == L.RPE_ERR_STATE
    for w in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(L.RpeError) as e:
            ctx.volume_mesh(w)
        assert e.value.code == L.RPE_ERR_ARG and "min_weight" in str(e.value), w
    assert lib.rpe_volume_mesh(ctx._h, 1.0, None, C.byref(nt)) == L.RPE_ERR_ARG
    V, N, T = assert_parity(ctx, G, vol, 1.0)
    # normals may be NULL
    V2 = np.empty_like(V)
    T2 = np.empty_like(T)
    assert lib.rpe_volume_mesh_download(ctx._h, V2.ctypes.data_as(C.c_void_p), None, T2.ctypes.data_as(C.c_void_p)) == L.RPE_OK
    assert same(V2, V) and np.array_equal(T2, T)
    # a failed extraction leaves no mesh; so does a re-init
    with pytest.raises(L.RpeError):
        ctx.volume_mesh(0.0)
    assert lib.rpe_volume_mesh_download(ctx._h, V2.ctypes.data_as(C.c_void_p), None, T2.ctypes.data_as(C.c_void_p)) == L.RPE_ERR_STATE
    ctx.volume_mesh(1.0)
    ctx.volume_init(G.dim, voxel_size=0.05, origin=(0, 0, 0), trunc=0.15)
    assert lib.rpe_volume_mesh_download(ctx._h, V2.ctypes.data_as(C.c_void_p), None, T2.ctypes.data_as(C.c_void_p)) == L.RPE_ERR_STATE
    # an empty (re-initialised) volume: an empty mesh
    V, N, T = ctx.volume_mesh(1.0)
    assert V.shape == N.shape == (0, 3) and T.shape == (0, 3)


def test_volume_mesh_cpp(tmp_path):
    """DepthFrontEnd::integrate / mesh / uploadVolume from plain C++ (tests/cpp/volume_mesh.cpp)."""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "volume_mesh")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "volume_mesh.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, RPE_QUIET="1"))
    print(r.stdout)
    assert r.returncode == 0 and "volume_mesh: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
