"""Thin numpy-facing wrapper of the C ABI (include/rgbd_pose_hip.h) used by tests, bench.py and the
multi-GPU driver.  All computation happens in librgbdpose_hip.so on the GPU; nothing here computes."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _np_dtype(dtype):
    return np.float64 if dtype == L.F64 else np.float32


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def pose7_from_Rt(R, t, dtype=L.F32) -> np.ndarray:
    """(qw qx qy qz tx ty tz) of the Sophus::SE3<Tp> a caller would build from R, t: the quaternion is extracted
    from the Tp-rounded matrix in Tp arithmetic (Eigen's Quaternion(Matrix3) branches, sophus/so3.hpp:561).
    Host-side input preparation only."""
    dt = _np_dtype(dtype)
    m = np.asarray(R, dt).reshape(3, 3)
    one, half = dt(1), dt(0.5)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4, dt)
    if tr > 0:
        s = np.sqrt(tr + one); q[0] = half * s; s = half / s
        q[1] = (m[2, 1] - m[1, 2]) * s; q[2] = (m[0, 2] - m[2, 0]) * s; q[3] = (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + one)
        q[1 + i] = half * s; s = half / s
        q[0] = (m[k, j] - m[j, k]) * s; q[1 + j] = (m[j, i] + m[i, j]) * s; q[1 + k] = (m[k, i] + m[i, k]) * s
    return np.concatenate([q.astype(np.float64), np.asarray(t, dt).astype(np.float64)])


class Context:
    """One GPU context holding a correspondence set resident in HBM (rpe_context)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        L.check(L.lib().rpe_create(C.byref(self._h), device, C.c_void_p(stream) if stream else None))
        self.n = 0
        self.dtype = L.F32
        self._keep = {}
        self._pixels = self._model_pixels = 0   # front end: pixels of the current frame / of the model view
        self._vol_dims = (0, 0, 0)              # TSDF volume: voxels per axis (volume_init)
        self._frame_hw = None                   # (height, width) of the current frame (frame_set_color's shape)
        self._mesh_nv = None                    # vertices of the last mesh (volume_mesh_colors)
        self._matches = 0                       # matches of the last features_match / relocalize

    def close(self):
        if self._h:
            L.lib().rpe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- data
    def set_problem(self, n: int, dtype=L.F32):
        L.check(L.lib().rpe_set_problem(self._h, n, dtype))
        self.n, self.dtype = n, dtype

    def upload(self, slot: int, host: np.ndarray):
        a = np.ascontiguousarray(host, dtype=_np_dtype(self.dtype))
        assert a.size == 3 * self.n, (a.shape, self.n)
        L.check(L.lib().rpe_upload(self._h, slot, _p(a)))
        L.check(L.lib().rpe_synchronize(self._h))

    def download(self, slot: int) -> np.ndarray:
        out = np.empty((self.n, 3), _np_dtype(self.dtype))
        L.check(L.lib().rpe_download(self._h, slot, _p(out)))
        return out

    def bind(self, slot: int, device_ptr: int):
        L.check(L.lib().rpe_bind(self._h, slot, C.c_void_p(device_ptr)))

    def load(self, dtype=L.F32, xw=None, xc=None, bv=None, nw=None, nc=None):
        n = next(len(a) for a in (xw, xc, bv) if a is not None)
        self.set_problem(n, dtype)
        for slot, a in ((L.XW, xw), (L.XC, xc), (L.BV, bv), (L.NW, nw), (L.NC, nc)):
            if a is not None:
                self.upload(slot, a)
        return self

    def upload_mask(self, modality: int, mask):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int16)
        L.check(L.lib().rpe_upload_mask(self._h, modality, _p(m)))

    def upload_weight(self, modality: int, w):
        a = None if w is None else np.ascontiguousarray(w, dtype=_np_dtype(self.dtype))
        L.check(L.lib().rpe_upload_weight(self._h, modality, _p(a)))

    def download_mask(self, modality: int) -> np.ndarray:
        m = np.zeros(self.n, np.int16)
        L.check(L.lib().rpe_download_mask(self._h, modality, _p(m)))
        return m

    def synchronize(self):
        L.check(L.lib().rpe_synchronize(self._h))

    # ---- kernels
    def p2p_moments(self, flags: int = 0) -> np.ndarray:
        out = np.zeros(18)
        L.check(L.lib().rpe_p2p_moments(self._h, flags, _p(out)))
        return out

    def sine_error_sum(self, pose7):
        """lsq_pnp (reference P3P.hpp:472-502): sum over all correspondences of |normalize(R Xw + t) x bv| at pose7 = (qw, qx, qy, qz, t);
        returns (sum, number of terms)."""
        q = np.ascontiguousarray(pose7, np.float64).reshape(7)
        out, cnt = np.zeros(1), np.zeros(1, np.int64)
        L.check(L.lib().rpe_sine_error_sum(self._h, _p(q), _p(out), _p(cnt)))
        return float(out[0]), int(cnt[0])

    def normal_eq(self, kind: int, pose, flags: int = 0):
        """Returns (record32, pose_used12)."""
        p = np.array(pose, np.float64).reshape(12).copy()
        out = np.zeros(32)
        L.check(L.lib().rpe_normal_eq(self._h, kind, flags, _p(p), _p(out)))
        return out, p

    def normal_eq_device(self, kind: int, pose, d_out_ptr: int, flags: int = 0):
        p = np.array(pose, np.float64).reshape(12).copy()
        L.check(L.lib().rpe_normal_eq_device(self._h, kind, flags, _p(p), C.c_void_p(d_out_ptr)))
        return p

    @staticmethod
    def _terms(terms):
        """terms: list of (kind, scale[, robust, robust_k]) tuples or dicts."""
        arr = (L.RpeTerm * len(terms))()
        for i, t in enumerate(terms):
            if isinstance(t, dict):
                t = (t["kind"], t.get("scale", 1.0), t.get("robust", 0), t.get("robust_k", 1.0))
            t = tuple(t) + (1.0, 0, 1.0)[len(t) - 1:]
            arr[i].kind, arr[i].scale, arr[i].robust, arr[i].robust_k = int(t[0]), float(t[1]), int(t[2]), float(t[3])
        return arr

    def normal_eq_joint(self, terms, pose, flags: int = 0) -> np.ndarray:
        arr = self._terms(terms)
        p = np.array(pose, np.float64).reshape(12).copy()
        out = np.zeros(32)
        L.check(L.lib().rpe_normal_eq_joint(self._h, len(arr), arr, flags, _p(p), _p(out)))
        return out

    def gn_refine_joint(self, terms, pose, flags: int = 0, max_iter: int = 20, tol: float = 1e-9):
        arr = self._terms(terms)
        p = np.array(pose, np.float64).reshape(12).copy()
        it, step, cost = C.c_int(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_gn_refine_joint(self._h, len(arr), arr, flags, _p(p), max_iter, tol, C.byref(it), C.byref(step), C.byref(cost)))
        return p, it.value, step.value, cost.value

    def gn_refine_device(self, terms, pose, flags: int = 0, max_iter: int = 20, tol: float = 1e-9):
        """Device-resident loop: one launch per iteration, solve + exp-map on the GPU, one host wait at the end."""
        arr = self._terms(terms)
        p = np.array(pose, np.float64).reshape(12).copy()
        it, step, cost = C.c_int(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_gn_refine_device(self._h, len(arr), arr, flags, _p(p), max_iter, tol, C.byref(it), C.byref(step), C.byref(cost)))
        return p, it.value, step.value, cost.value

    def gn_step(self, kind: int, pose12_inout: np.ndarray, flags: int = 0) -> float:
        """One GN step in place on a float64[12] array; returns |delta|."""
        step = C.c_double(0)
        L.check(L.lib().rpe_gn_step(self._h, kind, flags, _p(pose12_inout), None, C.byref(step)))
        return step.value

    def gn_step_dist(self, kind: int, pose12_inout: np.ndarray, flags: int = 0) -> float:
        """One sharded GN step in place (kernel -> RCCL all-reduce -> host solve); needs comm_init."""
        step = C.c_double(0)
        L.check(L.lib().rpe_gn_step_dist(self._h, kind, flags, _p(pose12_inout), None, C.byref(step)))
        return step.value

    # ---- front end (Part 3 of the C ABI): depth frame -> maps -> projective association -> ICP
    @staticmethod
    def _camera(cam) -> "L.RpeCamera":
        """cam: (fx, fy, cx, cy, width, height); defaults of the reference simulator: (585, 585, 320, 240, 640, 480)."""
        fx, fy, cx, cy, w, h = cam
        return L.RpeCamera(float(fx), float(fy), float(cx), float(cy), int(w), int(h))

    def frame_set_depth(self, depth: np.ndarray, cam=(585.0, 585.0, 320.0, 240.0, 640, 480), depth_scale: float | None = None,
                        dmin: float = 0.0, dmax: float = 1e30, max_jump: float = 0.1, levels: int = 1):
        """depth: (height, width) uint16 (default scale 0.001: millimetres) or float32 (default scale 1: metres).
        levels > 1 also builds the coarse-to-fine pyramid (rpe_frame_set_depth_pyramid); levels = 1 is rpe_frame_set_depth."""
        k = self._camera(cam)
        d = np.ascontiguousarray(depth)
        if d.shape != (k.height, k.width):
            raise ValueError(f"depth shape {d.shape} does not match the camera ({k.height}, {k.width})")
        if d.dtype == np.uint16:
            kind, scale = L.DEPTH_U16, 0.001 if depth_scale is None else depth_scale
        elif d.dtype == np.float32:
            kind, scale = L.DEPTH_F32, 1.0 if depth_scale is None else depth_scale
        else:
            raise TypeError("depth must be uint16 or float32")
        if levels == 1:
            L.check(L.lib().rpe_frame_set_depth(self._h, _p(d), kind, C.byref(k), scale, dmin, dmax, max_jump))
        else:
            L.check(L.lib().rpe_frame_set_depth_pyramid(self._h, _p(d), kind, C.byref(k), scale, dmin, dmax, max_jump, int(levels)))
        self._pixels = k.width * k.height
        self._frame_hw = (k.height, k.width)
        return self

    def frame_set_filter(self, radius: int = 3, sigma_space: float = 2.0, depth_cut: float = 0.01, depth_cut_z2: float = 0.02):
        """Bilateral filter on the metric depth of every later frame_set_depth (rpe_frame_set_filter): a (2 radius + 1)^2 window,
        Gaussian in space (sigma_space pixels), biweight in range with the cut-off depth_cut + depth_cut_z2 z^2 metres.
        frame_set_filter(0) turns it off again; the current frame is not touched."""
        f = L.RpeDepthFilter(int(radius), float(sigma_space), float(depth_cut), float(depth_cut_z2))
        L.check(L.lib().rpe_frame_set_filter(self._h, C.byref(f)))
        return self

    def frame_filter(self):
        """(radius, sigma_space, depth_cut, depth_cut_z2) of the depth filter; radius 0 = off."""
        f = L.RpeDepthFilter()
        L.check(L.lib().rpe_frame_get_filter(self._h, C.byref(f)))
        return (f.radius, f.sigma_space, f.depth_cut, f.depth_cut_z2)

    def frame_download(self, which: int, level: int = 0) -> np.ndarray:
        """One map as (pixels, 3) float32 (MAP_DEPTH: (pixels,) metres) of pyramid level `level`; pixels of the model's view for the
        MAP_MODEL_* maps."""
        if level == 0 and which != L.MAP_DEPTH:
            n = self._model_pixels if which >= L.MAP_MODEL_VERTEX else self._pixels
            out = np.empty((n, 3), np.float32)
            L.check(L.lib().rpe_frame_download(self._h, which, _p(out)))
            return out
        k = self.frame_camera(level, which in (L.MAP_MODEL_VERTEX, L.MAP_MODEL_NORMAL))
        n = k[4] * k[5]
        out = np.empty(n if which == L.MAP_DEPTH else (n, 3), np.float32)
        L.check(L.lib().rpe_frame_download_level(self._h, which, level, _p(out)))
        return out

    def frame_camera(self, level: int = 0, model: bool = False):
        """(fx, fy, cx, cy, width, height) of a pyramid level of the frame (or the model), the fp64 values the kernels' camera was cast from."""
        k = L.RpeCamera()
        L.check(L.lib().rpe_frame_level_camera(self._h, level, int(model), C.byref(k)))
        return (k.fx, k.fy, k.cx, k.cy, k.width, k.height)

    def model_build_pyramid(self, levels: int):
        """Levels 1 .. levels-1 of the model from its level 0 (KinectFusion resize)."""
        L.check(L.lib().rpe_model_build_pyramid(self._h, int(levels)))
        return self

    def model_from_frame(self, pose12):
        p = np.array(pose12, np.float64).reshape(12)
        L.check(L.lib().rpe_model_from_frame(self._h, _p(p)))
        self._model_pixels = self._pixels
        return self

    def model_upload(self, vertex_w: np.ndarray, normal_w: np.ndarray, cam, pose12):
        k = self._camera(cam)
        v = np.ascontiguousarray(vertex_w, np.float32).reshape(-1, 3)
        nw = np.ascontiguousarray(normal_w, np.float32).reshape(-1, 3)
        if len(v) != k.width * k.height or len(nw) != len(v):
            raise ValueError("model maps must hold width*height xyz triples")
        p = np.array(pose12, np.float64).reshape(12)
        L.check(L.lib().rpe_model_upload(self._h, _p(v), _p(nw), C.byref(k), _p(p)))
        self._model_pixels = len(v)
        return self

    def associate(self, pose12, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True, count: bool = True):
        """Fill XW XC BV NW NC of this context from the frame and the model; returns the number of pairs (or None)."""
        p = np.array(pose12, np.float64).reshape(12)
        m = C.c_int64(0)
        L.check(L.lib().rpe_associate(self._h, _p(p), dist_thr, cos_thr, int(use_normals), C.byref(m) if count else None))
        self.n, self.dtype = self._pixels, L.F32
        return m.value if count else None

    def icp(self, pose12, kind: int = L.RES_P2PLANE, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9,
            use_normals: bool = True, device_resident: bool = False, fused: bool = False):
        """Projective-association ICP; returns (pose12, iterations, last |delta|, cost, pairs of the last round)."""
        p, o, it, step, cost, m = self._icp_args(pose12, kind, max_iter, tol, dist_thr, cos_thr, use_normals, device_resident, fused)
        L.check(L.lib().rpe_icp(self._h, C.byref(o), _p(p), C.byref(it), C.byref(step), C.byref(cost), C.byref(m)))
        self.n, self.dtype = self._pixels, L.F32
        return p, it.value, step.value, cost.value, m.value

    @staticmethod
    def _icp_args(pose12, kind, max_iter, tol, dist_thr, cos_thr, use_normals, device_resident, fused):
        """What the single-level loops (icp, icp_rgbd, icp_sdf) hand the library: a copy of the pose, the options, and the words the
        iterations, the last |delta|, the cost and the pairs come back in."""
        p = np.array(pose12, np.float64).reshape(12).copy()
        o = L.RpeIcpOptions(kind, max_iter, tol, dist_thr, cos_thr, int(use_normals), int(device_resident), int(fused))
        return p, o, C.c_int(0), C.c_double(0), C.c_double(0), C.c_int64(0)

    @staticmethod
    def _pyramid_args(pose12, iters, dist_thr, kind, tol, cos_thr, use_normals, device_resident, fused):
        """What the coarse-to-fine loops (icp_pyramid, icp_pyramid_rgbd, icp_pyramid_sdf) hand the library: a copy of the pose, the
        number of levels, the rounds per level, the gates per level (None: the one gate is in the options), the options, the rounds run
        per level, and the words the last |delta|, the cost and the pairs of level 0 come back in."""
        p = np.array(pose12, np.float64).reshape(12).copy()
        levels = len(iters)
        it_in = np.ascontiguousarray(iters, np.int32)
        one = 0.1 if dist_thr is None else dist_thr
        thr = None if np.ndim(one) == 0 else np.ascontiguousarray(one, np.float64)
        if thr is not None and len(thr) != levels:
            raise ValueError("dist_thr needs one gate per level")
        o = L.RpeIcpOptions(kind, 1, tol, float(one) if thr is None else 0.0, cos_thr, int(use_normals), int(device_resident), int(fused))
        return p, levels, it_in, thr, o, np.zeros(levels, np.int32), C.c_double(0), C.c_double(0), C.c_int64(0)

    def icp_pyramid(self, pose12, iters=(10, 5, 4), dist_thr=None, kind: int = L.RES_P2PLANE, tol: float = 1e-6, cos_thr: float = 0.9,
                    use_normals: bool = True, device_resident: bool = False, fused: bool = False):
        """Coarse-to-fine ICP over len(iters) levels; iters[l] rounds at level l (0 = finest).  dist_thr: one gate per level, one gate
        for every level, or None (0.1 m, icp's default).  Returns (pose12, rounds per level, last |delta|, cost, pairs of the last round),
        the last three of level 0."""
        p, levels, it_in, thr, o, it_out, step, cost, m = self._pyramid_args(pose12, iters, dist_thr, kind, tol, cos_thr, use_normals,
                                                                             device_resident, fused)
        L.check(L.lib().rpe_icp_pyramid(self._h, C.byref(o), levels, _p(it_in), _p(thr), _p(p), _p(it_out), C.byref(step), C.byref(cost), C.byref(m)))
        self.n, self.dtype = self._pixels, L.F32
        return p, tuple(int(i) for i in it_out), step.value, cost.value, m.value

    # ---- TSDF volume (Part 3): frames fused into the context's volume, raycast into the model
    def volume_init(self, dims, voxel_size: float, origin, trunc: float, max_weight: int = 64):
        """(Re)allocate and clear the volume: dims = (d0, d1, d2) voxels (2 .. 1024 each), origin = world corner of voxel (0, 0, 0)."""
        d = L.RpeVolumeDesc((C.c_int * 3)(*[int(x) for x in dims]), float(voxel_size), (C.c_double * 3)(*[float(x) for x in origin]),
                            float(trunc), int(max_weight))
        L.check(L.lib().rpe_volume_init(self._h, C.byref(d)))
        self._vol_dims = tuple(int(x) for x in dims)
        self._mesh_nv = None
        return self

    def volume_integrate(self, pose12):
        """Fuse the current frame (level 0), seen from pose12 (Xc = R Xw + t), into the volume."""
        p = np.array(pose12, np.float64).reshape(12)
        L.check(L.lib().rpe_volume_integrate(self._h, _p(p)))
        return self

    def volume_raycast(self, pose12, cam, dmin: float, dmax: float, levels: int = 1):
        """The model := the volume raycast from pose12 with camera cam over camera depths (dmin, dmax); levels > 1 also builds the
        model pyramid (rpe_model_build_pyramid)."""
        k = self._camera(cam)
        p = np.array(pose12, np.float64).reshape(12)
        L.check(L.lib().rpe_volume_raycast(self._h, _p(p), C.byref(k), float(dmin), float(dmax)))
        self._model_pixels = k.width * k.height
        if levels > 1:
            self.model_build_pyramid(levels)
        return self

    def volume_download(self) -> np.ndarray:
        """The volume as (d2, d1, d0, 2) float32: [..., 0] = tsdf, [..., 1] = weight (0 = unobserved)."""
        d0, d1, d2 = self._vol_dims
        out = np.empty((d2, d1, d0, 2), np.float32)
        L.check(L.lib().rpe_volume_download(self._h, _p(out)))
        return out

    def volume_upload(self, vol):
        """Replace the volume's voxels with `vol`, (d2, d1, d0, 2) float32 as volume_download returns it; the bits are taken as given."""
        d0, d1, d2 = self._vol_dims
        a = np.ascontiguousarray(vol, np.float32)
        if a.shape != (d2, d1, d0, 2):
            raise ValueError(f"volume_upload: expected shape {(d2, d1, d0, 2)}, got {a.shape}")
        L.check(L.lib().rpe_volume_upload(self._h, _p(a)))
        return self

    def volume_mesh(self, min_weight: float = 1.0, box=None):
        """Marching cubes over the volume (corners with weight >= min_weight): (vertices (V, 3) float32, normals (V, 3) float32, NaN
        where the field is unknown, triangles (T, 3) int32), wound so that (v1 - v0) x (v2 - v0) points to free space.  box = (lo, hi):
        only the cubes with lo <= (i, j, k) < hi per axis (rpe_volume_mesh_box; 0 <= lo <= hi <= dim - 1), everything else unchanged."""
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._mesh_nv = None
        if box is None:
            L.check(L.lib().rpe_volume_mesh(self._h, float(min_weight), C.byref(nv), C.byref(nt)))
        else:
            lo, hi = (np.ascontiguousarray(b, np.int32).reshape(3) for b in box)
            L.check(L.lib().rpe_volume_mesh_box(self._h, float(min_weight), _p(lo), _p(hi), C.byref(nv), C.byref(nt)))
        self._mesh_nv = nv.value
        V = np.empty((nv.value, 3), np.float32)
        N = np.empty((nv.value, 3), np.float32)
        T = np.empty((nt.value, 3), np.int32)
        L.check(L.lib().rpe_volume_mesh_download(self._h, _p(V), _p(N), _p(T)))
        return V, N, T

    # ---- moving volume (Part 3): the window shifted by whole voxels, where it is, and the shift that follows the camera
    def volume_shift(self, shift):
        """Move the volume's window by shift = (di, dj, dk) whole voxels along +x, +y, +z: new voxel (i, j, k) := old voxel
        (i + di, j + dj, k + dk) where that was inside, cleared elsewhere; the colour volume (if any) likewise; the origin follows.  A
        non-zero shift drops the last mesh."""
        d = np.ascontiguousarray(shift, np.int32).reshape(3)
        L.check(L.lib().rpe_volume_shift(self._h, _p(d)))
        if d.any():
            self._mesh_nv = None
        return self

    def volume_geometry(self):
        """dict(dims, voxel_size, origin (3,) float64 -- where the window is NOW --, trunc, max_weight, total_shift (3,) int64)."""
        d, tot = L.RpeVolumeDesc(), np.zeros(3, np.int64)
        L.check(L.lib().rpe_volume_geometry(self._h, C.byref(d), _p(tot)))
        return dict(dims=tuple(d.dim), voxel_size=d.voxel_size, origin=np.array(list(d.origin), np.float64), trunc=d.trunc,
                    max_weight=d.max_weight, total_shift=tot)

    def volume_follow(self, pose12, look_ahead: float, granule: int = 1) -> np.ndarray:
        """The shift (3,) int32, in multiples of `granule` voxels, that brings the world point look_ahead metres in front of the camera
        at pose12 (Xc = R Xw + t) back towards the window's centre (rpe_volume_follow).  Nothing is applied: hand it to volume_shift."""
        p = np.array(pose12, np.float64).reshape(12)
        out = np.zeros(3, np.int32)
        L.check(L.lib().rpe_volume_follow(self._h, _p(p), float(look_ahead), int(granule), _p(out)))
        return out

    # ---- volume archive (Part 3): what a shift pushes out of the window is kept in bricks on the device and put back on return
    def volume_archive(self, capacity: int):
        """Switch the archive on with a pool of `capacity` bricks (8 x 8 x 8 voxels, 4 KB + 4 KB with colour), grow it to that, or, with
        0, switch it off and free it (rpe_volume_archive).  While it is on, volume_shift takes multiples of 8 only, keeps every
        non-zero brick that leaves and restores every archived brick the window returns over."""
        L.check(L.lib().rpe_volume_archive(self._h, int(capacity)))
        return self

    def volume_archive_info(self):
        """dict(held, capacity): the bricks the archive holds and the slots of its pool (0, 0 with the archive off)."""
        held, cap = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().rpe_volume_archive_info(self._h, C.byref(held), C.byref(cap)))
        return dict(held=held.value, capacity=cap.value)

    def volume_archive_download(self):
        """The held bricks sorted by (bz, by, bx): (coords (n, 3) int64 world bricks (bx, by, bz), tsdf (n, 8, 8, 8, 2) float32 in
        (z, y, x) order, colour (n, 8, 8, 8, 4) float16, or None where no held brick has a colour bit set)."""
        n = self.volume_archive_info()["held"]
        coords = np.zeros((n, 3), np.int64)
        tsdf = np.zeros((n, 8, 8, 8, 2), np.float32)
        colour = np.zeros((n, 8, 8, 8, 4), np.float16)
        L.check(L.lib().rpe_volume_archive_download(self._h, _p(coords), _p(tsdf), _p(colour)))
        return coords, tsdf, colour if colour.view(np.uint16).any() else None

    def volume_archive_clear(self):
        """Forget every archived brick and keep the pool.  (To correct the archived bricks after a loop closure instead of losing them,
        rebuild the map with volume_map_fuse_keyframes.)"""
        L.check(L.lib().rpe_volume_archive_clear(self._h))
        return self

    # ---- map mesh (Part 3): the window and the archived bricks meshed in one extraction
    def volume_map_bounds(self):
        """(lo, hi), (3,) int64 each: the world-voxel bounding box of the window and every archived brick, in multiples of 8
        (world voxel = total shift + window index)."""
        lo, hi = np.zeros(3, np.int64), np.zeros(3, np.int64)
        L.check(L.lib().rpe_volume_map_bounds(self._h, _p(lo), _p(hi)))
        return lo, hi

    def volume_map_raycast(self, pose12, cam, dmin: float, dmax: float, box=None, levels: int = 1, color: bool = False,
                           skip_empty: bool = False):
        """The model := the MAP -- the window plus the archived bricks -- raycast from pose12 with camera cam over camera depths
        (dmin, dmax), inside box = (lo, hi) in world voxels (multiples of 8; None: volume_map_bounds): bit for bit volume_raycast of a
        dense volume of the box holding the map's content (rpe_volume_map_raycast).  color: the model colour is sampled from the map
        in the same pass (model_color_map() returns it; the photometric term and the features take it as any model colour).
        skip_empty = True runs the occupancy pre-pass (flags without RPE_MAPRAY_NO_SKIP), which changes no bit; it is off here because
        as measured it does not pay: it reads the whole window, break-even at 256^3 and 0.25 ms lost at 512^3.
        levels > 1 also builds the model pyramid, as volume_raycast does."""
        k = self._camera(cam)
        p = np.array(pose12, np.float64).reshape(12)
        flags = (L.RPE_MAPRAY_COLOR if color else 0) | (0 if skip_empty else L.RPE_MAPRAY_NO_SKIP)
        if box is None:
            L.check(L.lib().rpe_volume_map_raycast(self._h, _p(p), C.byref(k), float(dmin), float(dmax), None, None, flags))
        else:
            lo, hi = (np.ascontiguousarray(b, np.int64).reshape(3) for b in box)
            L.check(L.lib().rpe_volume_map_raycast(self._h, _p(p), C.byref(k), float(dmin), float(dmax), _p(lo), _p(hi), flags))
        self._model_pixels = k.width * k.height
        if levels > 1:
            self.model_build_pyramid(levels)
        return self

    def volume_map_mesh(self, min_weight: float = 1.0, box=None):
        """Marching cubes over the MAP -- the window plus the archived bricks -- inside box = (lo, hi) in world voxels (multiples of 8;
        None: volume_map_bounds): (vertices, normals, triangles) as volume_mesh returns them, bit for bit the mesh of a dense volume
        of the box holding the map's content, in brick order (rpe_volume_map_mesh).  volume_mesh_colors works after it."""
        nv, nt = C.c_int64(0), C.c_int64(0)
        self._mesh_nv = None
        if box is None:
            L.check(L.lib().rpe_volume_map_mesh(self._h, float(min_weight), None, None, C.byref(nv), C.byref(nt)))
        else:
            lo, hi = (np.ascontiguousarray(b, np.int64).reshape(3) for b in box)
            L.check(L.lib().rpe_volume_map_mesh(self._h, float(min_weight), _p(lo), _p(hi), C.byref(nv), C.byref(nt)))
        self._mesh_nv = nv.value
        V = np.empty((nv.value, 3), np.float32)
        N = np.empty((nv.value, 3), np.float32)
        T = np.empty((nt.value, 3), np.int32)
        L.check(L.lib().rpe_volume_mesh_download(self._h, _p(V), _p(N), _p(T)))
        return V, N, T

    # ---- colour (Part 3): a registered RGB frame fused beside the depth, sampled back at the model's and the mesh's vertices
    def frame_set_color(self, rgb, order: str = "rgb"):
        """The current frame's colour: (height, width, 3) uint8 registered to its depth (pixel (u, v) of both sees the same ray), channels
        in `order` "rgb" or "bgr".  A new depth drops it."""
        fmt = {"rgb": L.COLOR_RGB8, "bgr": L.COLOR_BGR8}.get(str(order).lower())
        if fmt is None:
            raise ValueError(f"frame_set_color: order must be 'rgb' or 'bgr', got {order!r}")
        a = np.ascontiguousarray(rgb)
        if a.dtype != np.uint8:
            raise TypeError("frame_set_color: the image must be uint8")
        if self._frame_hw is not None and a.shape != self._frame_hw + (3,):
            raise ValueError(f"frame_set_color: expected shape {self._frame_hw + (3,)}, got {a.shape}")
        L.check(L.lib().rpe_frame_set_color(self._h, _p(a), fmt))
        return self

    @staticmethod
    def color_rig(cam, dist=(0.0, 0.0, 0.0, 0.0, 0.0), pose12=(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0), r2_max: float = 0.0, cell: int = 2,
                  occl_tol: float = 0.02, occl_tol_z2: float = 0.01) -> "L.ColorRig":
        """An rpe_color_rig: the colour camera (fx, fy, cx, cy, width, height), its distortion (k1, k2, p1, p2, k3), the pose depth
        camera -> colour camera (Xk = R Xd + t), the limit on x^2 + y^2 before distortion (0 = none), the z-buffer cell in colour
        pixels (0 = no occlusion test) and the occlusion tolerance occl_tol + occl_tol_z2 z^2 metres."""
        d = np.asarray(dist, np.float64).reshape(5)
        p = np.asarray(pose12, np.float64).reshape(12)
        return L.ColorRig(Context._camera(cam), (C.c_double * 5)(*d), (C.c_double * 12)(*p), float(r2_max), int(cell), float(occl_tol),
                          float(occl_tol_z2))

    def frame_register_color(self, pixels, rig, format: str = "rgb", want_known: bool = False):
        """The current frame's colour from a SEPARATE colour camera (rpe_frame_register_color): `pixels` is that camera's own
        (height, width, 3) uint8 image, `rig` a color_rig(...).  Every depth pixel gets the colour its vertex projects to, A = 255, or
        0 0 0 0 where it has none: outside the image, no depth, or hidden from the colour camera.  want_known: returns the number of
        A = 255 pixels (one host wait); otherwise returns self and waits for nothing."""
        fmt = {"rgb": L.COLOR_RGB8, "bgr": L.COLOR_BGR8}.get(str(format).lower())
        if fmt is None:
            raise ValueError(f"frame_register_color: format must be 'rgb' or 'bgr', got {format!r}")
        a = np.ascontiguousarray(pixels)
        if a.dtype != np.uint8:
            raise TypeError("frame_register_color: the image must be uint8")
        if a.shape != (rig.cam.height, rig.cam.width, 3):
            raise ValueError(f"frame_register_color: expected shape {(rig.cam.height, rig.cam.width, 3)}, got {a.shape}")
        known = C.c_int64(0)
        L.check(L.lib().rpe_frame_register_color(self._h, _p(a), fmt, C.byref(rig), C.byref(known) if want_known else None))
        return known.value if want_known else self

    def volume_integrate_color(self, pose12):
        """volume_integrate plus the colour of the frame fused into the voxels inside the truncation band."""
        p = np.array(pose12, np.float64).reshape(12)
        L.check(L.lib().rpe_volume_integrate_color(self._h, _p(p)))
        return self

    def volume_color_download(self) -> np.ndarray:
        """The colour volume as (d2, d1, d0, 4) float16: [..., :3] = r, g, b on the 0..255 scale, [..., 3] = colour weight (0 = none)."""
        d0, d1, d2 = self._vol_dims
        out = np.empty((d2, d1, d0, 4), np.float16)
        L.check(L.lib().rpe_volume_color_download(self._h, _p(out)))
        return out

    def volume_color_upload(self, cvol):
        """Replace the colour volume with `cvol`, (d2, d1, d0, 4) float16 as volume_color_download returns it; the bits are taken as
        given."""
        d0, d1, d2 = self._vol_dims
        a = np.ascontiguousarray(cvol)
        if a.dtype != np.float16 or a.shape != (d2, d1, d0, 4):
            raise ValueError(f"volume_color_upload: expected float16 of shape {(d2, d1, d0, 4)}, got {a.dtype} {a.shape}")
        L.check(L.lib().rpe_volume_color_upload(self._h, _p(a)))
        return self

    def frame_color(self) -> np.ndarray:
        """The frame colour as the device holds it: (height, width, 4) uint8 RGBA with A = 255."""
        h, w = self._frame_hw if self._frame_hw is not None else (0, 0)
        out = np.empty((h, w, 4) if h else (1, 1, 4), np.uint8)
        L.check(L.lib().rpe_color_download(self._h, L.COLOR_FRAME, _p(out)))
        return out

    def model_color(self) -> np.ndarray:
        """Samples the colour field at the model's level-0 vertices (rpe_model_sample_color) and returns the map: (height, width, 4)
        uint8 RGBA of the model's view, A = 255 where the colour is known and (0, 0, 0, 0) where it is not."""
        L.check(L.lib().rpe_model_sample_color(self._h))
        k = self.frame_camera(0, model=True)
        out = np.empty((k[5], k[4], 4), np.uint8)
        L.check(L.lib().rpe_color_download(self._h, L.COLOR_MODEL, _p(out)))
        return out

    def model_color_map(self) -> np.ndarray:
        """The model colour map as the device holds it, nothing sampled: (height, width, 4) uint8 RGBA.  What
        volume_map_raycast(color=True) left (model_color() would replace it with the WINDOW's colour field), or any other model colour."""
        k = self.frame_camera(0, model=True)
        out = np.empty((k[5], k[4], 4), np.uint8)
        L.check(L.lib().rpe_color_download(self._h, L.COLOR_MODEL, _p(out)))
        return out

    # ---- photometric term (Part 3): tracking against the model's colour beside its geometry
    def model_color_upload(self, rgba):
        """The model colour map given by the caller: (height, width, 4) uint8 RGBA at the model's level-0 size, A = 0: unknown."""
        k = self.frame_camera(0, model=True)
        a = np.ascontiguousarray(rgba)
        if a.dtype != np.uint8 or a.size != k[4] * k[5] * 4:
            raise ValueError(f"model_color_upload: expected uint8 of shape {(k[5], k[4], 4)}, got {a.dtype} {a.shape}")
        L.check(L.lib().rpe_model_color_upload(self._h, _p(a)))
        return self

    def model_color_from_frame(self):
        """Model colour := the current frame colour (for model_from_frame users: frame-to-frame RGB-D odometry)."""
        L.check(L.lib().rpe_model_color_from_frame(self._h))
        return self

    def photo_prepare(self, levels: int = 1):
        """The frame intensity pyramid and the model photometric map of `levels` levels, from the frame colour and the model colour."""
        L.check(L.lib().rpe_photo_prepare(self._h, int(levels)))
        return self

    def photo_download(self, which: int, level: int = 0) -> np.ndarray:
        """PHOTO_FRAME: the frame intensity of a level, (pixels,) float32; PHOTO_MODEL: the model map, (pixels, 4) = I, gx, gy, zm."""
        k = self.frame_camera(level, which == L.PHOTO_MODEL)
        n = k[4] * k[5]
        out = np.empty((n, 4) if which == L.PHOTO_MODEL else n, np.float32)
        L.check(L.lib().rpe_photo_download(self._h, int(which), int(level), _p(out)))
        return out

    def photo_normal_eq(self, pose12, level: int = 0, dist_thr: float = 0.1, weight: float = 0.01) -> np.ndarray:
        """The photometric normal equations alone: H upper triangle (21) | g (6) | cost | pairs | pivot floor | pad, 32 float64."""
        return self._level_call("rpe_photo_normal_eq", False, pose12, level, float(dist_thr), float(weight))

    def photo_rows(self, pose12, level: int = 0, dist_thr: float = 0.1) -> np.ndarray:
        """(7, pixels) float32: the unscaled residual (row 0: the residual image) and Jacobian row of every frame pixel of the level,
        NaN where the pixel has no pair."""
        p = np.array(pose12, np.float64).reshape(12)
        k = self.frame_camera(level)
        out = np.empty((7, k[4] * k[5]), np.float32)
        L.check(L.lib().rpe_photo_rows(self._h, int(level), _p(p), float(dist_thr), _p(out)))
        return out

    def icp_rgbd(self, pose12, weight: float = 0.01, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9):
        """icp with the photometric term (weight in metres per intensity level) beside point-to-plane, one launch per round; returns
        (pose12, iterations, last |delta|, geometric cost, geometric pairs, photometric cost, photometric pairs) of the last round."""
        out = self._loop("rpe_icp_rgbd", pose12, max_iter, tol, dist_thr, cos_thr, 1, weight)
        self.n, self.dtype = self._pixels, L.F32
        return out

    def icp_pyramid_rgbd(self, pose12, weight: float = 0.01, iters=(10, 5, 4), dist_thr=None, tol: float = 1e-6, cos_thr: float = 0.9):
        """icp_pyramid with the photometric term; returns (pose12, rounds per level, last |delta|, geometric cost, geometric pairs,
        photometric cost, photometric pairs), the last five of level 0."""
        out = self._pyramid_loop("rpe_icp_pyramid_rgbd", pose12, iters, dist_thr, tol, cos_thr, 1, weight)
        self.n, self.dtype = self._pixels, L.F32
        return out

    # ---- what the calls of the volume terms (and the RGB-D loops above) share, each stated once
    def _level_call(self, name, rows, pose12, level, *scalars, box=()):
        """The rows call (rows: a (7, pixels) float32 buffer sized for the level) or the normal-equations call (a record of 32 float64)
        `name` of the library: level, pose, the call's own scalars, a map call's box (what _box made of it), the buffer, which it returns."""
        if rows:    # a level's size is the frame's halved per level (no frame yet, no such level: the library says so)
            h, w = self._frame_hw or (0, 0)
            out = np.empty((7, max(1, (h >> max(level, 0)) * (w >> max(level, 0)))), np.float32)
        else:
            out = np.zeros(32, np.float64)
        L.check(getattr(L.lib(), name)(self._h, int(level), _p(np.array(pose12, np.float64).reshape(12)), *scalars, *map(_p, box), _p(out)))
        return out

    @staticmethod
    def _colour(weight):
        """what a loop with colour adds to its call: the photometric weight in front, the words its cost and rows come back in behind"""
        return ((), ()) if weight is None else ((float(weight),), (C.c_double(0), C.c_int64(0)))

    @staticmethod
    def _box(box):
        """(lo, hi) of a box of world voxels as the library takes them: two int64 triples, or two NULLs for the map's bounds"""
        if box is None:
            return None, None
        return tuple(np.ascontiguousarray(b, np.int64).reshape(3) for b in box)

    def _loop(self, name, pose12, max_iter, tol, dist_thr, cos_thr, use_normals, weight=None, box=()):
        """The single-level loop `name` of the library.  weight: the photometric weight of a loop with colour (None: a loop without,
        which returns no photometric figures); box: what _box made of a map call's box (() for a call on the window)."""
        p, o, it, step, cost, m = self._icp_args(pose12, L.RES_P2PLANE, max_iter, tol, dist_thr, cos_thr, use_normals, 0, 1)
        lam, photo = self._colour(weight)
        L.check(getattr(L.lib(), name)(self._h, C.byref(o), *lam, *map(_p, box), _p(p), *map(C.byref, (it, step, cost, m) + photo)))
        return (p, it.value, step.value, cost.value, m.value) + tuple(w.value for w in photo)

    def _pyramid_loop(self, name, pose12, iters, dist_thr, tol, cos_thr, use_normals, weight=None, box=()):
        """The coarse-to-fine loop `name` of the library; weight and box as _loop's."""
        p, levels, it_in, thr, o, it_out, step, cost, m = self._pyramid_args(pose12, iters, dist_thr, L.RES_P2PLANE, tol, cos_thr, use_normals, 0, 1)
        lam, photo = self._colour(weight)
        L.check(getattr(L.lib(), name)(self._h, C.byref(o), *lam, levels, _p(it_in), _p(thr), *map(_p, box), _p(p), _p(it_out),
                                       *map(C.byref, (step, cost, m) + photo)))
        return (p, tuple(int(i) for i in it_out), step.value, cost.value, m.value) + tuple(w.value for w in photo)

    # ---- volume term (Part 3): a frame tracked against the TSDF volume itself -- no raycast, no model
    def sdf_rows(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True) -> np.ndarray:
        """(7, pixels) float32: the residual in metres (row 0: the residual image) and Jacobian row of every frame pixel of the level in
        the volume's field under pose12, NaN where the pixel has no row."""
        return self._level_call("rpe_sdf_rows", True, pose12, level, float(dist_thr), float(cos_thr), int(use_normals))

    def sdf_normal_eq(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True) -> np.ndarray:
        """The volume term's normal equations of one level: H upper triangle (21) | g (6) | sum r^2 | rows | pivot floor | pad, 32 float64."""
        return self._level_call("rpe_sdf_normal_eq", False, pose12, level, float(dist_thr), float(cos_thr), int(use_normals))

    def icp_sdf(self, pose12, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True):
        """Gauss-Newton on the volume term, one launch per round; needs a frame and a volume, no model.  Returns (pose12, iterations,
        last |delta|, sum r^2, rows of the last round)."""
        return self._loop("rpe_icp_sdf", pose12, max_iter, tol, dist_thr, cos_thr, use_normals)

    def icp_pyramid_sdf(self, pose12, iters=(10, 5, 4), dist_thr=None, tol: float = 1e-6, cos_thr: float = 0.9, use_normals: bool = True):
        """icp_sdf coarse to fine over len(iters) levels of the frame; dist_thr as icp_pyramid's.  Returns (pose12, rounds per level,
        last |delta|, sum r^2, rows of the last round), the last three of level 0."""
        return self._pyramid_loop("rpe_icp_pyramid_sdf", pose12, iters, dist_thr, tol, cos_thr, use_normals)

    # ---- volume colour term (Part 3): a photometric term against the colour volume beside the volume term -- no model, no photo_prepare
    def sdf_photo_rows(self, pose12, level: int = 0, dist_thr: float = 0.1) -> np.ndarray:
        """(7, pixels) float32: the unscaled photometric residual in intensity levels (row 0: the residual image) and Jacobian row of
        every frame pixel of the level against the colour volume under pose12, NaN where the pixel has no row."""
        return self._level_call("rpe_sdf_photo_rows", True, pose12, level, float(dist_thr))

    def sdf_photo_normal_eq(self, pose12, level: int = 0, dist_thr: float = 0.1, weight: float = 0.01) -> np.ndarray:
        """The volume colour term's normal equations alone: H upper triangle (21) | g (6) | cost | rows | pivot floor | pad, 32 float64."""
        return self._level_call("rpe_sdf_photo_normal_eq", False, pose12, level, float(dist_thr), float(weight))

    def icp_sdf_rgbd(self, pose12, weight: float = 0.01, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9,
                     use_normals: bool = True):
        """icp_sdf with the photometric rows against the colour volume (weight in metres per intensity level) beside the geometric ones,
        one launch per round; needs a frame with colour, a volume and a colour volume.  Returns (pose12, iterations, last |delta|,
        geometric sum r^2, geometric rows, photometric cost, photometric rows) of the last round."""
        return self._loop("rpe_icp_sdf_rgbd", pose12, max_iter, tol, dist_thr, cos_thr, use_normals, weight)

    def icp_pyramid_sdf_rgbd(self, pose12, weight: float = 0.01, iters=(10, 5, 4), dist_thr=None, tol: float = 1e-6, cos_thr: float = 0.9,
                             use_normals: bool = True):
        """icp_sdf_rgbd coarse to fine over len(iters) levels of the frame; dist_thr as icp_pyramid's.  Returns (pose12, rounds per level,
        last |delta|, geometric sum r^2, geometric rows, photometric cost, photometric rows), the last five of level 0."""
        return self._pyramid_loop("rpe_icp_pyramid_sdf_rgbd", pose12, iters, dist_thr, tol, cos_thr, use_normals, weight)

    # ---- map volume term (Part 3): the volume term on the whole map -- the window plus the archived bricks -- inside a box
    def map_sdf_rows(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True, box=None) -> np.ndarray:
        """sdf_rows in the field of the MAP inside box = (lo, hi) in world voxels (multiples of 8; None: volume_map_bounds): bit for bit
        sdf_rows of a dense volume of the box holding the map's content (rpe_map_sdf_rows)."""
        return self._level_call("rpe_map_sdf_rows", True, pose12, level, float(dist_thr), float(cos_thr), int(use_normals), box=self._box(box))

    def map_sdf_normal_eq(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True, box=None) -> np.ndarray:
        """sdf_normal_eq on the map inside the box: the same 32 float64."""
        return self._level_call("rpe_map_sdf_normal_eq", False, pose12, level, float(dist_thr), float(cos_thr), int(use_normals),
                                box=self._box(box))

    def icp_map_sdf(self, pose12, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True,
                    box=None):
        """icp_sdf on the map inside the box; the brick grid is built and uploaded once for all rounds.  Returns what icp_sdf returns."""
        return self._loop("rpe_icp_map_sdf", pose12, max_iter, tol, dist_thr, cos_thr, use_normals, box=self._box(box))

    def icp_pyramid_map_sdf(self, pose12, iters=(10, 5, 4), dist_thr=None, tol: float = 1e-6, cos_thr: float = 0.9, use_normals: bool = True,
                            box=None):
        """icp_pyramid_sdf on the map inside the box: the tracker of a moving window with the archive on (volume_follow -> volume_shift ->
        icp_pyramid_map_sdf -> volume_integrate).  Returns what icp_pyramid_sdf returns."""
        return self._pyramid_loop("rpe_icp_pyramid_map_sdf", pose12, iters, dist_thr, tol, cos_thr, use_normals, box=self._box(box))

    # ---- map volume colour term (Part 3): the volume colour term on the whole map -- TSDF and colour of the window plus the archived bricks
    def map_sdf_photo_rows(self, pose12, level: int = 0, dist_thr: float = 0.1, box=None) -> np.ndarray:
        """sdf_photo_rows against the MAP inside box = (lo, hi) in world voxels (multiples of 8; None: volume_map_bounds): bit for bit
        sdf_photo_rows of a dense volume and colour volume of the box holding the map's content (rpe_map_sdf_photo_rows)."""
        return self._level_call("rpe_map_sdf_photo_rows", True, pose12, level, float(dist_thr), box=self._box(box))

    def map_sdf_photo_normal_eq(self, pose12, level: int = 0, dist_thr: float = 0.1, weight: float = 0.01, box=None) -> np.ndarray:
        """sdf_photo_normal_eq on the map inside the box: the same 32 float64."""
        return self._level_call("rpe_map_sdf_photo_normal_eq", False, pose12, level, float(dist_thr), float(weight), box=self._box(box))

    def icp_map_sdf_rgbd(self, pose12, weight: float = 0.01, max_iter: int = 10, tol: float = 1e-6, dist_thr: float = 0.1, cos_thr: float = 0.9,
                         use_normals: bool = True, box=None):
        """icp_sdf_rgbd on the map inside the box; the brick grid is built and uploaded once for both fetches and all rounds.  Returns
        what icp_sdf_rgbd returns."""
        return self._loop("rpe_icp_map_sdf_rgbd", pose12, max_iter, tol, dist_thr, cos_thr, use_normals, weight, self._box(box))

    def icp_pyramid_map_sdf_rgbd(self, pose12, weight: float = 0.01, iters=(10, 5, 4), dist_thr=None, tol: float = 1e-6, cos_thr: float = 0.9,
                                 use_normals: bool = True, box=None):
        """icp_pyramid_sdf_rgbd on the map inside the box: the colour tracker of a moving window with the archive on (volume_follow ->
        volume_shift -> icp_pyramid_map_sdf_rgbd -> volume_integrate_color).  Returns what icp_pyramid_sdf_rgbd returns."""
        return self._pyramid_loop("rpe_icp_pyramid_map_sdf_rgbd", pose12, iters, dist_thr, tol, cos_thr, use_normals, weight, self._box(box))

    # ---- robust volume terms (Part 3): an IRLS weight on the rows of the four volume terms above, off by default
    def sdf_set_robust(self, kind: int = L.ROBUST_NONE, k: float = 0.0, photo_k: float = 0.0):
        """The robust weight of the normal-equation calls and loops of the volume terms, on the window and on the map: kind ROBUST_NONE
        (off), ROBUST_HUBER or ROBUST_TUKEY; k the geometric row's scale in metres, photo_k the photometric row's in unscaled intensity
        levels (0: photometric rows at weight 1).  The context's: it survives new frames, volumes and shifts (rpe_sdf_set_robust)."""
        L.check(L.lib().rpe_sdf_set_robust(self._h, int(kind), float(k), float(photo_k)))
        return self

    def sdf_robust(self):
        """(kind, k, photo_k) as set; (ROBUST_NONE, 0.0, 0.0) when off."""
        kind, k, pk = C.c_int(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_sdf_robust(self._h, C.byref(kind), C.byref(k), C.byref(pk)))
        return kind.value, k.value, pk.value

    def _weights_call(self, name, pose12, level, dist_thr, cos_thr, use_normals, photo, box=()):
        h, w = self._frame_hw or (0, 0)
        out = np.empty(max(1, (h >> max(level, 0)) * (w >> max(level, 0))), np.float32)
        L.check(getattr(L.lib(), name)(self._h, int(level), _p(np.array(pose12, np.float64).reshape(12)), float(dist_thr), float(cos_thr),
                                       int(use_normals), int(photo), *map(_p, box), _p(out)))
        return out

    def sdf_robust_weights(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True,
                           photo: bool = False) -> np.ndarray:
        """(pixels,) float32: the weight of every frame pixel's row of the level under the setting of sdf_set_robust -- the geometric
        rows' (gates as sdf_rows') or, with photo, the photometric rows' (gate as sdf_photo_rows').  NaN where the pixel has no row."""
        return self._weights_call("rpe_sdf_robust_weights", pose12, level, dist_thr, cos_thr, use_normals, photo)

    def map_sdf_robust_weights(self, pose12, level: int = 0, dist_thr: float = 0.1, cos_thr: float = 0.9, use_normals: bool = True,
                               photo: bool = False, box=None) -> np.ndarray:
        """sdf_robust_weights against the map inside the box (None: volume_map_bounds), as map_sdf_rows / map_sdf_photo_rows read it."""
        return self._weights_call("rpe_map_sdf_robust_weights", pose12, level, dist_thr, cos_thr, use_normals, photo, self._box(box))

    # ---- features and relocalisation (Part 3): correspondences without a pose guess
    def features_detect(self, which: int = L.FEAT_FRAME, threshold: int = 12, max_keypoints: int = L.MAX_KEYPOINTS) -> int:
        """Detect and describe the keypoints of the frame's colour (FEAT_FRAME) or the model colour (FEAT_MODEL); returns their number."""
        o = L.RpeFeatureOptions(int(threshold), int(max_keypoints))
        n = C.c_int(0)
        L.check(L.lib().rpe_features_detect(self._h, int(which), C.byref(o), C.byref(n)))
        return n.value

    def features(self, which: int = L.FEAT_FRAME):
        """(xy (k, 2) int32, score (k,) int32, desc (k, 8) uint32) of the side's last detection, in pixel order (with scale levels: in
        (level, level pixel) order, xy the level-0 pixel a keypoint stands at; features_scale gives the rest)."""
        cap = L.MAX_KEYPOINTS
        xy, sc, de = np.zeros((cap, 2), np.int32), np.zeros(cap, np.int32), np.zeros((cap, 8), np.uint32)
        L.check(L.lib().rpe_features_download(self._h, int(which), _p(xy), _p(sc), _p(de)))
        k = int(np.count_nonzero(sc))     # every keypoint's score is > 0 (relocalize may have detected: the count is read off here)
        xy, sc, de = xy[:k].copy(), sc[:k].copy(), de[:k].copy()
        return xy, sc, de

    def features_set_descriptor(self, kind: int):
        """The descriptor of every later detection: L.DESC_UPRIGHT (the default) or L.DESC_ORIENTED, which survives a roll of the camera.
        A change of kind drops both sides' features and the match list."""
        L.check(L.lib().rpe_features_set_descriptor(self._h, int(kind)))

    def features_descriptor(self) -> int:
        k = C.c_int(-1)
        L.check(L.lib().rpe_features_get_descriptor(self._h, C.byref(k)))
        return k.value

    def features_angles(self, which: int = L.FEAT_FRAME) -> np.ndarray:
        """(k,) int32: the angle bins (0 .. 31) of the side's keypoints, all 0 for an upright detection."""
        bins = np.full(L.MAX_KEYPOINTS, -1, np.int32)
        L.check(L.lib().rpe_features_angles(self._h, int(which), _p(bins)))
        return bins[:int(np.count_nonzero(bins >= 0))].copy()

    def features_set_levels(self, levels: int):
        """The number of scale levels (1 .. 4; scale 1, 2/3, 1/2, 1/3) of every later detection: with more than one a frame taken
        closer to the scene than its keyframe still matches it.  1 is the default; a change drops both sides' features and the match
        list."""
        L.check(L.lib().rpe_features_set_levels(self._h, int(levels)))

    def features_levels(self) -> int:
        n = C.c_int(-1)
        L.check(L.lib().rpe_features_get_levels(self._h, C.byref(n)))
        return n.value

    def features_scale(self, which: int = L.FEAT_FRAME):
        """(level (k,) int32, lxy (k, 2) int32): the level and the level pixel of the side's keypoints (features()' xy is the level-0
        pixel a keypoint stands at).  With one level: zeros, and lxy = xy."""
        level, lxy = np.full(L.MAX_KEYPOINTS, -1, np.int32), np.zeros((L.MAX_KEYPOINTS, 2), np.int32)
        L.check(L.lib().rpe_features_scale(self._h, int(which), _p(level), _p(lxy)))
        k = int(np.count_nonzero(level >= 0))
        return level[:k].copy(), lxy[:k].copy()

    def features_match(self, max_dist: int = 64, ratio=(8, 10), cross_check: bool = False) -> int:
        """Match the frame's keypoints against the model's; XW XC BV NW NC of this context become the matches.  Returns their number."""
        o = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        m = C.c_int(0)
        L.check(L.lib().rpe_features_match(self._h, C.byref(o), C.byref(m)))
        self.n, self.dtype, self._matches = m.value, L.F32, m.value
        return m.value

    def matches(self):
        """(frame keypoint, model keypoint, d1, d2 int32, weight = 256 - d1 float32) of the last match list, in frame-keypoint order."""
        m = self._matches
        fi, mi, d1, d2 = (np.zeros(m, np.int32) for _ in range(4))
        w = np.zeros(m, np.float32)
        L.check(L.lib().rpe_matches_download(self._h, _p(fi), _p(mi), _p(d1), _p(d2), _p(w)))
        return fi, mi, d1, d2, w

    def relocalize(self, method: int, thre_3d: float = 0.0, thre_2d: float = 0.0, thre_nl: float = 0.0, iters: int = 0, confidence: float = 0.99,
                   seed: int = 1, ls: int = 0, min_matches: int = 12, threshold: int = 12, max_keypoints: int = L.MAX_KEYPOINTS,
                   max_dist: int = 64, ratio=(8, 10), cross_check: bool = False):
        """The frame's pose against the model without a pose guess: features on both sides (where missing), matches, rpe_run's solver
        `method` / `ls` on them.  Returns dict(pose12, matches, iters, max_votes, masks[3, matches]); RpeError with code
        RPE_ERR_DEGENERATE when fewer than min_matches matches were found.  Refine with icp_pyramid(_rgbd) from pose12."""
        fo = L.RpeFeatureOptions(int(threshold), int(max_keypoints))
        mo = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        p = np.zeros(12, np.float64)
        it, m, mv = C.c_int(int(iters)), C.c_int(0), C.c_int(0)
        mask = np.zeros(3 * L.MAX_KEYPOINTS, np.int16)
        try:
            L.check(L.lib().rpe_relocalize(self._h, C.byref(fo), C.byref(mo), int(method), thre_3d, thre_2d, thre_nl, C.byref(it), confidence,
                                           int(seed), int(ls), int(min_matches), _p(p), C.byref(m), C.byref(mv), _p(mask)))
        finally:
            self.n, self.dtype, self._matches = m.value, L.F32, m.value
        return dict(pose12=p, matches=m.value, iters=it.value, max_votes=mv.value, masks=mask[:3 * m.value].reshape(3, m.value).copy())

    # ---- keyframes (Part 3): the model side's features kept on the device, a frame relocalised against all of them at once
    def keyframe_add(self) -> int:
        """The model side's current features (features_detect(FEAT_MODEL)) become a keyframe of this context's store; returns its id."""
        i = C.c_int(-1)
        L.check(L.lib().rpe_keyframe_add(self._h, C.byref(i)))
        return i.value

    def keyframe_add_host(self, xy, desc, xw, nw, pose12, width: int, height: int) -> int:
        """A keyframe from host arrays, shaped as keyframe() returns them (a saved map restored); returns its id."""
        xy, desc = np.ascontiguousarray(xy, np.int32).reshape(-1, 2), np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
        xw, nw = np.ascontiguousarray(xw, np.float32).reshape(-1, 3), np.ascontiguousarray(nw, np.float32).reshape(-1, 3)
        if not len(xy) == len(desc) == len(xw) == len(nw):
            raise ValueError("xy, desc, xw and nw need one row per keypoint")
        p = np.ascontiguousarray(pose12, np.float64).reshape(12)
        i = C.c_int(-1)
        L.check(L.lib().rpe_keyframe_add_host(self._h, len(xy), _p(xy), _p(desc), _p(xw), _p(nw), _p(p), int(width), int(height), C.byref(i)))
        return i.value

    def keyframe(self, kf: int):
        """dict(xy (k, 2) int32, desc (k, 8) uint32, xw (k, 3), nw (k, 3) float32, pose12, width, height) of keyframe kf."""
        n, w, h = C.c_int(0), C.c_int(0), C.c_int(0)
        pose = np.zeros(12, np.float64)
        L.check(L.lib().rpe_keyframe_info(self._h, int(kf), C.byref(n), _p(pose), C.byref(w), C.byref(h)))
        k = n.value
        xy, de = np.zeros((k, 2), np.int32), np.zeros((k, 8), np.uint32)
        xw, nw = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32)
        L.check(L.lib().rpe_keyframe_download(self._h, int(kf), _p(xy), _p(de), _p(xw), _p(nw)))
        return dict(xy=xy, desc=de, xw=xw, nw=nw, pose12=pose, width=w.value, height=h.value)

    def keyframes_len(self) -> int:
        """The number of keyframes in the store."""
        n = C.c_int(0)
        L.check(L.lib().rpe_keyframes_count(self._h, C.byref(n)))
        return n.value

    def keyframes_descriptor(self) -> int:
        """The descriptor kind of the store's keyframes (L.DESC_*), -1 while the store is empty."""
        k = C.c_int(0)
        L.check(L.lib().rpe_keyframes_descriptor(self._h, C.byref(k)))
        return k.value

    def keyframes_clear(self):
        L.check(L.lib().rpe_keyframes_clear(self._h))

    def keyframes_query(self, max_dist: int = 64, ratio=(8, 10), cross_check: bool = False):
        """(counts, order): per keyframe the matches features_match would accept against it, and the ids by (count descending, id)."""
        k = self.keyframes_len()
        o = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        counts, order = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
        L.check(L.lib().rpe_keyframes_query(self._h, C.byref(o), _p(counts), _p(order)))
        return counts[:k], order[:k]

    def keyframe_match(self, kf: int, max_dist: int = 64, ratio=(8, 10), cross_check: bool = False) -> int:
        """features_match with keyframe kf in the model's place: the slots and matches() are this keyframe's.  Returns the matches."""
        o = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        m = C.c_int(0)
        L.check(L.lib().rpe_keyframe_match(self._h, int(kf), C.byref(o), C.byref(m)))
        self.n, self.dtype, self._matches = m.value, L.F32, m.value
        return m.value

    def relocalize_keyframes(self, method: int, candidates: int = 3, thre_3d: float = 0.0, thre_2d: float = 0.0, thre_nl: float = 0.0,
                             iters: int = 0, confidence: float = 0.99, seed: int = 1, ls: int = 0, min_matches: int = 12, threshold: int = 12,
                             max_keypoints: int = L.MAX_KEYPOINTS, max_dist: int = 64, ratio=(8, 10), cross_check: bool = False):
        """The frame's pose without a pose guess and without knowing which keyframe it sees: the query, then relocalize's solver run on
        each of the `candidates` best-ranked keyframes with at least min_matches matches; the one with the most votes wins.  Returns
        dict(pose12, keyframe, matches, iters, max_votes, masks[3, matches]); RpeError with code RPE_ERR_DEGENERATE (and the attributes
        keyframe / matches of the best-ranked one) when no keyframe has min_matches matches."""
        fo = L.RpeFeatureOptions(int(threshold), int(max_keypoints))
        mo = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        p = np.zeros(12, np.float64)
        it, kf, m, mv = C.c_int(int(iters)), C.c_int(-1), C.c_int(0), C.c_int(0)
        mask = np.zeros(3 * L.MAX_KEYPOINTS, np.int16)
        try:
            L.check(L.lib().rpe_relocalize_keyframes(self._h, C.byref(fo), C.byref(mo), int(candidates), int(method), thre_3d, thre_2d, thre_nl,
                                                     C.byref(it), confidence, int(seed), int(ls), int(min_matches), _p(p), C.byref(kf),
                                                     C.byref(m), C.byref(mv), _p(mask)))
        except L.RpeError as e:
            if e.code == L.RPE_ERR_DEGENERATE:      # the query ran: the match list is gone.  An argument or state error changed nothing
                e.keyframe, e.matches = kf.value, m.value
                self.n, self.dtype, self._matches = 0, L.F32, 0
            raise
        self.n, self.dtype, self._matches = m.value, L.F32, m.value
        return dict(pose12=p, keyframe=kf.value, matches=m.value, iters=it.value, max_votes=mv.value,
                    masks=mask[:3 * m.value].reshape(3, m.value).copy())

    # ---- keyframe graph (Part 3): the keyframes linked by their matches, every pose refined jointly
    def keyframes_link(self, first: int = 0, min_matches: int = 12, max_dist: int = 64, ratio=(8, 10), cross_check: bool = False):
        """(Re)build the edges of the keyframes >= first against every older keyframe; returns the graph's (edges, pairs)."""
        o = L.RpeMatchOptions(int(max_dist), int(ratio[0]), int(ratio[1]), int(cross_check))
        e, n = C.c_int(0), C.c_int64(0)
        L.check(L.lib().rpe_keyframes_link(self._h, int(first), C.byref(o), int(min_matches), C.byref(e), C.byref(n)))
        return e.value, n.value

    def graph_info(self):
        """(edges, pairs) of the graph."""
        e, n = C.c_int(0), C.c_int64(0)
        L.check(L.lib().rpe_graph_info(self._h, C.byref(e), C.byref(n)))
        return e.value, n.value

    def graph_edges(self) -> np.ndarray:
        """(edges, 3) int32: newer keyframe j, older keyframe i and the number of pairs, ordered by (j, i)."""
        out = np.zeros((self.graph_info()[0], 3), np.int32)
        L.check(L.lib().rpe_graph_edges(self._h, _p(out) if len(out) else None))
        return out

    def graph_edge(self, edge: int):
        """(a, b) of edge number `edge`: positions inside keyframe j / keyframe i, in the order of j's keypoints."""
        jic = self.graph_edges()
        if not 0 <= int(edge) < len(jic):
            raise L.RpeError(L.RPE_ERR_ARG, f"no edge {edge} ({len(jic)} in the graph)")
        a, b = np.zeros(jic[edge, 2], np.int32), np.zeros(jic[edge, 2], np.int32)
        L.check(L.lib().rpe_graph_edge_download(self._h, int(edge), _p(a), _p(b)))
        return a, b

    def graph_add_edge(self, j: int, i: int, a, b):
        """Edge (j, i) := the caller's pairs (a solver's inliers), replacing an existing one."""
        a, b = np.ascontiguousarray(a, np.int32).reshape(-1), np.ascontiguousarray(b, np.int32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("a and b need one entry per pair")
        L.check(L.lib().rpe_graph_add_edge_host(self._h, int(j), int(i), len(a), _p(a), _p(b)))

    def _graph_poses(self, poses12):
        if poses12 is None:
            return None
        p = np.ascontiguousarray(poses12, np.float64).reshape(-1, 12)
        if len(p) != self.keyframes_len():
            raise ValueError("one pose per keyframe")
        return p

    def graph_residuals(self, poses12=None, gate: float = 0.1) -> np.ndarray:
        """(pairs, 3) float32: r of every pair at the poses (None: the store's), NaN where the pair does not count."""
        p = self._graph_poses(poses12)
        out = np.zeros((self.graph_info()[1], 3), np.float32)
        L.check(L.lib().rpe_graph_residuals(self._h, None if p is None else _p(p), float(gate), _p(out)))
        return out

    def graph_normal_eq(self, poses12=None, gate: float = 0.1) -> np.ndarray:
        """(edges, GRAPH_RECORD) float64: the records of one round."""
        p = self._graph_poses(poses12)
        out = np.zeros((self.graph_info()[0], L.GRAPH_RECORD), np.float64)
        L.check(L.lib().rpe_graph_normal_eq(self._h, None if p is None else _p(p), float(gate), _p(out)))
        return out

    def keyframes_optimize(self, gates, anchor: int = 0, tol: float = 0.0, apply: bool = True):
        """Gated Gauss-Newton over every keyframe pose, one round per gate.  Returns (poses (K, 12), stats (rounds run, 3): counted
        pairs, cost and |delta| per round).  apply: the store takes the poses and its world points move with them."""
        g = np.ascontiguousarray(gates, np.float64).reshape(-1)
        poses = np.zeros((max(self.keyframes_len(), 1), 12), np.float64)
        stats, done = np.zeros((max(len(g), 1), 3), np.float64), C.c_int(0)
        L.check(L.lib().rpe_keyframes_optimize(self._h, int(anchor), len(g), _p(g), float(tol), int(bool(apply)), _p(poses), _p(stats), C.byref(done)))
        return poses[:self.keyframes_len()], stats[:done.value]

    # ---- keyframe depth (Part 3): a keyframe's depth and colour kept beside it, the volume rebuilt from a list of keyframes
    def keyframe_attach_frame(self, kf: int):
        """The current frame's level-0 depth (the z of its vertex map, NaN = invalid), its camera and, if it has one, its colour become
        keyframe kf's attachment, replacing an earlier one."""
        L.check(L.lib().rpe_keyframe_attach_frame(self._h, int(kf)))
        return self

    def keyframe_attach(self, kf: int, z, rgba=None, cam=(585.0, 585.0, 320.0, 240.0, 640, 480)):
        """The same from host arrays: z (height, width) float32 metric depth, NaN = invalid (the bits are taken as given); rgba
        (height, width, 4) uint8 or None; cam the camera they were taken with (its size must be the keyframe's)."""
        k = self._camera(cam)
        d = np.ascontiguousarray(z, np.float32)
        if d.size != k.width * k.height:
            raise ValueError(f"keyframe_attach: z has {d.size} values, the camera {k.width * k.height} pixels")
        c = None
        if rgba is not None:
            c = np.ascontiguousarray(rgba, np.uint8)
            if c.size != 4 * k.width * k.height:
                raise ValueError(f"keyframe_attach: rgba has {c.size} bytes, the camera {4 * k.width * k.height}")
        L.check(L.lib().rpe_keyframe_attach_host(self._h, int(kf), _p(d), None if c is None else _p(c), C.byref(k)))
        return self

    def keyframe_attachment(self, kf: int):
        """dict(z (height, width) float32 or None, rgba (height, width, 4) uint8 or None, cam (fx, fy, cx, cy, width, height) or None)
        of what keyframe kf carries."""
        hd, hc, k = C.c_int(0), C.c_int(0), L.RpeCamera()
        L.check(L.lib().rpe_keyframe_attachment_info(self._h, int(kf), C.byref(hd), C.byref(hc), C.byref(k)))
        if not hd.value:
            return dict(z=None, rgba=None, cam=None)
        z = np.empty((k.height, k.width), np.float32)
        c = np.empty((k.height, k.width, 4), np.uint8) if hc.value else None
        L.check(L.lib().rpe_keyframe_attachment_download(self._h, int(kf), _p(z), None if c is None else _p(c)))
        return dict(z=z, rgba=c, cam=(k.fx, k.fy, k.cx, k.cy, k.width, k.height))

    def volume_fuse_keyframes(self, ids=None, poses=None, clear: bool = True, color: bool = False, cull: bool = True):
        """Fuse the attachments of the keyframes `ids` (None: every keyframe that carries depth, by id) into the volume in list order,
        one launch: bit for bit what volume_init (clear) and one volume_integrate / volume_integrate_color (color) per entry leave.
        poses: one (12,) pose per list entry, None = the store's.  cull=False switches the per-workgroup cull off (the same bits)."""
        flags = (L.FUSE_CLEAR if clear else 0) | (L.FUSE_COLOR if color else 0) | (0 if cull else L.FUSE_NO_CULL)
        i = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
        p = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if p is not None and (i is None or len(p) != len(i)):
            raise ValueError("volume_fuse_keyframes: poses need ids, and one pose per list entry")
        L.check(L.lib().rpe_volume_fuse_keyframes(self._h, None if i is None else _p(i), 0 if i is None else len(i),
                                                  None if p is None else _p(p), flags))
        if clear:
            self._mesh_nv = None
        return self

    def volume_map_fuse_keyframes(self, ids=None, poses=None, clear: bool = True, color: bool = False, cull: bool = True, box=None) -> dict:
        """Rebuild the MAP -- the window plus the archived bricks -- from the keyframes: the list (as volume_fuse_keyframes takes it) fused
        into every brick of box = (lo, hi) in world voxels (multiples of 8; None: volume_map_bounds), in the window or not, bit for bit
        what volume_fuse_keyframes leaves in a dense volume of the box that held the map's content (rpe_volume_map_fuse_keyframes).
        Bricks outside the window that become non-empty take archive slots -- RPE_ERR_STATE, and nothing written, if the pool is too
        small --, held bricks that end empty under clear give theirs back.  Returns dict(bricks in the box, written, archived = slots
        newly taken, released).  After a loop closure: keyframes_optimize -> volume_map_fuse_keyframes(clear=True) -> volume_map_mesh."""
        flags = (L.FUSE_CLEAR if clear else 0) | (L.FUSE_COLOR if color else 0) | (0 if cull else L.FUSE_NO_CULL)
        i = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
        p = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if p is not None and (i is None or len(p) != len(i)):
            raise ValueError("volume_map_fuse_keyframes: poses need ids, and one pose per list entry")
        lo, hi = self._box(box)
        st = np.zeros(4, np.int64)
        L.check(L.lib().rpe_volume_map_fuse_keyframes(self._h, None if i is None else _p(i), 0 if i is None else len(i),
                                                      None if p is None else _p(p), flags, _p(lo), _p(hi), _p(st)))
        if clear:
            self._mesh_nv = None
        return dict(zip(("bricks", "written", "archived", "released"), (int(x) for x in st)))

    def volume_mesh_colors(self) -> np.ndarray:
        """(V, 4) uint8 RGBA of the last mesh's vertices (volume_mesh, volume_map_mesh): the colour field there, as model_color samples
        it."""
        n = self._mesh_nv or 0
        out = np.empty((n, 4), np.uint8)
        L.check(L.lib().rpe_volume_mesh_colors(self._h, _p(out) if n else None))
        return out

    def gn_steps_dist(self, kind: int, pose12_inout: np.ndarray, steps: int, flags: int = 0) -> float:
        """`steps` sharded GN steps in place, the loop inside the library; returns the last |delta|."""
        step = C.c_double(0)
        L.check(L.lib().rpe_gn_steps_dist(self._h, kind, flags, _p(pose12_inout), steps, C.byref(step)))
        return step.value

    def gn_steps_dist_device(self, kind: int, pose12_inout: np.ndarray, steps: int, flags: int = 0) -> float:
        """`steps` sharded GN steps over the RCCL communicator chained on the device (rpe_gn_steps_dist_device: solve + exp-map in the
        kernels, the host enqueues everything and waits once); returns the last |delta|."""
        step = C.c_double(0)
        L.check(L.lib().rpe_gn_steps_dist_device(self._h, kind, flags, _p(pose12_inout), steps, C.byref(step)))
        return step.value

    def comm_init(self, world: int, rank: int, id128: bytes):
        buf = (C.c_char * 128).from_buffer_copy(id128)
        L.check(L.lib().rpe_comm_init(self._h, world, rank, buf))

    def p2p_export(self) -> bytes:
        """64-byte HIP IPC handle of this context's mailbox (peer-to-peer all-reduce over xGMI)."""
        buf = (C.c_char * 64)()
        L.check(L.lib().rpe_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_init(self, world: int, rank: int, handles: bytes):
        assert len(handles) == 64 * world
        buf = (C.c_char * len(handles)).from_buffer_copy(handles)
        L.check(L.lib().rpe_p2p_init(self._h, world, rank, buf))

    def p2p_destroy(self):
        L.check(L.lib().rpe_p2p_destroy(self._h))

    def comm_count(self) -> int:
        """ranks of this context's RCCL communicator, from the communicator (ncclCommCount); 0 = none"""
        n = C.c_int(0)
        L.check(L.lib().rpe_comm_count(self._h, C.byref(n)))
        return n.value

    def bus_id(self) -> str:
        buf = C.create_string_buffer(64)
        L.check(L.lib().rpe_device_bus_id(self._h, buf, 64))
        return buf.value.decode()

    def comm_destroy(self):
        L.check(L.lib().rpe_comm_destroy(self._h))

    def hostex_init(self, world: int, rank: int, name: str, create: bool):
        """Host-side all-reduce between the node's rank processes (POSIX shared memory, sums in rank order); after this
        gn_step_dist / gn_steps_dist / gn_refine / score are sharded calls."""
        L.check(L.lib().rpe_hostex_init(self._h, world, rank, name.encode(), 1 if create else 0))

    def hostex_destroy(self):
        L.check(L.lib().rpe_hostex_destroy(self._h))

    def tune_host_thread(self, kind: int, pose, flags: int = 0, steps: int = 200, reps: int = 5):
        """rpe_tune_host_thread: measure candidate CPUs for the thread that drives the resident loop, leave THIS thread pinned to the
        fastest.  Returns dict(cpu, us_per_step, trials={cpu: us})."""
        p = np.ascontiguousarray(pose, np.float64).reshape(12)
        best, us, n = C.c_int(-1), C.c_double(0), C.c_int(0)
        cpus, tus = np.zeros(16, np.int32), np.zeros(16, np.float64)
        L.check(L.lib().rpe_tune_host_thread(self._h, kind, flags, _p(p), steps, reps, C.byref(best), C.byref(us), _p(cpus), _p(tus), 16, C.byref(n)))
        return {"cpu": best.value, "us_per_step": us.value, "trials": {int(cpus[i]): float(tus[i]) for i in range(n.value)}}

    def timing_enable(self, max_records: int, stride: int = 1):
        L.check(L.lib().rpe_timing_enable(self._h, max_records, stride))

    def timing_calibrate(self, pairs: int = 200):
        """(average, minimum) milliseconds an empty HIP event pair reports on this context's stream."""
        a, m = C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_timing_calibrate(self._h, pairs, C.byref(a), C.byref(m)))
        return a.value, m.value

    def timing_collect(self):
        cnt, tot, mn = C.c_int(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_timing_collect(self._h, C.byref(cnt), C.byref(tot), C.byref(mn)))
        return cnt.value, tot.value, mn.value

    def resident_state(self) -> dict:
        """enabled / lost grids / co-residency cap of this context's resident loops (rpe_debug_resident_state)."""
        en, lost, cap = C.c_int(0), C.c_int(0), C.c_int(0)
        L.check(L.lib().rpe_debug_resident_state(self._h, C.byref(en), C.byref(lost), C.byref(cap)))
        return {"enabled": bool(en.value), "host_driven": bool(en.value & 2), "solver": bool(en.value & 4), "lost": lost.value, "cap": cap.value}

    def inject_resident_fault(self, iteration: int = 0, pose_wait_s: float = 0.0):
        """Test hook (rpe_debug_inject_resident_fault): the last workgroup of the next host-driven resident loops withholds its sums of
        `iteration`; (0, 0) switches it off."""
        L.check(L.lib().rpe_debug_inject_resident_fault(self._h, iteration, pose_wait_s))

    def gn_refine(self, kinds, pose, scales=None, flags: int = 0, max_iter: int = 20, tol: float = 1e-9):
        kinds = np.ascontiguousarray(kinds, np.int32)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float64)
        p = np.array(pose, np.float64).reshape(12).copy()
        it, step, cost = C.c_int(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().rpe_gn_refine(self._h, len(kinds), _p(kinds), _p(sc), flags, _p(p), max_iter, tol, C.byref(it), C.byref(step),
                                      C.byref(cost)))
        return p, it.value, step.value, cost.value

    def score(self, kind: int, poses7, thre_3d=0.0, cos_thr=2.0, cos_nl=2.0, mode=L.SCORE_EXACT) -> np.ndarray:
        q = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
        v = np.zeros(len(q), np.int32)
        L.check(L.lib().rpe_score(self._h, kind, mode, _p(q), len(q), thre_3d, cos_thr, cos_nl, _p(v)))
        return v

    def inlier_mask(self, kind: int, pose7, thre_3d=0.0, cos_thr=2.0, cos_nl=2.0, mode=L.SCORE_EXACT) -> int:
        q = np.ascontiguousarray(pose7, np.float64).reshape(7)
        v = C.c_int(0)
        L.check(L.lib().rpe_inlier_mask(self._h, kind, mode, _p(q), thre_3d, cos_thr, cos_nl, C.byref(v)))
        return v.value

    def score_session_begin(self, kind: int, thre_3d=0.0, cos_thr=2.0, cos_nl=2.0, mode=L.SCORE_EXACT) -> bool:
        """Open a resident scoring session (rpe_score_session_begin): score() calls of <= 128 hypotheses and inlier_mask() calls with
        these parameters are then served by one resident launch.  False if the context cannot hold one (RPE_ERR_STATE)."""
        rc = L.lib().rpe_score_session_begin(self._h, kind, mode, thre_3d, cos_thr, cos_nl)
        if rc == L.RPE_ERR_STATE:
            return False
        L.check(rc)
        return True

    def score_session_end(self):
        L.check(L.lib().rpe_score_session_end(self._h))

    @contextlib.contextmanager
    def score_session(self, kind: int, thre_3d=0.0, cos_thr=2.0, cos_nl=2.0, mode=L.SCORE_EXACT):
        """`with ctx.score_session(kind, ...) as resident:` -- the session is ended on the way out whatever happens inside (an exception
        between _begin and _end would otherwise leave the device's resident slot to the session until its grid's bounded wait has run
        out: other contexts then run without resident grids for up to 2 s).  `resident` = whether a session could be opened."""
        opened = self.score_session_begin(kind, thre_3d, cos_thr, cos_nl, mode)
        try:
            yield opened
        finally:
            if opened and self._h:
                self.score_session_end()

    def nl_round(self, c_opt, Cw, Cc, Rwc) -> np.ndarray:
        a = [np.ascontiguousarray(x, np.float64) for x in (c_opt, Cw, Cc, Rwc)]
        out = np.zeros(44)
        L.check(L.lib().rpe_nl_round(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(out)))
        return out


def comm_unique_id() -> bytes:
    buf = (C.c_char * 128)()
    L.check(L.lib().rpe_comm_unique_id(buf))
    return bytes(buf)


def pose_from_moments(m17):
    m = np.ascontiguousarray(m17, np.float64)
    R, t = np.zeros(9), np.zeros(3)
    L.check(L.lib().rpe_pose_from_moments(_p(m), _p(R), _p(t)))
    return R.reshape(3, 3), t


def gn_solve(ne32):
    a = np.ascontiguousarray(ne32, np.float64)
    d = np.zeros(6)
    L.check(L.lib().rpe_gn_solve(_p(a), _p(d)))
    return d


def gn_apply(delta6, pose):
    d = np.ascontiguousarray(delta6, np.float64)
    p = np.array(pose, np.float64).reshape(12).copy()
    L.check(L.lib().rpe_gn_apply(_p(d), _p(p)))
    return p


def graph_solve(K: int, ji, records, fixed=None):
    """The joint update of a keyframe graph from its records (host, no GPU): delta (K, 6); fixed = ids or a mask of K."""
    ji = np.ascontiguousarray(ji, np.int32).reshape(-1, 2)
    rec = np.ascontiguousarray(records, np.float64).reshape(len(ji), L.GRAPH_RECORD)
    mask = np.zeros(int(K), np.uint8)
    if fixed is not None:
        f = np.asarray(fixed)
        if f.dtype == bool:
            mask[:] = f
        else:
            mask[f.astype(np.int64)] = 1
    d = np.zeros((int(K), 6), np.float64)
    L.check(L.lib().rpe_graph_solve(int(K), len(ji), _p(ji), _p(rec), _p(mask), _p(d)))
    return d


def ao(xw, xc):
    """Reference FFI: ao(x_w, x_c, n, R_cw, t) (Library.cpp:17)."""
    xw = np.ascontiguousarray(xw, np.float32)
    xc = np.ascontiguousarray(xc, np.float32)
    R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
    L.lib().ao(_p(xw), _p(xc), len(xw), _p(R), _p(t))
    return R.reshape(3, 3), t


def ao_ransac(xw, xc):
    """Reference FFI: ao_ransac(x_w, x_c, n, R_cw, t) (Library.cpp:47)."""
    xw = np.ascontiguousarray(xw, np.float32)
    xc = np.ascontiguousarray(xc, np.float32)
    R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
    L.lib().ao_ransac(_p(xw), _p(xc), len(xw), _p(R), _p(t))
    return R.reshape(3, 3), t


# ---- adapter-level pipelines (rpe_run): method / ls ids shared with the oracle's C API
M_SHINJI_RANSAC, M_SHINJI_RANSAC2, M_SHINJI_PROSAC, M_KNEIP_RANSAC, M_KNEIP_PROSAC = 0, 1, 2, 3, 4
M_SK_RANSAC, M_SK_PROSAC, M_NL_KNEIP_RANSAC, M_NL_SHINJI_RANSAC, M_NL_SK_RANSAC, M_NONE = 5, 6, 7, 8, 9, 10
LS_NONE, LS_SHINJI_INLIERS, LS_NL_BUGCOMPAT, LS_NL_FIXED, LS_SHINJI_ALL, LS_GN_P2P, LS_GN_JOINT, LS_GN_P2PLANE, LS_GN_BEARING, LS_GN_REPROJ = range(10)


def run(method, dtype=L.F32, xw=None, xc=None, bv=None, nw=None, nc=None, weights=None, f=585.0, thre_3d=0.0, thre_2d=0.0, thre_nl=0.0,
        iters=0, confidence=0.99, seed=1, ls=LS_NONE, score_mode=L.SCORE_EXACT, mask_in=None, pose_in=None, max_votes_in=1, want_masks=True):
    """Run one solver of pose/*.hpp on a freshly built adapter (AOOnly / PnP / AO / NormalAO chosen like the
    reference's demos do).  Returns dict(R, t, iters, max_votes, masks[3, n]); want_masks=False leaves the masks on the device
    (mask_out = NULL: no read-back), masks is then None."""
    dt = _np_dtype(dtype)
    arrs = {k: (None if a is None else np.ascontiguousarray(a, dtype=dt)) for k, a in dict(xw=xw, xc=xc, bv=bv, nw=nw, nc=nc).items()}
    n = len(arrs["xw"])
    w = None if weights is None else np.asfortranarray(weights, dtype=dt)
    prob = L.RpeProblem(n, dtype, _p(arrs["bv"]), _p(arrs["xc"]), _p(arrs["nc"]), _p(arrs["xw"]), _p(arrs["nw"]), _p(w),
                        0 if w is None else w.shape[1], f, f)
    R, t = np.zeros(9), np.zeros(3)
    if pose_in is not None:
        R[:] = np.asarray(pose_in[0], float).reshape(9)
        t[:] = np.asarray(pose_in[1], float)
    else:
        R[:] = np.eye(3).reshape(9)
    it, mv = C.c_int(iters), C.c_int(max_votes_in)
    mi = None if mask_in is None else np.ascontiguousarray(mask_in, dtype=np.int16)
    mo = np.zeros((3, n), np.int16) if want_masks else None
    L.check(L.lib().rpe_run(method, C.byref(prob), thre_3d, thre_2d, thre_nl, C.byref(it), confidence, seed, ls, score_mode, _p(mi), _p(R),
                            _p(t), C.byref(mv), _p(mo)))
    return dict(R=R.reshape(3, 3), t=t, iters=it.value, max_votes=mv.value, masks=mo)


def _problem(dtype, xw, xc, bv, nw, nc, weights, f):
    dt = _np_dtype(dtype)
    arrs = {k: (None if a is None else np.ascontiguousarray(a, dtype=dt)) for k, a in dict(xw=xw, xc=xc, bv=bv, nw=nw, nc=nc).items()}
    n = len(arrs["xw"])
    w = None if weights is None else np.asfortranarray(weights, dtype=dt)
    prob = L.RpeProblem(n, dtype, _p(arrs["bv"]), _p(arrs["xc"]), _p(arrs["nc"]), _p(arrs["xw"]), _p(arrs["nw"]), _p(w),
                        0 if w is None else w.shape[1], f, f)
    return prob, n, (arrs, w)   # the last item keeps the buffers alive


def host_hypotheses(method, dtype=L.F32, xw=None, xc=None, bv=None, nw=None, nc=None, weights=None, f=585.0, iters=0, seed=1):
    """rpe_host_hypotheses: the hypothesis stream `method` generates in `iters` iterations (no GPU).  Returns (q7[H, 7], first[iters + 1])."""
    prob, n, keep = _problem(dtype, xw, xc, bv, nw, nc, weights, f)
    cap = 3 * iters + 1
    q7, first = np.zeros((cap, 7)), np.zeros(iters + 1, np.int32)
    H = L.lib().rpe_host_hypotheses(method, C.byref(prob), iters, seed, _p(q7), cap, _p(first))
    if H < 0:
        L.check(H)
    return q7[:H].copy(), first


def run_replay(method, poses7, first, dtype=L.F32, xw=None, xc=None, bv=None, nw=None, nc=None, weights=None, f=585.0, thre_3d=0.0, thre_2d=0.0,
               thre_nl=0.0, iters=0, confidence=0.99, ls=LS_NONE, score_mode=L.SCORE_EXACT):
    """rpe_run_replay: rpe_run with the hypotheses of iteration i taken from poses7[first[i]:first[i+1]]."""
    prob, n, keep = _problem(dtype, xw, xc, bv, nw, nc, weights, f)
    poses7 = np.ascontiguousarray(poses7, np.float64).reshape(-1, 7)
    first = np.ascontiguousarray(first, np.int32)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    it, mv = C.c_int(iters), C.c_int(0)
    mo = np.zeros((3, n), np.int16)
    L.check(L.lib().rpe_run_replay(method, C.byref(prob), _p(poses7), _p(first), len(first) - 1, thre_3d, thre_2d, thre_nl, C.byref(it), confidence, ls,
                                   score_mode, _p(R), _p(t), C.byref(mv), _p(mo)))
    return dict(R=R.reshape(3, 3), t=t, iters=it.value, max_votes=mv.value, masks=mo)


class HostExchange:
    """The host-side exchange by itself (no GPU): all-reduce of up to 64 doubles / 8192 int32 between the rank processes of one node
    through a POSIX shared-memory segment; every rank gets bitwise the same sums (rank order)."""

    def __init__(self, name: str, world: int, rank: int, create: bool, timeout_s: float = 10.0):
        self._h = C.c_void_p()
        L.check(L.lib().rpe_host_exchange_open(name.encode(), world, rank, 1 if create else 0, float(timeout_s), C.byref(self._h)))
        self.world, self.rank = world, rank

    def allreduce_f64(self, v) -> np.ndarray:
        a = np.ascontiguousarray(v, np.float64).copy()
        L.check(L.lib().rpe_host_exchange_allreduce_f64(self._h, _p(a), a.size))
        return a

    def allreduce_i32(self, v) -> np.ndarray:
        a = np.ascontiguousarray(v, np.int32).copy()
        L.check(L.lib().rpe_host_exchange_allreduce_i32(self._h, _p(a), a.size))
        return a

    def set_label(self, label: str):
        L.check(L.lib().rpe_host_exchange_set_label(self._h, label.encode()))

    def labels_collide(self) -> bool:
        return bool(L.lib().rpe_host_exchange_labels_collide(self._h))

    def unlink(self):
        L.check(L.lib().rpe_host_exchange_unlink(self._h))

    def close(self):
        if self._h:
            L.lib().rpe_host_exchange_close(self._h)
            self._h = C.c_void_p()
