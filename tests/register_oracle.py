"""numpy statement of colour registration (include/rgbd_pose_hip.h Part 3, "Colour registration": rpe_frame_register_color), the
contract the R1 / R2 kernels of csrc/rpe_register.hip are held to BIT-EXACTLY, and of the alpha gate it brings to the colour integrate
(A = 0: the pixel has no colour).  Every intermediate is IEEE fp32 in the written order.  A rig is a Rig below; a frame colour is
(h*w, 4) uint8 RGBA as the device holds it; V is the depth frame's level-0 vertex map (h*w, 3) fp32, NaN = invalid."""
from dataclasses import dataclass, field

import numpy as np

import color_oracle as CO
import volume_oracle as VO
from frontend_util import FO

F = np.float32
I12 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


@dataclass
class Rig:
    cam: tuple                                   # the colour camera (fx, fy, cx, cy, width, height)
    dist: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)      # k1 k2 p1 p2 k3
    pose12: tuple = field(default=I12)           # depth camera -> colour camera
    r2_max: float = 0.0
    cell: int = 2
    occl_tol: float = 0.02
    occl_tol_z2: float = 0.01

    def grid(self):
        c = self.cell
        return ((self.cam[4] + c - 1) // c, (self.cam[5] + c - 1) // c) if c else (0, 0)


def project(V, rig):
    """the projection of every depth pixel: dict(ok, px, py, z, x0, y0), fp32 (x0, y0 int64, 0 where not ok)"""
    fx, fy, cx, cy = [F(x) for x in rig.cam[:4]]
    wc, hc = rig.cam[4], rig.cam[5]
    k1, k2, p1, p2, k3 = [F(x) for x in rig.dist]
    p = np.asarray(rig.pose12, np.float64)
    R, t = p[:9].astype(F), p[9:].astype(F)
    r2_max = F(rig.r2_max)
    V = np.asarray(V, F).reshape(-1, 3)
    X, Y, Z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        kx = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        ky = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        kz = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        ok &= kz > F(0)
        x, y = kx / kz, ky / kz
        r2 = x * x + y * y
        if r2_max > F(0):
            ok &= r2 <= r2_max
        rad = F(1.0) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + ((F(2.0) * p1) * (x * y) + p2 * (r2 + F(2.0) * (x * x)))
        yd = y * rad + (p1 * (r2 + F(2.0) * (y * y)) + (F(2.0) * p2) * (x * y))
        px, py = fx * xd + cx, fy * yd + cy
        ok &= np.isfinite(px) & np.isfinite(py)
        x0, y0 = np.floor(px), np.floor(py)
        ok &= (x0 >= F(0)) & (x0 <= F(wc - 2)) & (y0 >= F(0)) & (y0 <= F(hc - 2))
    for a in (kx, ky, kz, px, py, x0, y0):
        assert a.dtype == F
    return dict(ok=ok, px=px, py=py, z=kz, x0=np.where(ok, x0, F(0)).astype(np.int64), y0=np.where(ok, y0, F(0)).astype(np.int64))


def zbuffer(P, rig):
    """the z-buffer after every passing pixel has written: (gh, gw) uint32, 0xffffffff where nothing projects"""
    gw, gh = rig.grid()
    zb = np.full(gw * gh, 0xFFFFFFFF, np.uint32)
    ok = P["ok"]
    fc = F(rig.cell)
    i0 = np.floor((P["px"][ok] + F(0.5)) / fc - F(0.5)).astype(np.int64)
    j0 = np.floor((P["py"][ok] + F(0.5)) / fc - F(0.5)).astype(np.int64)
    bits = P["z"][ok].view(np.uint32)
    for dj in (0, 1):
        for di in (0, 1):
            ci, cj = i0 + di, j0 + dj
            m = (ci >= 0) & (ci < gw) & (cj >= 0) & (cj < gh)
            np.minimum.at(zb, cj[m] * gw + ci[m], bits[m])
    return zb.reshape(gh, gw)


def visible(P, rig):
    """the passing pixels the colour camera sees (cell = 0: all of them)"""
    ok = P["ok"].copy()
    if rig.cell == 0:
        return ok
    gw, gh = rig.grid()
    zb = zbuffer(P, rig)
    fc = F(rig.cell)
    a, b = F(rig.occl_tol), F(rig.occl_tol_z2)
    with np.errstate(invalid="ignore", over="ignore"):
        ci = np.floor(((P["px"] + F(0.5)) / fc - F(0.5)) + F(0.5))
        cj = np.floor(((P["py"] + F(0.5)) / fc - F(0.5)) + F(0.5))
    ci, cj = np.where(ok, ci, F(0)).astype(np.int64), np.where(ok, cj, F(0)).astype(np.int64)
    assert np.all((ci >= 0) & (ci < gw) & (cj >= 0) & (cj < gh))          # its own cell is always inside the grid
    zmin = zb[cj, ci].view(F)
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= (P["z"] - zmin) <= a + b * (zmin * zmin)
    return ok


def register(V, image, rig, order="rgb", with_info=False):
    """rpe_frame_register_color: the colour camera's (hc, wc, 3) uint8 image in `order` -> the frame colour (n, 4) uint8 RGBA,
    A = 255 where a colour was found and 0 0 0 0 elsewhere"""
    wc, hc = rig.cam[4], rig.cam[5]
    img = np.asarray(image, np.uint8).reshape(hc, wc, 3)
    if order == "bgr":
        img = img[..., ::-1]
    P = project(V, rig)
    vis = visible(P, rig)
    x0, y0 = P["x0"][vis], P["y0"][vis]
    s, u = (P["px"][vis] - x0.astype(F))[:, None], (P["py"][vis] - y0.astype(F))[:, None]
    c00, c10 = img[y0, x0].astype(F), img[y0, x0 + 1].astype(F)
    c01, c11 = img[y0 + 1, x0].astype(F), img[y0 + 1, x0 + 1].astype(F)
    lerp = VO._lerp
    top, bot = lerp(c00, c10, s), lerp(c01, c11, s)
    val = lerp(top, bot, u)
    assert val.dtype == F
    out = np.zeros((len(vis), 4), np.uint8)
    out[vis, :3] = CO.quantise(val)
    out[vis, 3] = 255
    return (out, P, vis) if with_info else out


def integrate(vol, cvol, G, V, rgba, cam, pose12, k0=0, with_band=False):
    """C2 with the alpha gate: color_oracle.integrate's rule plus "the frame pixel has A != 0" for the colour update (the tsdf half does
    not look at A).  With A = 255 everywhere this IS color_oracle.integrate."""
    out, up = VO.integrate(vol, G, V, cam, pose12, k0, with_mask=True)
    fx, fy, cx, cy, w, h_ = FO._cam(cam)
    R, t = FO._pose_f(pose12)
    px, py, pz = VO.voxel_centres(G, k0, k0 + vol.shape[0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qx = R[0] * px + R[1] * py + R[2] * pz + t[0]
        qy = R[3] * px + R[4] * py + R[5] * pz + t[1]
        qz = R[6] * px + R[7] * py + R[8] * pz + t[2]
        uf = np.floor(fx * (qx / qz) + cx + F(0.5))
        vf = np.floor(fy * (qy / qz) + cy + F(0.5))
        j = np.where(up, vf, F(0)).astype(np.int64) * w + np.where(up, uf, F(0)).astype(np.int64)
        sdf = V[j, 2] - qz
        band = up & (sdf <= G.tr) & (rgba[j, 3] != 0)
        o = rgba[j[band], :3].astype(F)
        c = CO.f32(cvol[band][:, :3])
        wc = CO.f32(cvol[band][:, 3])
        nc = CO.h((c * wc[:, None] + o) / (wc[:, None] + F(1.0)))
        nw = CO.h(np.fmin(wc + F(1.0), G.W))
    cout = cvol.copy()
    sel = cout[band]
    sel[:, :3] = nc
    sel[:, 3] = nw
    cout[band] = sel
    return (out, cout, band) if with_band else (out, cout)
