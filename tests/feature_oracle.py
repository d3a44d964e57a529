"""The numpy statement of the feature stage (include/rgbd_pose_hip.h Part 3, "Features and relocalisation"): luma, segment-test
detector with score and 3 x 3 non-maximum suppression, the cap, the 256-bit descriptor over 5 x 5 box sums, Hamming matching with the
ratio test and the cross-check, and the gather into the five solver slots.  Everything is integer arithmetic or a comparison, so the
GPU is held to it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import gen_brief_table as GB  # noqa: E402

BORDER = 16
MAX_KEYPOINTS = 4096
THRESHOLD = 12
MAX_DIST, RATIO_NUM, RATIO_DEN = 64, 8, 10
# the 16 pixels of the ring of radius 3, clockwise from the top (image y down)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2),
        (-1, -3))
PAIRS = np.array(GB.pairs(), np.int64)


def luma(rgba):
    """(h, w, 4) uint8 -> int32 (h, w): (77 r + 150 g + 29 b + 128) >> 8, 0 where A = 0"""
    c = rgba.astype(np.int32)
    y = (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
    return np.where(c[..., 3] != 0, y, 0).astype(np.int32)


def shifted(img, dx, dy, fill=0):
    """out[v, u] = img[v + dy, u + dx], `fill` outside the image"""
    h, w = img.shape
    out = np.full_like(img, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = img[ys, xs]
    return out


def box_sums(Y):
    """the 5 x 5 box sum of the luma around every pixel, pixels outside the image counting 0 (int32, <= 6375)"""
    S = np.zeros_like(Y)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            S += shifted(Y, dx, dy)
    return S


def scores(rgba, V, N, t=THRESHOLD):
    """the detector's score image (int32, 0 = no corner).  V, N: (h*w, 3) vertex / normal maps of the same view"""
    h, w = rgba.shape[:2]
    Y = luma(rgba)
    A = rgba[..., 3] != 0
    ring = np.stack([shifted(Y, dx, dy) for dx, dy in RING])
    ring_ok = np.all(np.stack([shifted(A, dx, dy, False) for dx, dy in RING]), 0)
    hi, lo = ring > Y + t, ring < Y - t
    seg = np.zeros((h, w), bool)
    for s in range(16):
        idx = [(s + k) % 16 for k in range(9)]
        seg |= hi[idx].all(0) | lo[idx].all(0)
    sc = np.maximum(np.abs(ring - Y) - t, 0).sum(0).astype(np.int32)
    inside = np.zeros((h, w), bool)
    inside[BORDER:h - BORDER, BORDER:w - BORDER] = True
    geo = (np.isfinite(V).all(1) & np.isfinite(N).all(1)).reshape(h, w)
    return np.where(seg & ring_ok & A & inside & geo, sc, 0).astype(np.int32)


def nms(sc):
    """survivors of the 3 x 3 suppression: score > 0 and beating all 8 neighbours, ties to the lower pixel index"""
    keep = sc > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            nb = shifted(sc, dx, dy)
            earlier = dy < 0 or (dy == 0 and dx < 0)     # the neighbour has the lower pixel index: it wins a tie
            keep &= (sc > nb) if earlier else (sc >= nb)
    return keep


def cap(pix, sc, max_keypoints):
    """the strongest max_keypoints by (score descending, pixel ascending), listed in pixel order"""
    if len(pix) <= max_keypoints:
        return pix, sc
    order = np.lexsort((pix, -sc.astype(np.int64)))[:max_keypoints]
    order = np.sort(order)               # pix is ascending already: index order = pixel order
    return pix[order], sc[order]


def describe(S, pix, w):
    """(k, 8) uint32: bit i = S(p + a_i) < S(p + b_i), bit i in word i / 32 at bit i % 32"""
    u, v = pix % w, pix // w
    a = S[v[:, None] + PAIRS[None, :, 1], u[:, None] + PAIRS[None, :, 0]]
    b = S[v[:, None] + PAIRS[None, :, 3], u[:, None] + PAIRS[None, :, 2]]
    bits = (a < b).reshape(len(pix), 8, 32).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def detect(rgba, V, N, threshold=THRESHOLD, max_keypoints=MAX_KEYPOINTS, with_survivors=False):
    """(xy (k, 2) int32, score (k,) int32, desc (k, 8) uint32) of one view; rgba (h, w, 4) uint8"""
    h, w = rgba.shape[:2]
    sc = scores(rgba, V, N, threshold)
    pix_all = np.flatnonzero(nms(sc).reshape(-1)).astype(np.int64)
    pix, s = cap(pix_all, sc.reshape(-1)[pix_all], max_keypoints)
    desc = describe(box_sums(luma(rgba)), pix, w) if len(pix) else np.zeros((0, 8), np.uint32)
    xy = np.stack([pix % w, pix // w], 1).astype(np.int32)
    if with_survivors:
        return xy, s.astype(np.int32), desc, len(pix_all)
    return xy, s.astype(np.int32), desc


def hamming(da, db):
    """(ka, kb) int32 Hamming distances of two descriptor lists (exact: sums of at most 256 ones)"""
    ba = np.unpackbits(da.view(np.uint8).reshape(len(da), 32), axis=1).astype(np.float32)
    bb = np.unpackbits(db.view(np.uint8).reshape(len(db), 32), axis=1).astype(np.float32)
    return np.rint(ba @ (1 - bb).T + (1 - ba) @ bb.T).astype(np.int32)


def best_two(D):
    """per row: (d1, index of the first smallest, d2 = the second smallest, 257 when there is no second); no column: (257, -1, 257)"""
    k, m = D.shape
    if m == 0:
        return np.full(k, 257, np.int32), np.full(k, -1, np.int32), np.full(k, 257, np.int32)
    i1 = np.argmin(D, 1).astype(np.int32)           # the first occurrence: ties go to the lower index
    d1 = D[np.arange(k), i1]
    if m == 1:
        return d1, i1, np.full(k, 257, np.int32)
    E = D.copy()
    E[np.arange(k), i1] = 1 << 20
    return d1, i1, E.min(1).astype(np.int32)


def match(df, dm, max_dist=MAX_DIST, ratio_num=RATIO_NUM, ratio_den=RATIO_DEN, cross_check=False):
    """(frame index, model index, d1, d2) of the accepted matches, in frame-keypoint order"""
    D = hamming(df, dm)
    d1, i1, d2 = best_two(D)
    ok = (d1 <= max_dist) & (d1.astype(np.int64) * ratio_den < d2.astype(np.int64) * ratio_num) & (i1 >= 0)
    if cross_check and len(dm):
        back = best_two(D.T)[1]
        ok &= back[np.maximum(i1, 0)] == np.arange(len(df))
    f = np.flatnonzero(ok).astype(np.int32)
    return f, i1[f], d1[f].astype(np.int32), d2[f].astype(np.int32)


def slots(fxy, mxy, fi, mi, d1, V, N, B, MV, MN, w, mw):
    """the five solver slots and the PROSAC weight of the matches: XW, XC, BV, NW, NC (k, 3) float32, weight (k,) float32"""
    fp = fxy[fi, 1].astype(np.int64) * w + fxy[fi, 0]
    mp = mxy[mi, 1].astype(np.int64) * mw + mxy[mi, 0]
    return MV[mp], V[fp], B[fp], MN[mp], N[fp], (256 - d1).astype(np.float32)
