"""The numpy statement of the SCALE LEVELS (include/rgbd_pose_hip.h Part 3, "Scale levels"): the ladder of resampled luma images with
their known masks, the level-0 pixel a level pixel stands at, and the detection over all levels -- feature_oracle's detector per level,
one list in (level, level pixel) order under one cap, feature_oracle's or oriented_oracle's descriptor on the keypoint's own level.
Matching, slots, keyframes and the graph are untouched: a keypoint reports its level-0 pixel.  Everything is integer arithmetic or a
comparison, so the GPU is held to it bit for bit."""
import numpy as np

import feature_oracle as FE
import oriented_oracle as OO

P = (1, 2, 1, 1)
Q = (1, 3, 2, 3)
MAX_LEVELS = 4
UPRIGHT, ORIENTED = 0, 1


def level_size(w, h, l):
    return w * P[l] // Q[l], h * P[l] // Q[l]


def centre(u, l):
    """the level-0 pixel that level pixel u of level l stands at (either axis)"""
    return ((2 * np.asarray(u, np.int64) + 1) * Q[l] - P[l]) // (2 * P[l])


def level_images(rgba, levels):
    """[(Y_l int32 (h_l, w_l), K_l bool (h_l, w_l))]: the image repeated P times per axis and averaged over Q x Q blocks, rounded;
    known where every source pixel of the block is"""
    h, w = rgba.shape[:2]
    Y0, A = FE.luma(rgba), rgba[..., 3] != 0
    out = []
    for l in range(levels):
        p, q = P[l], Q[l]
        wl, hl = level_size(w, h, l)
        sx = (q * np.arange(wl)[:, None] + np.arange(q)) // p             # (wl, q) source columns: all < w, since q wl <= p w
        sy = (q * np.arange(hl)[:, None] + np.arange(q)) // p
        assert (wl == 0 or sx.max() < w) and (hl == 0 or sy.max() < h)
        Y, K = np.zeros((hl, wl), np.int32), np.ones((hl, wl), bool)
        for j in range(q):
            for i in range(q):
                Y += Y0[sy[:, j][:, None], sx[:, i][None, :]]
                K &= A[sy[:, j][:, None], sx[:, i][None, :]]
        out.append(((Y + q * q // 2) // (q * q), K))
    return out


def level_scores(Y, K, V, N, w, l, t):
    """feature_oracle.scores on (Y_l, K_l), the geometry that of the level-0 pixels the level pixels stand at.  (A grey RGBA image
    with A = K carries the pair: its luma is Y wherever K holds, and where K fails nothing but the mask enters the score.)"""
    hl, wl = Y.shape
    grey = np.stack([Y, Y, Y, np.where(K, 255, 0)], -1).astype(np.uint8)
    at = (centre(np.arange(hl), l)[:, None] * w + centre(np.arange(wl), l)[None, :]).reshape(-1)
    return FE.scores(grey, V[at], N[at], t)


def detect(rgba, V, N, threshold=FE.THRESHOLD, max_keypoints=FE.MAX_KEYPOINTS, levels=1, kind=UPRIGHT, with_survivors=False):
    """(xy (k, 2) int32 -- the level-0 pixel, score (k,) int32, desc (k, 8) uint32, level (k,) int32, lxy (k, 2) int32 -- the level
    pixel, bins (k,) int32 -- zeros for the upright kind) of one view; rgba (h, w, 4) uint8, V / N (h * w, 3)"""
    h, w = rgba.shape[:2]
    images = level_images(rgba, levels)
    idx, sc, lev, base = [], [], [], 0
    for l, (Y, K) in enumerate(images):
        hl, wl = Y.shape
        if wl > 2 * FE.BORDER and hl > 2 * FE.BORDER:                      # a smaller level has no pixel 16 inside it
            s = level_scores(Y, K, V, N, w, l, threshold)
            pix = np.flatnonzero(FE.nms(s).reshape(-1)).astype(np.int64)
            idx.append(base + pix); sc.append(s.reshape(-1)[pix]); lev.append(np.full(len(pix), l, np.int32))
        base += wl * hl
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    sc = np.concatenate(sc) if sc else np.zeros(0, np.int32)
    lev = np.concatenate(lev) if lev else np.zeros(0, np.int32)
    survivors = [int((lev == l).sum()) for l in range(levels)]
    kept, s = FE.cap(idx, sc, max_keypoints)                               # (score descending, then the list's order), listed in order
    lev = lev[np.searchsorted(idx, kept)]
    k = len(kept)
    xy, lxy = np.zeros((k, 2), np.int32), np.zeros((k, 2), np.int32)
    desc, bins, base = np.zeros((k, 8), np.uint32), np.zeros(k, np.int32), 0
    for l, (Y, K) in enumerate(images):
        hl, wl = Y.shape
        m = lev == l
        if m.any():
            pix = kept[m] - base
            lxy[m] = np.stack([pix % wl, pix // wl], 1)
            xy[m] = np.stack([centre(pix % wl, l), centre(pix // wl, l)], 1)
            S = FE.box_sums(Y)
            if kind == ORIENTED:
                bins[m] = OO.angle_bin(*OO.moments(Y, pix, wl))
                desc[m] = OO.describe(S, pix, wl, bins[m])
            else:
                desc[m] = FE.describe(S, pix, wl)
        base += wl * hl
    out = (xy, s.astype(np.int32), desc, lev.astype(np.int32), lxy, bins)
    return out + (survivors,) if with_survivors else out
