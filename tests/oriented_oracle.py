"""The numpy statement of the ORIENTED descriptor (include/rgbd_pose_hip.h Part 3, "Oriented descriptor"): the patch's intensity
moments over a disc, the angle bin they fall in, the test pairs steered by that bin, and the tests with their out-of-image rule.
Luma, box sums, the detector and the matching are feature_oracle's: only the descriptor differs.  Everything is integer arithmetic or
a comparison, so the GPU is held to it bit for bit."""
import numpy as np

import feature_oracle as FE

BINS = 32
RADIUS2 = 169
# round(1024 cos(2 pi k / 32)), typed in as the header states them; the sine is the cosine a quarter turn back
COS = np.array([1024, 1004, 946, 851, 724, 569, 392, 200, 0, -200, -392, -569, -724, -851, -946, -1004,
                -1024, -1004, -946, -851, -724, -569, -392, -200, 0, 200, 392, 569, 724, 851, 946, 1004], np.int64)
SIN = COS[(np.arange(BINS) + 24) % BINS]
DISC = np.array([(dx, dy) for dy in range(-13, 14) for dx in range(-13, 14) if dx * dx + dy * dy <= RADIUS2], np.int64)


def moments(Y, pix, w):
    """(m10, m01) int64 per keypoint: sums of dx Y and dy Y over the disc (a keypoint is 16 px inside: the disc is in the image)"""
    u, v = pix % w, pix // w
    P = Y[v[:, None] + DISC[None, :, 1], u[:, None] + DISC[None, :, 0]].astype(np.int64)
    return (P * DISC[:, 0]).sum(1), (P * DISC[:, 1]).sum(1)


def angle_bin(m10, m01):
    """the k that maximises m10 C[k] + m01 S[k]; a tie goes to the lowest k"""
    m10, m01 = np.asarray(m10, np.int64), np.asarray(m01, np.int64)
    return np.argmax(m10[..., None] * COS + m01[..., None] * SIN, axis=-1).astype(np.int32)


def steer(bins):
    """(k, 256, 4) int64: the pairs of feature_oracle.PAIRS turned by each keypoint's bin, (ax', ay', bx', by')"""
    c, s = COS[bins][:, None], SIN[bins][:, None]
    out = np.empty((len(bins), len(FE.PAIRS), 4), np.int64)
    for o in (0, 2):
        x, y = FE.PAIRS[None, :, o], FE.PAIRS[None, :, o + 1]
        out[..., o] = (x * c - y * s + 512) >> 10              # arithmetic shift: floor
        out[..., o + 1] = (x * s + y * c + 512) >> 10
    return out


def sample(S, x, y):
    """S at (x, y), 0 outside the image"""
    h, w = S.shape
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(ok, S[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)


def describe(S, pix, w, bins):
    """(k, 8) uint32: bit i = S(p + a'_i) < S(p + b'_i), packed as feature_oracle.describe packs"""
    u, v = (pix % w)[:, None], (pix // w)[:, None]
    P = steer(bins)
    a = sample(S, u + P[..., 0], v + P[..., 1])
    b = sample(S, u + P[..., 2], v + P[..., 3])
    bits = (a < b).reshape(len(pix), 8, 32).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def detect(rgba, V, N, threshold=FE.THRESHOLD, max_keypoints=FE.MAX_KEYPOINTS):
    """(xy (k, 2) int32, score (k,) int32, desc (k, 8) uint32, bins (k,) int32) of one view: feature_oracle's keypoints, described
    in their own orientation"""
    h, w = rgba.shape[:2]
    xy, s, _ = FE.detect(rgba, V, N, threshold, max_keypoints)
    pix = xy[:, 1].astype(np.int64) * w + xy[:, 0]
    if not len(pix):
        return xy, s, np.zeros((0, 8), np.uint32), np.zeros(0, np.int32)
    Y = FE.luma(rgba)
    bins = angle_bin(*moments(Y, pix, w))
    return xy, s, describe(FE.box_sums(Y), pix, w, bins), bins
