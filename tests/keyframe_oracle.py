"""The numpy statement of the keyframe store (include/rgbd_pose_hip.h Part 3, "Keyframes") on top of tests/feature_oracle.py: what a
keyframe keeps, the query of a frame against every keyframe, one keyframe's matches in the solver slots, and the walk over the
best-ranked candidates.  Hamming distances, comparisons and sorts only: the GPU is held to it bit for bit."""
import numpy as np

import feature_oracle as FE

MAX_KEYFRAMES = 256
MOPT = (FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, False)


def keyframe(rgba, MV, MN, threshold=FE.THRESHOLD, max_keypoints=FE.MAX_KEYPOINTS):
    """a model view's keyframe: its detection and the world vertex / normal at every keypoint.  rgba (h, w, 4); MV, MN (h*w, 3)"""
    w = rgba.shape[1]
    xy, _, desc = FE.detect(rgba, MV, MN, threshold, max_keypoints)
    pix = xy[:, 1].astype(np.int64) * w + xy[:, 0]
    return dict(xy=xy, desc=desc, xw=MV[pix].astype(np.float32), nw=MN[pix].astype(np.float32))


def query(fd, keyframes, mopt=MOPT):
    """(counts, order): per keyframe the matches of the frame's descriptors fd against its keypoints alone; ids by (count descending,
    id ascending)"""
    counts = [len(FE.match(fd, k["desc"], *mopt)[0]) for k in keyframes]
    order = sorted(range(len(keyframes)), key=lambda i: (-counts[i], i))
    return np.array(counts, np.int32), np.array(order, np.int32)


def match(fxy, fd, V, N, B, w, kf, mopt=MOPT):
    """the match list of the frame (keypoints fxy / fd, maps V N B of width w) against the keyframe kf, and the five slots: XW / NW
    from the keyframe, XC / NC / BV from the frame's maps; model index = the keypoint's position inside the keyframe"""
    fi, mi, d1, d2 = FE.match(fd, kf["desc"], *mopt)
    fp = fxy[fi, 1].astype(np.int64) * w + fxy[fi, 0]
    return dict(fi=fi, mi=mi, d1=d1, d2=d2, XW=kf["xw"][mi], NW=kf["nw"][mi], XC=V[fp], NC=N[fp], BV=B[fp], w=(256 - d1).astype(np.float32))


def walk(counts, order, candidates, min_matches, run):
    """the candidate walk: the first `candidates` keyframes of the ranking, as long as they have min_matches matches, each through
    run(id) -> (votes, result) or None when the solver refuses it; the most votes win, a tie stays with the better rank.
    Returns (id, result), or (order[0], None) when there is no winner"""
    best = None
    for r in range(min(candidates, len(order))):
        i = int(order[r])
        if counts[i] < min_matches:
            break
        got = run(i)
        if got is not None and (best is None or got[0] > best[1][0]):
            best = (i, got)
    return (int(order[0]), None) if best is None else (best[0], best[1][1])
