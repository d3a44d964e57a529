"""Edge cases of the feature stage, shared by the CPU oracle test and the GPU test: cameras whose width, height and pixel count are
no multiple of the kernels' 32 x 8 tile and 256-pixel chunk, pairs whose frame and model have DIFFERENT cameras, a lattice of single
dots whose survivors all tie (the cut, the top of the score range), images with room for one keypoint or none, noise with geometry
holes, and flat models.  The figures next to each case are the ORACLE's (tests/feature_oracle.py);
tests/test_feature_edges_oracle.py recomputes every one of them."""
import numpy as np

import color_oracle as CO
import feature_cases as FC
import feature_oracle as FE
import volume_cases as VC
from frontend_util import FO, pose12

f32 = np.float32
IDENTITY = pose12(np.eye(3), np.zeros(3))
ODD_CAM = (585, 585, 320.5, 239.5, 641, 479)          # the reference camera, one column more and one row less
HALF_ODD = (292.5, 292.5, 160.5, 119.5, 321, 239)
NOISE_CAM = (146, 146, 80.5, 60.5, 163, 121)          # 5 tiles + 3 columns, 15 tiles + 1 row, 77 chunks + 11 pixels


# ---------------------------------------------------------------------------------------------- odd and mixed pairs
# (keypoints frame / model, matches, share of correct matches), defaults throughout
ODD_FIGURES = {
    "narrow": dict(keypoints=(1608, 1613), matches=1174, correct=0.923),
    "wide1": dict(keypoints=(1699, 1613), matches=844, correct=0.807),
}
# the oracle-side M_SK_PROSAC + LS_SHINJI_INLIERS on the oracle's matches of the odd wide1 pair (feature_cases.oracle_relocalise):
# its consensus, its adapted iterations, and its pose error against the truth (rotation rad, camera centre m).  The GPU's
# rpe_relocalize is held to 2 x the error, the margin volume_cases.py / photo_cases.py give GPU loops.
ODD_WIDE1_RELOC = dict(votes=1356, iters=6, error=(2.64e-04, 1.14e-03))


def odd_pair(motion):
    return FC.Pair(ODD_CAM, FC.MOTIONS[motion])


def on_limit_lines(xy, w, h):
    """keypoints on each of the four lines that bound the legal area: u = 16, u = w - 17, v = 16, v = h - 17"""
    b = FE.BORDER
    return ((xy[:, 0] == b).sum(), (xy[:, 0] == w - b - 1).sum(), (xy[:, 1] == b).sum(), (xy[:, 1] == h - b - 1).sum())


class MixedPair:
    """the WIDE1 pair with the frame seen through one camera and the keyframe (model maps, model colour, rpe_model_upload) through
    another: the frame of feature_cases.Pair(fcam), the model of feature_cases.Pair(mcam).  The attributes are Pair's, so
    test_gpu_feature.check_pair takes either."""
    def __init__(self, fcam, mcam, motion=FC.WIDE1, swap_model_width=False):
        f, m = FC.Pair(fcam, motion), FC.Pair(mcam, motion)
        self.cam, self.mcam, self.pa, self.pb = fcam, mcam, m.pa, f.pb
        self.db, self.cb, self.frame = f.db, f.cb, f.frame
        self.da, self.ca, self.model, self.model_rgba = m.da, m.ca, m.model, m.model_rgba
        self.model_width = fcam[4] if swap_model_width else mcam[4]     # swap_model_width: the WRONG gather, for the case condition

    def upload(self, ctx):
        ctx.frame_set_depth(self.db, self.cam, dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])
        ctx.frame_set_color(self.cb)
        ctx.model_upload(self.model.V, self.model.N, self.mcam, self.pa)
        ctx.model_color_upload(self.model_rgba)
        return ctx

    def oracle(self, fopt=(FE.THRESHOLD, FE.MAX_KEYPOINTS), mopt=(FE.MAX_DIST, FE.RATIO_NUM, FE.RATIO_DEN, False)):
        fxy, fs, fd = self.frame.detect(*fopt)
        mxy, ms, md = self.model.detect(*fopt)
        fi, mi, d1, d2 = FE.match(fd, md, *mopt)
        XW, XC, BV, NW, NC, wq = FE.slots(fxy, mxy, fi, mi, d1, self.frame.V, self.frame.N, self.frame.B, self.model.V, self.model.N,
                                          self.cam[4], self.model_width)
        return dict(fxy=fxy, fs=fs, fd=fd, mxy=mxy, ms=ms, md=md, fi=fi, mi=mi, d1=d1, d2=d2, XW=XW, XC=XC, BV=BV, NW=NW, NC=NC, w=wq)

    correct = FC.Pair.correct


# name -> (frame camera, model camera); figures as above.  In each, gathering the model through the frame's width changes every row
# of XW (test_feature_edges_oracle.py::test_mixed_pair_figures_and_the_two_widths).
MIXED = {
    "full_from_odd": (FC.FULL_CAM, ODD_CAM),
    "odd_from_full": (ODD_CAM, FC.FULL_CAM),
    "half_from_half_odd": (FC.HALF_CAM, HALF_ODD),
}
MIXED_FIGURES = {
    "full_from_odd": dict(keypoints=(1742, 1613), matches=872, correct=0.826),
    "odd_from_full": dict(keypoints=(1699, 1603), matches=830, correct=0.836),
    "half_from_half_odd": dict(keypoints=(1311, 1189), matches=590, correct=0.931),
}


def mixed_pair(name, **kw):
    return MixedPair(*MIXED[name], **kw)


# ---------------------------------------------------------------------------------------------- one view on either side
def camera(w, h):
    """a pinhole of the given size with the reference's field of view and a pixel-centred principal point"""
    return (585.0 * w / 640, 585.0 * w / 640, (w - 1) / 2, (h - 1) / 2, w, h)


class Scene:
    """one view for either side of a context: rgb (h, w, 3) uint8 and a depth (default: the plane z = 1, so that every interior pixel
    has a finite vertex and normal).  As the frame it is uploaded as depth + colour; as the model, its camera-frame maps under the
    identity pose with `rgba` (default: rgb with A = 255) as the model colour.  The oracle's maps are frontend_oracle.frame_maps of the
    same depth on both sides."""
    def __init__(self, rgb, cam, depth=None, rgba=None):
        h, w = cam[5], cam[4]
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8
        self.cam, self.rgb = cam, rgb
        self.depth = np.ones((h, w), f32) if depth is None else np.ascontiguousarray(depth, f32)
        self.V, self.N, self.B = FO.frame_maps(self.depth, cam, 1.0, *VC.RANGE)
        self.frame_rgba = CO.frame_rgba(rgb).reshape(h, w, 4)
        self.model_rgba = self.frame_rgba.copy() if rgba is None else rgba

    def view(self, which):
        return FC.View(self.model_rgba if which else self.frame_rgba, self.V, self.N, self.B, self.cam)

    def upload(self, ctx, which):
        if which:
            ctx.model_upload(self.V, self.N, self.cam, IDENTITY)
            ctx.model_color_upload(self.model_rgba)
        else:
            ctx.frame_set_depth(self.depth, self.cam, dmin=VC.RANGE[0], dmax=VC.RANGE[1], max_jump=VC.RANGE[2])
            ctx.frame_set_color(self.rgb)
        return ctx

    def detect(self, which, threshold=FE.THRESHOLD, max_keypoints=FE.MAX_KEYPOINTS, **kw):
        return self.view(which).detect(threshold, max_keypoints, **kw)


# ---------------------------------------------------------------------------------------------- lattices
# white, A = 255, single black pixels every 8 from (16, 16): every dot is a corner (its whole ring is brighter), no white pixel is
# (at most 2 ring pixels of a white pixel are dots), dots are 8 apart so none suppresses another, and ALL SURVIVORS HAVE ONE SCORE:
# 16 * (255 - t), which at t = 1 is 4064, the largest score there is.  More of them than RPE_MAX_KEYPOINTS: the cut falls inside a
# single tie class of thousands, above == 0, and the kept ones are the first `cap` in pixel order.
LATTICE_SIZES = {"640x480": (640, 480), "641x479": (641, 479)}
LATTICE_SURVIVORS = {"640x480": 4256, "641x479": 4312}
LATTICE_SCORE = {12: 3888, 1: 4064}
LATTICE_DISTINCT_DESCRIPTORS = 6             # of the 4096 kept by the default cap (9 uncapped: first / inner / last row x column; the
                                             # default cap drops the last rows)
LATTICE_MATCHES = 2                          # lattice against itself, 4096 x 4096: the descriptors that occur once; the rest tie at 0
LATTICE_CAPS =(1, 1000, 1023, 1024, 1025, 2048, 4096)
# the two-class lattice (640 x 480, luma 60 on the dots with (y // 8 + x // 8) % 3 == 0): score -> survivors at threshold 12
TWO_CLASS = {3888: 2838, 2928: 1418}
TWO_CLASS_CAPS = (4096, 2838, 2839, 1)


def lattice_rgb(w, h, two_class=False):
    img = np.full((h, w, 3), 255, np.uint8)
    ys, xs = np.meshgrid(np.arange(16, h - 16, 8), np.arange(16, w - 16, 8), indexing="ij")
    img[ys, xs] = 0
    if two_class:
        sel = (ys // 8 + xs // 8) % 3 == 0
        img[ys[sel], xs[sel]] = 60
    return img


def lattice(size="640x480", two_class=False):
    w, h = LATTICE_SIZES[size] if isinstance(size, str) else size
    return Scene(lattice_rgb(w, h, two_class), camera(w, h))


def lattice_pixels(w, h):
    """the dots' pixel indices, ascending"""
    ys, xs = np.meshgrid(np.arange(16, h - 16, 8), np.arange(16, w - 16, 8), indexing="ij")
    return (ys * w + xs).reshape(-1)


# the lattice construction at sizes with room for one keypoint or none: (w, h) -> the keypoints
TINY = {(33, 33): [(16, 16)], (40, 33): [(16, 16)], (32, 32): [], (1, 1): []}


# ---------------------------------------------------------------------------------------------- noise with holes
# feature_cases.noise_rgb(NOISE_CAM) over the NARROW pair's depths: the frame's image is seed 12, the model's seed 11.  Survivors of
# the FRAME side (threshold 12, uncapped): with all-finite geometry, with the rendered depth's own maps (NOISE_NAN_NORMALS pixels
# have a NaN normal), and with a further 5 % of the vertices set to NaN (NOISE_HOLE_SEED).
NOISE_SEEDS = (12, 11)                      # frame, model
NOISE_SURVIVORS = dict(finite=1239, rendered=1135, holed=1130)
NOISE_NAN_NORMALS = 2518
NOISE_HOLE_SEED, NOISE_HOLE_SHARE = 3, 0.05
M1_FRAME_CAPS = (1, 15, 16, 17, 300)        # around the 16 keypoints a workgroup of M1 owns
M1_MODEL_CAPS = (1, 255, 256, 257, 1000)    # around the 256 descriptors of an LDS tile; 1000 keeps all NOISE_MODEL_KEYPOINTS
NOISE_MODEL_KEYPOINTS = 766                 # with the alpha = 0 holes: two full tiles and a third of 254
M1_CROSS = ((17, 257), (300, 1000))


def noise_pair(holes=True):
    """the noise pair; `holes`: alpha = 0 holes in the model colour, as feature_cases.Pair(holes=True) makes them"""
    return FC.Pair(NOISE_CAM, FC.NARROW, rgb_a=FC.noise_rgb(NOISE_CAM, NOISE_SEEDS[1]), rgb_b=FC.noise_rgb(NOISE_CAM, NOISE_SEEDS[0]),
                   holes=holes)


def noise_holes():
    """bool (h * w,): the 5 % of pixels whose vertex is taken away"""
    return np.random.default_rng(NOISE_HOLE_SEED).random(NOISE_CAM[4] * NOISE_CAM[5]) < NOISE_HOLE_SHARE


def holed_depth_scenes():
    """(unholed, holed): the noise frame as Scenes over the pair's frame depth, and over that depth with noise_holes() set to 0 -- a
    depth the front end drops, so that ITS maps carry the holes (NaN vertex there, NaN normal there and beside it)"""
    p = noise_pair()
    d = p.db.copy()
    d.reshape(-1)[noise_holes()] = 0
    return Scene(p.cb, NOISE_CAM, p.db), Scene(p.cb, NOISE_CAM, d)


# ---------------------------------------------------------------------------------------------- flat models
def grey(cam, value=128):
    return np.full((cam[5], cam[4], 3), value, np.uint8)


def flat_model_pair(cam=NOISE_CAM):
    """the keyframe's colour is one grey, the frame is textured: no model keypoint, no match"""
    return FC.Pair(cam, FC.NARROW, rgb_a=grey(cam))


def both_flat_pair(cam=NOISE_CAM):
    return FC.Pair(cam, FC.NARROW, rgb_a=grey(cam), rgb_b=grey(cam))
