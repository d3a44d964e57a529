"""CPU: the numpy statement of the fuse's cull (tests/cull_oracle.py) over the case set of tests/cull_cases.py, against the voxels that
tests/volume_oracle.py integrate updates when every depth is valid.  What this file proves: the statement never culls a brick an entry
updates, it still culls most of the rest, and the case set is one on which three wrong forms of the rule DO cull needed bricks -- so
tests/test_gpu_volume_rules.py, which holds the device's decision to the statement's on the same cases with no exception allowed and
forbids a culled brick with an updated voxel, would fail for a library that had any of them.

What it does not prove: the rule's margins.  The rule without kCullEps, without the whole pixel or without the + 0.5 (each taken away
alone) culls no needed brick of this case set either; the margins are the slack
the rounding argument of csrc/rpe_volume_field.hpp asks for, not something a finite test tells apart, and no test here claims to.

Measured on the set (9000 random scenes and the fixed families, 76 990 cases; bricks of 8 x 8 x 8 are decided in both kernels' forms):
  rebuild form: 12 187 needed, 0 culled; 17 741 kept; 0.914 of the unneeded culled; 350 cases with exactly one updating voxel
  map form    :  6 444 needed of 37 323, 0 culled; 9 017 kept; 0.917 of the unneeded culled; 181 one-voxel cases
  needed bricks culled by no_fabs 4 757 / 2 603, by centre_behind 233 / 72, by zh_for_zl 282 / 140.  zh_for_zl is caught by the random
  scenes (260 / 133) and by the close-up entries of the "edges" family (22 / 7); the other fixed families, like the rendered scenes of
  the fuse's own tests, let it pass."""
import numpy as np
import pytest

import cull_cases as CC
import cull_oracle as CU


def forms():
    """(name, T, count) per kernel: every case in the rebuild kernel's form, the 8 x 8 x 8 cases also in the map fuse's"""
    _, T, _, n = CC.case_set()
    m = (T["n"] == 8).all(1)
    return (("rebuild", T, n), ("map", T[m], n[m]))


@pytest.mark.parametrize("form", (0, 1), ids=("rebuild", "map"))
def test_the_statement_culls_no_needed_brick_and_most_of_the_rest(form):
    name, T, n = forms()[form]
    keep, need = CU.decide(T, name), n > 0
    share = (~keep & ~need).sum() / (~need).sum()
    print(name, "cases", len(T), "needed", need.sum(), "kept", keep.sum(), "share of the unneeded culled", share, "one voxel", (n == 1).sum())
    assert need.sum() > 5000 and not (need & ~keep).any()
    assert share > 0.5                                             # measured: 0.914 (rebuild), 0.917 (map)
    assert (n == 1).sum() >= 100                                   # measured: 350 (rebuild), 181 (map)


@pytest.mark.parametrize("variant", CU.VARIANTS)
@pytest.mark.parametrize("form", (0, 1), ids=("rebuild", "map"))
def test_each_wrong_variant_culls_needed_bricks_of_the_set(form, variant):
    name, T, n = forms()[form]
    lost = ((n > 0) & ~CU.decide(T, name, variant)).sum()
    print(name, variant, "needed bricks culled:", lost)
    assert lost >= 10                                              # measured: see the docstring
    assert (CU.decide(T, name, variant) != CU.decide(T, name)).sum() >= lost   # ... so its decisions differ from the statement's there


def test_non_finite_poses_keep_every_entry():
    scenes = [s for s in CC.families() if s["name"].startswith("nonfinite")]
    T, _ = CC.table(scenes)
    bad = ~(np.isfinite(T["R"]).all(1) & np.isfinite(T["t"]).all(1))
    assert len(scenes) == 2 and bad.all()
    for form, sel in (("rebuild", np.ones(len(T), bool)), ("map", (T["n"] == 8).all(1))):
        keep = CU.decide(T[sel], form)
        # A NaN reaches both ends of its row's interval; an Inf makes the row's margin m infinite, so the ends are Inf - Inf or infinite
        # on the side no comparison can put outside.  Either way the comparisons that row enters never cull.  The camera's z row enters
        # all of them: such an entry is kept for every brick, even t_z = -Inf, which no voxel can pass.  A bad x or y row leaves the other
        # image axis and "behind" to decide on finite numbers, exactly as they do for the finite pose.
        zrow = ~(np.isfinite(T["R"][sel][:, 6:]).all(1) & np.isfinite(T["t"][sel][:, 2]))
        assert zrow.any() and (~zrow).any() and keep[zrow].all()
        base = T[sel].copy()
        base["R"], base["t"] = CC.NONFINITE_BASE[:9], CC.NONFINITE_BASE[9:]
        assert (keep >= CU.decide(base, form)).all() and not keep.all()


def test_needed_is_volume_oracle_integrate():
    """needed / brick_counts on a ragged volume: the per-brick sums of integrate's own mask, x fastest"""
    sc = [s for s in CC.families() if s["name"] == "roll/rebuild"][0]
    G, (cam, pose) = CC.geometry(sc), sc["entries"][1]
    mask = CU.updated(G, cam, pose)
    n = CU.brick_counts(mask, sc["brick"])
    nb = CC.bricks_per_axis(sc)
    assert mask.shape == G.dim[::-1] and n.sum() == mask.sum() > 0 and len(n) == np.prod(nb) and nb == [3, 3, 3]
    b = 1 + nb[0] * (2 + nb[1] * 1)                               # brick (1, 2, 1): the ragged end in y
    assert n[b] == mask[4:8, 16:19, 32:64].sum()
    assert np.array_equal(CU.needed(G, sc["brick"], cam, pose), n > 0)
