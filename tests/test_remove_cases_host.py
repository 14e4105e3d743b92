"""The property the layout check of tests/test_gpu_remove.py rests on, held without a GPU: a removal sorts nothing, and need
not.  If the survivors' finite bounding box is the scene's, morton_order quantises every survivor as before, so the Morton
order of the survivors alone (what a fresh upload of them computes) is the scene's order without the slots that went, in the
new numbering (remove_cases.compacted_order) -- ties included: equal codes keep index order, and the renumbering is monotone.
The Morton arithmetic is morton_order's of splat_amd/csrc/splat_scene.hip, restated in numpy float32 (remove_cases.py)."""
import numpy as np
import pytest

import remove_cases as RC

f32 = np.float32


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * np.array([1.0, 0.3, 2.5])).astype(f32)


def lattice(n, seed):
    """27 sites: ~n / 27 Gaussians of equal code at each"""
    site = np.random.default_rng(seed).integers(0, 27, n)
    return np.stack([site % 3 - 1, site // 3 % 3 - 1, site // 9 - 1], 1).astype(f32) * f32(0.5)


def spoiled(n, seed):
    """NaN and inf coordinates, some of them in Gaussians whose other coordinates count for the box"""
    p = cloud(n, seed)
    rng = np.random.default_rng(seed + 1)
    for v in (np.nan, np.inf, -np.inf):
        idx = rng.choice(n, max(1, n // 20), replace=False)
        p[idx, rng.integers(0, 3, len(idx))] = f32(v)
    return p


SCENES = {"cloud": cloud, "lattice": lattice, "spoiled": spoiled}


def masks(pos, seed):
    """selections to DELETE that spare the Gaussians holding the finite per-axis extremes"""
    n = len(pos)
    rng = np.random.default_rng(seed)
    spare = RC.extremes(pos)
    out = []
    for frac in (0.01, 0.5, 0.99):
        sel = rng.random(n) < frac
        out.append(sel)
    out.append(np.arange(n) % 2 == 0)
    block = np.zeros(n, bool)
    block[RC.morton_order(pos)[n // 3: n // 3 + 256]] = True          # a run of consecutive slots
    out.append(block)
    for sel in out:
        sel[spare] = False
    return out


def test_the_restated_order_is_a_permutation_that_sorts_the_codes():
    for name, make in SCENES.items():
        pos = make(3000, 11)
        order = RC.morton_order(pos)
        assert np.array_equal(np.sort(order), np.arange(3000)), name
        codes = RC.morton_codes(pos)[order]
        assert (np.diff(codes.astype(np.int64)) >= 0).all(), name
        ties = np.diff(codes.astype(np.int64)) == 0
        assert (np.diff(order.astype(np.int64))[ties] > 0).all(), name + ": ties keep index order"
    assert len(np.unique(RC.morton_codes(lattice(3000, 11)))) <= 27
    # a coordinate that is not finite quantises to 0 and takes no part in the box
    pos = spoiled(3000, 11)
    lo, hi = RC.finite_box(pos)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and not np.isfinite(pos).all()


@pytest.mark.parametrize("keep", [False, True], ids=["delete", "crop"])
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("n", (1, 2, 257, 3000))
def test_survivors_with_the_scenes_box_keep_the_scenes_order(n, name, keep):
    pos = SCENES[name](n, 100 + n)
    orig = RC.morton_order(pos)
    for k, gone in enumerate(masks(pos, 200 + n)):
        sel = ~gone if keep else gone                                 # the same survivors either way
        stay = RC.survives(sel, keep)
        assert np.array_equal(stay, ~gone)
        index_map = RC.index_map_of(sel, keep)
        survivors = pos[stay]
        for a, b in zip(RC.finite_box(survivors), RC.finite_box(pos)):
            assert a.tobytes() == b.tobytes(), "the masks are meant to spare the extremes"
        want = RC.morton_order(survivors)
        got = RC.compacted_order(orig, index_map)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (name, n, k)
        # ... and the map is what it says: the rank among the survivors, monotone, GONE elsewhere
        assert np.array_equal(index_map[stay], np.arange(stay.sum(), dtype=np.uint32))
        assert (index_map[~stay] == RC.GONE).all()


def test_a_box_that_shrinks_may_change_the_order():
    """why the layout check against a fresh upload spares the extremes: without them the quantisation is another"""
    pos = cloud(3000, 7)
    gone = np.zeros(3000, bool)
    gone[RC.extremes(pos)] = True
    index_map = RC.index_map_of(gone, False)
    got = RC.compacted_order(RC.morton_order(pos), index_map)
    want = RC.morton_order(pos[~gone])
    assert np.array_equal(np.sort(got), np.sort(want))                # the same Gaussians ...
    assert not np.array_equal(got, want)                              # ... in another order


def test_removed_gathers_every_field_in_index_order():
    import splat_amd
    g = splat_amd.synthetic_scene(100, 3)
    sel = np.arange(100) % 3 == 0
    for keep in (False, True):
        s, m = RC.removed(g, sel, keep)
        rows = np.flatnonzero(sel if keep else ~sel)
        assert len(s) == len(rows)
        for f in RC.FIELDS:
            assert np.array_equal(getattr(s, f), getattr(g, f)[rows]), f
        assert np.array_equal(np.flatnonzero(m != RC.GONE), rows)
