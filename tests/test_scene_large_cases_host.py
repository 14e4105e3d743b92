"""The cases of tests/scene_large_cases.py are what they claim, and they would catch the defects they are for -- shown on the
CPU, without a GPU and without a mutated kernel: each case lies on the side of its threshold that its name says, a scene box
that misses the rows of a later trip gives another order, and numpy models of the sort's pass and of the mask compaction, as
the kernels do them, reproduce the references with the scan's carry and miss them without it."""
import numpy as np
import pytest

import remove_cases as RC
import scene_large_cases as L

f32 = np.float32


# ---- every case on its side of its threshold --------------------------------------------------------------------------------------
def test_the_thresholds_are_the_constants():
    assert L.BOX == 256 * L.BOX_GROUPS_MAX and L.SORT == 256 * 256 * L.SORT_ITEMS and L.MASK == L.SELECT_SPAN * L.SELECT_SCAN_ROUND
    assert (L.box_trips(L.BOX), L.box_trips(L.BOX + 1)) == (1, 2)
    assert (L.sort_scan_rounds(L.SORT), L.sort_scan_rounds(L.SORT + 1)) == (1, 2)
    assert (L.mask_scan_rounds(0, L.MASK), L.mask_scan_rounds(0, L.MASK + 1), L.mask_scan_rounds(15, L.MASK - 15), L.mask_scan_rounds(15, L.MASK - 14)) == (1, 2, 1, 2)


# name: (n, box trips, sort workgroups, rounds of the sort's scan), stated in the constants
REGIMES = {"box": (L.BOX, 1, L.BOX // L.SORT_TILE, 1),
           "box+1": (L.BOX + 1, 2, L.BOX // L.SORT_TILE + 1, 1),
           "box-strides": (3 * L.BOX + 77, 4, 3 * L.BOX // L.SORT_TILE + 1, 1),
           "sort": (L.SORT, L.SORT // L.BOX, 256, 1),
           "sort+1": (L.SORT + 1, L.SORT // L.BOX + 1, 257, 2),
           "sort+tile lattice": (L.SORT + L.SORT_TILE + 1, L.SORT // L.BOX + 1, 258, 2),
           "one code": (L.SORT + 1, L.SORT // L.BOX + 1, 257, 2)}


@pytest.mark.parametrize("name", L.ORDER_NAMES)
def test_order_cases_lie_where_their_names_say(name):
    n, trips, groups, rounds = REGIMES[name]
    p = L.positions(name)
    assert len(p) == n == L.ORDER_CASES[name][0]
    assert (L.box_trips(n), L.sort_groups(n), L.sort_scan_rounds(n)) == (trips, groups, rounds)
    assert (p[:, 3] == 1).all()
    if name == "sort+1":
        assert n - (groups - 1) * L.SORT_TILE == 1, "the last tile holds one key"
    if name == "sort+tile lattice":
        assert len(np.unique(RC.morton_codes(p))) == 64
        assert len(np.unique(RC.morton_codes(p)[-(L.SORT_TILE + 1):])) == 64, "the tiles behind the carry hold every code"
    if name == "one code":
        assert np.array_equal(L.order(name), np.arange(n, dtype=np.uint32)), "the order is the identity"
    if name in ("box", "sort", "sort+1"):
        assert np.isfinite(p).all() and len(np.unique(RC.morton_codes(p))) > n // 64


def test_set_of_order_cases():
    assert set(REGIMES) == set(L.ORDER_NAMES) and set(L.TWINS) <= set(L.ORDER_NAMES)


def test_box_plus_one_holds_its_extremes_in_the_second_trip():
    p = L.positions("box+1")
    lo, hi = RC.finite_box(p)
    assert (p[L.BOX, :3] == hi).all() and (p[:L.BOX, :3].max(0) < hi).all()
    assert (p[:L.BOX, :3].min(0) == lo).all()


def test_box_strides_spreads_its_extremes_and_its_non_finite_rows_over_the_trips():
    p = L.positions("box-strides")
    lo, hi = RC.finite_box(p)
    trips = set()
    for axis, end, row, v in L.BOX_STRIDES_EXTREMES:
        assert p[row, axis] == f32(v) == (lo if end == "lo" else hi)[axis] and np.isfinite(p[row, :3]).all()
        col = p[:, axis]
        assert (np.flatnonzero(col == f32(v)) == [row]).all(), "one row holds the extreme"
        trips.add(row // L.BOX)
    assert trips == {0, 1, 2, 3} and L.BOX_STRIDES_EXTREMES[-1][:3] == (0, "hi", len(p) - 1)
    for trip in (1, 2, 3):
        rows = p[trip * L.BOX:(trip + 1) * L.BOX, :3]
        assert np.isnan(rows).any() and (rows == np.inf).any() and (rows == -np.inf).any(), trip
        zero = rows[:, 0] == 0
        assert (zero & np.signbit(rows[:, 0])).any() and (zero & ~np.signbit(rows[:, 0])).any(), trip
    assert np.isfinite(p[:L.BOX]).all()


# ---- a box that misses a trip gives another order -------------------------------------------------------------------------------------
def test_the_order_with_the_true_box_is_the_reference():
    for name in ("box+1", "box-strides"):
        p = L.positions(name)
        assert np.array_equal(L.order_with_box(p, *RC.finite_box(p)), L.order(name)), name


def test_box_plus_one_with_a_box_of_the_first_trip_alone():
    p = L.positions("box+1")
    got = L.order_with_box(p, *RC.finite_box(p[:L.BOX]))
    differ = int((got != L.order("box+1")).sum())
    print("box+1: a box without row BOX gives another Gaussian to %d of %d slots" % (differ, len(p)))
    assert differ > len(p) // 2


@pytest.mark.parametrize("missed", [1, 2, 3])
def test_box_strides_with_a_box_that_misses_a_trip(missed):
    """... the first BOX rows alone (missed = 1: trips 1 to 3 are not seen), and the box without trip 2, without trip 3"""
    p = L.positions("box-strides")
    seen = p[:L.BOX] if missed == 1 else np.concatenate([p[:missed * L.BOX], p[(missed + 1) * L.BOX:]])
    got = L.order_with_box(p, *RC.finite_box(seen))
    differ = int((got != L.order("box-strides")).sum())
    print("box-strides: a box that misses trip %d%s differs in %d of %d slots" % (missed, " and later" if missed == 1 else "", differ, len(p)))
    assert differ > len(p) // 2


def test_box_strides_with_a_box_that_lets_the_non_finite_rows_of_a_later_trip_in():
    """the box a stride loop would make that tests for finite values on its first trip only: +inf as a maximum, -inf as a minimum"""
    p = L.positions("box-strides")
    later = p[L.BOX:, :3]
    with np.errstate(all="ignore"):
        lo = np.fmin(RC.finite_box(p)[0], np.nanmin(later, 0))
        hi = np.fmax(RC.finite_box(p)[1], np.nanmax(later, 0))
    assert np.isinf(lo).all() and np.isinf(hi).all()
    assert not np.array_equal(L.order_with_box(p, lo, hi), L.order("box-strides"))


# ---- the sort's pass, with its carry and without -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sort", "box", "sort+1", "sort+tile lattice", "one code"])
def test_lsd_model_is_the_reference_with_the_carry_and_not_without(name):
    p = L.positions(name)
    assert np.array_equal(L.lsd_order(p), L.order(name)), "four passes of the model are morton_order"
    dropped = L.lsd_order(p, drop_carry=True)
    if L.sort_scan_rounds(len(p)) == 1:
        assert np.array_equal(dropped, L.order(name)), "a control: there is no second round to lose a carry in"
    else:
        differ = int((dropped != L.order(name)).sum())
        print("%s: without the carry %d of %d slots hold another Gaussian" % (name, differ, len(p)))
        assert differ > 0
        with pytest.raises(AssertionError):
            np.testing.assert_array_equal(dropped, L.order(name))


# ---- the mask scan, with its carry and without -----------------------------------------------------------------------------------------
# spans and rounds per mask case, stated in the constants
MASK_REGIMES = {(0, L.MASK): (256, 1), (0, L.MASK + 1): (257, 2), (15, L.MASK - 14): (257, 2), (1, 2 * L.MASK + L.SELECT_SPAN + 1): (514, 3)}
# the (mask case, pattern) pairs WITHOUT a selected byte behind round 0, where no defect of a later round can show: the
# control's, and the seeded 30 % of (0, MASK + 1), whose second round holds one byte -- a byte the seed does not select
NOTHING_BEHIND_ROUND_0 = {((0, L.MASK), pattern) for pattern in L.PATTERNS} | {((0, L.MASK + 1), "30 %")}


def test_mask_cases_lie_where_they_say():
    assert set(MASK_REGIMES) == set(L.MASK_CASES) and L.MASK_CASES[0] == (0, L.MASK)
    for head, n in L.MASK_CASES:
        assert (L.selection_groups(head, n), L.mask_scan_rounds(head, n)) == MASK_REGIMES[(head, n)]
    assert L.MASK_CASES[2][1] < L.MASK, "fewer than MASK bytes: the address decides"


@pytest.mark.parametrize("pattern", L.PATTERNS)
@pytest.mark.parametrize("head,n", L.MASK_CASES)
def test_scan_model_is_flatnonzero_with_the_carry_and_not_without(head, n, pattern):
    mask = L.mask_bytes(head, n, pattern)
    want = np.flatnonzero(mask).astype(np.uint32)
    assert len(mask) == n and want.size > 0 and set(np.unique(mask)) <= {0, 1, 2, 0x80, 0xFF}
    if pattern == "the last byte":
        assert want.tolist() == [n - 1]
    if pattern == "the last span":
        first = (L.selection_groups(head, n) - 1) * L.SELECT_SPAN - head
        assert want[0] == first and want.size == n - first and not mask[:first].any()
    if pattern == "30 %":
        assert 0.29 < want.size / n < 0.31
    count, got = L.scan_indices(mask, head)
    assert count == want.size and np.array_equal(got, want)
    before, behind = L.selected_in_rounds(mask, head)
    assert behind == (((head, n), pattern) not in NOTHING_BEHIND_ROUND_0)
    assert before == (pattern in ("all ones", "30 %") or (head, n) == L.MASK_CASES[0])
    # a carry lost between the rounds shows where a byte is selected behind round 0 and the carry into its round is not 0:
    # all ones and the 30 %.  The last byte and the last span alone have nothing to carry; they are for a scan that ends
    # after its first round, which shows wherever a byte is selected behind round 0
    count, got = L.scan_indices(mask, head, defect="carry")
    assert count == want.size, "(the model keeps the total: the defect is in the offsets)"
    assert (not np.array_equal(got, want)) == (behind and before)
    count, got = L.scan_indices(mask, head, defect="one round")
    assert (count != want.size or not np.array_equal(got, want)) == behind
    if behind:
        assert not np.array_equal(got, want)


# ---- the removal's scene and selections ------------------------------------------------------------------------------------------------
def test_the_removals_selections_leave_the_box_alone_in_both_modes():
    p = L.remove_positions()
    n = L.REMOVE_N
    assert len(p) == n == L.MASK + 1 and (n + 255) // 256 > 16 * L.SELECT_SCAN_ROUND, "the block scan takes 17 rounds"
    box = RC.finite_box(p)
    for (axis, end, v), (a, b) in zip(L.REMOVE_PAIRS, L.remove_pair_rows()):
        assert p[a, axis] == p[b, axis] == f32(v) == box[0 if end == "lo" else 1][axis] and n - 1 not in (a, b)
    for which in L.REMOVE_SELECTIONS:
        sel = L.remove_selection(which)
        for keep in (False, True):
            stay = RC.survives(sel, keep)
            if stay.sum() > 1:
                for got, want in zip(RC.finite_box(p[stay]), box):
                    assert got.tobytes() == want.tobytes(), (which, keep)
            # ... so the compacted order is the order a fresh upload of the survivors computes
            if which == "30 %":
                assert np.array_equal(RC.compacted_order(RC.morton_order(p), RC.index_map_of(sel, keep)), RC.morton_order(p[stay]))
    sel = L.remove_selection("30 %")
    assert 0.29 < sel.mean() < 0.31 and sel[n - 1]


# ---- block_bounds without the loop ---------------------------------------------------------------------------------------------------
def block_bounds_loop(pos4, cov3d, orig):
    """block_bounds_np of tests/test_gpu_scene_update.py (a GPU module, not imported here), Gaussian by Gaussian"""
    n = len(orig)
    out = np.zeros(((n + 255) // 256, 8), f32)
    inf = f32(np.inf)
    for b in range(out.shape[0]):
        lo, hi, fmax = [inf] * 3, [-inf] * 3, f32(0.0)
        for i in orig[256 * b: min(n, 256 * (b + 1))]:
            p = pos4[i, :3]
            if not np.isfinite(p).all():
                continue
            for a in range(3):
                if p[a] < lo[a]:
                    lo[a] = p[a]
                if hi[a] < p[a]:
                    hi[a] = p[a]
            with np.errstate(all="ignore"):
                f2 = np.float64(0.0)
                for e in range(9):
                    f2 = f2 + np.float64(cov3d[i, e]) * np.float64(cov3d[i, e])
                f = f32(f32(np.sqrt(f2)) * f32(1.0001))
            if not (f >= 0):
                f = inf
            if fmax < f:
                fmax = f
        if not (lo[0] <= hi[0]):
            lo, hi = [f32(np.nan)] * 3, [f32(np.nan)] * 3
        out[b] = np.array(lo + hi + [fmax, f32(0.0)], f32)
    return out


def test_block_bounds_is_the_loop_bit_for_bit():
    n = 1500
    rng = np.random.default_rng(7)
    pos = L.random_positions(n, 8).copy()
    cov = (rng.standard_normal((n, 9)) * 1e-3).astype(f32)
    pos[:, 0] = np.abs(pos[:, 0])                                # (x >= 0: a block that holds a zero has it as its lower bound)
    pos[rng.permutation(n)[:400], 0] = f32(0.0)
    pos[rng.permutation(n)[:400], 0] = f32(-0.0)
    pos[:, 1] = np.round(pos[:, 1] * 4) / 4                      # ties on an axis, signed zeros among them
    pos[rng.permutation(n)[:200], 1] = f32(-0.0)
    for v in (np.nan, np.inf, -np.inf):
        pos[rng.permutation(n)[:40], rng.integers(0, 3, 40)] = f32(v)
    orig = rng.permutation(n).astype(np.uint32)
    pos[orig[512:768], 2] = np.nan                               # a block without a finite centre
    cov[orig[5], 4], cov[orig[300], 0] = np.nan, np.inf
    got, want = L.block_bounds(pos, cov, orig), block_bounds_loop(pos, cov, orig)
    assert np.isnan(want[2, :6]).all() and np.isinf(want[:, 6]).sum() == 2
    zero = want[:, 0] == 0
    assert (zero & np.signbit(want[:, 0])).any() and (zero & ~np.signbit(want[:, 0])).any()
    nan = np.isnan(got) & np.isnan(want)
    assert ((got.view(np.uint32) == want.view(np.uint32)) | nan).all()
