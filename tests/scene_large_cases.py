"""Scenes and masks on both sides of the sizes at which the multi-round kernels of the device scene order and of the mask scan
take a second round, for the tests that hold those kernels to numpy there (tests/test_gpu_scene_large.py,
tests/test_scene_large_cases_host.py).  The thresholds are derived from the constants in the sources, so the cases move if a
constant does:

  BOX  = 256 * BOX_GROUPS_MAX           beyond it a thread of scene_box_kernel takes a second row (a second "trip")
  SORT = 256 * 256 * SORT_ITEMS         beyond it a digit's row of the (digit, workgroup) table is longer than one round of
                                        radix_scan_kernel, and radix_scatter_kernel reads the table from column 256 on
  MASK = SELECT_SPAN * SELECT_SCAN_ROUND   beyond it ((address & 15) + n) mask_scan_kernel takes a second round

Also here: numpy models of one LSD pass and of the mask compaction AS THE KERNELS DO THEM (per-tile counts, a scan in rounds
with a carry, a scatter by base + prefix + rank), with a switch that drops the carry -- the defect the cases are for -- and a
vectorised block_bounds for a million slots.  Every scene is made once and shared: no test writes into what these return."""
import functools
import os
import re

import numpy as np

import splat_amd
import remove_cases as RC

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "splat_amd", "csrc")


def constant(name, source):
    text = open(os.path.join(CSRC, source)).read()
    return int(re.search(r"constexpr\s+(?:unsigned\s+)?int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


SORT_ITEMS = constant("SORT_ITEMS", "splat_kernels.hip")
BOX_GROUPS_MAX = constant("BOX_GROUPS_MAX", "splat_kernels.hip")
SELECT_SPAN = constant("SELECT_SPAN", "splat_internal.h")
SELECT_SCAN_ROUND = constant("SELECT_SCAN_ROUND", "splat_internal.h")
SORT_TILE = 256 * SORT_ITEMS
BOX = 256 * BOX_GROUPS_MAX
SORT = 256 * SORT_TILE
MASK = SELECT_SPAN * SELECT_SCAN_ROUND
GUARD = 64
SENTINEL = 0xA5


# ---- which regime a size is in ------------------------------------------------------------------------------------------------
def box_trips(n):
    """rows the busiest thread of scene_box_kernel takes: the grid is min(blocks, BOX_GROUPS_MAX) workgroups of 256"""
    groups = min((n + 255) // 256, BOX_GROUPS_MAX)
    return (n + 256 * groups - 1) // (256 * groups)


def sort_groups(n):
    return (n + SORT_TILE - 1) // SORT_TILE


def sort_scan_rounds(n):
    return (sort_groups(n) + 255) // 256


def selection_groups(head, n):
    """selection_groups of splat_internal.h, restated: spans of SELECT_SPAN bytes on 16-byte boundaries of the ADDRESS"""
    return (head + n + SELECT_SPAN - 1) // SELECT_SPAN


def mask_scan_rounds(head, n):
    return (selection_groups(head, n) + SELECT_SCAN_ROUND - 1) // SELECT_SCAN_ROUND


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def random_positions(n, seed):
    p = np.ones((n, 4), f32)
    p[:, :3] = np.random.default_rng(seed).random((n, 3), dtype=f32) * f32(2.0) - f32(1.0)
    return p


def box_plus_one():
    """the maximum of every axis sits in row BOX, the only row of the second trip (one row holds one extreme per axis: the
    three minima are in the first trip)"""
    p = random_positions(BOX + 1, 101)
    p[BOX, :3] = (1.5, 1.25, 1.75)
    return p


BOX_STRIDES_N = 3 * BOX + 77
# (axis, which end, row, value): trips 0 1 1 2 2 3 -- the x maximum in the last row of the last, partial trip
BOX_STRIDES_EXTREMES = ((0, "lo", 5, -1.5), (1, "lo", BOX + 1000, -1.25), (2, "hi", BOX + 70000, 1.75), (2, "lo", 2 * BOX + 3, -1.375),
                        (1, "hi", 2 * BOX + 200000, 1.625), (0, "hi", 3 * BOX + 76, 1.875))


def box_strides():
    n = BOX_STRIDES_N
    p = random_positions(n, 102)
    rng = np.random.default_rng(103)
    for trip in (1, 2):
        rows = trip * BOX + rng.permutation(BOX)[:2900]
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            r = rows[300 * k: 300 * (k + 1)]
            p[r, rng.integers(0, 3, 300)] = f32(v)
        p[rows[900:1900], 0] = f32(0.0)
        p[rows[1900:2900], 0] = f32(-0.0)
    last = 3 * BOX
    p[last + 10, 0], p[last + 11, 1], p[last + 12, 2], p[last + 13, 0], p[last + 14, 2] = np.nan, np.inf, -np.inf, np.inf, np.inf
    p[last + 20, 0], p[last + 21, 0] = f32(0.0), f32(-0.0)
    for axis, _, row, v in BOX_STRIDES_EXTREMES:
        p[row, :3] = random_positions(1, 104 + row)[0, :3]       # (a finite row, whatever was sprinkled there)
        p[row, axis] = f32(v)
    return p


def lattice(n, seed):
    """a 4 x 4 x 4 lattice: 64 codes, thousands of Gaussians each -- the order among equal codes decides"""
    p = np.ones((n, 4), f32)
    p[:, :3] = np.random.default_rng(seed).integers(0, 4, (n, 3)).astype(f32) - f32(1.5)
    return p


def one_code(n):
    p = np.ones((n, 4), f32)
    p[:, :3] = (0.25, -0.5, 0.125)
    return p


ORDER_CASES = {                                                  # name: (n, positions)
    "box": (BOX, lambda: random_positions(BOX, 100)),
    "box+1": (BOX + 1, box_plus_one),
    "box-strides": (BOX_STRIDES_N, box_strides),
    "sort": (SORT, lambda: random_positions(SORT, 105)),
    "sort+1": (SORT + 1, lambda: random_positions(SORT + 1, 106)),
    "sort+tile lattice": (SORT + SORT_TILE + 1, lambda: lattice(SORT + SORT_TILE + 1, 107)),
    "one code": (SORT + 1, lambda: one_code(SORT + 1)),
}
ORDER_NAMES = list(ORDER_CASES)
TWINS = ("sort+1", "box-strides")                                # these are also taken through the host upload on a second context


@functools.lru_cache(maxsize=None)
def positions(name):
    n, make = ORDER_CASES[name]
    p = make()
    assert p.shape == (n, 4) and p.dtype == f32
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def order(name):
    """the reference: remove_cases.morton_order of the case's positions"""
    o = RC.morton_order(positions(name))
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def second_positions(n):
    """another seeded set for the scene of n Gaussians: what the reorder test edits the positions to"""
    p = random_positions(n, 108)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def shared_fields(n):
    """(scales, opacities, rotations, sh, cov3d) every scene here shares: one small isotropic covariance, one opacity, a DC-only
    sh of the Gaussian's own colour.  Plain arrays: synthetic_scene takes seconds at a million rows."""
    sigma = f32(0.004)
    scales = np.full((n, 3), sigma, f32)
    rotations = np.zeros((n, 4), f32)
    rotations[:, 3] = 1
    cov3d = np.zeros((n, 9), f32)
    cov3d[:, (0, 4, 8)] = sigma * sigma
    sh = np.zeros((n, 48), f32)
    sh[:, :3] = np.random.default_rng(109).random((n, 3), dtype=f32) * f32(3.0) - f32(1.5)
    out = (scales, np.full(n, 0.6, f32), rotations, sh, cov3d)
    for a in out:
        a.setflags(write=False)
    return out


N_MAX = max(n for n, _ in ORDER_CASES.values())


def scene_of(pos4):
    """a GaussianList of these positions over (views of) the shared fields"""
    n = len(pos4)
    scales, opacities, rotations, sh, cov3d = (a[:n] for a in shared_fields(max(n, N_MAX)))
    return splat_amd.GaussianList(pos4, scales, opacities, rotations, sh, cov3d)


@functools.lru_cache(maxsize=None)
def scene(name):
    return scene_of(positions(name))


@functools.lru_cache(maxsize=None)
def small_scene(n=257, seed=110):
    """the few rows the appends pair with a large scene (values of their own, so that a row taken from the wrong side shows)"""
    rng = np.random.default_rng(seed)
    g = splat_amd.GaussianList(random_positions(n, seed + 1), np.full((n, 3), 0.01, f32), rng.random(n, dtype=f32), np.tile(np.array([0, 0, 0, 1], f32), (n, 1)),
                               rng.random((n, 48), dtype=f32) - f32(0.5), None)
    g.cov3d[:, (0, 4, 8)] = rng.random((n, 1), dtype=f32) * f32(1e-4) + f32(1e-5)
    return g


# ---- the scene the removal runs on ----------------------------------------------------------------------------------------------
REMOVE_N = MASK + 1
REMOVE_PAIRS = ((0, "lo", -1.5), (0, "hi", 1.5), (1, "lo", -1.25), (1, "hi", 1.25), (2, "lo", -1.75), (2, "hi", 1.75))


def remove_pair_rows():
    """[(row a, row b)] per extreme: both rows hold it, so that the finite box keeps its bits while either of them stays"""
    rows = np.random.default_rng(111).permutation(REMOVE_N - 1)[:12]          # (never the last Gaussian)
    return [(int(rows[2 * k]), int(rows[2 * k + 1])) for k in range(6)]


@functools.lru_cache(maxsize=None)
def remove_positions():
    p = random_positions(REMOVE_N, 112)
    for (axis, _, v), (a, b) in zip(REMOVE_PAIRS, remove_pair_rows()):
        p[a, axis] = p[b, axis] = f32(v)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def remove_scene():
    return scene_of(remove_positions())


def remove_selection(which):
    """the three selections of the removal, n = REMOVE_N bools.  The seeded 30 % selects exactly one row of every pair that holds
    an extreme, so in either keep mode the survivors' box is the scene's and their order is a fresh upload's"""
    n = REMOVE_N
    if which == "30 %":
        sel = np.random.default_rng(113).random(n) < 0.3
        for a, b in remove_pair_rows():
            sel[a], sel[b] = True, False
        sel[n - 1] = True                                        # (a selected byte behind the scan's first round)
        return sel
    sel = np.zeros(n, bool)
    if which == "all but the last":
        sel[: n - 1] = True
    else:
        assert which == "only the last"
        sel[n - 1] = True
    return sel


REMOVE_SELECTIONS = ("30 %", "all but the last", "only the last")


# ---- the order with a box of one's choosing, and one LSD pass as the kernels do it --------------------------------------------------
def codes_with_box(pos, lo, hi):
    """remove_cases.morton_codes with the box handed in: what a box kernel that saw other rows would lead to"""
    pos = np.asarray(pos, f32)
    code = np.zeros(len(pos), np.uint32)
    with np.errstate(all="ignore"):
        for a in range(3):
            sc = f32(1023.0) / f32(hi[a] - lo[a]) if hi[a] > lo[a] else f32(0.0)
            v = pos[:, a]
            t = ((v - lo[a]).astype(f32) * sc).astype(f32)
            t = np.where(f32(0.0) < t, t, f32(0.0))
            t = np.where(t < f32(1023.0), t, f32(1023.0))
            q = np.where(np.isfinite(v), t, f32(0.0)).astype(np.uint32)
            code |= RC.spread3(q) << np.uint32(a)
    return code


def order_with_box(pos, lo, hi):
    return np.argsort(codes_with_box(pos, lo, hi), kind="stable").astype(np.uint32)


UNWRITTEN = 0xFFFFFFFF


def lsd_pass(keys, vals, shift, drop_carry=False):
    """one 8-bit pass of the device sort: radix_hist_kernel's table[digit][tile], radix_scan_kernel's exclusive scan along every
    digit's row in rounds of 256 columns with a carry (drop_carry: every round after the first starts from 0), and
    radix_scatter_kernel's destination = keys of the digits below + the row's prefix + the rank among the tile's keys of the
    digit.  Returns (keys, vals) after the pass; a slot nothing was scattered to holds UNWRITTEN."""
    n = len(keys)
    nwg = sort_groups(n)
    d = ((keys >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
    tile = np.arange(n, dtype=np.int64) // SORT_TILE
    cell = d * nwg + tile
    table = np.bincount(cell, minlength=256 * nwg).reshape(256, nwg)
    prefix = np.zeros_like(table)
    carry = np.zeros(256, np.int64)
    for c0 in range(0, nwg, 256):
        chunk = table[:, c0:c0 + 256]
        incl = np.cumsum(chunk, axis=1)
        start = np.zeros(256, np.int64) if (drop_carry and c0) else carry
        prefix[:, c0:c0 + 256] = start[:, None] + incl - chunk
        carry = carry + incl[:, -1]
    base = np.cumsum(carry) - carry                              # (the digit totals, scanned by the scatter itself)
    by_cell = np.argsort(tile * 256 + d, kind="stable")          # within a tile, within a digit: index order
    first = np.cumsum(table.T.reshape(-1)) - table.T.reshape(-1)  # where each (tile, digit) group starts in by_cell
    rank = np.empty(n, np.int64)
    rank[by_cell] = np.arange(n, dtype=np.int64) - first[(tile * 256 + d)[by_cell]]
    dest = base[d] + prefix.reshape(-1)[cell] + rank
    out_k, out_v = np.full(n, UNWRITTEN, np.uint32), np.full(n, UNWRITTEN, np.uint32)
    out_k[dest], out_v[dest] = keys, vals
    return out_k, out_v


def lsd_order(pos, drop_carry=False):
    """four passes over the 30-bit codes, as launch_scene_order runs them"""
    keys = RC.morton_codes(pos)
    vals = np.arange(len(keys), dtype=np.uint32)
    for p in range(4):
        keys, vals = lsd_pass(keys, vals, 8 * p, drop_carry)
    return vals


# ---- masks ----------------------------------------------------------------------------------------------------------------------
MASK_CASES = ((0, MASK), (0, MASK + 1), (15, MASK - 14), (1, 2 * MASK + SELECT_SPAN + 1))      # (head, n); the first is the control
PATTERNS = ("all ones", "30 %", "the last byte", "the last span")
NONZERO = np.array([1, 2, 0x80, 0xFF], np.uint8)                 # nonzero means selected, whatever the byte


def mask_bytes(head, n, pattern):
    if pattern == "all ones":
        sel = np.ones(n, bool)
    elif pattern == "30 %":
        sel = np.random.default_rng(1000 * head + n % 1000).random(n) < 0.3
    else:
        sel = np.zeros(n, bool)
        if pattern == "the last byte":
            sel[n - 1] = True
        else:
            assert pattern == "the last span"
            sel[max(0, (selection_groups(head, n) - 1) * SELECT_SPAN - head):] = True      # zeros throughout every round before
    return np.where(sel, NONZERO[np.arange(n) % 4], 0).astype(np.uint8)


def spans_of(mask, head):
    """(selected per byte of the spans, span by span; counts per span)"""
    g = selection_groups(head, len(mask))
    padded = np.zeros(g * SELECT_SPAN, bool)
    padded[head:head + len(mask)] = np.asarray(mask) != 0
    return padded, padded.reshape(g, SELECT_SPAN).sum(1).astype(np.int64)


def selected_in_rounds(mask, head):
    """(is a byte selected in the scan's first round, is one selected behind it)"""
    padded, _ = spans_of(mask, head)
    return bool(padded[:SELECT_SPAN * SELECT_SCAN_ROUND].any()), bool(padded[SELECT_SPAN * SELECT_SCAN_ROUND:].any())


def scan_indices(mask, head, defect=None):
    """the compaction as the kernels do it: mask_count_kernel's count per span, mask_scan_kernel's exclusive scan in rounds of
    SELECT_SCAN_ROUND with a carry, mask_scatter_kernel's place = the span's offset + the rank in the span.  defect "carry":
    every round after the first starts from 0; "one round": the scan ends after its first round, the later counts stay as
    they were counted and the total is the first round's.  Returns (count, indices), an entry nothing was scattered to
    UNWRITTEN."""
    assert defect in (None, "carry", "one round")
    padded, counts = spans_of(mask, head)
    offsets = counts.copy()
    carry = 0
    for b in range(0, len(counts), SELECT_SCAN_ROUND):
        if b and defect == "one round":
            break
        chunk = counts[b:b + SELECT_SCAN_ROUND]
        incl = np.cumsum(chunk)
        offsets[b:b + SELECT_SCAN_ROUND] = (0 if (b and defect == "carry") else carry) + incl - chunk
        carry += int(incl[-1])
    where = np.flatnonzero(padded)
    span = where // SELECT_SPAN
    place = offsets[span] + np.arange(len(where), dtype=np.int64) - (np.cumsum(counts) - counts)[span]
    out = np.full(max(carry, int(place.max()) + 1 if len(place) else 0), UNWRITTEN, np.uint32)
    out[place] = (where - head).astype(np.uint32)
    return carry, out


# ---- block bounds for a million slots ---------------------------------------------------------------------------------------------
def block_bounds(pos4, cov3d, orig):
    """block_bounds_np of tests/test_gpu_scene_update.py without its loop over the Gaussians: per block of 256 slots of `orig`
    the keep-first min and max over the finite centres (argmin / argmax give the FIRST of equal values: +0 and -0), the nine
    squares summed in float64 in order, float32(sqrt) * float32(1.0001), NaN -> inf, and a NaN box for a block without a
    finite centre"""
    orig = np.asarray(orig, np.int64)
    n = len(orig)
    nb = (n + 255) // 256
    p = np.asarray(pos4, f32)[orig, :3]
    ok = np.isfinite(p).all(1)

    def blocks(a, fill):
        out = np.full((nb * 256,) + a.shape[1:], fill, a.dtype)
        out[:n] = a
        return out.reshape((nb, 256) + a.shape[1:])

    out = np.zeros((nb, 8), f32)
    lo_in, hi_in = blocks(np.where(ok[:, None], p, f32(np.inf)), f32(np.inf)), blocks(np.where(ok[:, None], p, f32(-np.inf)), f32(-np.inf))
    out[:, 0:3] = np.take_along_axis(lo_in, lo_in.argmin(1)[:, None, :], 1)[:, 0, :]
    out[:, 3:6] = np.take_along_axis(hi_in, hi_in.argmax(1)[:, None, :], 1)[:, 0, :]
    c = np.asarray(cov3d, f32)[orig].astype(np.float64)
    f2 = np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        for e in range(9):
            f2 = f2 + c[:, e] * c[:, e]
        f = (np.sqrt(f2).astype(f32) * f32(1.0001)).astype(f32)
    f = np.where(f >= 0, f, f32(np.inf))
    out[:, 6] = blocks(np.where(ok, f, f32(0.0)).astype(f32), f32(0.0)).max(1)
    out[~blocks(ok, False).any(1), 0:6] = np.nan
    return out


# ---- PLY rows ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ply_rows(n):
    """n rows of the canonical 62-float layout (splat_amd.gaussians.PLY_PROPS): positions and f_dc of their own, one scale,
    one opacity logit, the identity rotation"""
    from splat_amd.gaussians import PLY_PROPS
    col = {name: k for k, name in enumerate(PLY_PROPS)}
    rng = np.random.default_rng(114)
    rows = np.zeros((n, len(PLY_PROPS)), f32)
    rows[:, col["x"]:col["z"] + 1] = rng.random((n, 3), dtype=f32) * f32(2.0) - f32(1.0)
    rows[:, col["f_dc_0"]:col["f_dc_2"] + 1] = rng.random((n, 3), dtype=f32) * f32(3.0) - f32(1.5)
    rows[:, col["opacity"]] = f32(0.4)
    rows[:, col["scale_0"]:col["scale_2"] + 1] = f32(-5.5)
    rows[:, col["rot_0"]] = f32(1.0)
    rows.setflags(write=False)
    return rows
