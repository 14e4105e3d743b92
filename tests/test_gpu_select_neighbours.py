"""A selection by neighbourhood on the GPU (splat_select_neighbours_device, Renderer.select_neighbours; -m gpu).

The reference is never the library: it is numpy in float32 with the operation order include/splat_hip.h states -- all pairs,
in chunks, d2 = (dx dx + dy dy) + dz dz <= r2 with r2 = f32(radius) * f32(radius), the self pair taken out by index, the
source mask applied, the count saturated at count_max + 1, the op restated byte by byte -- and the work bound restated from
splat_get_scene_layout's bounds with the header's gap formula.  Nothing here has a tolerance: the counts, the bytes, the
selected count and block_pairs must EQUAL the reference's.

Shapes: single blocks and block edges (1 .. 513 Gaussians), an 8x8x8 integer lattice whose ties d2 == r2 are exact (once
with every point twice), synthetic_scene(6000, 1) -- 24 blocks, the largest all-pairs reference here (about a second,
computed once per radius and shared) --, 600 rows half of them non-finite, and scenes edited in place, whose slot order is
stale and whose bounds were recomputed."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from helpers import make_camera, with_oracle_cov3d

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STILL = int(re.search(r"#define SPLAT_POLICY_STILL_FRAMES (\d+)", open(os.path.join(ROOT, "include", "splat_policy.h")).read()).group(1))
UNBOUNDED = 0xFFFFFFFF
SENTINEL8, SENTINEL32 = 0xA5, 0xDEADBEEF
OPS = ("set", "add", "subtract", "intersect")


# ---- plumbing -------------------------------------------------------------------------------------------------------
class Session:
    """a Renderer and the device buffers made on it, released together (the buffers first)"""

    def __init__(self, **conventions):
        self.R = splat_amd.Renderer(**conventions)
        self._held = []

    def alloc(self, nbytes):
        R = self.R
        p = R._L.splat_device_alloc(R._h, max(int(nbytes), 4))
        assert p
        self._held.append(p)
        return p

    def put(self, a, at=None, skew=0):
        """device copy of a numpy array (at: an address to write to; skew: bytes past an allocation's start); its address"""
        a = np.ascontiguousarray(a)
        p = (self.alloc(a.nbytes + skew) + skew) if at is None else at
        if a.nbytes:
            self.R._check(self.R._L.splat_device_upload(self.R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def get(self, p, count, dtype=np.uint8):
        out = np.zeros(count, dtype)
        if out.nbytes:
            self.R._check(self.R._L.splat_device_download(self.R._h, C.c_void_p(out.ctypes.data), C.c_void_p(p), out.nbytes))
        return out

    def release(self):
        for p in reversed(self._held):
            self.R.device_free(p)
        self._held = []

    def close(self):
        self.release()
        self.R.close()


@contextlib.contextmanager
def session(**conventions):
    s = Session(**conventions)
    try:
        yield s
    finally:
        s.close()


@pytest.fixture(scope="module")
def S():
    """one context for the module; every test uploads its own scene and releases its buffers"""
    s = Session()
    yield s
    s.close()


def scene_at(pos, seed=3):
    """a scene whose centres are the rows of pos (n x 3); everything else is a synthetic scene's"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    g = splat_amd.synthetic_scene(len(pos), seed)
    g.positions[:, :3] = pos
    return with_oracle_cov3d(g)


CLOUD = {}


def cloud():
    if "g" not in CLOUD:
        CLOUD["g"] = with_oracle_cov3d(splat_amd.synthetic_scene(6000, 1))
    return CLOUD["g"]


# ---- the reference --------------------------------------------------------------------------------------------------
def within(pos, radius):
    """n x n: j within reach of i, the diagonal (the Gaussian itself) cleared -- all pairs in float32, in chunks"""
    p = np.ascontiguousarray(pos[:, :3], f32)
    n = len(p)
    r2 = f32(radius) * f32(radius)
    assert np.isfinite(r2)
    out = np.zeros((n, n), bool)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, 500):
            d = p[i0:i0 + 500, None, :] - p[None, :, :]
            assert d.dtype == f32
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            out[i0:i0 + 500] = d2 <= r2
    out[np.arange(n), np.arange(n)] = False
    assert np.array_equal(out, out.T)                       # the relation is symmetric
    return out


ADJ = {}


def cloud_within(radius):
    """the cloud's relation, computed once per radius and left unchanged"""
    if radius not in ADJ:
        ADJ[radius] = within(cloud().positions, radius)
        ADJ[radius].flags.writeable = False
    return ADJ[radius]


def ref_counts(adj, source=None, count_max=UNBOUNDED):
    c = (adj if source is None else adj[:, np.asarray(source) != 0]).sum(1).astype(np.int64)
    return np.minimum(c, count_max + 1) if count_max < UNBOUNDED else c


def ref_pass(c, count_min, count_max):
    return (count_min <= c) & (c <= count_max)


def ref_op(old, passes, op):
    """(bytes, count) after the op: the library writes only 0 and 1, ADD and SUBTRACT leave the bytes that do not pass"""
    old = np.asarray(old, np.uint8)
    if op == "set":
        out = passes.astype(np.uint8)
    elif op == "add":
        out = np.where(passes, 1, old).astype(np.uint8)
    elif op == "subtract":
        out = np.where(passes, 0, old).astype(np.uint8)
    else:
        out = ((old != 0) & passes).astype(np.uint8)
    return out, int((out != 0).sum())


def ref_block_pairs(R, radius):
    """the ordered pairs of K1 blocks within reach of each other, from the resident bounds with the header's gap formula"""
    _, b = R.scene_layout()
    lo, hi = np.ascontiguousarray(b[:, 0:3], f32), np.ascontiguousarray(b[:, 3:6], f32)
    r2 = f32(radius) * f32(radius)
    with np.errstate(all="ignore"):
        # [t, s, axis]
        g = np.maximum(np.maximum(lo[None, :, :] - hi[:, None, :], lo[:, None, :] - hi[None, :, :]), f32(0.0))
        assert g.dtype == f32
        g2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        return int((g2 <= r2).sum())


# ---- one call against the reference ------------------------------------------------------------------------------------
def check(s, adj, radius, *, source=None, count_min=0, count_max=UNBOUNDED, op="set", old=None, want_counts=True, want_sel=True,
          skew=0, what=""):
    """one call on the session's resident scene, held to the reference; returns (bytes, counts) as the GPU left them"""
    n = len(adj)
    rng = np.random.default_rng(n + int(count_min))
    old = rng.integers(0, 2, n).astype(np.uint8) if old is None else np.asarray(old, np.uint8)
    d_sel = s.put(old, skew=skew) if want_sel else None
    d_src = s.put(np.asarray(source, np.uint8), skew=(skew and skew + 2)) if source is not None else None
    if skew:                                                  # an odd skew: both buffers at odd byte addresses, and apart mod 4
        assert skew & 1 and (d_sel is None or d_sel & 1) and (d_src is None or d_src & 1)
    d_cnt = s.put(np.full(n, SENTINEL32, np.uint32)) if want_counts else None
    k = s.R.select_neighbours(d_sel, radius, source=d_src, at_least=count_min, at_most=None if count_max == UNBOUNDED else count_max,
                              op=op, counts=d_cnt, max_block_pairs=0)
    c = ref_counts(adj, source, count_max)
    passes = ref_pass(c, count_min, count_max)
    assert s.R.block_pairs == ref_block_pairs(s.R, radius), what
    got_c = got_b = None
    if want_counts:
        got_c = s.get(d_cnt, n, np.uint32)
        bad = np.flatnonzero(got_c.astype(np.int64) != c)
        assert bad.size == 0, "%s: %d of %d counts differ, first %d: %d, want %d" % (what, bad.size, n, bad[0], got_c[bad[0]], c[bad[0]])
    if want_sel:
        want_b, want_k = ref_op(old, passes, op)
        got_b = s.get(d_sel, n)
        bad = np.flatnonzero(got_b != want_b)
        assert bad.size == 0, "%s: %d of %d bytes differ, first %d: %d, want %d" % (what, bad.size, n, bad[0], got_b[bad[0]], want_b[bad[0]])
        assert k == want_k, what
    else:
        assert k == int(passes.sum()), what                   # counts only: how many pass
    return got_b, got_c


# ---- 1. block edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_block_edges(S, n):
    rng = np.random.default_rng(100 + n)
    pos = rng.random((n, 3)).astype(f32)
    g = scene_at(pos)
    try:
        S.R.upload(g)
        # reaches a few neighbours / across the blocks of the unit cube / everything
        for radius in (0.12, 0.4, 2.0):
            adj = within(g.positions, radius)
            check(S, adj, radius, what="n=%d r=%g" % (n, radius))
            check(S, adj, radius, count_min=1, count_max=3, op="add", what="n=%d r=%g window" % (n, radius))
        if n > 1:
            assert within(g.positions, 2.0).sum(1).min() == n - 1     # everyone counts everyone but itself
    finally:
        S.release()


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------
def lattice(twice=False):
    p = np.array([(x, y, z) for x in range(8) for y in range(8) for z in range(8)], f32)
    return np.concatenate([p, p]) if twice else p


def interior(p):
    return ((p >= 1) & (p <= 6)).all(1)


@pytest.mark.parametrize("twice", [False, True])
def test_exact_ties_on_an_integer_lattice(S, twice):
    p = lattice(twice)
    rng = np.random.default_rng(7)
    p = p[rng.permutation(len(p))]                            # (the index order says nothing about the place)
    g = scene_at(p)
    inner = interior(p)
    try:
        S.R.upload(g)
        for radius, inside in ((1.0, 13 if twice else 6), (0.0, 1 if twice else 0), (2.0, None)):
            adj = within(g.positions, radius)
            c = ref_counts(adj)
            if inside is not None:
                assert (c[inner] == inside).all()             # (the reference itself: 6 face neighbours, twins included twice)
            if radius == 0.0:
                assert (c == (1 if twice else 0)).all()
            _, got = check(S, adj, radius, what="lattice r=%g" % radius)
            if inside is not None:
                assert (got[inner] == inside).all()
            check(S, adj, radius, count_max=5, what="lattice r=%g saturated" % radius)
    finally:
        S.release()


# ---- 3. the cloud ---------------------------------------------------------------------------------------------------------
RADII = (0.25, 0.5)
WINDOWS = ((0, 0), (0, 7), (1, UNBOUNDED), (3, 7))


@pytest.mark.parametrize("radius", RADII)
def test_cloud_windows_counts_and_ops(S, radius):
    g, adj = cloud(), cloud_within(radius)
    n = len(g)
    c = ref_counts(adj)
    assert (c == 0).any() and ((c >= 1) & (c <= 7)).any() and (c > 7).any(), "the windows below would test nothing"
    rng = np.random.default_rng(11)
    prior = rng.integers(0, 2, n).astype(np.uint8)
    try:
        S.R.upload(g)
        for lo, hi in WINDOWS:
            # counts saturated at count_max + 1, exact when unbounded; selection set
            check(S, adj, radius, count_min=lo, count_max=hi, what="window %d..%d" % (lo, hi))
            S.release()
        for lo, hi in ((0, 7), (1, UNBOUNDED)):
            check(S, adj, radius, count_min=lo, count_max=hi, want_sel=False, what="counts only %d..%d" % (lo, hi))
            check(S, adj, radius, count_min=lo, count_max=hi, want_counts=False, what="no counts %d..%d" % (lo, hi))
            S.release()
        for op in OPS:
            check(S, adj, radius, count_min=3, count_max=7, op=op, old=prior, what="op " + op)
            # ... with the selection and the source at odd byte addresses
            check(S, adj, radius, count_min=0, count_max=7, op=op, old=prior, source=np.ones(n, np.uint8), skew=1, what="odd, op " + op)
            S.release()
    finally:
        S.release()


def test_source_masks_and_growing_in_place(S):
    g, radius = cloud(), 0.25
    adj = cloud_within(radius)
    n = len(g)
    rng = np.random.default_rng(13)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()))        # any nonzero byte is a source
    try:
        S.R.upload(g)
        check(S, adj, radius, source=mask, what="30 % mask")
        check(S, adj, radius, source=mask, count_min=1, count_max=2, op="intersect", skew=3, what="30 % mask, odd")
        _, c = check(S, adj, radius, source=np.zeros(n, np.uint8), what="empty mask")
        assert not c.any()
        # grow in place: d_source IS d_selection
        seed = (rng.random(n) < 0.02).astype(np.uint8)
        d = S.put(seed, skew=1)                                # ... at an odd byte address
        assert d & 1
        want1 = ((seed != 0) | (adj[:, seed != 0].sum(1) >= 1))
        k1 = S.R.select_neighbours(d, radius, source=d, at_least=1, op="add", max_block_pairs=0)
        got1 = S.get(d, n)
        assert np.array_equal(got1, want1.astype(np.uint8)) and k1 == int(want1.sum())
        assert want1.sum() > (seed != 0).sum()
        want2 = want1 | (adj[:, want1].sum(1) >= 1)
        k2 = S.R.select_neighbours(d, radius, source=d, at_least=1, op="add", max_block_pairs=0)
        assert np.array_equal(S.get(d, n), want2.astype(np.uint8)) and k2 == int(want2.sum())
        assert want2.sum() > want1.sum()
        # ADD and SUBTRACT leave the bytes of Gaussians that do not pass as they are, whatever they hold
        odd = rng.integers(0, 256, n).astype(np.uint8)
        for op in ("add", "subtract"):
            got, _ = check(S, adj, radius, count_min=2, count_max=5, op=op, old=odd, what="odd bytes, " + op)
            keep = ~ref_pass(ref_counts(adj, None, 5), 2, 5)
            assert np.array_equal(got[keep], odd[keep]) and (odd[keep] > 1).any()
    finally:
        S.release()


# ---- 4. non-finite rows -------------------------------------------------------------------------------------------------
def spoil(pos, rows, rng):
    """a NaN, +inf or -inf in one, two or three coordinates of each of `rows`"""
    bad = np.array([np.nan, np.inf, -np.inf], f32)
    for i in rows:
        axes = rng.permutation(3)[: rng.integers(1, 4)]
        pos[i, axes] = bad[rng.integers(0, 3, len(axes))]


@pytest.mark.parametrize("finite", [300, 5])
def test_non_finite_rows_count_nothing_and_are_counted_by_nobody(S, finite):
    n = 600
    rng = np.random.default_rng(17 + finite)
    pos = (rng.random((n, 3)) * 0.8).astype(f32)
    rows = rng.permutation(n)[: n - finite]
    spoil(pos, rows, rng)
    if finite == 5:
        # ... here in all three coordinates, so that blocks without any finite centre occur (such rows sort first)
        pos[rows] = np.array([np.nan, np.inf, -np.inf], f32)[rng.integers(0, 3, (len(rows), 3))]
    assert np.isfinite(pos).all(1).sum() == finite
    g = scene_at(pos)
    try:
        S.R.upload(g)
        _, b = S.R.scene_layout()
        if finite == 5:
            assert np.isnan(b[:, 0]).any(), "a block without a finite centre is meant to occur"
        for radius in (0.1, 0.3, 5.0):
            adj = within(g.positions, radius)
            assert not adj[rows].any() and not adj[:, rows].any()
            _, c = check(S, adj, radius, what="%d finite, r=%g" % (finite, radius))
            assert not c[rows].any()
            check(S, adj, radius, count_min=0, count_max=0, what="%d finite, r=%g, floaters" % (finite, radius))
        assert within(g.positions, 5.0).sum() == finite * (finite - 1)
    finally:
        S.release()


# ---- 5. after edits: the order is stale, the bounds are recomputed -------------------------------------------------------
def resident_positions(s, n):
    d = s.alloc(16 * n)
    s.R.read_device(positions=d, n=n)
    return s.get(d, 4 * n, f32).reshape(n, 4)


def test_after_an_indexed_update_moved_centres_far_away(S):
    n, k = 3000, 200
    g = with_oracle_cov3d(splat_amd.synthetic_scene(n, 4))
    rng = np.random.default_rng(19)
    idx = np.sort(rng.permutation(n)[:k]).astype(np.uint32)
    moved = np.ones((k, 4), f32)
    moved[:, :3] = (40.0 + rng.random((k, 3)) * 0.5).astype(f32)           # far from the cloud, close to each other
    try:
        S.R.upload(g)
        order_before = S.R.scene_layout()[0].copy()
        S.R.update_indexed(S.put(idx), positions=S.put(moved), k=k)
        assert np.array_equal(S.R.scene_layout()[0], order_before), "an edit keeps the order: it is stale now"
        pos = resident_positions(S, n)
        assert np.array_equal(pos[idx, :3], moved[:, :3])
        for radius in (0.3, 1.0):
            adj = within(pos, radius)
            assert adj[idx][:, idx].any() and not adj[idx][:, np.setdiff1d(np.arange(n), idx)].any()
            check(S, adj, radius, what="moved, r=%g" % radius)
            check(S, adj, radius, count_max=7, op="subtract", what="moved, r=%g, floaters off" % radius)
    finally:
        S.release()


def test_after_a_selection_was_rotated_and_scaled(S):
    n = 3000
    g = with_oracle_cov3d(splat_amd.synthetic_scene(n, 5))
    rng = np.random.default_rng(23)
    idx = np.sort(rng.permutation(n)[:700]).astype(np.uint32)
    a = 0.7
    m = np.array([[np.cos(a), -np.sin(a), 0, 0.4], [np.sin(a), np.cos(a), 0, -0.2], [0, 0, 1, 0.1]], f32)
    m[:, :3] *= f32(1.6)
    try:
        S.R.upload(g)
        S.R.transform(m, index=S.put(idx), k=len(idx))
        pos = resident_positions(S, n)
        assert not np.array_equal(pos[idx, :3], g.positions[idx, :3])
        for radius in (0.35, 0.8):
            adj = within(pos, radius)
            check(S, adj, radius, what="transformed, r=%g" % radius)
            check(S, adj, radius, count_min=1, count_max=4, op="intersect", what="transformed, r=%g, window" % radius)
    finally:
        S.release()


# ---- 6. the work bound ------------------------------------------------------------------------------------------------------
def test_the_work_bound_refuses_before_anything_is_written(S):
    g, radius = cloud(), 0.5
    n = len(g)
    adj = cloud_within(radius)
    try:
        S.R.upload(g)
        span = 40.0                                           # every block within reach of every block
        pairs = ref_block_pairs(S.R, span)
        assert pairs == ((n + 255) // 256) ** 2
        d_sel, d_cnt = S.put(np.full(n, SENTINEL8, np.uint8)), S.put(np.full(n, SENTINEL32, np.uint32))
        with pytest.raises(splat_amd.SplatError) as e:
            S.R.select_neighbours(d_sel, span, counts=d_cnt, max_block_pairs=1)
        assert e.value.code == _lib.ERR_CAPACITY
        assert str(pairs) in str(e.value) and re.search(r"\b1\b", str(e.value).split(str(pairs), 1)[1]), str(e.value)
        assert S.R.block_pairs == pairs
        assert (S.get(d_sel, n) == SENTINEL8).all() and (S.get(d_cnt, n, np.uint32) == SENTINEL32).all()
        # the limit itself, and none, let it through
        for limit in (pairs, 0):
            k = S.R.select_neighbours(d_sel, span, counts=d_cnt, max_block_pairs=limit)
            assert k == n and S.R.block_pairs == pairs
            assert (S.get(d_cnt, n, np.uint32) == n - 1).all() and (S.get(d_sel, n) == 1).all()
            S.put(np.full(n, SENTINEL8, np.uint8), at=d_sel)
        # a radius within the default: the same result as without a limit, and one pair short of its need is refused
        need = ref_block_pairs(S.R, radius)
        assert need <= 64 * ((n + 255) // 256)
        k = S.R.select_neighbours(d_sel, radius, at_most=7, counts=d_cnt)
        c = ref_counts(adj, None, 7)
        assert S.R.block_pairs == need and k == int((c <= 7).sum()) and np.array_equal(S.get(d_cnt, n, np.uint32), c)
        with pytest.raises(splat_amd.SplatError) as e:
            S.R.select_neighbours(d_sel, radius, max_block_pairs=need - 1)
        assert e.value.code == _lib.ERR_CAPACITY and S.R.block_pairs == need
        # the C ABI itself: block_pairs_out is written on the refusal, count_out is not
        pairs_out, count_out = C.c_uint64(7), C.c_uint64(SENTINEL32)
        rc = S.R._L.splat_select_neighbours_device(S.R._h, span, None, 0, UNBOUNDED, _lib.SEL_OP_SET, C.c_void_p(d_sel), None, 1,
                                                   C.byref(pairs_out), C.byref(count_out), None)
        assert rc == _lib.ERR_CAPACITY and pairs_out.value == pairs and count_out.value == SENTINEL32
    finally:
        S.release()


def test_the_default_limit_is_64_pairs_per_block(S):
    # 67 blocks: a radius that spans the cloud pairs every block with every block, 67 > 64 each (no all-pairs reference needed)
    n = 17000
    g = with_oracle_cov3d(splat_amd.synthetic_scene(n, 2))
    nb = (n + 255) // 256
    try:
        S.R.upload(g)
        assert ref_block_pairs(S.R, 40.0) == nb * nb > 64 * nb
        d_sel = S.put(np.full(n, SENTINEL8, np.uint8))
        with pytest.raises(splat_amd.SplatError) as e:
            S.R.select_neighbours(d_sel, 40.0)
        assert e.value.code == _lib.ERR_CAPACITY and S.R.block_pairs == nb * nb
        assert str(nb * nb) in str(e.value) and str(64 * nb) in str(e.value)
        assert (S.get(d_sel, n) == SENTINEL8).all()
        # ... and a radius the default lets through
        small = 0.05
        need = ref_block_pairs(S.R, small)
        assert need <= 64 * nb
        S.R.select_neighbours(d_sel, small, at_most=0)
        assert S.R.block_pairs == need
    finally:
        S.release()


# ---- 7. it reads only ------------------------------------------------------------------------------------------------------
def test_it_reads_the_scene_and_nothing_a_frame_depends_on_changes():
    n, h, w = 3000, 96, 128
    g = with_oracle_cov3d(splat_amd.synthetic_scene(n, 6))
    cam = make_camera(h, w).to_c(0.01, 15)
    adj = within(g.positions, 0.4)

    def run(s, select):
        R = s.R
        R.upload(g)
        img = np.zeros((h, w), np.uint32)

        def frame():
            img[:] = SENTINEL32
            R.render_frame(cam, img)
            return img.copy()

        frames = [frame() for _ in range(STILL + 4)]
        d_sel, d_cnt = s.put(np.zeros(n, np.uint8)), s.put(np.zeros(n, np.uint32))
        held = R.device_bytes()[0]
        for _ in range(3):
            if select:
                assert R.select_neighbours(d_sel, 0.4, at_most=3, counts=d_cnt) == int((ref_counts(adj) <= 3).sum())
                assert R.select_neighbours(d_sel, 0.4, source=d_sel, at_least=1, op="add") > 0      # (a temporary of 4 n bytes)
                assert R.device_bytes()[0] == held, "temporaries live for the call"
            frames.append(frame())
        return frames, R.frames_retained(), R.frames_dropped()

    with session() as a, session() as b:
        fa, ra, da = run(a, True)
        fb, rb, db = run(b, False)
    assert fa[0].any() and all(np.array_equal(fa[0], f) for f in fa + fb)
    assert ra == rb and ra > 0, "the retained lists survive the call"
    assert da == db == 0


# ---- 8. refusals that need a context ------------------------------------------------------------------------------------------
def test_no_scene():
    with session() as s:
        d = s.alloc(64)
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.select_neighbours(d, 1.0)
        assert e.value.code == _lib.ERR_NO_SCENE and "no resident scene" in str(e.value)
