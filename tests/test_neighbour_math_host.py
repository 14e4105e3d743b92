"""The two predicates of the neighbourhood selection (splat_amd/csrc/splat_neighbour_math.h), compiled for the host behind
tests/native/libneighbour_math_probe.so, held to a numpy float32 restatement bit for bit -- and the property the kernels'
culling rests on: the gap of a box is never above the squared distance of any point inside it.  No GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "tests", "native", "libneighbour_math_probe.so")
f32 = np.float32
_fp = C.POINTER(C.c_float)
_bp = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def P():
    L = C.CDLL(LIB)
    L.neighbour_probe_radius2.restype = C.c_float
    L.neighbour_probe_radius2.argtypes = [C.c_float]
    L.neighbour_probe_points.restype = None
    L.neighbour_probe_points.argtypes = [C.c_uint64, _fp, _fp, C.c_float, _fp, _bp]
    L.neighbour_probe_point_box.restype = None
    L.neighbour_probe_point_box.argtypes = [C.c_uint64, _fp, _fp, _fp, C.c_float, _fp, _bp]
    L.neighbour_probe_box_box.restype = None
    L.neighbour_probe_box_box.argtypes = [C.c_uint64, _fp, _fp, _fp, _fp, C.c_float, _fp, _bp]
    return L


def fp(a):
    assert a.dtype == f32 and a.flags.c_contiguous
    return a.ctypes.data_as(_fp)


def rows(a):
    return np.ascontiguousarray(a, f32).reshape(-1, 3)


# ---- the restatement: every difference, product and sum rounded to float32 once, in the header's order ------------------
def ref_d2(p, q):
    d = p - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def ref_gap2(lo_s, hi_s, lo_t, hi_t):
    g = np.maximum(np.maximum(lo_s - hi_t, lo_t - hi_s), f32(0.0))       # (np.maximum hands a NaN on)
    return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def ref_within(v2, radius):
    r2 = f32(radius) * f32(radius)
    return (v2 <= r2).astype(np.uint8)


# ---- the probe ---------------------------------------------------------------------------------------------------------
def points(P, p, q, radius):
    p, q = rows(p), rows(q)
    d2, w = np.empty(len(p), f32), np.empty(len(p), np.uint8)
    P.neighbour_probe_points(len(p), fp(p), fp(q), radius, fp(d2), w.ctypes.data_as(_bp))
    return d2, w


def point_box(P, lo, hi, p, radius):
    lo, hi, p = rows(lo), rows(hi), rows(p)
    g2, w = np.empty(len(p), f32), np.empty(len(p), np.uint8)
    P.neighbour_probe_point_box(len(p), fp(lo), fp(hi), fp(p), radius, fp(g2), w.ctypes.data_as(_bp))
    return g2, w


def box_box(P, lo_s, hi_s, lo_t, hi_t, radius):
    a = [rows(x) for x in (lo_s, hi_s, lo_t, hi_t)]
    g2, w = np.empty(len(a[0]), f32), np.empty(len(a[0]), np.uint8)
    P.neighbour_probe_box_box(len(a[0]), *[fp(x) for x in a], radius, fp(g2), w.ctypes.data_as(_bp))
    return g2, w


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def check_points(P, p, q, radius):
    p, q = rows(p), rows(q)
    with np.errstate(all="ignore"):
        want = ref_d2(p, q)
    d2, w = points(P, p, q, radius)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(d2))
    assert same_bits(d2[~nan], want[~nan])
    assert np.array_equal(w, ref_within(want, radius))
    # symmetric bit for bit
    d2b, wb = points(P, q, p, radius)
    assert same_bits(d2b[~nan], d2[~nan]) and np.array_equal(w, wb)
    # ... and a point is a box of no extent: the same values through both gap routines
    with np.errstate(all="ignore"):
        g2, gw = point_box(P, q, q, p, radius)
        b2, bw = box_box(P, q, q, p, p, radius)
        wantg = ref_gap2(q, q, p, p)
    assert np.array_equal(np.isnan(wantg), np.isnan(g2)) and np.array_equal(np.isnan(wantg), np.isnan(b2))
    ok = ~np.isnan(wantg)
    assert same_bits(g2[ok], wantg[ok]) and same_bits(b2[ok], wantg[ok])
    assert np.array_equal(gw, ref_within(wantg, radius)) and np.array_equal(bw, gw)
    return d2, w


@pytest.mark.parametrize("radius", [1.0, 2.0, 0.5])
def test_ties_on_an_integer_lattice(P, radius):
    # every pair of a 5x5x5 lattice, at unit and at half spacing: d2 is exact, and d2 == r2 happens (it is within reach)
    g = np.array(list(itertools.product(range(5), repeat=3)), f32)
    ties = 0
    for spacing in (1.0, 0.5):
        pts = g * f32(spacing)
        i, j = np.meshgrid(np.arange(len(pts)), np.arange(len(pts)), indexing="ij")
        p, q = pts[i.ravel()], pts[j.ravel()]
        d2, w = check_points(P, p, q, radius)
        r2 = f32(radius) * f32(radius)
        ties += int((d2 == r2).sum())
        assert w[d2 == r2].all() and not w[d2 > r2].any() and w[d2 < r2].all()
    assert ties > 0                                      # (r = 0.5 ties at half spacing only)


def test_radius_zero(P):
    p = np.array([[1, 2, 3], [1, 2, 3], [0, 0, 0], [1e-30, 0, 0], [-0.0, 0.0, -0.0]], f32)
    q = np.array([[1, 2, 3], [1, 2, 3.0000002], [0, 0, 1e-45], [0, 0, 0], [0.0, -0.0, 0.0]], f32)
    d2, w = check_points(P, p, q, 0.0)
    # coincident: within reach; distinct: not -- unless the difference's square underflows to zero (1e-30, the denormal)
    assert list(w) == [1, 0, 1, 1, 1]
    assert P.neighbour_probe_radius2(0.0) == 0.0 and P.neighbour_probe_radius2(-0.0) == 0.0


def test_signed_zeros_and_denormals(P):
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, 3e-23, -3e-23], f32)
    pts = np.array(list(itertools.product(tiny, repeat=3)), f32)
    rng = np.random.default_rng(5)
    a, b = pts[rng.integers(0, len(pts), 4000)], pts[rng.integers(0, len(pts), 4000)]
    for radius in (0.0, 1e-45, 1.1754944e-38, 3e-23, 6e-23, 1e-19):
        check_points(P, a, b, radius)


def test_nan_and_inf_coordinates(P):
    special = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, -3.5, 3.4e38, -3.4e38], f32)
    pts = np.array(list(itertools.product(special, repeat=3)), f32)
    i, j = np.meshgrid(np.arange(len(pts)), np.arange(len(pts)), indexing="ij")
    p, q = pts[i.ravel()], pts[j.ravel()]
    for radius in (0.0, 1.0, 1e19):
        d2, w = check_points(P, p, q, radius)
        bad = ~np.isfinite(p).all(1) | ~np.isfinite(q).all(1)
        assert not w[bad].any()                          # a non-finite coordinate is within nobody's reach
    # boxes with NaN bounds reach nothing, whatever the radius
    nanb = np.full((4, 3), np.nan, f32)
    fin = np.zeros((4, 3), f32)
    for radius in (0.0, 1.0, 1e19):
        assert not box_box(P, nanb, nanb, fin, fin, radius)[1].any()
        assert not box_box(P, fin, fin, nanb, nanb, radius)[1].any()
        assert not point_box(P, nanb, nanb, fin, radius)[1].any()
        one = np.array([[np.nan, 0, 0]], f32)
        z = np.zeros((1, 3), f32)
        assert not box_box(P, z, one, z, z, radius)[1].any()      # a single NaN bound is enough


def random_boxes(rng, n, scale):
    """n boxes: a third of the axes flat (lo == hi), so that boxes flat in one, two and three axes all occur"""
    c = (rng.standard_normal((n, 3)) * scale).astype(f32)
    e = (rng.random((n, 3)) * scale).astype(f32)
    e[rng.random((n, 3)) < 0.34] = 0.0
    lo, hi = c, (c + e).astype(f32)
    return lo, hi


def inside(rng, lo, hi):
    t = rng.random(lo.shape).astype(f32)
    t[rng.random(lo.shape) < 0.2] = 0.0                  # on the faces as well
    t[rng.random(lo.shape) < 0.2] = 1.0
    p = (lo + t * (hi - lo)).astype(f32)
    return np.minimum(np.maximum(p, lo), hi)


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e6])
def test_the_gap_is_a_lower_bound_of_every_distance(P, scale):
    rng = np.random.default_rng(int(scale * 1000) % 9973 + 1)
    n = 120_000
    lo, hi = random_boxes(rng, n, scale)
    flat = (lo == hi).sum(1)
    assert all((flat == k).sum() > 1000 for k in (1, 2, 3))
    p = inside(rng, lo, hi)
    assert ((lo <= p) & (p <= hi)).all()
    # the other point: far, near, and inside the box
    q = (p + rng.standard_normal((n, 3)).astype(f32) * f32(scale) * rng.choice(np.array([0.01, 1.0, 30.0], f32), (n, 1))).astype(f32)
    g2, _ = point_box(P, lo, hi, q, 1.0)
    d2, _ = points(P, p, q, 1.0)
    d2b, _ = points(P, q, p, 1.0)
    assert same_bits(g2, ref_gap2(lo, hi, q, q))
    assert (g2 <= d2).all() and (g2 <= d2b).all()
    assert (g2 > 0).sum() > n // 10 and (g2 == 0).sum() > 100        # both kinds occurred
    assert (g2 == d2).sum() > 10                                      # ... and the bound is attained (nothing to spare)

    # box to box, against every pair of their corners -- and against a point inside each
    lo2, hi2 = random_boxes(rng, n, scale)
    shift = (rng.standard_normal((n, 3)) * scale * 2).astype(f32)
    lo2, hi2 = (lo2 + shift).astype(f32), (hi2 + shift).astype(f32)
    hi2 = np.maximum(hi2, lo2)
    b2, _ = box_box(P, lo, hi, lo2, hi2, 1.0)
    assert same_bits(b2, ref_gap2(lo, hi, lo2, hi2))
    assert same_bits(b2, box_box(P, lo2, hi2, lo, hi, 1.0)[0])       # symmetric bit for bit
    for ca in itertools.product((0, 1), repeat=3):
        a = np.where(np.array(ca, bool), hi, lo)
        for cb in itertools.product((0, 1), repeat=3):
            b = np.where(np.array(cb, bool), hi2, lo2)
            assert (b2 <= ref_d2(a, b)).all()
    pa, pb = inside(rng, lo, hi), inside(rng, lo2, hi2)
    assert (b2 <= points(P, pa, pb, 1.0)[0]).all()
    # ... and the box gap is no larger than the point gap of any point inside the other box (the wave's test is the tighter one)
    assert (b2 <= point_box(P, lo, hi, pb, 1.0)[0]).all()
