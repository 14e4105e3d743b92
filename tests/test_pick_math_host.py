"""The arithmetic of the pick (splat_amd/csrc/splat_pick_math.h), compiled for the HOST behind
tests/native/libpick_math_probe.so and held to numpy and to the oracle bit for bit -- no GPU: the order the keys give (ties,
-0.0 / +0.0, negative depths), the coverage chain against its float32 restatement, and the fragment against the oracle's
fragment_n on the tuples of tests/device_math_cases.fragment_cases (which sit ON the branches of fragment())."""
import ctypes as C
import os

import numpy as np
import pytest

import device_math_cases as DK
import pick_cases as K
from oracle import oracle as O

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "tests", "native", "libpick_math_probe.so")
f32 = np.float32
_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def P():
    L = C.CDLL(LIB)
    L.pick_probe_keys.restype = None
    L.pick_probe_keys.argtypes = [C.c_uint64, _fp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _fp]
    L.pick_probe_fragment.restype = None
    L.pick_probe_fragment.argtypes = [C.c_uint64, _fp, _fp, _fp, C.c_int32, _fp]
    L.pick_probe_chain.restype = None
    L.pick_probe_chain.argtypes = [C.c_uint64, _fp, _fp]
    return L


def fp(a):
    assert a.dtype == f32 and a.flags.c_contiguous
    return a.ctypes.data_as(_fp)


def keys(P, depth, index):
    depth, index = np.ascontiguousarray(depth, f32), np.ascontiguousarray(index, np.uint32)
    k, back = np.empty(len(depth), np.uint64), np.empty(len(depth), f32)
    P.pick_probe_keys(len(depth), fp(depth), index.ctypes.data_as(C.POINTER(C.c_uint32)), k.ctypes.data_as(C.POINTER(C.c_uint64)), fp(back))
    return k, back


def test_descending_keys_are_nearest_first(P):
    rng = np.random.default_rng(7)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 3.4e38, -3.4e38, np.inf, -np.inf, 5.0, 5.0, -5.0, -5.0, 0.0, -0.0], f32)
    depth = np.concatenate([special, rng.normal(0, 4, 4000).astype(f32), np.repeat(rng.normal(0, 4, 500).astype(f32), 3)])
    index = rng.permutation(len(depth)).astype(np.uint32)
    k, back = keys(P, depth, index)
    assert len(np.unique(k)) == len(k)                                   # distinct, because the indices are
    got = np.argsort(k, kind="stable")[::-1]                             # descending key
    want = np.lexsort((-index.astype(np.int64), -depth))                 # descending depth (the zeros tie), then descending index
    assert (got == want).all()
    assert ((k & np.uint64(0xFFFFFFFF)) == index).all()
    # the depth comes back bit for bit, a -0.0 as +0.0
    canon = np.where(depth == 0, f32(0.0), depth)
    assert (back.view(np.uint32) == canon.view(np.uint32)).all()


def test_the_zeros_tie_and_the_index_decides(P):
    k, _ = keys(P, [0.0, -0.0, -0.0, 0.0], [1, 2, 0, 3])
    assert (k >> np.uint64(32) == k[0] >> np.uint64(32)).all()
    assert list(np.argsort(k)[::-1]) == [3, 1, 0, 2]                     # indices 3, 2, 1, 0
    k, _ = keys(P, [-1.0, -2.0, 1.0, 2.0, -0.0], [0, 0, 0, 0, 0])
    assert list(np.argsort(k)[::-1]) == [3, 2, 4, 0, 1]


def chain(P, alpha):
    alpha = np.ascontiguousarray(alpha, f32)
    out = np.empty(len(alpha), f32)
    P.pick_probe_chain(len(alpha), fp(alpha), fp(out))
    return out


def test_the_coverage_chain_bit_for_bit(P):
    rng = np.random.default_rng(11)
    for n in (1, 2, 100, 4096):
        alpha = rng.uniform(1.0 / 255, 0.99, n).astype(f32)
        assert (chain(P, alpha).view(np.uint32) == K.chain(alpha).view(np.uint32)).all()
    alpha = np.full(64, 0.99, f32)
    got = chain(P, alpha)
    assert (got.view(np.uint32) == K.chain(alpha).view(np.uint32)).all()
    assert got[0] == f32(1.0) - (f32(1.0) - f32(0.99)) and (np.diff(got) >= 0).all() and got[-1] == 1.0
    small = np.full(5000, 1.0 / 255, f32)                                # a long chain: 1 - T rounds to 1 once T is below 2^-25
    got = chain(P, small)
    assert (got.view(np.uint32) == K.chain(small).view(np.uint32)).all() and got[100] < 1.0 and got[-1] == 1.0


@pytest.mark.parametrize("y_up", (1, 0))
def test_the_fragment_is_the_oracles(P, y_up):
    sxy, ra, rb = DK.fragment_cases(1 << 18)
    want, cov = O.fragment_n(sxy, ra, rb)
    shares = DK.fragment_branch_shares(sxy, ra, rb, want, cov)
    assert min(shares.values()) >= 0.01, shares                          # every branch of fragment() is populated
    if not y_up:
        # y down, dy = sy - cy: with the sample's and the centre's y exchanged that is the oracle's cy - sy, the same
        # operation on the same operands, so the same tuples serve and the reference stands
        sxy, ra = sxy.copy(), ra.copy()
        sxy[:, 1], ra[:, 1] = ra[:, 1].copy(), sxy[:, 1].copy()
    got = np.empty(len(sxy), f32)
    P.pick_probe_fragment(len(sxy), fp(sxy), fp(ra), fp(rb), y_up, fp(got))
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, sxy[bad[0]], ra[bad[0]], rb[bad[0]], got[bad[0]], want[bad[0]])
    assert (got == DK.T255).sum() > 50 and (got == f32(0.99)).sum() > 50 and (got == 0).sum() > 50
