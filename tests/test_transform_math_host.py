"""The affine map of one Gaussian (transform_point and transform_cov3d of splat_amd/csrc/splat_transform_math.h), compiled
for the HOST by the probe library (tests/native/transform_math_probe.hip), against the numpy float32 restatement of the
header's formulas (tests/transform_cases.py), bit for bit -- no GPU needed.  The device compile of the same text is held to
the host compile by tests/test_gpu_scene_read.py, and the kernels to the restatement by tests/test_gpu_scene_transform.py.
The restatement itself is checked against float64 A S A^T with a bound derived from the operands, which a transposed
index would miss by orders of magnitude."""
import numpy as np
import pytest

import transform_cases as T

f32 = np.float32
K = 4000
U = 2.0 ** -24                                       # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -149                                   # the smallest subnormal: the absolute error of an underflowing operation


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def test_probe_library_is_built():
    T.probe()


@pytest.mark.parametrize("name", list(T.MATRICES))
def test_host_compile_is_the_restatement_bit_for_bit(name):
    m = T.MATRICES[name]
    pos, cov = T.random_gaussians(K, 7 + len(name))
    got_p, got_c = T.run_probe(m, pos, cov)
    want_p, want_c = T.transform_np(m, pos, cov)
    assert same_bits(got_p, want_p), "%s: %d position words differ" % (name, int((got_p.view(np.uint32) != want_p.view(np.uint32)).sum()))
    assert same_bits(got_c, want_c), "%s: %d covariance words differ" % (name, int((got_c.view(np.uint32) != want_c.view(np.uint32)).sum()))


def test_identity_gives_the_values_back():
    pos, cov = T.random_gaussians(K, 3)
    got_p, got_c = T.run_probe(T.MATRICES["identity"], pos, cov)
    assert np.array_equal(got_p, pos) and np.array_equal(got_c, cov)      # ==: a -0 may have become +0
    want_p, want_c = T.transform_np(T.MATRICES["identity"], pos, cov)
    assert same_bits(got_p, want_p) and same_bits(got_c, want_c)


def test_zero_matrix_gives_zeros():
    pos, cov = T.random_gaussians(K, 4)
    got_p, got_c = T.run_probe(T.MATRICES["zero"], pos, cov)
    assert not got_p.any() and not got_c.any()


@pytest.mark.parametrize("name", list(T.MATRICES))
def test_the_restatement_is_a_sigma_a_transposed(name):
    """Loose, against float64.  Every entry of S' is a sum of nine triple products A(r,k) S(k,l) A(c,l); each passes through
    at most six float32 roundings on its way (product, two sums, product, two sums), so the result is within
    gamma_6 = 6u / (1 - 6u) of the sum of their magnitudes (Higham, Accuracy and Stability, lemma 3.1), plus one smallest
    subnormal for each of the 30 operations that may underflow.  8u stands for gamma_6.  The centre: three products and
    three sums, at most four roundings on any path: 5u of the magnitudes' sum."""
    m = T.MATRICES[name]
    pos, cov = T.random_gaussians(K, 11 + len(name))
    got_p, got_c = T.transform_np(m, pos, cov)
    A = m[:, :3].astype(np.float64)
    t = m[:, 3].astype(np.float64)
    S = cov.astype(np.float64).reshape(K, 3, 3).transpose(0, 2, 1)          # S[i, r, c] = cov[i, 3c + r]
    want_c = np.einsum("rk,ikl,cl->irc", A, S, A)
    mag_c = np.einsum("rk,ikl,cl->irc", np.abs(A), np.abs(S), np.abs(A))
    got_S = got_c.astype(np.float64).reshape(K, 3, 3).transpose(0, 2, 1)
    assert (np.abs(got_S - want_c) <= 8 * U * mag_c + 30 * TINY).all(), float(np.abs(got_S - want_c).max())
    P = pos.astype(np.float64)
    want_p = P @ A.T + t
    mag_p = np.abs(P) @ np.abs(A).T + np.abs(t)
    assert (np.abs(got_p.astype(np.float64) - want_p) <= 5 * U * mag_p + 7 * TINY).all()
    if name in ("rotation", "shear"):                                     # the bound does tell a transposed index apart
        wrong = np.einsum("kr,ikl,cl->irc", A, S, A)
        assert (np.abs(wrong - want_c) > 8 * U * mag_c + 30 * TINY).mean() > 0.5
