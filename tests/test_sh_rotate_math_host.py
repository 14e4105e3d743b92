"""The sh rotation as far as it shows without a GPU: the blocks of splat_sh_rotation_blocks against numpy's float64
least-squares blocks, and rotate_sh_bands of splat_amd/csrc/splat_sh_math.h, compiled for the HOST by the probe library
(tests/native/sh_rotate_probe.hip), against the numpy float32 restatement of the header's formula (tests/sh_rotate_cases.py),
bit for bit.  The restatement itself is held to the float64 product with a bound derived from the operands, and to the
property the feature exists for: eval_sh of the rotated coefficients at R d is eval_sh of the original ones at d.  The
device compile of the same text is held to the host compile by tests/test_gpu_sh_rotate.py."""
import ctypes as C

import numpy as np
import pytest

import sh_rotate_cases as S
from splat_amd import _lib

f32 = np.float32
K = 4000
NAMES = list(S.ROTATIONS)


def test_probe_library_is_built():
    S.probe()


# ---- the blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_blocks_are_numpys_float64_blocks_rounded(name):
    """the snap moves an entry by at most 2^-41, the rounding to float32 by at most 2^-24 of it"""
    got, want = S.lib_blocks(S.ROTATIONS[name]), S.blocks_f64(S.ROTATIONS[name])
    for n, g, w in zip((3, 5, 7), got, want):
        assert g.shape == (n, n) and g.dtype == f32
        err = np.abs(g.astype(np.float64) - w)
        print(name, n, "worst error / bound", float((err / (S.U * np.abs(w) + 2.0 ** -40)).max()))
        assert (err <= S.U * np.abs(w) + 2.0 ** -40).all(), (name, n, float(err.max()))


def test_band_one_is_the_rotation_in_the_basis_order():
    """D_1 = P R P^T with P the map (x, y, z) -> (-y, z, -x): band 1's functions are -y, z, -x times one constant"""
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    for name in NAMES:
        R = S.as_seen(S.ROTATIONS[name])
        assert np.abs(S.lib_blocks(S.ROTATIONS[name])[0].astype(np.float64) - P @ R @ P.T).max() <= 2.0 ** -23, name


@pytest.mark.parametrize("name", S.PERMUTATIONS)
def test_axis_aligned_maps_give_exact_signed_permutations(name):
    for D in S.lib_blocks(S.ROTATIONS[name]):
        assert np.isin(D, (-1.0, 0.0, 1.0)).all(), (name, D)
        assert (np.abs(D).sum(0) == 1).all() and (np.abs(D).sum(1) == 1).all(), (name, D)
        if name == "identity":
            assert np.array_equal(D, np.eye(len(D), dtype=f32))


def test_blocks_compose():
    R1, R2 = S.ROTATIONS["rot20"], S.ROTATIONS["rot173"]
    for A, B in ((R1, R2), (R2, R1), (R1, S.ROTATIONS["mirror_x"]), (S.ROTATIONS["quarter_z"], R2)):
        for dab, da, db in zip(S.lib_blocks(A @ B), S.lib_blocks(A), S.lib_blocks(B)):
            err = np.abs(dab.astype(np.float64) - da.astype(np.float64) @ db.astype(np.float64)).max()
            print("composition", len(dab), float(err))
            assert err <= 1e-6, float(err)


def test_what_is_not_orthogonal_is_refused_and_nothing_is_written():
    L = _lib.lib()
    fp = C.POINTER(C.c_float)
    R = S.ROTATIONS["rot20"]
    shear = np.array([[1.0, 0.25, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = R.copy()
    nan[1, 2] = np.nan
    inf = R.copy()
    inf[0, 0] = np.inf
    for what, r in (("1.01 R", 1.01 * R), ("shear", shear), ("nan", nan), ("inf", inf), ("zero", np.zeros((3, 3)))):
        r = np.ascontiguousarray(r, f32).reshape(9)
        d = [np.full(n * n, -7.5, f32) for n in (3, 5, 7)]
        assert L.splat_sh_rotation_blocks(r.ctypes.data_as(fp), *[a.ctypes.data_as(fp) for a in d]) == _lib.ERR_INVALID, what
        assert all((a == f32(-7.5)).all() for a in d), what
        assert L.splat_last_error(None), what
        with pytest.raises(ValueError):
            S.lib_blocks(r)
    # ... a NULL pointer, in any place
    r = np.ascontiguousarray(R, f32).reshape(9)
    d = [np.full(n * n, -7.5, f32) for n in (3, 5, 7)]
    for hole in range(4):
        args = [r.ctypes.data_as(fp)] + [a.ctypes.data_as(fp) for a in d]
        args[hole] = None
        assert L.splat_sh_rotation_blocks(*args) == _lib.ERR_INVALID, hole
        assert all((a == f32(-7.5)).all() for a in d), hole
    # ... and what is orthogonal to float32 accuracy, a reflection included, is served
    assert L.splat_sh_rotation_blocks(r.ctypes.data_as(fp), *[a.ctypes.data_as(fp) for a in d]) == _lib.SPLAT_OK
    S.lib_blocks(-np.eye(3))
    with pytest.raises(ValueError):
        S.lib_blocks(np.eye(4))


# ---- one Gaussian -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_compile_is_the_restatement_bit_for_bit(name):
    blocks = S.lib_blocks(S.ROTATIONS[name])
    sh = S.random_sh(K, 20 + len(name))
    got, want = S.run_probe(blocks, sh), S.rotate_np(blocks, sh)
    assert S.same_bits(got, want), "%s: %d words differ" % (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert S.same_bits(got[:, :3], sh[:, :3])


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_the_float64_product(name):
    """per coefficient within (n + 3) u sum_k |D(m,k)| |c_k| + n 2^-149 (sh_rotate_cases.coefficient_bound) of the float64
    product with numpy's blocks, snapped as the library's definition snaps them (how far the snap moves an entry is held by
    test_blocks_are_numpys_float64_blocks_rounded)"""
    R = S.ROTATIONS[name]
    sh = S.random_sh(K, 40 + len(name))
    D64 = S.blocks_f64(R, snapped=True)
    got = S.rotate_np(S.lib_blocks(R), sh).astype(np.float64)
    err, bound = np.abs(got - S.product_f64(D64, sh)), S.coefficient_bound(D64, sh)
    print(name, "worst error / bound", float((err[:, 3:] / bound[:, 3:]).max()))
    assert (err <= bound).all(), float((err[:, 3:] / bound[:, 3:]).max())
    if name in ("rot20", "rot173"):                  # the bound does tell a transposed block apart
        wrong = np.abs(S.product_f64([D.T for D in D64], sh) - S.product_f64(D64, sh))
        assert (wrong[:, 3:] > bound[:, 3:]).mean() > 0.5


@pytest.mark.parametrize("name", NAMES)
def test_the_rotated_colour_at_the_rotated_direction_is_the_colour(name):
    """eval_sh, in float64, of the rotated float32 coefficients at R d against the original coefficients at d, for 64
    directions: within sum_m |Y_m(R d)| bound_m, the coefficients' own bound carried through the evaluation.  Coefficients
    left as they are miss that bound by orders of magnitude, so a rotation that does nothing cannot pass."""
    R = S.ROTATIONS[name]
    sh = S.random_sh(400, 60 + len(name))
    d = S.spiral(64)
    Rd = d @ S.as_seen(R).T
    rot = S.rotate_np(S.lib_blocks(R), sh)
    want = S.eval_sh64(sh, d)                                                # [k, 64, 3]
    bound = np.einsum("mk,ikc->imc", np.abs(S.basis(Rd)), S.coefficient_bound(S.blocks_f64(R), sh).reshape(len(sh), 16, 3)[:, 1:])
    err = np.abs(S.eval_sh64(rot, Rd) - want)
    print(name, "worst error / bound", float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    if name != "identity":
        lazy = np.abs(S.eval_sh64(sh, Rd) - want) / bound
        print(name, "unrotated: median error / bound", float(np.median(lazy)))
        assert np.median(lazy) > 1e3, float(np.median(lazy))


def test_identity_gives_the_values_back():
    sh = S.random_sh(K, 5)
    got = S.run_probe(S.lib_blocks(np.eye(3)), sh)
    assert (np.signbit(sh) & (sh == 0)).any()
    assert np.array_equal(got, sh)                                           # ==: a -0 may have become +0


def test_four_quarter_turns_give_the_original_bits_back():
    """a signed permutation moves each value exactly and adds zeros to it, so every coefficient that is not zero comes back
    with its bits; a zero comes back a zero, with the sign the zero products around it leave (0 * c is -0 for c < 0)"""
    sh = S.random_sh(K, 6)
    blocks = S.lib_blocks(S.ROTATIONS["quarter_z"])
    got = sh
    for turn in range(4):
        got = S.run_probe(blocks, got)
        assert (turn == 3) == np.array_equal(got[:, 3:], sh[:, 3:]), turn
    assert np.array_equal(got, sh)
    keep = sh != 0
    assert keep.mean() > 0.9 and np.array_equal(got.view(np.uint32)[keep], sh.view(np.uint32)[keep])
    # ... also without a zero anywhere: the whole array, bit for bit
    full = np.where(sh == 0, f32(0.25), sh)
    got = full
    for turn in range(4):
        got = S.run_probe(blocks, got)
    assert S.same_bits(got, full)
