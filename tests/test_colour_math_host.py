"""The colour tools as far as they show without a GPU: splat_amd/csrc/splat_colour_math.h, compiled for the HOST by the probe
library (tests/native/colour_math_probe.hip), against the numpy float32 restatements of the header's formulas
(tests/colour_cases.py), bit for bit; the restatement of the colour against oracle.preprocess's rgb, bit for bit; the test
on a colour with its thresholds exactly on sampled colours; and the property the recolour exists for -- the colour of the
mapped coefficients is the mapped colour, from every direction and at every sh_dim -- with a bound derived from the operands.
The device compile of the same text is held to the host compile by tests/test_gpu_colour.py."""
import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
import colour_cases as CC
from helpers import make_camera
from scene_gpu import in_view

f32 = np.float32
K = 4000
H, W = 160, 256


@pytest.fixture(scope="module")
def scene():
    """4000 Gaussians in view with lively higher bands, the camera, and oracle.preprocess's rgb at every sh_dim"""
    g = in_view(K, 6100)
    g.sh[:] = CC.lively_sh(g.sh, 6101)
    cam = make_camera(H, W, (0.3, 0.2, 4.0), 0.2, -0.1)
    rgb = {sd: CC.oracle_rgb(g, cam, sd) for sd in CC.SH_DIMS}
    return g, cam, list(cam.to_c(0.01, 15).cam_pos), rgb


def test_probe_library_is_built():
    CC.probe()


# ---- the colour under a camera -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_dim", CC.SH_DIMS)
def test_the_restatement_is_the_oracles_rgb_bit_for_bit(scene, sh_dim):
    g, cam, cam_pos, rgb = scene
    CC.assert_same_bits(CC.colours_np(g.positions, cam_pos, sh_dim, g.sh), rgb[sh_dim], "sh_dim %d" % sh_dim)
    if sh_dim > 3:                                    # the bands do show: another sh_dim gives other colours
        assert not CC.same_bits(rgb[sh_dim], rgb[3])


@pytest.mark.parametrize("sh_dim", CC.SH_DIMS)
def test_host_compile_of_the_colour_is_the_restatement_bit_for_bit(scene, sh_dim):
    g, cam, cam_pos, rgb = scene
    sp, ss = CC.specials(cam_pos)
    pos, sh = np.concatenate([g.positions[:, :3], sp]), np.concatenate([g.sh, ss])
    got, want = CC.probe_colours(pos, cam_pos, sh_dim, sh), CC.colours_np(pos, cam_pos, sh_dim, sh)
    CC.assert_same_bits(got, want, "sh_dim %d" % sh_dim)
    CC.assert_same_bits(got[:K], rgb[sh_dim], "sh_dim %d against the oracle" % sh_dim)
    # the corners are met: at the camera band 0 alone is finite; an inf or NaN coefficient shows in its channel
    at_cam = got[K]
    assert np.isnan(at_cam).all() if sh_dim > 3 else np.isfinite(at_cam).all()
    assert got[K + 1, 0] == np.inf and np.isnan(got[K + 4, 2])
    assert np.isfinite(got[K + 7]).all()


def test_the_oracle_gives_the_specials_the_same_colours():
    """oracle.preprocess on the special rows themselves (its records hold rgb for every Gaussian, visible or not)"""
    cam = make_camera(H, W)
    cam_pos = list(cam.to_c(0.01, 15).cam_pos)
    sp, ss = CC.specials(cam_pos)
    k = len(sp)
    g = splat_amd.GaussianList(np.concatenate([sp, np.ones((k, 1), f32)], 1), np.full((k, 3), 0.1, f32), np.full(k, 0.5, f32),
                               np.tile(np.array([0, 0, 0, 1], f32), (k, 1)), ss, np.tile(np.eye(3, dtype=f32).ravel() * f32(0.01), (k, 1)))
    for sh_dim in CC.SH_DIMS:
        CC.assert_same_bits(CC.colours_np(sp, cam_pos, sh_dim, ss), CC.oracle_rgb(g, cam, sh_dim), "specials, sh_dim %d" % sh_dim)


# ---- the test on a colour ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.QUERIES))
def test_host_compile_of_the_test_is_the_restatement(scene, name):
    g, cam, cam_pos, rgb = scene
    q = CC.QUERIES[name]
    colours = np.concatenate([rgb[15], CC.colours_np(*CC.specials(cam_pos)[:1], cam_pos, 48, CC.specials(cam_pos)[1])])
    got, want = CC.probe_passes(q, colours), CC.passes_np(q, colours)
    assert np.array_equal(got, want), int((got != want).sum())
    assert 0.02 < want[:K].mean() < 0.98, "the query is meant to pass a part of the scene"


def _u(m, c):
    """u of one colour, operation by operation in float32 scalars (not passes_np's array code)"""
    return [f32(f32(f32(m[k, 0] * c[0]) + f32(m[k, 1] * c[1])) + f32(m[k, 2] * c[2])) + m[k, 3] for k in range(3)]


def test_a_threshold_exactly_on_a_sampled_colour_passes(scene):
    """the box edge, then the ball's radius, placed so that u == 1 and |u|^2 == 1 EXACTLY for chosen rows of the oracle's
    rgb: the inclusive edge must pass, and the first float further out that moves u must fail"""
    g, cam, cam_pos, rgb = scene
    colours = rgb[15]
    rows = [i for i in np.random.default_rng(6110).permutation(K) if (np.abs(colours[i]) < 4).all()][:64]
    # box: row 0 is r + (1 - r), rows 1 and 2 are zero; rows whose 1 - r is not a float32 that gives 1 back are skipped
    hits = 0
    for i in rows:
        c = colours[i]
        m = np.zeros((3, 4), f32)
        m[0, 0], m[0, 3] = 1.0, f32(1.0) - c[0]
        if _u(m, c)[0] != f32(1.0):
            continue
        hits += 1
        out = m.copy()
        for e in range(-23, -16):                     # (the smallest shift of the edge that moves u off 1)
            out[0, 3] = m[0, 3] + f32(2.0 ** e)
            if _u(out, c)[0] > f32(1.0):
                break
        assert _u(out, c)[0] > f32(1.0)
        for shape in ("box", "ellipsoid"):
            for fn in (CC.passes_np, CC.probe_passes):
                assert fn((m, shape, False), colours[i:i + 1])[0], (i, shape, fn.__name__)
                assert not fn((out, shape, False), colours[i:i + 1])[0], (i, shape, fn.__name__)
    assert hits >= 32, hits
    # ball: centred on row j's colour, 1 / radius scanned float by float around 1 / |c_i - c_j| until |u|^2 of row i is 1
    hits = 0
    for i, j in zip(rows[:32], rows[32:]):
        c, centre = colours[i], colours[j].astype(np.float64)
        s0 = f32(1.0 / np.linalg.norm(c.astype(np.float64) - centre))
        found, beyond = None, None
        s = s0
        for _ in range(64):                           # downwards first: a smaller scale brings |u|^2 down
            s = np.nextafter(s, f32(0.0))
        for _ in range(128):
            m = np.concatenate([np.diag([s, s, s]), (-float(s) * centre)[:, None]], 1).astype(f32)
            u = _u(m, c)
            r2 = f32(f32(u[0] * u[0]) + f32(u[1] * u[1])) + f32(u[2] * u[2])
            if r2 == f32(1.0) and found is None:
                found = m
            if r2 > f32(1.0) and found is not None:
                beyond = m
                break
            s = np.nextafter(s, f32(np.inf))
        if found is None or beyond is None:
            continue
        hits += 1
        for fn in (CC.passes_np, CC.probe_passes):
            assert fn((found, "ellipsoid", False), colours[i:i + 1])[0], (i, j, fn.__name__)
            assert not fn((beyond, "ellipsoid", False), colours[i:i + 1])[0], (i, j, fn.__name__)
    assert hits >= 8, hits
    # clamp brings a colour beyond [0, 1] onto the edge of the unit ball, where it passes; unclamped it fails
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32)
    far = np.array([[7.0, 0.0, -3.0]], f32)
    for fn in (CC.passes_np, CC.probe_passes):
        assert fn((eye, "ellipsoid", True), far)[0] and not fn((eye, "ellipsoid", False), far)[0]


@pytest.mark.parametrize("clamp", (True, False))
@pytest.mark.parametrize("shape", ("box", "ellipsoid"))
def test_a_nan_channel_fails(shape, clamp):
    """... also when the map gives that channel no weight in a row of its own: 0 * NaN is NaN"""
    accept_all = np.zeros((3, 4), f32)                # u = 0: everything finite passes
    q = (accept_all, shape, clamp)
    colours = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.nan, 0.5], [0.5, 0.5, np.nan], [np.nan] * 3], f32)
    want = np.array([True, False, False, False, False])
    assert np.array_equal(CC.passes_np(q, colours), want)
    assert np.array_equal(CC.probe_passes(q, colours), want)
    inf = np.array([[np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5]], f32)                # 0 * inf is NaN: fails unless clamped first
    assert np.array_equal(CC.probe_passes(q, inf), np.array([clamp, clamp]))
    assert np.array_equal(CC.passes_np(q, inf), np.array([clamp, clamp]))


# ---- the recolour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.MATRICES))
def test_host_compile_of_the_recolour_is_the_restatement_bit_for_bit(scene, name):
    g, cam, cam_pos, rgb = scene
    m = CC.MATRICES[name]
    sh = np.concatenate([g.sh, CC.specials(cam_pos)[1]])
    CC.assert_same_bits(CC.probe_recolour(m, sh), CC.recolour_np(m, sh), name)


@pytest.mark.parametrize("name", list(CC.MATRICES))
def test_the_offset_is_the_float64_formula_rounded(name):
    m = CC.MATRICES[name].astype(np.float64)
    want = ((m[:, 3] + 0.5 * m[:, :3].sum(1) - 0.5) / float(f32(0.28209479177387814)))
    refused, a, o = CC.probe_map(CC.MATRICES[name])
    assert not refused and CC.same_bits(a, CC.MATRICES[name][:, :3])
    assert CC.same_bits(o, CC.offset_np(CC.MATRICES[name]))
    assert (np.abs(o.astype(np.float64) - want) <= CC.U * np.abs(want) + 1e-15).all(), (o, want)


def test_what_is_not_finite_is_refused():
    m = CC.MATRICES["tinted_contrast"]
    for at, v in ((0, np.nan), (5, np.inf), (11, -np.inf), (3, np.nan)):
        bad = m.copy().ravel()
        bad[at] = v
        assert CC.probe_map(bad)[0], (at, v)
    huge = m.copy()
    huge[1, 3] = f32(3e38)                            # finite, but the offset (t ... ) / C0 is not, in f32
    assert CC.probe_map(huge)[0]
    assert not CC.probe_map(m)[0]


@pytest.mark.parametrize("sh_dim", CC.SH_DIMS)
@pytest.mark.parametrize("name", list(CC.MATRICES))
def test_the_colour_of_the_mapped_coefficients_is_the_mapped_colour(name, sh_dim):
    """oracle.eval_sh (float32) of recolour_np(sh) against A colour64(sh, d) + t (float64, the float32 matrix and directions
    widened) over sh_rotate_cases.spiral().  The bound, per channel i, is derived and not tuned.  With u = 2^-24,
    M_k,i = sum_j |A_ij| |sh_kj| (+ |o_i| for k = 0) the size of a mapped coefficient, Y_k the weight eval_sh gives it and
    Yabs_k that weight with every monomial by its absolute value:
      * a mapped coefficient is 3 products and 2 sums (3 for k = 0), so each term passes through at most 4 roundings:
        5 u M_k,i covers it (gamma_4 to first order, one u of slack), plus 4 subnormal steps for products that underflow;
        carried through the evaluation that is sum_k |Y_k| (5 u M_k,i + 4 tiny);
      * o itself was rounded to float32 once: C0 u |o_i|;
      * the float32 evaluation: a weight is its f32 constant times a polynomial of at most 6 roundings on any path (8 u Yabs_k
        with slack), the term's product and up to 16 sums behind it, the + 0.5 among them (18 u): 27 u (sum_k Yabs_k M_k,i + 0.5)
        covers both and their second-order product.
    Coefficients left as they are miss the bound by orders of magnitude for every matrix but the identity."""
    m = CC.MATRICES[name]
    sh = CC.lively_sh(in_view(200, 6200).sh, 6201 + len(name), scale=0.3)
    d32, d64 = CC.spiral32()
    mapped = CC.recolour_np(m, sh)
    got = np.array([[O.eval_sh(row, sh_dim, d) for d in d32] for row in mapped], np.float64)          # [k, 32, 3]
    want = CC.mapped64(m, CC.colour64(sh, sh_dim, d64))
    A = np.abs(m[:, :3].astype(np.float64))
    o = np.abs(CC.offset_np(m).astype(np.float64))
    M = np.einsum("ij,kcj->kci", A, np.abs(sh.astype(np.float64)).reshape(len(sh), 16, 3))            # [k, 16, 3]
    M[:, 0] += o
    Y, Yabs = np.abs(CC.weights64(d64, sh_dim)), CC.weights_abs64(d64, sh_dim)
    bound = (np.einsum("mc,kci->kmi", Y, 5 * CC.U * M + 4 * CC.TINY) + float(f32(0.28209479177387814)) * CC.U * o
             + 27 * CC.U * (np.einsum("mc,kci->kmi", Yabs, M) + 0.5))
    err = np.abs(got - want)
    print(name, sh_dim, "worst error / bound", float((err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    if name != "identity":
        lazy = np.abs(np.array([[O.eval_sh(row, sh_dim, d) for d in d32[:4]] for row in sh[:50]], np.float64) - want[:50, :4]) / bound[:50, :4]
        print(name, sh_dim, "unmapped: median error / bound", float(np.median(lazy)))
        assert np.median(lazy) > 1e3, float(np.median(lazy))


@pytest.mark.parametrize("name", CC.PERMUTATIONS)
def test_permutations_and_the_identity_reproduce_the_values(scene, name):
    """A holds one 1 a row and t = 0: the offset is exactly 0 and every coefficient is its source plus two signed zeros and,
    in band 0, + 0.0 -- the value moves exactly; a zero comes out with the sign the restatement gives it"""
    g, cam, cam_pos, rgb = scene
    m = CC.MATRICES[name]
    assert np.array_equal(CC.offset_np(m), np.zeros(3, f32))
    sh = g.sh.copy()
    sh[::7, 5] = f32(-0.0)
    got = CC.probe_recolour(m, sh)
    src = np.argmax(m[:, :3], 1)
    want = sh.reshape(-1, 16, 3)[:, :, src].reshape(-1, 48)
    assert np.array_equal(got, want)                  # ==: a -0 may have become +0
    keep = want != 0
    assert keep.mean() > 0.9 and np.array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])
    CC.assert_same_bits(got, CC.recolour_np(m, sh), "zero signs follow the restatement")


# ---- colour_matrix -----------------------------------------------------------------------------------------------------------
def test_colour_matrix_is_its_definition():
    w = np.array([0.2126, 0.7152, 0.0722])
    assert np.array_equal(splat_amd.colour_matrix(), np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32))
    assert splat_amd.colour_matrix().dtype == f32 and splat_amd.colour_matrix().shape == (3, 4)
    grey = splat_amd.colour_matrix(saturation=0)
    assert np.array_equal(grey[:, :3], np.tile(w.astype(f32), (3, 1))) and not grey[:, 3].any()
    for c in ((0.2, 0.7, 0.4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)):                # equal channels, and a grey keeps its level
        out = CC.mapped64(grey, np.array(c))
        assert np.ptp(out) == 0.0 and abs(out[0] - w @ np.array(c)) < 1e-7
    s, tint, c, b = 0.7, np.array([1.1, 0.9, 0.8]), 1.3, -0.05
    A = np.diag(tint) @ (s * np.eye(3) + (1 - s) * np.outer(np.ones(3), w))
    want = np.concatenate([c * A, np.full((3, 1), 0.5 * (1 - c) + b)], 1).astype(f32)
    assert np.array_equal(splat_amd.colour_matrix(saturation=s, tint=tint, contrast=c, brightness=b), want)
    # the order is the stated one: the tint scales what the saturation made, contrast pivots about 0.5, brightness comes last
    assert np.array_equal(splat_amd.colour_matrix(contrast=0)[:, :3], np.zeros((3, 3), f32))
    assert np.array_equal(splat_amd.colour_matrix(contrast=0, brightness=0.1)[:, 3], np.full(3, 0.6, f32))
    assert np.array_equal(splat_amd.colour_matrix(tint=(2, 1, 0.5))[:, :3], np.diag([2, 1, 0.5]).astype(f32))
    with pytest.raises(ValueError):
        splat_amd.colour_matrix(tint=(1, 1))
