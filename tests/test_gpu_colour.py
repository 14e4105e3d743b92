"""The colour tools on the GPU (splat_eval_colours_device, splat_select_colour_device, splat_recolour_scene_device,
splat_recolour_gaussians_device, -m gpu).  The colours are oracle.preprocess's rgb bit for bit (a NaN equal to a NaN), whole
and by index, also after every kind of edit; a selection's bytes and count are the numpy restatement's on the oracle's rgb,
combined by the op; the sh values after a recolour are the numpy float32 restatement's (tests/colour_cases.py, in original
index order) bit for bit, everything else keeps its bits, the order and the block bounds stay, and the frames are those of a
FRESH Renderer that takes the restated arrays through splat_upload_scene.  Nothing here has a tolerance.  Scenes and targets
are those of tests/scene_gpu.py (n in 1, 255, 256, 257, 1000)."""
import functools
import math

import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import make_camera, oracle_camera, scene_dict
import append_cases as AC
import colour_cases as CC
import remove_cases as RC
import transform_cases as T
from scene_gpu import (SENTINEL, SIZES, TARGETS, assert_bounds, assert_resident, assert_same_bits, assert_same_frames, copy_of, frame,
                       frames, fresh_upload, in_view, index_sets, session)
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2
K = 4000
GUARD = 64                                           # sentinel bytes in front of and behind every output buffer
NAMES = list(CC.MATRICES)


@functools.lru_cache(maxsize=None)
def lively(n, seed):
    """made once and shared: no test writes into what this returns.  A synthetic scene in view with sh rows at magnitudes of
    their own in every band, so that the bands and a recolour show"""
    g = in_view(n, seed)
    g.sh[:] = CC.lively_sh(g.sh, seed + 1)
    return g


def poses(h, w):
    """in front of the scene, and INSIDE it: from there the directions point every way"""
    return [make_camera(h, w), make_camera(h, w, (0.3, 0.2, 0.4), 1.0, -0.2)]


def recoloured(g, m, rows=None):
    """g with the sh of the rows named (all: None) recoloured, restated on the host"""
    out = copy_of(g)
    out.sh[:] = CC.recoloured_rows(m, g.sh, rows)
    return out


def guarded(s, nbytes):
    """a device buffer of nbytes between two guards, every byte the sentinel: (address of the buffer, check)"""
    base = s.alloc(nbytes + 2 * GUARD, SENTINEL)

    def fetch(shape, dtype=f32):
        raw = s.fetch(base, (nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + nbytes:] == SENTINEL).all(), "a guard byte was written"
        return raw[GUARD:GUARD + nbytes].view(dtype).reshape(shape).copy()

    return base + GUARD, fetch


def with_duplicates(n, seed):
    """index_sets plus one set that names Gaussians twice, in any order (k <= n)"""
    sets = index_sets(n, seed)
    sets.append(np.random.default_rng(seed + 1).integers(0, n, min(n, 300)).astype(np.uint32))
    return sets


def assert_colours(s, g, cam, sh_dim, seed, what):
    """R.colours of the resident scene, whole and by index, is oracle.preprocess's rgb of g"""
    n = len(g)
    want = CC.oracle_rgb(g, cam, sh_dim)
    cam_c = cam.to_c(0.01, sh_dim)
    out, fetch = guarded(s, 12 * n)
    assert s.R.colours(cam_c, out=out) == out
    CC.assert_same_bits(fetch((n, 3)), want, what + " whole")
    CC.assert_same_bits(s.R.colours(cam_c), want, what + " whole, downloaded")
    for idx in with_duplicates(n, seed):
        k = len(idx)
        out, fetch = guarded(s, 12 * k)
        s.R.colours(cam_c, s.array(idx) if k else 0, out=out, k=k)
        CC.assert_same_bits(fetch((k, 3)), want[idx.astype(np.int64)], "%s k=%d" % (what, k))
    return want


# ---- the device compile of splat_colour_math.h ---------------------------------------------------------------------------------
def test_device_compile_equals_host_compile():
    g = lively(K, 7000)
    cam_pos = list(make_camera(160, 256, (0.3, 0.2, 4.0), 0.2, -0.1).to_c(0.01, 15).cam_pos)
    sp, ss = CC.specials(cam_pos)
    pos, sh = np.concatenate([g.positions[:, :3], sp]), np.concatenate([g.sh, ss])
    for sh_dim in CC.SH_DIMS:
        host, dev = CC.probe_colours(pos, cam_pos, sh_dim, sh), CC.probe_colours(pos, cam_pos, sh_dim, sh, device=True)
        CC.assert_same_bits(dev, host, "colour, sh_dim %d" % sh_dim)
    colours = CC.probe_colours(pos, cam_pos, 48, sh)
    for name, q in CC.QUERIES.items():
        host, dev = CC.probe_passes(q, colours), CC.probe_passes(q, colours, device=True)
        assert np.array_equal(host, dev), name
        assert 0.02 < host.mean() < 0.98, name
    for name, m in CC.MATRICES.items():
        CC.assert_same_bits(CC.probe_recolour(m, sh, device=True), CC.probe_recolour(m, sh), "recolour " + name)


# ---- colours -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sh_dim", CC.SH_DIMS)
def test_colours_whole_and_by_index(sh_dim, n):
    g = lively(n, 7100 + n)
    h, w = TARGETS[0]
    with session() as s:
        s.R.upload(g)
        held = s.R.device_bytes()[0]
        for p, cam in enumerate(poses(h, w)):
            assert_colours(s, g, cam, sh_dim, 7150 + n, "n=%d sh_dim=%d pose %d" % (n, sh_dim, p))
        assert s.R.frames_dropped() == 0
        assert s.R.device_bytes()[0] >= held           # (the guarded buffers are this context's; the inverse order stays)


def test_colours_of_hostile_rows():
    """the special rows resident: a Gaussian at the camera, +-inf and NaN coefficients, signed zeros, subnormals -- the NaNs
    come back as NaNs, not as K1's +-FLT_MAX"""
    h, w = TARGETS[0]
    cam = make_camera(h, w)
    sp, ss = CC.specials(list(cam.to_c(0.01, 15).cam_pos))
    k = len(sp)
    g = splat_amd.GaussianList(np.concatenate([sp, np.ones((k, 1), f32)], 1), np.full((k, 3), 0.1, f32), np.full(k, 0.5, f32),
                               np.tile(np.array([0, 0, 0, 1], f32), (k, 1)), ss, np.tile(np.eye(3, dtype=f32).ravel() * f32(0.01), (k, 1)))
    with session() as s:
        s.R.upload(g)
        for sh_dim in CC.SH_DIMS:
            want = assert_colours(s, g, cam, sh_dim, 7190, "specials sh_dim=%d" % sh_dim)
            assert np.isnan(want).any() and np.isinf(want).any()


@pytest.mark.parametrize("sh_dim", (15, 48))
def test_colours_after_every_kind_of_edit(sh_dim):
    """an indexed transform (the order goes stale), an update_indexed of sh, a remove and an append (another n: another plane
    stride) and a reorder (another order and inverse): the colours are the oracle's for the model after each"""
    n, (h, w) = 1000, TARGETS[0]
    cam = poses(h, w)[1]
    E = copy_of(lively(n, 7200))
    rng = np.random.default_rng(7201)
    with session() as s:
        R = s.R
        R.upload(E)
        assert_colours(s, E, cam, sh_dim, 7210, "uploaded")
        rows = rng.permutation(n)[:300].astype(np.uint32)
        m = T.MATRICES["rotation"]
        R.transform(m, s.array(rows), k=len(rows))
        pos, cov = T.transformed(E, m, rows)
        E = copy_of(E, pos, cov)
        assert_colours(s, E, cam, sh_dim, 7211, "after an indexed transform")
        rows = rng.permutation(n)[:200].astype(np.uint32)
        new_sh = CC.lively_sh(E.sh[rows.astype(np.int64)], 7202)
        R.update_indexed(s.array(rows), sh=s.array(new_sh), k=len(rows))
        E.sh[rows.astype(np.int64)] = new_sh
        assert_colours(s, E, cam, sh_dim, 7212, "after update_indexed of sh")
        gone = rng.random(n) < 0.3
        assert R.remove(s.array(gone.astype(np.uint8)), n=n) == int((~gone).sum())
        E, _ = RC.removed(E, gone)
        assert_colours(s, E, cam, sh_dim, 7213, "after a remove")
        extra = lively(257, 7203)
        assert R.append(s.device(extra)) == len(E) + 257
        E = AC.appended(E, extra)
        assert_colours(s, E, cam, sh_dim, 7214, "after an append")
        R.reorder()
        assert_colours(s, E, cam, sh_dim, 7215, "after a reorder")
        assert_resident(s, E, "the model at the end")


# ---- select_colour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_select_colour_every_query_and_op(n):
    g = lively(n, 7300 + n)
    h, w = TARGETS[0]
    cam = poses(h, w)[0]
    cam_c = cam.to_c(0.01, 15)
    rgb = CC.oracle_rgb(g, cam, 15)
    start = np.random.default_rng(7350 + n).choice(np.array([0, 1, 7], np.uint8), n)
    passed_any = False
    with session() as s:
        s.R.upload(g)
        for name, (m, shape, clamp) in CC.QUERIES.items():
            passed = CC.passes_np((m, shape, clamp), rgb)
            passed_any |= bool(passed.any())
            for op in CC.OPS:
                what = "%s %s n=%d" % (name, op, n)
                sel, fetch = guarded(s, n)
                s.R._check(s.R._L.splat_device_upload(s.R._h, sel, start.ctypes.data, n))
                count = s.R.select_colour(cam_c, sel, matrix=m, shape=shape, clamp=clamp, op=op)
                got = fetch((n,), np.uint8)
                want, selected = CC.combine(op, start, passed)
                assert np.array_equal(got, want), what
                assert count == int(selected.sum()), what
                if op in ("set", "intersect"):
                    assert np.isin(got, (0, 1)).all(), what
                else:                                  # what does not pass keeps its byte, a 7 included; what passes is 0 or 1
                    assert np.array_equal(got[~passed], start[~passed]) and np.isin(got[passed], (0, 1)).all(), what
    assert passed_any or n == 1


def test_select_colour_by_rgb_and_tolerance_is_the_ball_around_a_picked_colour():
    """the wand: the colour of one Gaussian, then everything within a tolerance of it -- the map the Renderer builds is
    colour_cases.ball's, scalar and per channel"""
    n, (h, w) = 1000, TARGETS[0]
    g = lively(n, 7400)
    cam = poses(h, w)[0]
    cam_c = cam.to_c(0.01, 15)
    rgb = CC.oracle_rgb(g, cam, 15)
    with session() as s:
        s.R.upload(g)
        i = int(np.argmin(np.abs(rgb - 0.5).sum(1)))
        picked = s.R.colours(cam_c, [i])[0]
        CC.assert_same_bits(picked, rgb[i], "the picked colour")
        for tol, shape in ((0.3, "ellipsoid"), ((0.3, 0.2, 0.4), "box"), ((0.25, 0.3, 0.2), "ellipsoid")):
            sel, fetch = guarded(s, n)
            count = s.R.select_colour(cam_c, sel, rgb=picked, tolerance=tol, shape=shape)
            want = CC.passes_np((CC.ball(picked, tol), shape, True), rgb)
            assert np.array_equal(fetch((n,), np.uint8), want.astype(np.uint8)), (tol, shape)
            assert count == int(want.sum()) and want[i] and 1 < count < n, (tol, shape, count)


def test_select_colour_into_a_torch_bool_selection_made_on_a_side_stream():
    import torch
    n, (h, w) = 1000, TARGETS[0]
    g = lively(n, 7500)
    cam = poses(h, w)[1]
    q = CC.QUERIES["box_raw"]
    passed = CC.passes_np(q, CC.oracle_rgb(g, cam, 48))
    with session() as s:
        s.R.upload(g)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            sel = (torch.arange(n, device=dev) % 3) == 0          # torch.bool, written on the side stream
            count = s.R.select_colour(cam.to_c(0.01, 48), sel, matrix=q[0], shape=q[1], clamp=q[2], op="subtract")
        old = (np.arange(n) % 3) == 0
        assert sel.dtype == torch.bool and np.array_equal(sel.cpu().numpy(), old & ~passed)
        assert count == int((old & ~passed).sum()) and 0 < count < int(old.sum())
        del sel


def test_the_queries_are_reads_retention_goes_on():
    n, (h, w) = 1000, TARGETS[1]
    g = lively(n, 7600)
    cam = make_camera(h, w)
    cam_c = cam.to_c(0.01, 15)
    with session() as s:
        R = s.R
        R.upload(g)
        img = R.host_image(h, w)

        def rest_frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam_c, img)
            return img.copy()

        rest = [rest_frame() for _ in range(STILL + 4)]
        retained = R.frames_retained()
        assert retained > 0 and rest[0].any()
        sel, out, idx = s.alloc(n), s.alloc(12 * n), s.array(np.arange(0, n, 3, dtype=np.uint32))
        R.colours(cam_c, idx, out=out, k=len(range(0, n, 3)))      # (makes the inverse order: device memory grows once, here)
        held = R.device_bytes()[0]
        for step in range(3):
            R.colours(cam_c, out=out)
            R.colours(cam_c, idx, out=out, k=len(range(0, n, 3)))
            assert R.select_colour(cam_c, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.3) > 0
            assert R.device_bytes()[0] == held, "temporaries live for the call"
            # nothing of the frame-to-frame state went: the very next frame at rest is a retained one, and the same frame
            assert np.array_equal(rest_frame(), rest[0])
            assert R.frames_retained() > retained
            retained = R.frames_retained()
        assert R.frames_dropped() == 0


# ---- recolour ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_recolour_whole_and_by_index(name, n):
    m = CC.MATRICES[name]
    A = lively(n, 7700 + n)
    E = A
    with session() as s:
        s.R.upload(A)
        orig_a, bounds_a = s.R.scene_layout()
        first = frames(s.R)
        for idx in [None] + index_sets(n, 7750 + n):
            what = "%s n=%d %s" % (name, n, "whole" if idx is None else "k=%d" % len(idx))
            if idx is None:
                s.R.recolour(m)
            else:
                s.R.recolour(m, s.array(idx) if len(idx) else 0, k=len(idx))
            E = recoloured(E, m, idx)
            # sh of the chosen rows is the restatement's; the other rows and every other field keep their bits
            assert_resident(s, E, what)
            orig, bounds = s.R.scene_layout()
            assert np.array_equal(orig, orig_a), what
            assert_bounds(bounds, bounds_a, what)
            with fresh_upload(E) as ref:
                got = frames(s.R)
                assert_same_frames(got, frames(ref), what)
            if name == "identity":
                assert np.array_equal(E.sh, A.sh)                     # ==: a -0 may be +0 now
                assert_same_frames(got, first, what)
        if n >= 255 and name != "identity":
            assert any(not np.array_equal(a, b) for a, b in zip(got, first)), "the recolour is meant to show in the frames"


def test_recolour_takes_host_indices_and_a_torch_tensor_on_a_side_stream():
    import torch
    n = 1000
    m = CC.MATRICES["tinted_contrast"]
    A = lively(n, 7800)
    rows = np.arange(0, n, 7)
    E = recoloured(A, m, rows)
    E2 = recoloured(E, CC.MATRICES["grey"], [3, 999, 17])
    with session() as s, fresh_upload(E2) as ref:
        s.R.upload(A)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            idx = torch.arange(0, n, 7, dtype=torch.int32, device=dev)
            s.R.recolour(m.ravel().tolist(), idx)                # twelve numbers; k and the stream from the tensor
        assert_resident(s, E, "torch index on a side stream")
        s.R.recolour(splat_amd.colour_matrix(saturation=0), [3, 999, 17])       # a host list
        assert_resident(s, E2, "host indices")
        assert_same_frames(frames(s.R), frames(ref), "host indices")
        del idx


def test_an_index_out_of_range_applies_and_writes_nothing():
    n, (h, w) = 1000, TARGETS[0]
    A = lively(n, 7900)
    cam_c = make_camera(h, w).to_c(0.01, 15)
    with session() as s:
        s.R.upload(A)
        before, layout = frames(s.R), s.R.scene_layout()
        idx = np.arange(100, dtype=np.uint32)
        idx[57] = n                                   # the first index that names no Gaussian
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.recolour(CC.MATRICES["negative"], s.array(idx), k=len(idx))
        assert e.value.code == _lib.ERR_INVALID
        out, fetch = guarded(s, 12 * len(idx))
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.colours(cam_c, s.array(idx), out=out, k=len(idx))
        assert e.value.code == _lib.ERR_INVALID
        assert (fetch((len(idx) * 12,), np.uint8) == SENTINEL).all(), "nothing was written"
        for k, index in ((n + 1, s.alloc(4 * (n + 1), 0)), (n - 1, 0)):          # more rows than Gaussians; a whole read of another size
            with pytest.raises(splat_amd.SplatError) as e:
                s.R._check(s.R._L.splat_eval_colours_device(s.R._h, cam_c, k, index or None, s.alloc(12 * (n + 1)), None))
            assert e.value.code == _lib.ERR_INVALID
        assert_resident(s, A, "after the refused calls")
        after = s.R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert_bounds(after[1], layout[1], "after the refused calls")
        assert_same_frames(frames(s.R), before, "after the refused calls")


def test_a_matrix_that_is_not_finite_is_refused_and_retention_goes_on():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(n, 8000)
    idx = np.arange(0, n, 3, dtype=np.uint32)
    cam = make_camera(h, w).to_c(0.01, 15)
    nan, inf, huge = [CC.MATRICES["tinted_contrast"].copy() for _ in range(3)]
    nan[1, 2], inf[0, 3], huge[2, 3] = np.nan, np.inf, 3e38
    with session() as s:
        R = s.R
        R.upload(A)
        img = R.host_image(h, w)

        def rest_frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam, img)
            return img.copy()

        rest = [rest_frame() for _ in range(STILL + 4)]
        retained = R.frames_retained()
        assert retained > 0 and rest[0].any()
        d_idx = s.array(idx)
        for bad in (nan, inf, huge):
            with pytest.raises(splat_amd.SplatError) as e:
                R.recolour(bad)
            assert e.value.code == _lib.ERR_INVALID
            with pytest.raises(splat_amd.SplatError) as e:
                R.recolour(bad, d_idx, k=len(idx))
            assert e.value.code == _lib.ERR_INVALID
        # nothing of the frame-to-frame state went: the very next frame at rest is a retained one (after an edit it is binned)
        assert np.array_equal(rest_frame(), rest[0])
        assert R.frames_retained() > retained
        assert_resident(s, A, "after the refused matrices")


def test_a_recolour_at_rest_ends_retention_and_retention_starts_over():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(n, 8100)
    idx = np.random.default_rng(8101).permutation(n)[:300].astype(np.uint32)
    m = CC.MATRICES["negative"]
    E = recoloured(A, m, idx)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s, fresh_upload(E) as ref:
        R = s.R
        R.upload(A)
        img = R.host_image(h, w)

        def rest_frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam, img)
            return img.copy()

        rest = [rest_frame() for _ in range(STILL + 4)]
        retained = R.frames_retained()
        assert retained > 0 and rest[0].any()
        R.recolour(m, s.array(idx), k=len(idx))
        want = frame(ref, make_camera(h, w), h, w)
        assert not np.array_equal(want, rest[0]), "the recolour is meant to change the frame"
        assert np.array_equal(rest_frame(), want)
        assert R.frames_retained() == retained, "the frame after an edit is binned, not retained"
        more = [rest_frame() for _ in range(STILL + 4)]
        assert all(np.array_equal(f, want) for f in more)
        assert R.frames_retained() > retained and R.frames_dropped() == 0


def test_libm_exp_mode_is_the_oracle_frame_of_the_restated_arrays():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(n, 8200)
    idx = np.random.default_rng(8201).permutation(n)[:300].astype(np.uint32)
    m = CC.MATRICES["tinted_contrast"]
    E = recoloured(recoloured(A, m, idx), CC.MATRICES["swap"])
    cam = make_camera(h, w)

    def frame48(R):                                   # sh_dim = 48: all four bands are evaluated (15, the other frames', stops at band 2)
        img = np.full((h, w), 0xDEADBEEF, np.uint32)
        R.render_frame(cam.to_c(0.01, 48), img)
        return img

    with session(mode=MODE_LIBM_EXP) as s:
        s.R.upload(A)
        before = frame48(s.R)
        s.R.recolour(m, s.array(idx), k=len(idx))
        s.R.recolour(CC.MATRICES["swap"])
        got = frame48(s.R)
    ref, _ = O.render(scene_dict(E), oracle_camera(cam, 0.01, 48), nthreads=8)
    assert ref.any() and np.array_equal(got, ref), int((got != ref).sum())
    assert not np.array_equal(got, before), "the recolour is meant to change the frame"


# ---- one fixed program ---------------------------------------------------------------------------------------------------------
def test_one_fixed_program():
    """upload, append, recolour by index of the appended rows, remove of a tenth, recolour whole, reorder, colours: the values
    are the numpy restatement's after every step, the frames a fresh upload's at the end"""
    n, m_rows, (h, w) = 1000, 300, TARGETS[0]
    cam = poses(h, w)[1]
    E = copy_of(lively(n, 8300))
    extra = lively(m_rows, 8301)
    with session() as s:
        R = s.R
        R.upload(E)
        assert_resident(s, E, "uploaded")
        assert R.append(s.device(extra)) == n + m_rows
        E = AC.appended(E, extra)
        assert_resident(s, E, "appended")
        new = np.arange(n, n + m_rows, dtype=np.uint32)[::-1].copy()
        R.recolour(CC.MATRICES["tinted_contrast"], s.array(new), k=len(new))
        E = recoloured(E, CC.MATRICES["tinted_contrast"], new)
        assert_resident(s, E, "the appended rows recoloured")
        gone = np.random.default_rng(8302).random(len(E)) < 0.1
        assert R.remove(s.array(gone.astype(np.uint8)), n=len(E)) == int((~gone).sum())
        E, _ = RC.removed(E, gone)
        assert_resident(s, E, "a tenth removed")
        R.recolour(CC.MATRICES["grey"])
        E = recoloured(E, CC.MATRICES["grey"])
        assert_resident(s, E, "recoloured whole")
        R.reorder()
        assert_resident(s, E, "reordered")
        for sh_dim in (15, 48):
            rgb = assert_colours(s, E, cam, sh_dim, 8303, "at the end, sh_dim %d" % sh_dim)
        assert np.abs(rgb - rgb[:, :1]).max() < 1e-4, "a grey scene: the three channels agree to rounding"
        with fresh_upload(E) as ref:
            assert_same_frames(frames(R), frames(ref), "at the end")
