"""View-dependent colour turned where it lies (splat_rotate_sh_scene_device, splat_rotate_sh_gaussians_device, -m gpu).  The
sh values afterwards are the numpy float32 restatement's (tests/sh_rotate_cases.py, with the library's blocks, in original
index order) bit for bit; everything else keeps its bits, the order and the block bounds stay; the frames are those of a
FRESH Renderer that takes the restated arrays through splat_upload_scene.  Nothing here has a tolerance.  Scenes and targets
are those of tests/scene_gpu.py (n in 1, 255, 256, 257, 1000)."""
import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import make_camera, oracle_camera, scene_dict
import sh_rotate_cases as S
import transform_cases as T
from scene_gpu import (SIZES, TARGETS, assert_bounds, assert_resident, assert_same_frames, copy_of, frame, frames, fresh_upload, in_view,
                       index_sets, session)
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2
K = 4000
NAMES = list(S.ROTATIONS)


def lively(g, seed):
    """g with sh rows at magnitudes of their own in every band (a synthetic scene's higher bands are faint), so that a turn
    shows in the frames"""
    out = copy_of(g)
    sh = S.random_sh(len(g), seed)
    sh[:, :3] = g.sh[:, :3]
    sh[:, 3:] *= f32(0.05)                            # colours stay near the scene's own
    out.sh[:] = sh
    return out


def turned(g, blocks, rows=None):
    """g with the sh of the rows named (all: None) rotated, restated on the host"""
    out = copy_of(g)
    out.sh[:] = S.rotated_rows(blocks, g.sh, rows)
    return out


# ---- the device compile of splat_sh_math.h -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_compile_equals_host_compile(name):
    blocks = S.lib_blocks(S.ROTATIONS[name])
    sh = S.random_sh(K, 80 + len(name))
    host, dev = S.run_probe(blocks, sh), S.run_probe(blocks, sh, device=True)
    assert S.same_bits(dev, host), "%s: %d words differ" % (name, int((dev.view(np.uint32) != host.view(np.uint32)).sum()))


# ---- every rotation, whole and by index, at every size ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_rotate_whole_and_by_index(name, n):
    R3 = S.ROTATIONS[name]
    blocks = S.lib_blocks(R3)
    A = lively(in_view(n, 5000 + n), 5050 + n)
    E = A
    with session() as s:
        s.R.upload(A)
        orig_a, bounds_a = s.R.scene_layout()
        first = frames(s.R)
        for idx in [None] + index_sets(n, 5100 + n):
            what = "%s n=%d %s" % (name, n, "whole" if idx is None else "k=%d" % len(idx))
            if idx is None:
                s.R.rotate_sh(R3)
            else:
                s.R.rotate_sh(R3, s.array(idx) if len(idx) else 0, k=len(idx))
            E = turned(E, blocks, idx)
            # sh of the chosen rows is the restatement's; the other rows, band 0 and every other field keep their bits
            assert_resident(s, E, what)
            assert S.same_bits(E.sh[:, :3], A.sh[:, :3])
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
            assert any(not np.array_equal(a, b) for a, b in zip(got, first)), "the turn is meant to show in the frames"


def test_indices_as_a_torch_tensor_on_a_side_stream():
    import torch
    n = 1000
    R3 = S.ROTATIONS["rot173"]
    blocks = S.lib_blocks(R3)
    A = lively(in_view(n, 5201), 5202)
    rows = np.arange(0, n, 7)
    E = turned(A, blocks, rows)
    with session() as s, fresh_upload(E) as ref:
        s.R.upload(A)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            idx = torch.arange(0, n, 7, dtype=torch.int32, device=dev)
            s.R.rotate_sh(R3.ravel().tolist(), idx)              # nine numbers; k and the stream from the tensor
        assert_resident(s, E, "torch index on a side stream")
        assert_same_frames(frames(s.R), frames(ref), "torch index on a side stream")
        del idx


# ---- what is refused applies nothing ----------------------------------------------------------------------------------------------
def test_an_index_out_of_range_applies_nothing():
    n = 1000
    A = lively(in_view(n, 5301), 5302)
    with session() as s:
        s.R.upload(A)
        before, layout = frames(s.R), s.R.scene_layout()
        idx = np.arange(100, dtype=np.uint32)
        idx[57] = n                                   # the first index that names no Gaussian
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.rotate_sh(S.ROTATIONS["rot20"], s.array(idx), k=len(idx))
        assert e.value.code == _lib.ERR_INVALID
        assert_resident(s, A, "after the refused rotation")
        after = s.R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert_bounds(after[1], layout[1], "after the refused rotation")
        assert_same_frames(frames(s.R), before, "after the refused rotation")


def test_a_matrix_that_is_not_orthogonal_is_refused_and_retention_goes_on():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(in_view(n, 5401), 5402)
    idx = np.arange(0, n, 3, dtype=np.uint32)
    cam = make_camera(h, w).to_c(0.01, 15)
    shear = T.MATRICES["shear"][:, :3]
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
        for bad in (shear, 1.01 * S.ROTATIONS["rot20"], np.full((3, 3), np.nan)):
            with pytest.raises(splat_amd.SplatError) as e:
                R.rotate_sh(bad)
            assert e.value.code == _lib.ERR_INVALID
            with pytest.raises(splat_amd.SplatError) as e:
                R.rotate_sh(bad, d_idx, k=len(idx))
            assert e.value.code == _lib.ERR_INVALID
        # nothing of the frame-to-frame state went: the very next frame at rest is a retained one (after an edit it is binned)
        assert np.array_equal(rest_frame(), rest[0])
        assert R.frames_retained() > retained
        assert_resident(s, A, "after the refused matrices")


# ---- at rest, with retained lists active -------------------------------------------------------------------------------------------
def test_a_rotation_at_rest_ends_retention_and_retention_starts_over():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(in_view(n, 5501), 5502)
    idx = np.random.default_rng(5503).permutation(n)[:300].astype(np.uint32)
    R3 = S.ROTATIONS["rot173"]
    E = turned(A, S.lib_blocks(R3), idx)
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
        R.rotate_sh(R3, s.array(idx), k=len(idx))
        want = frame(ref, make_camera(h, w), h, w)
        assert not np.array_equal(want, rest[0]), "the rotation is meant to change the frame"
        assert np.array_equal(rest_frame(), want)
        assert R.frames_retained() == retained, "the frame after an edit is binned, not retained"
        more = [rest_frame() for _ in range(STILL + 4)]
        assert all(np.array_equal(f, want) for f in more)
        assert R.frames_retained() > retained and R.frames_dropped() == 0


# ---- transform(..., rotate_sh=True) ------------------------------------------------------------------------------------------------
def test_transform_with_rotate_sh_is_transform_then_rotate_sh():
    n = 1000
    A = lively(in_view(n, 5601), 5602)
    m = T.MATRICES["rotation"]                        # rigid: 20 degrees about a pivot
    lin = m[:, :3]
    rows = np.random.default_rng(5603).permutation(n)[:300].astype(np.uint32)
    blocks = S.lib_blocks(lin)
    pos, cov = T.transformed(A, m, rows)
    E = turned(copy_of(A, pos, cov), blocks, rows)
    pos, cov = T.transformed(E, m)
    E2 = turned(copy_of(E, pos, cov), blocks)
    with session() as s, session() as twin, fresh_upload(E2) as ref:
        s.R.upload(A)
        twin.R.upload(A)
        s.R.transform(m, s.array(rows), k=len(rows), rotate_sh=True)
        twin.R.transform(m, twin.array(rows), k=len(rows))
        twin.R.rotate_sh(lin, twin.array(rows), k=len(rows))
        assert_resident(s, E, "indexed, rotate_sh=True")
        assert_resident(twin, E, "indexed, transform then rotate_sh")
        s.R.transform(m, rotate_sh=True)
        assert_resident(s, E2, "whole, rotate_sh=True")
        assert_same_frames(frames(s.R), frames(ref), "whole, rotate_sh=True")
        # a shear: refused before anything is applied
        before = frames(s.R)
        for index in (None, s.array(rows)):
            with pytest.raises(ValueError):
                s.R.transform(T.MATRICES["shear"], index, k=None if index is None else len(rows), rotate_sh=True)
            assert_resident(s, E2, "after the refused shear")
        assert_same_frames(frames(s.R), before, "after the refused shear")
        # without the keyword sh keeps its bits, as before
        s.R.transform(m)
        pos, cov = T.transformed(E2, m)
        assert_resident(s, copy_of(E2, pos, cov), "without the keyword")


# ---- the verification mode against the oracle -----------------------------------------------------------------------------------
def test_libm_exp_mode_is_the_oracle_frame_of_the_restated_arrays():
    n, (h, w) = 1000, TARGETS[1]
    A = lively(in_view(n, 5701), 5702)
    idx = np.random.default_rng(5703).permutation(n)[:300].astype(np.uint32)
    R3 = S.ROTATIONS["rot173"]
    E = turned(A, S.lib_blocks(R3), idx)
    cam = make_camera(h, w)

    def frame48(R):                                   # sh_dim = 48: all four bands are evaluated (15, the other frames', stops at band 2)
        img = np.full((h, w), 0xDEADBEEF, np.uint32)
        R.render_frame(cam.to_c(0.01, 48), img)
        return img

    with session(mode=MODE_LIBM_EXP) as s:
        s.R.upload(A)
        before = frame48(s.R)
        s.R.rotate_sh(R3, s.array(idx), k=len(idx))
        got = frame48(s.R)
    ref, _ = O.render(scene_dict(E), oracle_camera(cam, 0.01, 48), nthreads=8)
    assert ref.any() and np.array_equal(got, ref), int((got != ref).sum())
    assert not np.array_equal(got, before), "the rotation is meant to change the frame"
