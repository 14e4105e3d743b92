"""The resident scene mapped where it lies (splat_transform_scene_device, splat_transform_gaussians_device, -m gpu).  The
values afterwards are the numpy float32 restatement's (tests/transform_cases.py) bit for bit; the frames, records, tile lists
and counts are those of a FRESH Renderer that takes the restated arrays through splat_upload_scene; order and block bounds
are those of a twin Renderer that took the same upload and then the restated values through splat_update_*.  Nothing here
has a tolerance.  Scenes and targets are those of tests/test_gpu_scene_update.py (n in 1, 255, 256, 257, 1000)."""
import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import make_camera, oracle_camera, scene_dict
import transform_cases as T
from scene_gpu import (SIZES, TARGETS, assert_bounds, assert_resident, assert_same_frames, assert_same_stage, copy_of, frame, frames,
                       fresh_upload, in_view, index_sets, session)
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2


def mapped(g, m, rows=None):
    """g with the rows named (all: None) mapped by m, restated on the host"""
    pos, cov = T.transformed(g, m, rows)
    return copy_of(g, pos, cov)


# ---- 1-5. every matrix, by index and whole, at every size --------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(T.MATRICES))
def test_transform_by_index_and_whole(name, n):
    m = T.MATRICES[name]
    A = in_view(n, 4000 + n)
    E = A
    with session() as s, session() as twin:
        s.R.upload(A)
        twin.R.upload(A)
        orig_a, _ = s.R.scene_layout()
        slot_of = np.empty(n, np.int64)
        slot_of[orig_a] = np.arange(n)
        first = frames(s.R)
        for idx in index_sets(n, 4100 + n) + [None]:
            what = "%s n=%d %s" % (name, n, "whole" if idx is None else "k=%d" % len(idx))
            bounds_before = s.R.scene_layout()[1]
            if idx is None:
                s.R.transform(m)
                E = mapped(E, m)
                twin.R.update_device(positions=twin.array(E.positions), cov3d=twin.array(E.cov3d), n=n)
            else:
                s.R.transform(m, s.array(idx) if len(idx) else 0, k=len(idx))
                E = mapped(E, m, idx)
                if len(idx):
                    twin.R.update_indexed(twin.array(idx), k=len(idx), positions=twin.array(E.positions[idx]), cov3d=twin.array(E.cov3d[idx]))
            # the selected rows are the restatement's, the others and every opacity and sh keep their bytes
            assert_resident(s, E, what)
            # order and bounds against the twin
            orig, bounds = s.R.scene_layout()
            assert np.array_equal(orig, orig_a), what
            assert_bounds(bounds, twin.R.scene_layout()[1], what)
            if idx is not None:
                untouched = np.setdiff1d(np.arange(bounds.shape[0]), np.unique(slot_of[idx.astype(np.int64)] // 256))
                assert_bounds(bounds, bounds_before, what + " (blocks without a selected Gaussian)", untouched)
            # frames, records, tile lists and counts (n_singular among them) against a fresh upload of the restated arrays
            with fresh_upload(E) as ref:
                got = frames(s.R)
                assert_same_frames(got, frames(ref), what)
                assert_same_stage(s.R, ref, what)
            if name == "identity":
                assert np.array_equal(E.positions, A.positions) and np.array_equal(E.cov3d, A.cov3d)      # ==: a -0 may be +0 now
                assert_same_frames(got, first, what)
        if n >= 255 and name not in ("zero",):
            assert any(img.any() for img in got), "the scene is meant to stay in view"


# ---- 6. at rest, with retained lists active -----------------------------------------------------------------------------------
def test_a_transform_at_rest_ends_retention_and_retention_starts_over():
    n, (h, w) = 1000, TARGETS[1]
    A = in_view(n, 4201)
    idx = np.random.default_rng(4202).permutation(n)[:300].astype(np.uint32)
    m = T.MATRICES["rotation"]
    E = mapped(A, m, idx)
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
        R.transform(m, s.array(idx), k=len(idx))
        want = frame(ref, make_camera(h, w), h, w)
        assert not np.array_equal(want, rest[0]), "the rotation is meant to change the frame"
        assert np.array_equal(rest_frame(), want)
        assert R.frames_retained() == retained, "the frame after an edit is binned, not retained"
        more = [rest_frame() for _ in range(STILL + 4)]
        assert all(np.array_equal(f, want) for f in more)
        assert R.frames_retained() > retained and R.frames_dropped() == 0


# ---- 7. select -> indices -> transform -> render, with nothing on the host but the count ----------------------------------------
def test_select_indices_transform_render():
    n = 1000
    A = in_view(n, 4301)
    box = np.array([[1.0, 0.0, 0.0, -0.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], f32)       # |x - 0.5| <= 1, |y| <= 1, |z| <= 1
    m = T.MATRICES["rotation"]
    u = T.transform_np(box, A.positions, A.cov3d)[0][:, :3]           # the header's VOLUME formula is the centre's
    rows = np.flatnonzero((np.abs(u) <= 1).all(1))
    assert 0 < len(rows) < n
    E = mapped(A, m, rows)
    with session() as s, fresh_upload(E) as ref:
        s.R.upload(A)
        sel, idx = s.alloc(n), s.alloc(4 * n)
        k = s.R.select(sel, box=box)
        assert k == len(rows)
        assert s.R.selection_indices(sel, idx, n=n, capacity=n) == k
        s.R.transform(m, idx, k=k)
        assert_same_frames(frames(s.R), frames(ref), "select -> indices -> transform")
        assert_resident(s, E, "select -> indices -> transform")


# ---- 8. the verification mode against the oracle -------------------------------------------------------------------------------
def test_libm_exp_mode_is_the_oracle_frame_of_the_restated_arrays():
    n, (h, w) = 1000, TARGETS[1]
    A = in_view(n, 4401)
    idx = np.random.default_rng(4402).permutation(n)[:300].astype(np.uint32)
    m = T.MATRICES["shear"]
    E = mapped(A, m, idx)
    cam = make_camera(h, w)
    with session(mode=MODE_LIBM_EXP) as s:
        s.R.upload(A)
        s.R.transform(m, s.array(idx), k=len(idx))
        got = frame(s.R, cam, h, w)
    ref, _ = O.render(scene_dict(E), oracle_camera(cam, 0.01), nthreads=8)
    assert ref.any() and np.array_equal(got, ref), int((got != ref).sum())


# ---- 9. a bad index applies nothing ----------------------------------------------------------------------------------------------
def test_an_index_out_of_range_applies_nothing():
    n = 1000
    A = in_view(n, 4501)
    with session() as s:
        s.R.upload(A)
        before, layout = frames(s.R), s.R.scene_layout()
        idx = np.arange(100, dtype=np.uint32)
        idx[57] = n                                   # the first index that names no Gaussian
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.transform(T.MATRICES["scale"], s.array(idx), k=len(idx))
        assert e.value.code == _lib.ERR_INVALID
        assert_resident(s, A, "after the refused transform")
        after = s.R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert_bounds(after[1], layout[1], "after the refused transform")
        assert_same_frames(frames(s.R), before, "after the refused transform")


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_transform_takes_a_4x4_and_torch_indices():
    import torch
    n = 1000
    A = in_view(n, 4601)
    m = T.MATRICES["mirror"]
    m4 = np.concatenate([m, np.array([[0, 0, 0, 1]], f32)]).astype(np.float64)
    rows = np.arange(0, n, 7)
    E = mapped(mapped(A, m), m, rows)
    with session() as s, fresh_upload(E) as ref:
        s.R.upload(A)
        s.R.transform(m4)                             # float64 4x4: cast to float32, the last row dropped
        idx = torch.arange(0, n, 7, dtype=torch.int32, device=torch.device("cuda", 0))
        s.R.transform(m.ravel().tolist(), idx)        # twelve numbers; k from the tensor
        assert_resident(s, E, "4x4, then a torch index")
        assert_same_frames(frames(s.R), frames(ref), "4x4, then a torch index")
        out = torch.full((len(rows), 4), float("nan"), dtype=torch.float32, device=idx.device)
        s.R.read_indexed(idx, positions=out)
        want = E.positions[rows].copy()
        want[:, 3] = 1.0
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        del idx, out
