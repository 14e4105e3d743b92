"""Gaussians appended to a resident scene and its slots put back in order (splat_append_gaussians_device,
splat_reorder_scene_device, Renderer.append / reorder / duplicate, -m gpu).  Nothing here has a tolerance: the resident and the
appended values are what they were bit for bit, the count and the scene's order are the numpy restatement's
(tests/append_cases.py), the bounds are block_bounds_np's -- those of the blocks wholly below the seam the very bits read before
the call -- and frames, records, tile lists and counts are those of a FRESH Renderer that takes the concatenated arrays through
splat_upload_scene.  After a reorder the layout is that Renderer's outright.  The pairs (n, m): the smallest scene, a block
exactly filled, a block boundary crossed, a new block opened, two that end on a boundary, several new blocks, a tail of 18 sort
tiles (more than one radix workgroup and more than one scan row), and 274 resident blocks."""
import ctypes as C
import functools

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from splat_amd.gaussians import PLY_PROPS, inria_layout
from helpers import make_camera
import append_cases as AC
import remove_cases as RC
import scene_model as M
import transform_cases as T
from scene_gpu import (TARGETS, assert_bounds, assert_resident, assert_same_frames, assert_same_stage, copy_of, frame, frames, fresh_upload,
                       in_view, session, stage)
from test_gpu_ply_encode import rows_of, slot_values
from test_gpu_remove import assert_layout, put_mask
from test_gpu_scene_update import block_bounds_np, spoil
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2
BIG = 70001
PAIRS = ((1, 1), (255, 1), (255, 2), (256, 1), (257, 255), (1000, 24), (1000, 1000), (1000, BIG), (BIG, 1000))
# which side carries signed zeros, NaN / inf centres and a NaN covariance: (resident, appended)
SPOILED = {(257, 255): (True, False), (1000, 24): (False, True), (1000, 1000): (True, True), (1000, BIG): (False, True), (BIG, 1000): (True, False)}


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(n, seed, spoiled=False):
    """made once and shared: no test writes into what this returns"""
    g = in_view(n, seed)
    return spoil(g) if spoiled else g


def pair(n, m, base):
    sa, se = SPOILED.get((n, m), (False, False))
    A, E = scene(n, base + n, sa), scene(m, base + 500 + m, se)
    return A, E, AC.appended(A, E)


def append(s, g, whole=False):
    """Renderer.append of the Gaussians g from device buffers made here: four addresses with m=, or the DeviceGaussians itself"""
    d = s.device(g)
    return s.R.append(d) if whole else s.R.append(d.positions, d.cov3d, d.opacities, d.sh, m=len(g))


def identity(n):
    return np.arange(n, dtype=np.uint32)


def assert_fresh_layout(R, ref, what):
    (orig, bounds), (ref_orig, ref_bounds) = R.scene_layout(), ref.scene_layout()
    assert np.array_equal(orig, ref_orig), what + ": the order is the fresh upload's"
    assert_bounds(bounds, ref_bounds, what + ": the bounds are the fresh upload's")


def rest_frames(R, cam, h, w):
    img = R.host_image(h, w)

    def rest_frame():
        img[:] = 0xDEADBEEF
        R.render_frame(cam, img)
        return img.copy()
    return rest_frame


# ---- 1. values, count, order, bounds, storage ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", PAIRS)
def test_values_layout_and_bounds_after_append_and_after_reorder(n, m):
    A, E, both = pair(n, m, 9000)
    what = "n=%d m=%d" % (n, m)
    with session() as s:
        R = s.R
        if (n + m) % 2:
            R.upload(A)
        else:
            d = s.device(A)
            R.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=n)
        orig_a, bounds_a = R.scene_layout()
        got = append(s, E, whole=bool(m % 2))
        assert got == n + m == R.n, what
        assert_resident(s, both, what)
        want = AC.appended_order(orig_a, E.positions)
        assert np.array_equal(want[:n], orig_a) and np.array_equal(np.sort(want), identity(n + m))
        orig, bounds = assert_layout(R, both, want, identity(n + m), what, n + m)
        whole = n // 256
        assert bounds[:whole].tobytes() == bounds_a[:whole].tobytes(), what + ": the blocks wholly below the seam keep their bits"
        # ... and put back in order
        expect_moved = AC.moved(orig, both.positions)
        moved = R.reorder()
        print(what, "-> reorder moved", moved)
        assert moved == expect_moved, what
        assert R.n == n + m
        assert_resident(s, both, what + " reordered")
        want2 = AC.reordered_order(both.positions)
        orig2, bounds2 = assert_layout(R, both, want2, identity(n + m), what + " reordered", n + m + 1)
        with fresh_upload(both) as ref:
            assert_fresh_layout(R, ref, what + " reordered")
        assert R.reorder() == 0, what + ": a second reorder finds nothing to move"
        assert np.array_equal(R.scene_layout()[0], orig2)


@pytest.mark.parametrize("n,m", PAIRS)
def test_storage_is_a_fresh_uploads(n, m):
    A, E, both = pair(n, m, 9000)
    with session() as s, session() as twin:
        s.R.upload(A)
        d = s.device(E)
        twin.device(E)                                                 # (both ledgers count the caller's buffers)
        assert s.R.append(d) == n + m
        twin.R.upload(both)
        assert s.R.device_bytes()[0] == twin.R.device_bytes()[0], "after the append"
        moved = s.R.reorder()
        assert s.R.device_bytes()[0] == twin.R.device_bytes()[0], "after the reorder (moved %d)" % moved


# ---- 2. frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
@pytest.mark.parametrize("n,m", PAIRS)
def test_frames_are_those_of_a_fresh_upload_of_the_concatenation(n, m, mode):
    A, E, both = pair(n, m, 9100)
    what = "n=%d m=%d" % (n, m)
    with session(mode=mode) as s, fresh_upload(both, mode=mode) as ref:
        R = s.R
        R.upload(A)
        if (n + m) % 2:
            frames(R)                                                  # hints, layouts and lists of the old scene exist
        assert append(s, E) == n + m
        ref_frames = frames(ref)
        assert any(img.any() for img in ref_frames)
        assert_same_frames(frames(R), ref_frames, what + " appended")
        moved = R.reorder()
        assert_same_frames(frames(R), ref_frames, what + " reordered (moved %d)" % moved)
        seen, pairs = assert_same_stage(R, ref, what + " reordered")
        assert seen > 0 and pairs > 0
        assert_fresh_layout(R, ref, what)


@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
@pytest.mark.parametrize("which", ["half", "all"])
def test_depth_ties_across_the_seam(which, mode):
    """a copy has its original's centre, so it ties it in depth at every camera: only the index -- n .. for the copies -- tells
    them apart, and the slot order must not"""
    n = 1000
    A = scene(n, 9201)
    rng = np.random.default_rng(9202)
    idx = (rng.permutation(n)[: n // 2] if which == "half" else rng.permutation(n)).astype(np.uint32)
    both = AC.appended(A, RC.rows_of(A, idx.astype(np.int64)))
    with session(mode=mode) as s, fresh_upload(both, mode=mode) as ref:
        R = s.R
        R.upload(A)
        before = frames(R)
        first, got = R.duplicate(s.array(idx), k=len(idx))
        assert (first, got) == (n, n + len(idx)) and R.n == got
        assert_resident(s, both, "duplicated")
        ref_frames = frames(ref)
        assert any(not np.array_equal(a, b) for a, b in zip(before, ref_frames)), "the copies are meant to change the frames"
        assert_same_frames(frames(R), ref_frames, "ties, appended")
        _, records, _, _, _ = stage(R)
        assert records["depth"][n:].tobytes() == records["depth"][idx.astype(np.int64)].tobytes(), "every copy ties its original"
        assert R.reorder() > 0
        assert_same_frames(frames(R), ref_frames, "ties, reordered")
        assert_same_stage(R, ref, "ties, reordered")
        assert_fresh_layout(R, ref, "ties")
        # duplicates in the index list are fine, and the temporaries of the call are gone on return
        with session(mode=mode) as t:
            t.R.upload(A)
            twice = np.array([5, 5, 999, 0, 5], np.uint32)
            assert t.R.duplicate(t.array(twice), k=5) == (n, n + 5)
            assert_resident(t, AC.appended(A, RC.rows_of(A, twice.astype(np.int64))), "duplicates")
            d_bad = t.array(np.array([n + 5], np.uint32))
            held = []
            for _ in range(2):                                         # an index out of range: nothing appended, nothing leaked
                with pytest.raises(splat_amd.SplatError) as e:
                    t.R.duplicate(d_bad, k=1)
                assert e.value.code == _lib.ERR_INVALID and t.R.n == n + 5
                held.append(t.R.device_bytes()[0])
            assert held[0] == held[1], "the rows' temporary is freed on the way out of a refused call"


@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
def test_a_short_tile_list_becomes_a_long_one(mode):
    n, step = 1500, 500
    A = M.Model.source(n, 9301, dense=True)                            # every Gaussian over the tiles at the middle of the target
    pool = M.Model.source(6 * step, 9302, dense=True)
    h, w = TARGETS[1]
    cam = make_camera(h, w).to_c(0.01, 15)
    with session(mode=mode) as s:
        R = s.R
        R.upload(A)
        long_before = stage(R)[4].max_tile_len
        assert 0 < long_before <= 2048
        rest_frame = rest_frames(R, cam, h, w)
        for _ in range(3):
            rest_frame()
        both, k = A, 0
        while stage(R)[4].max_tile_len <= 2048:
            assert k < 6, "the pool is meant to take a tile list beyond 2048 keys"
            E = RC.rows_of(pool, np.arange(k * step, (k + 1) * step))
            both, k = AC.appended(both, E), k + 1
            assert append(s, E) == len(both)
        long_after = stage(R)[4].max_tile_len
        print("longest tile list", long_before, "->", long_after, "after", k, "appends")
        assert long_before <= 2048 < long_after
        with fresh_upload(both, mode=mode) as ref:
            want = frame(ref, make_camera(h, w), h, w)
            assert want.any()
            for j in range(STILL + 2):                                 # the camera at rest: the near selection's hints, retained lists
                assert np.array_equal(rest_frame(), want), "frame %d at rest is not the fresh upload's" % j
            ref_frames = frames(ref)
            assert_same_frames(frames(R), ref_frames, "short to long")
            assert R.reorder() > 0
            for j in range(STILL + 2):
                assert np.array_equal(rest_frame(), want), "frame %d at rest after the reorder" % j
            assert_same_frames(frames(R), ref_frames, "short to long, reordered")
            assert_same_stage(R, ref, "short to long, reordered")
        assert R.frames_dropped() == 0


# ---- 3. a reorder is worth calling --------------------------------------------------------------------------------------------
def far_moved(n=1000, seed=9401):
    """(scene, indices, matrix, moved scene): a random tenth of the Gaussians translated by many scene diameters"""
    A = scene(n, seed)
    idx = np.random.default_rng(seed + 1).permutation(n)[: n // 10].astype(np.uint32)
    m = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 64]], f32)
    pos, cov = T.transformed(A, m, idx.astype(np.int64))
    return A, idx, m, copy_of(A, pos, cov)


def test_a_reorder_after_a_far_move_tightens_the_blocks():
    A, idx, m, moved_scene = far_moved()
    n = len(A)
    with session() as s:
        R = s.R
        R.upload(A)
        orig_a, _ = R.scene_layout()
        R.transform(m, s.array(idx), k=len(idx))
        orig, before = R.scene_layout()
        assert np.array_equal(orig, orig_a)
        assert_bounds(before, block_bounds_np(moved_scene.positions, moved_scene.cov3d, orig), "moved")
        moved = R.reorder()
        assert moved == AC.moved(orig, moved_scene.positions) and moved > 0
        orig2, after = R.scene_layout()
        assert np.array_equal(orig2, AC.reordered_order(moved_scene.positions))
        assert_bounds(after, block_bounds_np(moved_scene.positions, moved_scene.cov3d, orig2), "reordered")
        v0, v1 = AC.bounds_volume(before), AC.bounds_volume(after)
        print("sum of block AABB volumes", v0, "->", v1, "; moved", moved, "of", n)
        assert v1 <= v0
        assert_resident(s, moved_scene, "reordered")
        with fresh_upload(moved_scene) as ref:
            assert_same_frames(frames(R), frames(ref), "far move, reordered")
            assert_same_stage(R, ref, "far move, reordered")


# ---- 4. reads --------------------------------------------------------------------------------------------------------------------
def test_an_append_of_nothing_and_a_reorder_in_order_are_reads_retention_goes_on():
    n, (h, w) = 1000, TARGETS[1]
    A = scene(n, 9501)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s:
        R = s.R
        R.upload(A)
        rest_frame = rest_frames(R, cam, h, w)
        rest = [rest_frame() for _ in range(STILL + 4)]
        retained = R.frames_retained()
        assert retained > 0 and rest[0].any()
        layout = R.scene_layout()
        d = s.device(scene(24, 9502))
        held = R.device_bytes()[0]
        calls = (lambda: R.append(d.positions, d.cov3d, d.opacities, d.sh, m=0), lambda: R.append(0, 0, 0, 0, m=0), lambda: R.reorder())
        for call, want in zip(calls, (n, n, 0)):
            assert call() == want and R.n == n
            assert np.array_equal(rest_frame(), rest[0])
            assert R.frames_retained() > retained, "the frame behind a call that changed nothing is composited from the retained lists"
            retained = R.frames_retained()
        assert R.device_bytes()[0] == held and R.frames_dropped() == 0
        after = R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert after[1].tobytes() == layout[1].tobytes()
        # refused calls change nothing either
        for bad in (n - 1, n + 1):
            out = C.c_uint64(0xABCD)
            rc = R._L.splat_append_gaussians_device(R._h, bad, 24, *[C.c_void_p(p) for p in (d.positions, d.cov3d, d.opacities, d.sh)],
                                                    C.byref(out), None)
            assert rc == _lib.ERR_INVALID and out.value == 0xABCD
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() > retained
        assert R.device_bytes()[0] == held


# ---- 5. edits --------------------------------------------------------------------------------------------------------------------
def test_frames_in_flight_and_the_first_frame_after_an_edit():
    n, (h, w) = 1000, TARGETS[1]
    A, E = scene(n, 9601), scene(300, 9602)
    both = AC.appended(A, E)
    _, idx, m, _ = far_moved(n, 9601)
    pos, cov = T.transformed(both, m, idx.astype(np.int64))
    final = copy_of(both, pos, cov)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s, fresh_upload(both) as ref, fresh_upload(final) as ref2:
        R = s.R
        R.upload(A)
        rest_frame = rest_frames(R, cam, h, w)
        rest = [rest_frame() for _ in range(STILL + 4)]                 # a camera at rest: retention is running
        assert R.frames_retained() > 0 and rest[0].any()
        images = [R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        d = s.device(E)
        try:
            for p in images:
                R.render_frame_device(cam, p, sync=False)
            assert R.append(d) == n + 300
            for p in images:                                           # queued before the append: the scene as it was
                assert np.array_equal(R.device_download(p, h, w), rest[0])
        finally:
            for p in images:
                R.device_free(p)
        want = frame(ref, make_camera(h, w), h, w)
        assert want.any() and not np.array_equal(want, rest[0])
        retained = R.frames_retained()
        assert np.array_equal(rest_frame(), want)
        assert R.frames_retained() == retained, "the frame after an append is binned, not retained"
        assert all(np.array_equal(rest_frame(), want) for _ in range(STILL + 4))
        assert R.frames_retained() > retained and R.frames_dropped() == 0
        # ... and the same behind a reorder that moves something
        R.transform(m, s.array(idx), k=len(idx))
        want2 = frame(ref2, make_camera(h, w), h, w)
        assert all(np.array_equal(rest_frame(), want2) for _ in range(STILL + 4))
        retained = R.frames_retained()
        assert R.reorder() > 0
        assert np.array_equal(rest_frame(), want2)
        assert R.frames_retained() == retained, "the frame after a reorder that moved something is binned, not retained"
        assert all(np.array_equal(rest_frame(), want2) for _ in range(STILL + 4))
        assert R.frames_retained() > retained and R.frames_dropped() == 0
        R.sync()


# ---- 6. no scene -----------------------------------------------------------------------------------------------------------------
def test_without_a_scene_the_c_call_refuses_and_the_renderer_uploads():
    n = 1000
    A, E = scene(n, 9701), scene(257, 9702, True)
    with session() as s, fresh_upload(E) as ref:
        R = s.R
        d = s.device(E)
        ptrs = [C.c_void_p(p) for p in (d.positions, d.cov3d, d.opacities, d.sh)]

        def c_calls(what):
            out = C.c_uint64(0xABCD)
            for n_arg in (0, n):
                assert R._L.splat_append_gaussians_device(R._h, n_arg, 257, *ptrs, C.byref(out), None) == _lib.ERR_NO_SCENE, what
            assert R._L.splat_append_gaussians_device(R._h, 0, 0, None, None, None, None, C.byref(out), None) == _lib.ERR_NO_SCENE, what
            assert out.value == 0xABCD, what
            with pytest.raises(splat_amd.SplatError) as e:
                R.reorder()
            assert e.value.code == _lib.ERR_NO_SCENE, what

        c_calls("a new context")
        R.upload(A)
        frames(R)
        assert R.remove(put_mask(s, np.ones(n, bool)), n=n) == 0 == R.n
        c_calls("an emptied context")
        assert R.append(d) == 257 == R.n                               # Renderer.append into an emptied scene is upload_device
        assert_resident(s, E, "pasted into an emptied scene")
        assert_fresh_layout(R, ref, "pasted into an emptied scene")
        assert_same_frames(frames(R), frames(ref), "pasted into an emptied scene")
        assert_same_stage(R, ref, "pasted into an emptied scene")


# ---- 7. torch tensors on a side stream ---------------------------------------------------------------------------------------
def test_torch_rows_on_a_side_stream():
    import torch
    n, m = 1000, 300
    A, E = scene(n, 9801), scene(m, 9802)
    both = AC.appended(A, E)
    dev = torch.device("cuda", 0)
    with session() as s, fresh_upload(both) as ref:
        s.R.upload(A)
        side = torch.cuda.Stream(device=dev)
        host = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (E.positions, E.cov3d, E.opacities, E.sh)]
        rows = [torch.full(tuple(a.shape), 7.0, dtype=torch.float32, device=dev) for a in host]
        junk = torch.zeros(16 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(10):                                        # work in front of the copies: they have not run when the call is made
                junk.add_(1.0)
            for r, a in zip(rows, host):
                r.copy_(a, non_blocking=True)
        assert s.R.append(*rows, stream=side) == n + m == s.R.n
        assert_resident(s, both, "torch rows")
        with pytest.raises(ValueError):
            s.R.append(rows[0], rows[1][:-1], rows[2], rows[3])        # 299 covariances for 300 positions
        assert_same_frames(frames(s.R), frames(ref), "torch rows")
        del rows, junk


# ---- 8. load, append a second PLY, reorder, save, load -------------------------------------------------------------------------
def write_ply(path, rows):
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rows))
        for p in PLY_PROPS:
            f.write(("property float %s\n" % p).encode())
        f.write(b"end_header\n")
        f.write(np.ascontiguousarray(rows).tobytes())


def ply_rows_of(g):
    return rows_of(slot_values(g.positions, g.cov3d, g.opacities, g.sh), inria_layout(len(g)))


def test_load_ply_append_a_second_ply_reorder_save_ply_load_ply(tmp_path):
    na, nb = 1000, 300
    rows_a, rows_b = ply_rows_of(scene(na, 9901)), ply_rows_of(scene(nb, 9902))
    first, out, want_path = str(tmp_path / "first.ply"), str(tmp_path / "merged.ply"), str(tmp_path / "want.ply")
    write_ply(first, rows_a)
    # what the host makes of the two files, concatenated
    both = AC.appended(M.Model.loaded_from_rows(rows_a), M.Model.loaded_from_rows(rows_b))
    with session() as s, session() as t, fresh_upload(both) as ref:
        R = s.R
        assert R.load_ply(first) == na == R.n
        lay = inria_layout(nb)
        bufs = {f: s.alloc(4 * per * nb) for f, per in (("positions", 4), ("scales", 3), ("opacities", 1), ("rotations", 4), ("sh", 48), ("cov3d", 9))}
        R.decode_ply_device(s.array(rows_b), lay, bufs["positions"], bufs["scales"], bufs["opacities"], bufs["rotations"], bufs["sh"])
        R.compute_cov3d_device(bufs["scales"], bufs["rotations"], bufs["cov3d"], n=nb)
        assert R.append(bufs["positions"], bufs["cov3d"], bufs["opacities"], bufs["sh"], m=nb) == na + nb
        assert R.reorder() > 0
        assert_resident(s, both, "merged")
        assert_fresh_layout(R, ref, "merged")
        assert R.save_ply(out) == na + nb
        assert ref.save_ply(want_path) == na + nb
        assert open(out, "rb").read() == open(want_path, "rb").read(), "the rows the concatenated host arrays save to"
        assert t.R.load_ply(out) == na + nb == t.R.n
        saved = np.frombuffer(open(out, "rb").read()[-(na + nb) * 4 * len(PLY_PROPS):], f32).reshape(na + nb, len(PLY_PROPS))
        assert_resident(t, M.Model.loaded_from_rows(saved), "loaded again")
