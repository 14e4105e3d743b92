"""Gaussians taken out of a resident scene (splat_remove_gaussians_device, Renderer.remove, -m gpu).  Nothing here has a
tolerance: the survivors' values are what they were bit for bit, the count, the index map and the scene's order are the numpy
restatement's (tests/remove_cases.py), the bounds are block_bounds_np's, and frames, records, tile lists and counts are those of
a FRESH Renderer that takes the survivors through splat_upload_scene.  Scenes are those of tests/test_gpu_scene_update.py
(n in 1, 255, 256, 257, 1000); for values and layout also n = 70 001: 274 K1 blocks -- more than one 256-count round of
mask_scan_kernel over the block counts -- and 18 spans of the mask.  Every mask is used in both modes and placed at
addresses base + 0, 1 and 3 (n = 70 001: at one of the three, in turn)."""
import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from helpers import make_camera
import remove_cases as RC
import transform_cases as T
from scene_gpu import (SENTINEL, SIZES, TARGETS, assert_bounds, assert_resident, assert_same_frames, assert_same_stage, copy_of, frame,
                       frames, fresh_upload, in_view, session, stage)
from test_gpu_scene_update import block_bounds_np, spoil
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2
BIG = 70001
OFFSETS = (0, 1, 3)
NONZERO = np.array([1, 2, 0x80, 0xFF], np.uint8)     # nonzero means selected, whatever the byte


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def put_mask(s, sel, off=0):
    """the selection as bytes at a device address that is `off` beyond a 16-byte boundary, every byte around it NONZERO (a kernel
    that read beyond mask[0..n) would count them); returns the address"""
    sel = np.asarray(sel) != 0
    a = np.where(sel, NONZERO[np.arange(len(sel)) % 4], 0).astype(np.uint8)
    base = s.alloc(len(a) + 32, 0xFF)
    assert base % 16 == 0
    if len(a):
        s.R._check(s.R._L.splat_device_upload(s.R._h, base + 16 + off, a.ctypes.data, a.nbytes))
    return base + 16 + off


def remove(s, sel, keep, off=0, with_map=True):
    """Renderer.remove of `sel` on the resident scene; returns (n_after, the map read back or None), the map buffer's bytes beyond
    4 n checked for their sentinel"""
    n = s.R.n
    pm = s.alloc(4 * n + 16, SENTINEL) if with_map else None
    got = s.R.remove(put_mask(s, sel, off), keep=keep, index_map=pm, n=n)
    if pm is None:
        return got, None
    words = s.fetch(pm, n + 4, np.uint32)
    assert (words[n:] == 0xA5A5A5A5).all(), "the map buffer beyond 4 n bytes is not the call's to write"
    return got, words[:n]


def mask_cases(n, orig, seed):
    """[(name, selected)]: each is used as the set to delete AND as the set to keep"""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, idx):
        sel = np.zeros(n, bool)
        sel[np.asarray(idx, np.int64)] = True
        out.append((name, sel))

    add("a single Gaussian", [n // 2])
    add("every other one", np.arange(0, n, 2))
    add("a whole wave of slots", orig[64:128] if n >= 128 else orig[:64])
    add("a whole block of slots", orig[256:512] if n >= 512 else orig[:256])
    add("all but the last slot of the last block", orig[:n - 1])
    for pct in (1, 50, 99):
        out.append(("random %d %%" % pct, rng.random(n) < pct / 100.0))
    for left in (1, 255, 256, 257):
        if left < n:
            add("n' = %d" % left, rng.permutation(n)[:left])          # (kept: n' survivors; deleted: n - n' of them)
    return out


def scene(n, seed):
    g = in_view(n, seed)
    return spoil(g) if n in (257, 1000) else g                         # signed zeros, NaN and inf centres, a NaN covariance


def some_blocks(nb, seed):
    """every block of a small scene; of a large one the first two, the last two (a full one and the partial one) and four others"""
    if nb <= 8:
        return np.arange(nb)
    return np.unique(np.concatenate([[0, 1, nb - 2, nb - 1], np.random.default_rng(seed).integers(2, nb - 2, 4)]))


def assert_layout(R, want, orig_before, index_map, what, seed=0):
    """the order is the old one without the slots that went; the bounds are block_bounds of the survivors under it"""
    orig, bounds = R.scene_layout()
    assert np.array_equal(orig, RC.compacted_order(orig_before, index_map)), what
    blocks = some_blocks(bounds.shape[0], seed)
    slots = np.concatenate([np.arange(256 * b, min(len(orig), 256 * (b + 1))) for b in blocks])
    # (block_bounds_np takes any order: the slots of the chosen blocks, the partial block last, are blocks of their own)
    assert_bounds(bounds[blocks], block_bounds_np(want.positions, want.cov3d, orig[slots]), what)
    return orig, bounds


# ---- 1, 2. values, count, map, order, bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + (BIG,))
def test_survivors_keep_their_bits_and_the_layout_is_the_compacted_one(n):
    A = scene(n, 7000 + n)
    with session() as s:
        R = s.R
        R.upload(A)
        orig_a, bounds_a = R.scene_layout()
        turn = 0
        for name, sel in mask_cases(n, orig_a, 7100 + n):
            for keep in (False, True):
                offsets = OFFSETS if n != BIG else (OFFSETS[turn % 3],)
                turn += 1
                for off in offsets:
                    what = "n=%d %s, %s, mask at +%d" % (n, name, "kept" if keep else "deleted", off)
                    want, want_map = RC.removed(A, sel, keep)
                    if R.n != n:
                        R.upload(A)
                    got, got_map = remove(s, sel, keep, off)
                    print(what, "->", got)
                    assert got == len(want) == R.n, what
                    assert np.array_equal(got_map, want_map), what
                    if got == 0:
                        with pytest.raises(splat_amd.SplatError) as e:
                            R.read_device(n=0)
                        assert e.value.code == _lib.ERR_NO_SCENE, what
                        continue
                    assert_resident(s, want, what)
                    if got == n:
                        orig, bounds = R.scene_layout()
                        assert np.array_equal(orig, orig_a), what
                        assert_bounds(bounds, bounds_a, what)
                    elif off == offsets[0]:
                        assert_layout(R, want, orig_a, want_map, what, turn)
                    else:
                        assert np.array_equal(R.scene_layout()[0], RC.compacted_order(orig_a, want_map)), what


@pytest.mark.parametrize("n", SIZES + (BIG,))
def test_with_the_extremes_spared_the_layout_is_a_fresh_uploads(n):
    A = scene(n, 7200 + n)
    rng = np.random.default_rng(7300 + n)
    spare = RC.extremes(A.positions)
    with session() as s:
        for k, gone in enumerate((rng.random(n) < 0.5, np.arange(n) % 2 == 1, rng.random(n) < 0.97)):
            gone[spare] = False
            for keep in (False, True):
                sel = ~gone if keep else gone
                want, want_map = RC.removed(A, sel, keep)
                for a, b in zip(RC.finite_box(want.positions), RC.finite_box(A.positions)):
                    assert a.tobytes() == b.tobytes()
                s.R.upload(A)
                orig_a, _ = s.R.scene_layout()
                got, _ = remove(s, sel, keep, OFFSETS[k], with_map=False)
                assert got == len(want)
                orig, bounds = s.R.scene_layout()
                assert np.array_equal(orig, RC.compacted_order(orig_a, want_map))
                with fresh_upload(want) as ref:
                    ref_orig, ref_bounds = ref.scene_layout()
                assert np.array_equal(orig, ref_orig), "n=%d case %d: the order is the one a fresh upload computes" % (n, k)
                assert_bounds(bounds, ref_bounds, "n=%d case %d" % (n, k))
                assert np.array_equal(ref_orig, RC.morton_order(want.positions)), "the restated Morton order is the library's"


# ---- 3. frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
@pytest.mark.parametrize("n", SIZES)
def test_frames_are_those_of_a_fresh_upload_of_the_survivors(n, mode):
    A = in_view(n, 7400 + n)
    with session(mode=mode) as s:
        s.R.upload(A)
        orig_a, _ = s.R.scene_layout()
        cases = dict(mask_cases(n, orig_a, 7500 + n))
        seen_any = False
        for k, (name, keep) in enumerate((("every other one", False), ("random 50 %", True), ("a whole block of slots", False),
                                          ("random 99 %", False), ("a single Gaussian", False), ("a single Gaussian", True))):
            sel = cases[name]
            want, _ = RC.removed(A, sel, keep)
            what = "n=%d %s %s" % (n, name, "kept" if keep else "deleted")
            if len(want) in (0, n):
                continue
            s.R.upload(A)
            if k % 2:
                frames(s.R)                                            # hints, layouts and lists of the old scene exist
            got, _ = remove(s, sel, keep, OFFSETS[k % 3], with_map=bool(k & 2))
            assert got == len(want)
            with fresh_upload(want, mode=mode) as ref:
                ref_frames = frames(ref)
                assert_same_frames(frames(s.R), ref_frames, what)
                seen, pairs = assert_same_stage(s.R, ref, what)
                seen_any = seen_any or (seen > 0 and pairs > 0 and any(img.any() for img in ref_frames))
        assert seen_any or n == 1


@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
def test_depth_ties_follow_the_new_index_after_members_of_each_tie_went(mode):
    n = 1000
    A = in_view(n, 7610)
    rng = np.random.default_rng(7611)
    site = rng.integers(0, 27, n)                     # a 3 x 3 x 3 lattice: ~37 Gaussians of different colour at every site
    A.positions[:, 0] = (site % 3 - 1).astype(f32) * f32(0.5)
    A.positions[:, 1] = (site // 3 % 3 - 1).astype(f32) * f32(0.5)
    A.positions[:, 2] = (site // 9 - 1).astype(f32) * f32(0.5)
    A.cov3d[:] = A.cov3d[0]                           # the same footprint, the same opacity: only the order tells them apart
    A.cov3d *= f32(40.0)
    A.opacities[:] = f32(0.6)
    gone = rng.random(n) < 0.4                        # some members of every tie
    assert all(0 < gone[site == k].sum() < (site == k).sum() for k in range(27))
    want, _ = RC.removed(A, gone, False)
    with session(mode=mode) as s, fresh_upload(want, mode=mode) as ref:
        s.R.upload(A)
        before = frames(s.R)
        assert remove(s, gone, False, 3)[0] == len(want)
        ref_frames = frames(ref)
        assert any(img.any() for img in ref_frames)
        assert any(not np.array_equal(a, b) for a, b in zip(before, ref_frames)), "the removal is meant to change the frames"
        assert_same_frames(frames(s.R), ref_frames, "ties")
        assert_same_stage(s.R, ref, "ties")


@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
def test_a_long_tile_list_becomes_a_short_one(mode):
    n = 4000
    A = in_view(n, 7700)
    A.positions[:, :3] *= f32(0.02)                   # every Gaussian over the tiles at the middle of the target
    keep = np.random.default_rng(7701).random(n) < 0.05
    want, _ = RC.removed(A, keep, True)
    with session(mode=mode) as s, fresh_upload(want, mode=mode) as ref:
        s.R.upload(A)
        long_before = stage(s.R)[4].max_tile_len
        rest = [frame(s.R, make_camera(*TARGETS[1]), *TARGETS[1]) for _ in range(3)]
        assert rest[0].any()
        assert remove(s, keep, True, 1)[0] == len(want)
        assert_same_frames(frames(s.R), frames(ref), "long to short")
        assert_same_stage(s.R, ref, "long to short")
        long_after = stage(s.R)[4].max_tile_len
        print("longest tile list", long_before, "->", long_after)
        assert long_before > 2048 >= long_after > 0


# ---- 4. composition --------------------------------------------------------------------------------------------------------------
def test_floaters_out_then_edits_by_the_new_indices():
    n = 1000
    A, B = in_view(n, 7801), in_view(n, 7802)
    p = A.positions[:, :3].astype(np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    radius = float(np.sqrt(np.median(d2.min(1))))     # about half of the Gaussians have nobody within it
    m = T.MATRICES["rotation"]
    with session() as s:
        R = s.R
        R.upload(A)
        sel = s.alloc(n, 0)
        floaters = R.select_neighbours(sel, radius, at_most=0)
        gone = s.fetch(sel, n, np.uint8) != 0
        assert 0 < floaters == gone.sum() < n
        E, want_map = RC.removed(A, gone, False)
        pm = s.alloc(4 * n, SENTINEL)
        assert R.remove(sel, index_map=pm, n=n) == len(E) == R.n
        assert np.array_equal(s.fetch(pm, n, np.uint32), want_map)
        # the first indexed call after a removal: the inverse order is made again, for the new numbering
        n2 = len(E)
        idx = np.random.default_rng(7803).permutation(n2)[: n2 // 3].astype(np.uint32)
        for f in ("positions", "cov3d", "opacities", "sh"):
            getattr(E, f)[idx] = getattr(B, f)[idx]
        rows = dict(positions=s.array(B.positions[idx]), cov3d=s.array(B.cov3d[idx]), opacities=s.array(B.opacities[idx]), sh=s.array(B.sh[idx]))
        d_idx = s.array(idx)
        held = R.device_bytes()[0]
        R.update_indexed(d_idx, k=len(idx), **rows)
        assert 4 * n2 + (n2 + 255) // 256 <= R.device_bytes()[0] - held <= 4 * n2 + (n2 + 255) // 256 + 64      # of the NEW n
        idx2 = np.arange(n2 - 1, -1, -3).astype(np.uint32)
        E = copy_of(E, *T.transformed(E, m, idx2))
        R.transform(m, s.array(idx2), k=len(idx2))
        with pytest.raises(splat_amd.SplatError) as e:                 # an old index is out of range now
            R.transform(m, s.array(np.array([n2], np.uint32)), k=1)
        assert e.value.code == _lib.ERR_INVALID
        assert_resident(s, E, "floaters out, edited")
        with fresh_upload(E) as ref:
            assert_same_frames(frames(R), frames(ref), "floaters out, edited")
            assert_same_stage(R, ref, "floaters out, edited")


def test_remove_under_a_stale_order_and_twice():
    n = 1000
    A, B = in_view(n, 7901), in_view(n, 7902)
    rng = np.random.default_rng(7903)
    with session() as s:
        R = s.R
        R.upload(A)
        orig_a, _ = R.scene_layout()
        R.update_device(positions=s.array(B.positions), n=n)           # the order is A's, the positions are B's
        E = copy_of(A, B.positions.copy())
        first = rng.random(n) < 0.3
        E1, map1 = RC.removed(E, first, False)
        assert remove(s, first, False, 1)[0] == len(E1)
        orig1, _ = assert_layout(R, E1, orig_a, map1, "stale order")
        with fresh_upload(E1) as ref:
            assert_same_frames(frames(R), frames(ref), "stale order")
            assert_same_stage(R, ref, "stale order")
        second = rng.random(len(E1)) < 0.5                             # a mask of n' bytes, in the new numbering
        E2, map2 = RC.removed(E1, second, True)
        got, got_map = remove(s, second, True, 3)
        assert got == len(E2) == R.n and np.array_equal(got_map, map2)
        assert_resident(s, E2, "twice")
        assert_layout(R, E2, orig1, map2, "twice")
        with fresh_upload(E2) as ref:
            assert_same_frames(frames(R), frames(ref), "twice")
            assert_same_stage(R, ref, "twice")


def test_remove_then_save_ply_then_load_ply(tmp_path):
    n = 1000
    A = in_view(n, 8001)
    gone = np.random.default_rng(8002).random(n) < 0.4
    want, _ = RC.removed(A, gone, False)
    path = str(tmp_path / "survivors.ply")
    with session() as s, session() as t:
        s.R.upload(A)
        assert remove(s, gone, False)[0] == len(want)
        assert s.R.save_ply(path) == len(want)
        assert t.R.load_ply(path) == len(want) == t.R.n


# ---- 5. nothing to remove, nothing left ----------------------------------------------------------------------------------------------
def test_a_mask_that_removes_nothing_is_a_read_retention_goes_on():
    n, (h, w) = 1000, TARGETS[1]
    A = in_view(n, 8101)
    cam = make_camera(h, w).to_c(0.01, 15)
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
        layout = R.scene_layout()
        masks = [put_mask(s, np.zeros(n, bool), 1), put_mask(s, np.ones(n, bool), 3)]
        pm = s.alloc(4 * n + 16, SENTINEL)
        held = R.device_bytes()[0]
        for mask, keep in zip(masks, (False, True)):
            assert R.remove(mask, keep=keep, index_map=pm, n=n) == n == R.n
            assert np.array_equal(s.fetch(pm, n, np.uint32), np.arange(n, dtype=np.uint32)), "the identity map"
            assert np.array_equal(rest_frame(), rest[0])
            assert R.frames_retained() > retained, "the frame behind a removal of nothing is composited from the retained lists"
            retained = R.frames_retained()
        assert R.remove(masks[0], n=n) == n                            # (without a map)
        assert R.device_bytes()[0] == held and R.frames_dropped() == 0
        after = R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert_bounds(after[1], layout[1])


@pytest.mark.parametrize("keep", [False, True], ids=["delete", "crop"])
def test_a_mask_that_removes_everything_leaves_no_scene(keep):
    """The context is as splat_upload_scene(n = 0) leaves it: held to a twin that made that call.  (A render of an empty scene
    does not answer ERR_NO_SCENE in this library -- it gives a frame with nothing in it, before this call existed and after --
    so the render is held to the twin's answer, code, pixels and counts; the calls that need a scene do answer ERR_NO_SCENE.)"""
    n, (h, w) = 1000, TARGETS[0]
    A, B = in_view(n, 8201), in_view(257, 8202)
    cam = make_camera(h, w)
    with session() as s, session() as twin, fresh_upload(B) as ref:
        R = s.R
        R.upload(A)
        twin.R.upload(A)
        first = frame(R, cam, h, w), frame(twin.R, cam, h, w)
        assert first[0].any()
        sel = np.zeros(n, bool) if keep else np.ones(n, bool)
        twin.alloc(n + 32, 0xFF), twin.alloc(4 * n + 16, SENTINEL)      # (what remove() below allocates in s: both ledgers count them)
        got, got_map = remove(s, sel, keep, 1)
        assert got == 0 == R.n and (got_map == RC.GONE).all()
        twin.R.upload(splat_amd.GaussianList(np.zeros((0, 4), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros((0, 4), f32),
                                             np.zeros((0, 48), f32), np.zeros((0, 9), f32)))
        assert R.device_bytes()[0] == twin.R.device_bytes()[0], "as splat_upload_scene(n = 0) leaves it"
        # whatever a render answers after splat_upload_scene(n = 0) -- ERR_NO_SCENE, or a frame with nothing in it, which is what
        # the library does today (tests/test_gpu_device_upload.py leaves that open the same way) -- it answers here
        answers = []
        for X in (R, twin.R):
            out = np.full((h, w), 0xDEADBEEF, np.uint32)
            try:
                st = X.render(cam.to_c(0.01, 15), out)
                answers.append((_lib.SPLAT_OK, out, (st.n_gaussians, st.n_visible, st.n_pairs)))
            except splat_amd.SplatError as err:
                answers.append((err.code, out, None))
        assert answers[0][0] == answers[1][0] and answers[0][0] in (_lib.SPLAT_OK, _lib.ERR_NO_SCENE)
        assert np.array_equal(answers[0][1], answers[1][1]) and answers[0][2] == answers[1][2]
        # ... and every call that needs a scene says that there is none
        with pytest.raises(splat_amd.SplatError) as e:
            R.remove(put_mask(s, np.ones(4, bool)), n=4)
        assert e.value.code == _lib.ERR_NO_SCENE
        with pytest.raises(splat_amd.SplatError) as e:
            R.select(s.alloc(4, 0), opacity=(0.0, 1.0))
        assert e.value.code == _lib.ERR_NO_SCENE
        assert R.scene_layout()[0].size == 0
        R.upload(B)
        assert_same_frames(frames(R), frames(ref), "an upload after the scene went")


# ---- 6. state and storage ---------------------------------------------------------------------------------------------------------
def test_frames_in_flight_state_and_storage():
    n, (h, w) = 1000, TARGETS[1]
    A = in_view(n, 8301)
    gone = np.random.default_rng(8302).random(n) < 0.5
    want, want_map = RC.removed(A, gone, False)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s, session() as twin, fresh_upload(want) as ref:
        R = s.R
        R.upload(A)
        twin.R.upload(A)

        def at_rest(R_):
            img = R_.host_image(h, w)

            def rest_frame():
                img[:] = 0xDEADBEEF
                R_.render_frame(cam, img)
                return img.copy()
            return rest_frame

        rest_frame, twin_frame = at_rest(R), at_rest(twin.R)            # (the twin makes every call this context makes but the removal)
        rest = [rest_frame() for _ in range(STILL + 4)]                 # a camera at rest: retention is running
        retained = R.frames_retained()
        assert retained > 0 and rest[0].any() and all(np.array_equal(rest[0], f) for f in rest)
        for _ in range(STILL + 5):
            twin_frame()
        images = [R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        twin_images = [twin.R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        mask = put_mask(s, gone, 3)
        pm = s.alloc(4 * n + 16, SENTINEL)
        twin.alloc(n + 32, 0xFF), twin.alloc(4 * n + 16, SENTINEL)      # (both ledgers count the caller's buffers)
        try:
            # a refused call first: a wrong n changes neither layout nor frames, and writes nothing
            layout = R.scene_layout()
            for bad in (n - 1, n + 1):
                with pytest.raises(splat_amd.SplatError) as e:
                    R.remove(mask, index_map=pm, n=bad)
                assert e.value.code == _lib.ERR_INVALID
            assert R.n == n and (s.fetch(pm, n + 4, np.uint32) == 0xA5A5A5A5).all()
            after = R.scene_layout()
            assert np.array_equal(after[0], layout[0])
            assert_bounds(after[1], layout[1], "after the refused call")
            assert np.array_equal(rest_frame(), rest[0])
            retained = R.frames_retained()
            for p, q in zip(images, twin_images):
                R.render_frame_device(cam, p, sync=False)
                twin.R.render_frame_device(cam, q, sync=False)
            assert R.remove(mask, index_map=pm, n=n) == len(want) == R.n
            twin.R.upload(want)
            for p, q in zip(images, twin_images):                     # queued before the removal: the scene as it was
                assert np.array_equal(R.device_download(p, h, w), rest[0])
                assert np.array_equal(twin.R.device_download(q, h, w), rest[0])
            # the memory of what went is given back: a twin that uploaded the survivors over the same scene holds as much
            assert R.device_bytes()[0] == twin.R.device_bytes()[0]
        finally:
            for p in images:
                R.device_free(p)
            for q in twin_images:
                twin.R.device_free(q)
        assert np.array_equal(s.fetch(pm, n, np.uint32), want_map)
        retained = R.frames_retained()
        want_img = frame(ref, make_camera(h, w), h, w)
        assert want_img.any() and not np.array_equal(want_img, rest[0])
        assert np.array_equal(rest_frame(), want_img)
        assert R.frames_retained() == retained, "the frame after a removal is binned, not retained"
        more = [rest_frame() for _ in range(STILL + 4)]
        assert all(np.array_equal(f, want_img) for f in more)
        assert R.frames_retained() > retained and R.frames_dropped() == 0
        R.sync()


def test_storage_without_a_frame_is_the_twins():
    n = 1000
    A = in_view(n, 8401)
    gone = np.arange(n) % 3 != 0
    want, _ = RC.removed(A, gone, False)
    with session() as s, session() as twin:
        s.R.upload(A)
        twin.R.upload(A)
        twin.alloc(n + 32, 0xFF)
        assert remove(s, gone, False, with_map=False)[0] == len(want)
        twin.R.upload(want)
        assert s.R.device_bytes()[0] == twin.R.device_bytes()[0]
        # ... and a context that never held the larger scene holds no more per Gaussian either
        assert_resident(s, want, "storage")


def test_torch_masks_on_a_side_stream():
    import torch
    n = 1000
    A = in_view(n, 8501)
    dev = torch.device("cuda", 0)
    gone = np.random.default_rng(8502).random(n) < 0.5
    want, want_map = RC.removed(A, gone, False)
    with session() as s, fresh_upload(want) as ref:
        s.R.upload(A)
        side = torch.cuda.Stream(device=dev)
        host = torch.from_numpy(gone).pin_memory()
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        index_map = torch.full((n,), 7, dtype=torch.int32, device=dev)
        junk = torch.zeros(16 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(10):                                        # work in front of the copy: it has not run when the call is made
                junk.add_(1.0)
            mask.copy_(host, non_blocking=True)
        assert s.R.remove(mask, index_map=index_map, stream=side) == len(want) == s.R.n
        assert np.array_equal(index_map.cpu().numpy().view(np.uint32), want_map)
        with pytest.raises(ValueError):
            s.R.remove(mask)                                           # n bytes are not the scene's n' any more
        assert_same_frames(frames(s.R), frames(ref), "torch mask")
        del mask, index_map, junk
