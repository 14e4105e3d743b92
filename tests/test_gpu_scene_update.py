"""A resident scene edited in place (splat_update_scene_device, splat_update_gaussians_device, -m gpu).  The reference is
always a FRESH Renderer that takes the edited arrays through splat_upload_scene -- the host path, the specification: the
frames, the records, the tile lists and the block bounds after an edit must be its, bit for bit, although the edited scene
keeps the order of the upload it began with.  Nothing here has a tolerance.  Scenes are as small as the block logic allows
(n in 1, 255, 256, 257, 1000: one block, a full block, a block plus one, three blocks and a partial one), targets
128 x 96 and 256 x 160."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from helpers import make_camera, with_oracle_cov3d

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (1, 255, 256, 257, 1000)
TARGETS = ((96, 128), (160, 256))                    # (h, w)
FIELDS = {"positions": _lib.FIELD_POS, "cov3d": _lib.FIELD_COV3D, "opacities": _lib.FIELD_OPACITY, "sh": _lib.FIELD_SH}
MODE_LIBM_EXP = 2


# ---- plumbing -------------------------------------------------------------------------------------------------------
class Session:
    """a Renderer and the device buffers made on it, released together (the buffers first)"""

    def __init__(self, **conventions):
        self.R = splat_amd.Renderer(**conventions)
        self._held = []

    def device(self, g):
        d = g.to_device(self.R)
        self._held.append(d.free)
        return d

    def array(self, a):
        """device copy of a numpy array; returns its address"""
        a = np.ascontiguousarray(a)
        R = self.R
        p = R._L.splat_device_alloc(R._h, max(a.nbytes, 4))
        assert p
        self._held.append(lambda: R.device_free(p))
        if a.nbytes:
            R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def close(self):
        for free in reversed(self._held):
            free()
        self._held = []
        self.R.close()


@contextlib.contextmanager
def session(**conventions):
    s = Session(**conventions)
    try:
        yield s
    finally:
        s.close()


@contextlib.contextmanager
def fresh_upload(g, **conventions):
    """the reference: a fresh Renderer that takes g through splat_upload_scene"""
    R = splat_amd.Renderer(**conventions)
    try:
        R.upload(g)
        yield R
    finally:
        R.close()


def cameras(h, w):
    """at rest in front of the scene, turned, INSIDE the scene, and close"""
    return [make_camera(h, w), make_camera(h, w, yaw=math.radians(10.0)), make_camera(h, w, (0.3, 0.2, 0.4), 1.0, -0.2),
            make_camera(h, w, (0.0, 0.0, 3.0), pitch=0.1)]


def frame(R, cam, h, w):
    img = np.full((h, w), 0xDEADBEEF, np.uint32)
    R.render_frame(cam.to_c(0.01, 15), img)
    return img


def frames(R):
    return [frame(R, cam, h, w) for (h, w) in TARGETS for cam in cameras(h, w)]


def assert_same_frames(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s frame %d: %d pixels differ" % (what, k, int((a != b).sum()))


def stage(R, h=160, w=256):
    """(image, records, tile offsets, tile order) of one frame rendered with statistics"""
    img = np.zeros((h, w), np.uint32)
    st = R.render(make_camera(h, w).to_c(0.01, 15), img)
    n_tiles = ((h + _lib.TILE - 1) // _lib.TILE) * ((w + _lib.TILE - 1) // _lib.TILE)
    if st.n_pairs == 0:                               # (no list to fetch)
        return img, R.records(), np.zeros(n_tiles + 1, np.uint32), np.zeros(0, np.uint32)
    off, order = R.tile_lists(n_tiles, st.n_pairs)
    return img, R.records(), off, order


def assert_same_stage(R, ref, what=""):
    (ia, ra, oa, la), (ib, rb, ob, lb) = stage(R), stage(ref)
    assert np.array_equal(ia, ib), what
    # depth and pixel rectangle exist for every Gaussian; the rest of a record is K1's, which writes none for a Gaussian
    # it culls: compared where the frame defined it (as tests/test_gpu_device_upload.py does)
    assert ra["depth"].tobytes() == rb["depth"].tobytes(), what
    seen = ra["px0"] <= ra["px1"]
    assert np.array_equal(seen, rb["px0"] <= rb["px1"]), what
    assert ra[seen].tobytes() == rb[seen].tobytes(), what
    assert np.array_equal(oa, ob) and np.array_equal(la, lb), what
    return int(seen.sum()), la.size


# ---- scenes ---------------------------------------------------------------------------------------------------------
def in_view(n, seed):
    return with_oracle_cov3d(splat_amd.synthetic_scene(n, seed))


def off_screen(n, seed):
    """a small cluster far along the vertical axis, which every camera of cameras() looks across: none sees it, and its
    blocks' bounds say so"""
    g = in_view(n, seed)
    rng = np.random.default_rng(seed)
    g.positions[:, :3] = np.array([0.0, 300.0, 0.0], f32) + (0.01 * rng.standard_normal((n, 3))).astype(f32)
    return g


def copy_of(g):
    return splat_amd.GaussianList(g.positions.copy(), g.scales.copy(), g.opacities.copy(), g.rotations.copy(), g.sh.copy(), g.cov3d.copy())


def with_field(a, b, field, rows=None):
    """a copy of a with `field` (all rows, or the rows named) taken from b"""
    e = copy_of(a)
    if rows is None:
        getattr(e, field)[...] = getattr(b, field)
    else:
        getattr(e, field)[rows] = getattr(b, field)[rows]
    return e


def spoil(g, orig=None):
    """signed zeros, NaN and inf coordinates, a NaN and an inf covariance; with orig (n >= 512): the second block of that
    order loses every finite centre"""
    n = len(g)
    rng = np.random.default_rng(n)
    p = g.positions
    if n >= 8:
        z = rng.choice(n, n // 4, replace=False)
        p[z[: len(z) // 2], 0] = f32(0.0)
        p[z[len(z) // 2:], 0] = f32(-0.0)
        p[z[: len(z) // 3], 1] = f32(-0.0)
        p[z[len(z) // 3:], 1] = f32(0.0)
        for v in (np.nan, np.inf, -np.inf):
            idx = rng.choice(n, max(1, n // 50), replace=False)
            p[idx, rng.integers(0, 3, len(idx))] = f32(v)
    if orig is not None and n >= 512:
        p[orig[256:512], :3] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), (256, 3))
    if n >= 8:                                        # (at finite centres: a Gaussian without one is skipped, covariance and all)
        ok = np.flatnonzero(np.isfinite(p[:, :3]).all(1))
        g.cov3d[ok[len(ok) // 3], 4] = np.nan
        g.cov3d[ok[2 * len(ok) // 3], 0] = np.inf
    return g


def block_bounds_np(pos4, cov3d, orig):
    """block_bounds of the library's host upload, restated: per block of 256 slots of `orig`, keep-first min and max over
    the finite centres, the nine squares summed in float64 in order, float32(sqrt) * float32(1.0001), NaN -> inf, and a NaN
    box for a block without a finite centre"""
    n = len(orig)
    out = np.zeros(((n + 255) // 256, 8), f32)
    inf = f32(np.inf)
    for b in range(out.shape[0]):
        lo, hi, fmax = [inf] * 3, [-inf] * 3, f32(0.0)
        for i in orig[256 * b: min(n, 256 * (b + 1))]:
            p = pos4[i, :3]
            if not np.isfinite(p).all():
                continue
            for a in range(3):
                if p[a] < lo[a]:                      # std::min(lo, p): the earlier of two equal values stays
                    lo[a] = p[a]
                if hi[a] < p[a]:
                    hi[a] = p[a]
            f2 = np.float64(0.0)
            for e in range(9):
                v = np.float64(cov3d[i, e])
                with np.errstate(all="ignore"):
                    f2 = f2 + v * v
            with np.errstate(all="ignore"):
                f = f32(f32(np.sqrt(f2)) * f32(1.0001))
            if not (f >= 0):
                f = inf
            if fmax < f:
                fmax = f
        if not (lo[0] <= hi[0]):
            lo, hi = [f32(np.nan)] * 3, [f32(np.nan)] * 3
        out[b] = np.array(lo + hi + [fmax, f32(0.0)], f32)
    return out


def assert_bounds(got, want, what="", blocks=None):
    sel = slice(None) if blocks is None else blocks
    got, want = np.ascontiguousarray(got[sel]), np.ascontiguousarray(want[sel])
    assert got.shape == want.shape, what
    nan = np.isnan(got) & np.isnan(want)              # NaN matches NaN, whatever its payload
    bits = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bits.any(), "%s: bounds differ in %d words, first block %d: got %r, want %r" % (
        what, int(bits.sum()), np.argwhere(bits)[0][0], got[np.argwhere(bits)[0][0]], want[np.argwhere(bits)[0][0]])


def update_all(s, g, fields=("positions", "cov3d", "opacities", "sh")):
    d = s.device(g)
    s.R.update_device(n=len(g), **{f: getattr(d, f) for f in fields})


# ---- 1. whole-field update under a stale order ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, MODE_LIBM_EXP], ids=["default", "libm_exp"])
@pytest.mark.parametrize("n", SIZES)
def test_whole_field_update_under_a_stale_order(n, mode):
    A, B = off_screen(n, 100 + n), in_view(n, 200 + n)
    with session(mode=mode) as s, fresh_upload(B, mode=mode) as ref:
        s.R.upload(A)
        orig_a, bounds_a = s.R.scene_layout()
        assert not any(img.any() for img in frames(s.R)), "scene A is meant to be off-screen"
        update_all(s, B)
        want = frames(ref)
        assert_same_frames(frames(s.R), want, "n=%d" % n)
        if n >= 255:
            assert any(img.any() for img in want), "scene B is meant to be in view (stale bounds would cull all of it)"
        seen, pairs = assert_same_stage(s.R, ref, "n=%d" % n)
        if n >= 255:
            assert seen > 0 and pairs > 0
        orig, bounds = s.R.scene_layout()
        assert np.array_equal(orig, orig_a), "the order must stay"
        assert_bounds(bounds, block_bounds_np(B.positions, B.cov3d, orig_a), "n=%d" % n)


# ---- 2. bounds, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_bounds_are_block_bounds_of_the_edited_values_under_the_kept_order(n):
    A = spoil(in_view(n, 300 + n))
    with session() as s:
        s.R.upload(A)
        orig_a, bounds_a = s.R.scene_layout()
        # the restatement against the existing path first
        assert_bounds(bounds_a, block_bounds_np(A.positions, A.cov3d, orig_a), "restatement, n=%d" % n)
        B = spoil(in_view(n, 400 + n), orig_a)
        update_all(s, B)
        orig, bounds = s.R.scene_layout()
        assert np.array_equal(orig, orig_a)
        want = block_bounds_np(B.positions, B.cov3d, orig_a)
        assert_bounds(bounds, want, "after the update, n=%d" % n)
        if n >= 512:
            assert np.isnan(want[1, :6]).all() and not np.isnan(want[0, :6]).any()
        if n >= 255:
            assert np.isinf(want[:, 6]).any()         # the NaN and the inf covariance: an unbounded extent
        # naming only one of the two is enough: the bounds come from the resident values
        C_ = spoil(in_view(n, 500 + n))
        update_all(s, C_, ("cov3d",))
        assert_bounds(s.R.scene_layout()[1], block_bounds_np(B.positions, C_.cov3d, orig_a), "cov3d alone, n=%d" % n)
        update_all(s, C_, ("positions",))
        assert_bounds(s.R.scene_layout()[1], block_bounds_np(C_.positions, C_.cov3d, orig_a), "positions alone, n=%d" % n)


# ---- 3. each single field ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (257, 1000))
@pytest.mark.parametrize("field", list(FIELDS))
def test_each_single_field(field, n):
    A, B = in_view(n, 600 + n), in_view(n, 700 + n)
    E = with_field(A, B, field)
    with session() as s, fresh_upload(E) as ref:
        s.R.upload(A)
        orig_a, bounds_a = s.R.scene_layout()
        update_all(s, B, (field,))                    # (the other three buffers of B are on the device too, and not named)
        want = frames(ref)
        assert any(img.any() for img in want)
        assert_same_frames(frames(s.R), want, field)
        seen, pairs = assert_same_stage(s.R, ref, field)   # the shared float4s kept their other halves: records and frames say so
        assert seen > 0 and pairs > 0
        orig, bounds = s.R.scene_layout()
        assert np.array_equal(orig, orig_a)
        assert_bounds(bounds, block_bounds_np(E.positions, E.cov3d, orig_a), field)
        if field in ("opacities", "sh"):
            assert_bounds(bounds, bounds_a, field)


# ---- 4. depth ties ----------------------------------------------------------------------------------------------------
def test_depth_ties_follow_the_original_index_under_the_kept_order():
    n = 1000
    A = in_view(n, 810)
    rng = np.random.default_rng(811)
    site = rng.integers(0, 27, n)                     # a 3 x 3 x 3 lattice: ~37 Gaussians of different colour at every site
    A.positions[:, 0] = (site % 3 - 1).astype(f32) * f32(0.5)
    A.positions[:, 1] = (site // 3 % 3 - 1).astype(f32) * f32(0.5)
    A.positions[:, 2] = (site // 9 - 1).astype(f32) * f32(0.5)
    A.cov3d[:] = A.cov3d[0]                           # the same footprint, the same opacity: only the order tells them apart
    A.cov3d *= f32(40.0)
    A.opacities[:] = f32(0.6)
    perm = rng.permutation(n)
    B = copy_of(A)
    B.positions[:] = A.positions[perm]                # which original index sits where is permuted
    assert len(np.unique(A.positions[:, :3], axis=0)) == 27
    with session() as s, fresh_upload(B) as ref:
        s.R.upload(A)
        before = frames(s.R)
        update_all(s, B, ("positions",))
        want = frames(ref)
        assert any(img.any() for img in want)
        assert any(not np.array_equal(a, b) for a, b in zip(before, want)), "the permutation is meant to change the frames"
        assert_same_frames(frames(s.R), want, "ties")
        assert_same_stage(s.R, ref, "ties")


# ---- 5. by index ------------------------------------------------------------------------------------------------------
def index_cases(n, orig):
    """k = 1; k = 37 spread over all blocks (slots less than a block apart, the first and the last among them); k = n in
    reversed order; indices confined to the last, partial block"""
    spread = orig[np.unique(np.linspace(0, n - 1, 37).astype(np.int64))]
    last0 = 256 * ((n + 255) // 256 - 1)
    return [("k=1", orig[n // 2: n // 2 + 1]), ("k=37 over all blocks", spread), ("k=n reversed", np.arange(n, dtype=np.uint32)[::-1]),
            ("the last block", orig[last0:][::2])]


@pytest.mark.parametrize("n", SIZES)
def test_indexed_update(n):
    A, B = in_view(n, 900 + n), in_view(n, 1000 + n)
    with session() as s:
        s.R.upload(A)
        orig_a, _ = s.R.scene_layout()
        slot_of = np.empty(n, np.int64)
        slot_of[orig_a] = np.arange(n)
        E = copy_of(A)
        for what, idx in index_cases(n, orig_a):
            idx = np.ascontiguousarray(idx, np.uint32)
            assert len(np.unique(idx)) == len(idx) and len(idx) >= 1
            bounds_before = s.R.scene_layout()[1]
            for f in FIELDS:
                getattr(E, f)[idx] = getattr(B, f)[idx]
            s.R.update_indexed(s.array(idx), k=len(idx), positions=s.array(B.positions[idx]), cov3d=s.array(B.cov3d[idx]),
                               opacities=s.array(B.opacities[idx]), sh=s.array(B.sh[idx]))
            orig, bounds = s.R.scene_layout()
            assert np.array_equal(orig, orig_a), what
            assert_bounds(bounds, block_bounds_np(E.positions, E.cov3d, orig_a), what)
            untouched = np.setdiff1d(np.arange(bounds.shape[0]), np.unique(slot_of[idx] // 256))
            if what == "the last block" and bounds.shape[0] > 1:
                assert untouched.size == bounds.shape[0] - 1
            assert_bounds(bounds, bounds_before, what + " (blocks without an edited slot)", untouched)
            with fresh_upload(E) as ref:
                assert_same_frames(frames(s.R), frames(ref), what)
                assert_same_stage(s.R, ref, what)
            B = in_view(n, 1100 + n + len(idx))       # other values for the next case
        # a single field by index keeps the rest of the shared float4s
        idx = np.ascontiguousarray(orig_a[::3], np.uint32)
        E.opacities[idx] = B.opacities[idx]
        s.R.update_indexed(s.array(idx), k=len(idx), opacities=s.array(B.opacities[idx]))
        E.cov3d[idx] = B.cov3d[idx]
        s.R.update_indexed(s.array(idx), k=len(idx), cov3d=s.array(B.cov3d[idx]))
        assert_bounds(s.R.scene_layout()[1], block_bounds_np(E.positions, E.cov3d, orig_a), "cov3d by index")
        with fresh_upload(E) as ref:
            assert_same_frames(frames(s.R), frames(ref), "single fields by index")
            assert_same_stage(s.R, ref, "single fields by index")


def test_an_index_out_of_range_applies_nothing():
    n = 1000
    A, B = in_view(n, 1201), in_view(n, 1202)
    with session() as s:
        s.R.upload(A)
        before = frames(s.R)
        layout = s.R.scene_layout()
        idx = np.arange(100, dtype=np.uint32)
        idx[57] = n                                   # the first index that names no Gaussian
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.update_indexed(s.array(idx), k=len(idx), positions=s.array(B.positions[:100]), cov3d=s.array(B.cov3d[:100]),
                               opacities=s.array(B.opacities[:100]), sh=s.array(B.sh[:100]))
        assert e.value.code == _lib.ERR_INVALID
        assert_same_frames(frames(s.R), before, "after the refused edit")
        after = s.R.scene_layout()
        assert np.array_equal(after[0], layout[0])
        assert_bounds(after[1], layout[1], "after the refused edit")
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.update_indexed(s.array(np.zeros(n + 1, np.uint32)), k=n + 1, opacities=s.array(np.zeros(n + 1, f32)))
        assert e.value.code == _lib.ERR_INVALID       # more indices than Gaussians cannot be distinct


# ---- 6. state and storage ---------------------------------------------------------------------------------------------
def test_frames_in_flight_state_and_storage():
    n, (h, w) = 1000, TARGETS[1]
    A, B = in_view(n, 1301), in_view(n, 1302)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s, fresh_upload(B) as ref:
        R = s.R
        R.upload(A)
        rest = [frame(R, make_camera(h, w), h, w) for _ in range(6)]        # a camera at rest: hints are armed
        assert rest[0].any() and all(np.array_equal(rest[0], f) for f in rest)
        d = s.device(B)
        images = [R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        dropped, held = R.frames_dropped(), R.device_bytes()[0]
        try:
            for p in images:
                R.render_frame_device(cam, p, sync=False)
            R.update_device(d.positions, d.cov3d, d.opacities, d.sh, n=n)
            assert R.device_bytes()[0] == held, "a whole-field update allocates nothing"
            for p in images:                          # queued before the edit: the scene as it was
                assert np.array_equal(R.device_download(p, h, w), rest[0])
        finally:
            for p in images:
                R.device_free(p)
        want = frame(ref, make_camera(h, w), h, w)
        assert want.any() and not np.array_equal(want, rest[0])
        assert np.array_equal(frame(R, make_camera(h, w), h, w), want)
        assert np.array_equal(frame(R, make_camera(h, w), h, w), want)
        idx = s.array(np.arange(10, dtype=np.uint32))
        op = s.array(B.opacities[:10])
        held = R.device_bytes()[0]
        R.update_indexed(idx, k=10, opacities=op)     # the first indexed edit of a scene makes the inverse order
        first = R.device_bytes()[0]
        assert 4 * n + (n + 255) // 256 <= first - held <= 4 * n + (n + 255) // 256 + 64      # 4 B per Gaussian, a byte per block
        R.update_indexed(idx, k=10, opacities=op)
        R.update_device(opacities=d.opacities, n=n)
        assert R.device_bytes()[0] == first, "later edits allocate nothing"
        assert np.array_equal(frame(R, make_camera(h, w), h, w), want)
        assert R.frames_dropped() == dropped
        R.sync()


# ---- 7. refusals with a live context ----------------------------------------------------------------------------------
def test_refusals_with_a_live_context():
    n = 1000
    A, B = in_view(n, 1401), in_view(n, 1402)
    (h, w) = TARGETS[0]
    with session() as s, session() as empty:
        R = s.R
        R.upload(A)
        d = s.device(B)
        before = frame(R, make_camera(h, w), h, w)
        held = R.device_bytes()
        p = C.c_void_p

        def code(call, *a, **kw):
            with pytest.raises(splat_amd.SplatError) as e:
                call(*a, **kw)
            return e.value.code

        assert code(R.update_device, positions=d.positions, n=n + 1) == _lib.ERR_INVALID              # a wrong n
        assert code(R.update_device, positions=d.positions, n=n - 1) == _lib.ERR_INVALID
        assert code(R.update_device, positions=0, n=n) == _lib.ERR_INVALID                            # a named field's pointer NULL
        assert code(R.update_indexed, d.positions, k=4, sh=0) == _lib.ERR_INVALID
        assert code(R.update_indexed, 0, k=4, sh=d.sh) == _lib.ERR_INVALID                            # NULL index
        L = R._L
        assert L.splat_update_scene_device(R._h, n, 16, p(d.positions), p(d.cov3d), p(d.opacities), p(d.sh), None) == _lib.ERR_INVALID
        assert L.splat_update_gaussians_device(R._h, 4, p(d.positions), 31, p(d.positions), p(d.cov3d), p(d.opacities), p(d.sh),
                                               None) == _lib.ERR_INVALID                              # an unknown field bit
        # a context without a scene (the buffers are another context's allocations: nothing touches them)
        assert code(empty.R.update_device, positions=d.positions, n=n) == _lib.ERR_NO_SCENE
        assert code(empty.R.update_indexed, d.positions, k=4, sh=d.sh) == _lib.ERR_NO_SCENE
        # nothing to do
        R.update_device(n=n)
        assert L.splat_update_gaussians_device(R._h, 0, None, 15, None, None, None, None, None) == _lib.SPLAT_OK
        assert L.splat_update_gaussians_device(R._h, 4, p(d.positions), 0, None, None, None, None, None) == _lib.SPLAT_OK
        assert R.device_bytes() == held
        assert np.array_equal(frame(R, make_camera(h, w), h, w), before)


# ---- 8. the Python surface --------------------------------------------------------------------------------------------
def test_device_gaussians_refresh():
    n = 1000
    A, B = in_view(n, 1501), in_view(n, 1502)
    E = with_field(A, B, "positions")
    with session() as s, session() as t:
        d = s.device(A).upload()
        d.update("positions", B.positions)
        d.refresh("positions")
        t.device(E).upload()
        assert_same_frames(frames(s.R), frames(t.R), "refresh(positions)")
        for f in ("cov3d", "opacities", "sh"):
            d.update(f, getattr(B, f))
        d.refresh()                                   # all four
        t.R.upload(B)
        assert_same_frames(frames(s.R), frames(t.R), "refresh()")
        with pytest.raises(ValueError):
            d.refresh("scales")


def test_update_device_takes_torch_tensors_written_on_a_side_stream():
    import torch
    n = 1000
    A, B = in_view(n, 1601), in_view(n, 1602)
    with session() as s, fresh_upload(B) as ref:
        s.R.upload(A)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        host = [torch.from_numpy(a).pin_memory() for a in (B.positions, B.cov3d, B.opacities, B.sh)]
        bufs = [torch.full(h.shape, float("nan"), dtype=torch.float32, device=dev) for h in host]
        junk = torch.zeros(16 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(10):                       # work in front of the copies: they have not run when the call is made
                junk.add_(1.0)
            for b, h in zip(bufs, host):
                b.copy_(h, non_blocking=True)
        s.R.update_device(*bufs, stream=side)
        want = frames(ref)
        assert_same_frames(frames(s.R), want, "side stream")
        # ... and by index, the indices a torch tensor as well
        idx = torch.arange(0, n, 7, dtype=torch.int32, device=dev)
        rows = torch.from_numpy(A.sh[::7].copy()).to(dev)
        s.R.update_indexed(idx, sh=rows)
        with fresh_upload(with_field(B, A, "sh", np.arange(0, n, 7))) as ref2:
            assert_same_frames(frames(s.R), frames(ref2), "torch indices")
        del bufs, junk, idx, rows
