"""The resident scene read back (splat_read_scene_device, splat_read_gaussians_device, -m gpu): what comes back is what the
uploads and edits put there, byte for byte, in original index order or as compact rows; a buffer that is not named keeps its
sentinel; a read changes nothing a frame depends on.  Nothing here has a tolerance.  Scenes and targets are those of
tests/test_gpu_scene_update.py (n in 1, 255, 256, 257, 1000)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from helpers import make_camera
import transform_cases as T
from scene_gpu import (FIELDS, PER, SENTINEL, SIZES, TARGETS, assert_resident, assert_same_bits, assert_same_frames, copy_of, frame,
                       frames, in_view, index_sets, session)
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32 = np.float32
BIT = {"positions": _lib.FIELD_POS, "cov3d": _lib.FIELD_COV3D, "opacities": _lib.FIELD_OPACITY, "sh": _lib.FIELD_SH}


def shape_of(f, rows):
    return (rows,) if PER[f] == 1 else (rows, PER[f])


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all()


# ---- 1. after each kind of upload ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_read_after_upload_and_upload_device(n):
    g = in_view(n, 2100 + n)
    g.positions[:, 3] = f32(7.0)                      # the uploads never read w; the read gives 1
    with session() as s:
        s.R.upload(g)
        got = assert_resident(s, g, "upload, n=%d" % n)
        assert (got["positions"][:, 3] == f32(1.0)).all()
    with session() as s:
        s.device(g).upload()
        assert_resident(s, g, "upload_device, n=%d" % n)


@pytest.mark.parametrize("n", (257, 1000))
def test_read_after_load_ply(n, tmp_path):
    path = str(tmp_path / "scene.ply")
    splat_amd.write_ply(path, splat_amd.synthetic_raw(n, 2200 + n), n)
    g = splat_amd.load_from_ply(path)                 # the host loader: the activated, recentred arrays the caller never had
    with session() as s:
        g.compute_cov3d(s.R)                          # (kernel K0, as load_ply runs it)
        assert s.R.load_ply(path) == n
        assert_resident(s, g, "load_ply, n=%d" % n)


# ---- 2. after an edit ---------------------------------------------------------------------------------------------------
def test_the_read_shows_an_indexed_update():
    n = 1000
    A, B = in_view(n, 2301), in_view(n, 2302)
    idx = np.random.default_rng(2303).permutation(n)[:300].astype(np.uint32)
    E = copy_of(A)
    for f in FIELDS:
        getattr(E, f)[idx] = getattr(B, f)[idx]
    with session() as s:
        s.R.upload(A)
        s.R.update_indexed(s.array(idx), k=len(idx), **{f: s.array(getattr(B, f)[idx]) for f in FIELDS})
        assert_resident(s, E, "after update_indexed")


# ---- 3. every subset of fields, whole and by index -----------------------------------------------------------------------
def test_every_subset_of_fields_leaves_the_others_untouched():
    n = 257
    g = in_view(n, 2401)
    idx = np.random.default_rng(2402).permutation(n)[:100].astype(np.uint32)
    with session() as s:
        s.R.upload(g)
        d_idx = s.array(idx)
        for r in range(len(FIELDS) + 1):
            for named in itertools.combinations(FIELDS, r):
                for rows, read in ((n, lambda **kw: s.R.read_device(n=n, **kw)), (len(idx), lambda **kw: s.R.read_indexed(d_idx, k=len(idx), **kw))):
                    bufs = {f: s.alloc(4 * PER[f] * rows, SENTINEL) for f in FIELDS}
                    read(**{f: bufs[f] for f in named})           # the others: None, a NULL pointer
                    for f in FIELDS:
                        got = s.fetch(bufs[f], shape_of(f, rows))
                        if f not in named:
                            assert untouched(got), (named, f, rows)
                            continue
                        want = getattr(g, f) if rows == n else getattr(g, f)[idx]
                        if f == "positions":
                            want = want.copy()
                            want[:, 3] = f32(1.0)
                        assert_same_bits(got, want, "%r %s rows=%d" % (named, f, rows))
        # ... and with every pointer given but only one field named, through the C call
        p = C.c_void_p
        for f in FIELDS:
            bufs = {x: s.alloc(4 * PER[x] * n, SENTINEL) for x in FIELDS}
            rc = s.R._L.splat_read_scene_device(s.R._h, n, BIT[f], *[p(bufs[x]) for x in FIELDS])
            assert rc == _lib.SPLAT_OK
            for x in FIELDS:
                assert untouched(s.fetch(bufs[x], shape_of(x, n))) == (x != f), (f, x)


# ---- 4. by index ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_read_indexed_equals_fancy_indexing(n):
    g = in_view(n, 2500 + n)
    cases = index_sets(n, 2600 + n)
    if n > 1:
        dup = np.random.default_rng(n).integers(0, n, min(300, n)).astype(np.uint32)      # drawn with replacement
        dup[-1] = dup[0]
        assert len(np.unique(dup)) < len(dup)
        cases.append(dup)
    with session() as s:
        s.R.upload(g)
        for idx in cases:
            k = len(idx)
            bufs = {f: s.alloc(4 * PER[f] * max(k, 1), SENTINEL) for f in FIELDS}
            s.R.read_indexed(s.array(idx) if k else 0, k=k, **bufs)
            for f in FIELDS:
                got = s.fetch(bufs[f], shape_of(f, max(k, 1)))
                if k == 0:
                    assert untouched(got), f
                    continue
                want = getattr(g, f)[idx.astype(np.int64)]
                if f == "positions":
                    want = want.copy()
                    want[:, 3] = f32(1.0)
                assert_same_bits(got, want, "n=%d k=%d %s" % (n, k, f))


def test_a_bad_index_writes_nothing():
    n = 1000
    g = in_view(n, 2701)
    with session() as s:
        s.R.upload(g)
        idx = np.arange(100, dtype=np.uint32)
        idx[57] = n                                   # the first index that names no Gaussian
        bufs = {f: s.alloc(4 * PER[f] * 100, SENTINEL) for f in FIELDS}
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.read_indexed(s.array(idx), k=100, **bufs)
        assert e.value.code == _lib.ERR_INVALID
        for f in FIELDS:
            assert untouched(s.fetch(bufs[f], shape_of(f, 100))), f


def test_refusals_with_a_live_context():
    n = 257
    g = in_view(n, 2801)
    with session() as s, session() as empty:
        R, L, p = s.R, s.R._L, C.c_void_p
        R.upload(g)
        bufs = {f: s.alloc(4 * PER[f] * n, SENTINEL) for f in FIELDS}
        four = [p(bufs[f]) for f in FIELDS]
        m = (C.c_float * 12)(*T.MATRICES["identity"].ravel())

        def code(call, *a, **kw):
            with pytest.raises(splat_amd.SplatError) as e:
                call(*a, **kw)
            return e.value.code

        assert code(R.read_device, positions=bufs["positions"], n=n + 1) == _lib.ERR_INVALID          # a wrong n
        assert code(R.read_device, positions=0, n=n) == _lib.ERR_INVALID                              # a named field's pointer NULL
        assert code(R.read_indexed, 0, k=4, sh=bufs["sh"]) == _lib.ERR_INVALID                        # NULL index
        assert code(R.read_indexed, bufs["sh"], k=n + 1, opacities=bufs["sh"]) == _lib.ERR_INVALID    # k > n
        assert L.splat_read_scene_device(R._h, n, 16, *four) == _lib.ERR_INVALID                      # an unknown field bit
        assert L.splat_read_gaussians_device(R._h, 4, p(bufs["sh"]), 31, *four, None) == _lib.ERR_INVALID
        assert L.splat_transform_scene_device(R._h, None) == _lib.ERR_INVALID                         # NULL matrix
        assert L.splat_transform_gaussians_device(R._h, 4, None, m, None) == _lib.ERR_INVALID         # NULL index
        assert L.splat_transform_gaussians_device(R._h, n + 1, p(bufs["sh"]), m, None) == _lib.ERR_INVALID
        with pytest.raises(ValueError):
            R.transform(np.eye(4, dtype=f32) * 2)     # a 4x4 whose last row is not 0 0 0 1
        with pytest.raises(ValueError):
            R.transform(np.eye(3))
        assert code(empty.R.read_device, positions=bufs["positions"], n=n) == _lib.ERR_NO_SCENE
        assert code(empty.R.read_indexed, bufs["sh"], k=4, sh=bufs["sh"]) == _lib.ERR_NO_SCENE
        assert code(empty.R.transform, T.MATRICES["scale"]) == _lib.ERR_NO_SCENE
        assert code(empty.R.transform, T.MATRICES["scale"], bufs["sh"], k=4) == _lib.ERR_NO_SCENE
        # nothing to do
        R.read_device(n=n)
        assert L.splat_read_gaussians_device(R._h, 0, None, 15, None, None, None, None, None) == _lib.SPLAT_OK
        assert L.splat_read_gaussians_device(R._h, 4, p(bufs["sh"]), 0, None, None, None, None, None) == _lib.SPLAT_OK
        assert L.splat_transform_gaussians_device(R._h, 0, None, m, None) == _lib.SPLAT_OK
        for f in FIELDS:
            assert untouched(s.fetch(bufs[f], shape_of(f, n))), f
        assert_resident(s, g, "after the refusals")


# ---- 5. read, then update ---------------------------------------------------------------------------------------------------
def test_updating_what_was_read_leaves_the_frames_unchanged():
    n = 1000
    g = in_view(n, 2901)
    idx = np.random.default_rng(2902).permutation(n)[:300].astype(np.uint32)
    with session() as s:
        s.R.upload(g)
        before = frames(s.R)
        assert any(img.any() for img in before)
        d_idx = s.array(idx)
        bufs = {f: s.alloc(4 * PER[f] * len(idx), SENTINEL) for f in FIELDS}
        s.R.read_indexed(d_idx, k=len(idx), **bufs)
        s.R.update_indexed(d_idx, k=len(idx), **bufs)
        assert_same_frames(frames(s.R), before, "read_indexed -> update_indexed")
        d = s.device(in_view(n, 2903))                # other values, overwritten by pull()
        d.pull()
        d.refresh()
        assert_same_frames(frames(s.R), before, "pull -> refresh")
        assert_resident(s, g, "after both round trips")
        with pytest.raises(ValueError):
            d.pull("scales")


# ---- 6. a read changes nothing -----------------------------------------------------------------------------------------------
def test_a_read_changes_nothing_a_frame_depends_on():
    n, (h, w) = 1000, TARGETS[1]
    g = in_view(n, 3001)
    cam = make_camera(h, w).to_c(0.01, 15)
    with session() as s:
        R = s.R
        R.upload(g)
        img = R.host_image(h, w)

        def rest_frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam, img)
            return img.copy()

        rest = [rest_frame() for _ in range(STILL + 4)]
        assert rest[0].any() and all(np.array_equal(rest[0], f) for f in rest)
        retained = R.frames_retained()
        assert retained > 0, "the camera is at rest: its frames are meant to come from retained lists by now"
        idx = s.array(np.arange(0, n, 3, dtype=np.uint32))
        k = len(range(0, n, 3))
        bufs = {f: s.alloc(4 * PER[f] * n, SENTINEL) for f in FIELDS}
        held, dropped = R.device_bytes()[0], R.frames_dropped()
        R.read_device(n=n, **bufs)
        assert R.device_bytes()[0] == held, "a whole read allocates nothing"
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 1
        R.read_indexed(idx, k=k, **bufs)              # the first indexed read of a scene makes the inverse order
        first = R.device_bytes()[0]
        assert 4 * n + (n + 255) // 256 <= first - held <= 4 * n + (n + 255) // 256 + 64
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 2
        R.read_indexed(idx, k=k, **bufs)
        R.read_device(n=n, **bufs)
        assert R.device_bytes()[0] == first, "later reads allocate nothing"
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 3
        assert R.frames_dropped() == dropped
        # ... nor do asynchronous frames in flight lose anything: the read comes behind them
        images = [R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        try:
            for p in images:
                R.render_frame_device(cam, p, sync=False)
            R.read_device(n=n, **bufs)
            for p in images:
                assert np.array_equal(R.device_download(p, h, w), rest[0])
        finally:
            for p in images:
                R.device_free(p)
        R.sync()


# ---- 7. the probe: device compile against host compile -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.MATRICES))
def test_the_device_compile_of_the_math_is_the_host_compile(name):
    pos, cov = T.random_gaussians(4000, 31 + len(name))
    hp, hc = T.run_probe(T.MATRICES[name], pos, cov)
    dp, dc = T.run_probe(T.MATRICES[name], pos, cov, device=True)
    assert_same_bits(dp, hp, name + " positions")
    assert_same_bits(dc, hc, name + " covariances")
