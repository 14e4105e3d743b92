"""The pick on the GPU (splat_pick_device, Renderer.pick; -m gpu).

Every field of every result and every layer row written equals tests/pick_cases.reference_pick -- the oracle's records, the
oracle's fragment_n and numpy float32 for the order and the chain -- EXACTLY: the results and the layers are compared as
bytes, so integers are equal, floats are equal bit for bit, and a layer row that is not due still holds the sentinel it was
filled with.  Nothing here has a tolerance.  tests/test_pick_cases_host.py shows on the CPU that these cases have hits, empty
pixels, depth ties, deep surfaces and truncation to compare.

Shapes: clouds of 1, 255, 256, 257 (one block, a full one, one plus a Gaussian) and 3000 Gaussians at 64x48 and 40x24 under
four cameras, pixel sets of 1, 64, 65 and 256 (below, at and past a wave; the most a call takes); stacks of 5, 300 and 5000
Gaussians on one pixel (lists of 5, 300 -> 512 padded, 4000 -> 4096: the whole LDS list; 5000: past the cap)."""
import os
import re

import numpy as np
import pytest

import pick_cases as K
import scene_gpu
import splat_amd
from splat_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STILL = int(re.search(r"#define SPLAT_POLICY_STILL_FRAMES (\d+)", open(os.path.join(ROOT, "include", "splat_policy.h")).read()).group(1))
MODE_CORRECTED = 1
STACK_PARTIAL = {5: (34, 24), 5000: (33, 24)}      # a pixel that only some of the stack's Gaussians hit (3 and 422 of them)


# ---- plumbing -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    with scene_gpu.session() as s:
        yield s


def run_pick(s, cam_c, pixels, alpha_min=0.0, coverage_min=0.5, mask=None, max_hits=1024, max_layers=0):
    """(results, layers) as the library wrote them into sentinel-filled device buffers"""
    P = len(pixels)
    pr = s.alloc(32 * P, K.SENTINEL)
    pl = s.alloc(16 * P * max_layers, K.SENTINEL) if max_layers else None
    pm = s.array(np.asarray(mask, np.uint8)) if mask is not None else None
    assert s.R.pick(cam_c, pixels, alpha_min=alpha_min, coverage=coverage_min, mask=pm, max_hits=max_hits, layers=max_layers, results=pr,
                    layers_out=pl) is None
    res = s.fetch(pr, P, K.RESULT)
    lay = s.fetch(pl, (P, max_layers), K.LAYER) if max_layers else np.zeros((P, 0), K.LAYER)
    return res, lay


def assert_equal(got, want, what):
    """got and want: (results, layers); byte for byte"""
    (gr, gl), (wr, wl) = got, want
    assert gr.shape == wr.shape and gl.shape == wl.shape, what
    for p in range(len(wr)):
        assert gr[p].tobytes() == wr[p].tobytes(), "%s: pixel %d: got %r, want %r" % (what, p, gr[p], wr[p])
    if gl.size:
        bad = np.argwhere(gl.view(np.uint32).reshape(gl.shape + (4,)) != wl.view(np.uint32).reshape(wl.shape + (4,)))
        assert bad.size == 0, "%s: %d layer words differ, first (pixel, row, word) %r: got %r, want %r" % (
            what, len(bad), tuple(bad[0]), gl[bad[0][0], bad[0][1]], wl[bad[0][0], bad[0][1]])


def assert_pick(s, rec, conv, cam_c, pixels, what, **q):
    want = K.reference_pick(rec, conv, pixels, **q)
    assert_equal(run_pick(s, cam_c, pixels, **q), want[:2], what)
    return want


# ---- 1. clouds: every block edge, two targets, four cameras, every size of pixel set ----------------------------------------
@pytest.mark.parametrize("h,w", K.CLOUD_TARGETS)
@pytest.mark.parametrize("n", K.CLOUD_SIZES)
def test_clouds(S, n, h, w):
    g = K.cloud(n)
    S.R.upload(g)
    conv = O.default_conventions()
    pixels = K.pixel_set(K.MAX_PIXELS, w, h)
    seen = 0
    for ci, cam in enumerate(scene_gpu.cameras(h, w)):
        rec = K.records(g, cam)
        wr, wl, _ = K.reference_pick(rec, conv, pixels, max_layers=3)        # once per camera; the smaller sets are prefixes
        for count in K.PIXEL_COUNTS:
            sl = K.prefix(count)
            got = run_pick(S, cam.to_c(0.01, 15), K.pixel_set(count, w, h), max_layers=3)
            assert_equal(got, (wr[sl], wl[sl]), "n %d %dx%d camera %d, %d pixels" % (n, w, h, ci, count))
        seen += int(wr["n_hits"].sum())
    if n == 3000:
        assert seen > 1000


# ---- 2. stacks: long lists, depth ties, deep surfaces, layers ---------------------------------------------------------------
@pytest.mark.parametrize("layers", ("none", "one", "all"))
@pytest.mark.parametrize("k,opacity", K.STACKS[:2])
def test_stacks(S, k, opacity, layers):
    g = K.stack(k, opacity)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY, np.int32)
    ml = {"none": 0, "one": 1, "all": k}[layers]
    for max_hits in (k, K.MAX_HITS):
        res, lay, _ = assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels, "stack %d, max_hits %d" % (k, max_hits),
                                  max_hits=max_hits, max_layers=ml)
        assert (res["n_hits"][:2] == k).all() and (res["flags"] == 0).all()
        assert (res["surface_index"][:2] != res["front_index"][:2]).all()
        if ml:
            assert (lay[2:].view(np.uint8) == K.SENTINEL).all()              # the empty pixels' rows keep their fill


def test_the_whole_list_of_4096(S):
    # 4000 of the 5000 stack under a mask: the list is padded to 4096, all of the resolve kernel's LDS, and the surface lies deep
    k, opacity = K.STACKS[2]
    g = K.stack(k, opacity)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    mask = np.zeros(k, np.uint8)
    mask[np.random.default_rng(3).permutation(k)[:4000]] = 1
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY + (STACK_PARTIAL[k],), np.int32)
    res, lay, _ = assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels, "4000 of 5000", mask=mask, max_hits=K.MAX_HITS,
                              max_layers=100)
    assert (res["n_hits"][:2] == 4000).all() and (res["flags"] == 0).all() and (res["surface_index"][:2] != K.NONE).all()
    assert 0 < res["n_hits"][-1] < 4000


# ---- 3. truncation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,opacity,max_hits", ((5, 0.5, 1), (5, 0.5, 4), (5000, 0.01, 4096)))
def test_truncation(S, k, opacity, max_hits):
    g = K.stack(k, opacity)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY + (STACK_PARTIAL[k],), np.int32)
    for ml in (0, min(2, max_hits)):
        res, lay, lists = assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels, "stack %d, max_hits %d" % (k, max_hits),
                                      max_hits=max_hits, max_layers=ml)
        for p in (0, 1):                             # what the comparison above held the library to
            assert res[p]["flags"] == K.TRUNCATED and res[p]["n_hits"] == k and res[p]["front_index"] == k - 1
            assert res[p]["front_alpha"] == lists[p][2][0] > 0 and res[p]["surface_index"] == K.NONE
            assert res[p]["surface_depth"] == 0 and res[p]["surface_coverage"] == 0
            assert (lay[p].view(np.uint8) == K.SENTINEL).all()
        if max_hits > 1:                             # the other pixels of the same call are unaffected
            assert res[-1]["flags"] == 0 and 0 < res[-1]["n_hits"] <= max_hits and res[-1]["surface_coverage"] > 0
        assert (res["flags"][2:5] == 0).all() and (res["n_hits"][2:5] == 0).all()


# ---- 4. queries ------------------------------------------------------------------------------------------------------------------
def test_alpha_cuts(S):
    h, w = K.CLOUD_TARGETS[0]
    g = K.cloud(3000)
    S.R.upload(g)
    cam = scene_gpu.cameras(h, w)[0]
    rec = K.records(g, cam)
    pixels = K.pixel_set(K.MAX_PIXELS, w, h)
    for cut in (0.0, -1.0) + K.ALPHA_CUTS + (1.0, float("inf")):
        assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels, "alpha_min %r" % cut, alpha_min=cut, max_layers=2)
    # a cut ON an alpha that occurs: >= keeps it
    _, _, lists = K.reference_pick(rec, O.default_conventions(), pixels[4:5])
    a = float(lists[0][2][len(lists[0][2]) // 2])
    res, _, _ = assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels[4:5], "alpha_min on an alpha", alpha_min=a)
    assert res["n_hits"][0] == int((lists[0][2] >= f32(a)).sum()) > 0


@pytest.mark.parametrize("coverage_min", (0.5, 1.0, 1e-6, 0.9))
def test_coverage_thresholds(S, coverage_min):
    g = K.stack(300, 0.05)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY, np.int32)
    res, _, _ = assert_pick(S, rec, O.default_conventions(), cam.to_c(0.01, 15), pixels, "coverage_min %r" % coverage_min,
                            coverage_min=coverage_min, max_hits=300, max_layers=300)
    if coverage_min == 1.0:                          # never reached: NONE and the total coverage
        assert (res["surface_index"] == K.NONE).all() and (res["surface_coverage"][:2] > 0.99).all() and (res["surface_depth"] == 0).all()
    if coverage_min == 1e-6:                         # the front is the surface
        assert (res["surface_index"][:2] == res["front_index"][:2]).all() and (res["front_index"][:2] == 299).all()


def test_masks(S):
    g = K.stack(300, 0.05)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY, np.int32)
    conv = O.default_conventions()
    hide_front = np.ones(300, np.uint8)
    hide_front[299] = 0
    res, _, _ = assert_pick(S, rec, conv, cam.to_c(0.01, 15), pixels, "front hidden", mask=hide_front, max_layers=4)
    assert (res["front_index"][:2] == 298).all() and (res["n_hits"][:2] == 299).all()
    odd = (np.arange(300) % 2 * 255).astype(np.uint8)                        # (any nonzero byte selects)
    res, _, _ = assert_pick(S, rec, conv, cam.to_c(0.01, 15), pixels, "odd ones", mask=odd, max_layers=4)
    assert (res["n_hits"][:2] == 150).all()
    res, lay, _ = assert_pick(S, rec, conv, cam.to_c(0.01, 15), pixels, "all hidden", mask=np.zeros(300, np.uint8), max_layers=4)
    assert (res["n_hits"] == 0).all() and (res["front_index"] == K.NONE).all() and (lay.view(np.uint8) == K.SENTINEL).all()


# ---- 5. the resident values, not those of the upload --------------------------------------------------------------------------
def resident(s, n):
    r = s.read_all(n)
    return splat_amd.GaussianList(r["positions"], np.ones((n, 3), f32), r["opacities"], np.zeros((n, 4), f32), r["sh"], r["cov3d"])


def test_after_edits(S):
    h, w = K.CLOUD_TARGETS[0]
    g = K.cloud(3000)
    S.R.upload(g)
    cam = scene_gpu.cameras(h, w)[0]
    conv = O.default_conventions()
    pixels = K.pixel_set(64, w, h)
    before, _, _ = assert_pick(S, K.records(g, cam), conv, cam.to_c(0.01, 15), pixels, "as uploaded", max_layers=2)
    # the front Gaussians of the pixels that have one: opacity 0, by index
    fronts = np.unique(before["front_index"][before["n_hits"] > 0]).astype(np.uint32)
    assert fronts.size > 5
    S.R.update_indexed(S.array(fronts), opacities=S.array(np.zeros(fronts.size, f32)), k=fronts.size)
    e = resident(S, len(g))
    assert (e.opacities[fronts] == 0).all() and np.array_equal(e.positions[:, :3], g.positions[:, :3])
    after, _, _ = assert_pick(S, K.records(e, cam), conv, cam.to_c(0.01, 15), pixels, "fronts hidden", max_layers=2)
    assert not np.isin(after["front_index"], fronts).any() and (after["n_hits"] < before["n_hits"]).any()
    # ... and a selection moved and scaled
    sel = np.flatnonzero(g.positions[:, 0] > 0).astype(np.uint32)
    m = np.array([[1.5, 0, 0, -0.4], [0, 0.75, 0.1, 0.2], [0, 0, 1.25, 0.3]], f32)
    S.R.transform(m, index=S.array(sel), k=sel.size)
    t = resident(S, len(g))
    assert not np.array_equal(t.positions, e.positions)
    moved, _, _ = assert_pick(S, K.records(t, cam), conv, cam.to_c(0.01, 15), pixels, "a selection transformed", max_layers=2)
    assert moved.tobytes() != after.tobytes()


# ---- 6. conventions: each once on the 3000 cloud ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ctx,oracle", (("y_down", dict(y_up=0), dict(y_up=0)), ("corner_samples", dict(sample_half=0), dict(sample_half=0)),
                                             ("no_zclip", dict(zclip=0), dict(zclip=0)),
                                             ("corrected", dict(mode=MODE_CORRECTED), dict(corrected_projection=1))))
def test_conventions(name, ctx, oracle):
    h, w = K.CLOUD_TARGETS[0]
    g = K.cloud(3000)
    conv = O.default_conventions(**oracle)
    pixels = K.pixel_set(K.MAX_PIXELS, w, h)
    with scene_gpu.session(**ctx) as s:
        s.R.upload(g)
        for cam in scene_gpu.cameras(h, w)[1:3]:     # turned, and INSIDE the cloud (where the z-clip bites)
            res, _, _ = assert_pick(s, K.records(g, cam, conv), conv, cam.to_c(0.01, 15), pixels, name, max_layers=3)
            assert (res["n_hits"] > 1).any()


# ---- 7. the default route of Renderer.pick: numpy arrays --------------------------------------------------------------------------
def test_renderer_pick_returns_numpy(S):
    g = K.stack(300, 0.05)
    S.R.upload(g)
    cam = K.stack_camera()
    rec = K.records(g, cam)
    pixels = np.array(K.STACK_CENTRES + K.STACK_EMPTY, np.int32)
    held = S.R.device_bytes()[0]
    res = S.R.pick(cam.to_c(0.01, 15), [tuple(p) for p in pixels])
    want, _, _ = K.reference_pick(rec, O.default_conventions(), pixels)
    assert res.dtype == K.RESULT and res.tobytes() == want.tobytes()
    res, lay = S.R.pick(cam.to_c(0.01, 15), pixels, layers=7, max_hits=512)
    want, wl, _ = K.reference_pick(rec, O.default_conventions(), pixels, max_hits=512, max_layers=7)
    wl[2:] = np.zeros((), K.LAYER)                   # (rows that are not due come back zero from this route)
    assert res.tobytes() == want.tobytes() and lay.dtype == K.LAYER and lay.tobytes() == wl.tobytes()
    assert S.R.device_bytes()[0] == held, "temporaries live for the call"
    assert len(S.R.pick(cam.to_c(0.01, 15), [])) == 0


# ---- 8. nothing else moves ------------------------------------------------------------------------------------------------------
def test_it_reads_the_scene_and_nothing_a_frame_depends_on_changes():
    n, h, w = 3000, 96, 128
    g = K.cloud(n, 6)
    cam = scene_gpu.make_camera(h, w).to_c(0.01, 15)
    pixels = K.pixel_set(64, w, h)

    def run(s, pick):
        R = s.R
        R.upload(g)
        img = np.zeros((h, w), np.uint32)

        def frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam, img)
            return img.copy()

        frames = [frame() for _ in range(STILL + 4)]
        held = R.device_bytes()[0]
        for _ in range(3):
            if pick:
                assert R.pick(cam, pixels, layers=4)[0]["n_hits"].sum() > 0
                assert R.device_bytes()[0] == held, "temporaries live for the call"
            frames.append(frame())
        return frames, R.frames_retained(), R.frames_dropped()

    with scene_gpu.session() as a, scene_gpu.session() as b:
        fa, ra, da = run(a, True)
        fb, rb, db = run(b, False)
    assert fa[0].any() and all(np.array_equal(fa[0], f) for f in fa + fb)
    assert ra == rb and ra > 0, "the retained lists survive the call"
    assert da == db == 0


# ---- 9. refusals that need a context -----------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    h, w = K.STACK_TARGET
    cam = K.stack_camera().to_c(0.01, 15)
    with scene_gpu.session() as s:
        d = s.alloc(64, K.SENTINEL)
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.pick(cam, [(1, 1)], results=d)
        assert e.value.code == _lib.ERR_NO_SCENE and "no resident scene" in str(e.value)
        s.R.pick(cam, [], results=d)                 # nothing asked: fine, also without a scene
        s.R.upload(K.stack(5, 0.5))
        for bad in ((w, 0), (0, h), (-1, 3)):
            with pytest.raises(splat_amd.SplatError) as e:
                s.R.pick(cam, [(1, 1), bad], results=d)
            assert e.value.code == _lib.ERR_INVALID and "pixels_xy" in str(e.value)
        assert (s.fetch(d, 64, np.uint8) == K.SENTINEL).all(), "a refusal writes nothing"
        s.R.pick(cam, [(w - 1, h - 1)], results=d)
        assert s.fetch(d, 1, K.RESULT)["n_hits"][0] == 0
