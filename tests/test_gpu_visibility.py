"""The visibility query on the GPU (splat_visibility_device, splat_select_counts_device, Renderer.visibility / select_counts /
select_visible; -m gpu).

Every comparison is np.array_equal on all three arrays -- pixels (uint32), max_weight (float32, compared as bits) and weight_sum
(uint64) -- against tests/visibility_cases.reference: pick_cases.hits_of per pixel and numpy float32 / integers for the chain,
the product, the Q24 truncation and the sums.  Nothing here has a tolerance.  tests/test_visibility_cases_host.py shows on the
CPU that the cases have something to compare.  Every output buffer starts filled with 0xA5 and sits between guard bytes, so
every SET is a SET over garbage and every call is checked for writing outside its arrays.

Shapes: clouds of 1, 255, 256, 257 and 3000 Gaussians at 64x48 and 40x24 (partial tiles on both axes); stacks of 300 and 5000
(one list beyond 2048 and 4096 keys: the mid sort launch, twenty chunks of the walk); wide stacks of 300 and 2100 whose
Gaussians collect from up to six workgroups, the second with lists just above 2048 keys in several tiles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pick_cases as K
import scene_gpu
import splat_amd
import visibility_cases as V
from splat_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STILL = int(re.search(r"#define SPLAT_POLICY_STILL_FRAMES (\d+)", open(os.path.join(ROOT, "include", "splat_policy.h")).read()).group(1))
MODE_CORRECTED, MODE_LIBM_EXP = 1, 2
GUARD = 64
SIZES = {"pixels": 4, "max_weight": 4, "weight_sum": 8}
DTYPES = {"pixels": np.uint32, "max_weight": np.uint32, "weight_sum": np.uint64}      # (the floats as their bits)
SH, SW = K.STACK_TARGET


# ---- plumbing -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    with scene_gpu.session() as s:
        yield s


class Outputs:
    """the three arrays in device memory, each between guard bytes, every byte 0xA5 -- or `start`: (pixels, max_weight, weight_sum)"""

    def __init__(self, s, n, names=("pixels", "max_weight", "weight_sum"), start=None):
        self.s, self.n, self.base = s, n, {}
        for name in names:
            self.base[name] = s.alloc(2 * GUARD + SIZES[name] * n, V_FILL)
        if start is not None:
            for name, a in zip(("pixels", "max_weight", "weight_sum"), start):
                if name in self.base and n:
                    raw = np.ascontiguousarray(a).view(np.uint8)
                    s.R._check(s.R._L.splat_device_upload(s.R._h, C.c_void_p(self.base[name] + GUARD), C.c_void_p(raw.ctypes.data), raw.nbytes))

    def args(self):
        return {name: p + GUARD for name, p in self.base.items()}

    def fetch(self):
        """{name: array}, the guards checked"""
        out = {}
        for name, p in self.base.items():
            raw = self.s.fetch(p, 2 * GUARD + SIZES[name] * self.n, np.uint8)
            assert (raw[:GUARD] == V_FILL).all() and (raw[len(raw) - GUARD:] == V_FILL).all(), "%s: a guard byte was written" % name
            out[name] = raw[GUARD:len(raw) - GUARD].view(DTYPES[name]).copy()
        return out


V_FILL = 0xA5


def want_of(ref):
    return {"pixels": ref[0], "max_weight": ref[1].view(np.uint32), "weight_sum": ref[2]}


def assert_arrays(got, want, what):
    for name in got:
        w = want[name]
        assert got[name].dtype == w.dtype and np.array_equal(got[name], w), "%s: %s differs at %d of %d Gaussians, first %r: got %r, want %r" % (
            what, name, int((got[name] != w).sum()), len(w), np.flatnonzero(got[name] != w)[:4], got[name][got[name] != w][:4], w[got[name] != w][:4])


def check(s, cam_c, lists, n, w, h, weight_min, what, rect=None, pixel_mask=None, mask=None, names=("pixels", "max_weight", "weight_sum")):
    """one SET call into garbage-filled arrays against the reference; returns the reference"""
    out = Outputs(s, n, names)
    pm = s.array(pixel_mask) if pixel_mask is not None else None
    gm = s.array(np.asarray(mask, np.uint8)) if mask is not None else None
    assert s.R.visibility(cam_c, weight_min=weight_min, rect=rect, pixel_mask=pm, mask=gm, **out.args()) is None
    ref = V.reference(masked(lists, mask), n, w, h, weight_min, rect=rect, pixel_mask=pixel_mask)
    assert_arrays(out.fetch(), want_of(ref), what)
    return ref


def masked(lists, mask):
    """the hit lists without the Gaussians whose mask byte is 0 (hits_of drops them before anything else: the same lists)"""
    if mask is None:
        return lists
    keep = np.asarray(mask) != 0
    return [(idx[keep[idx]], a[keep[idx]]) for idx, a in lists]


# ---- 1. every scene at every weight_min ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", V.CLOUD_TARGETS)
@pytest.mark.parametrize("n", V.CLOUD_SIZES)
def test_clouds(S, n, h, w):
    g, cam, lists = V.cloud_case(n, h, w)
    S.R.upload(g)
    for wm in V.WEIGHTS:
        ref = check(S, cam.to_c(0.01, 15), lists, n, w, h, wm, "cloud %d %dx%d weight_min %r" % (n, w, h, wm))
    if n == 3000 and (h, w) == (48, 64):
        assert int((ref[0] > 0).sum()) == 874


@pytest.mark.parametrize("k,opacity,wide", tuple(s + (False,) for s in V.STACKS) + tuple(s + (True,) for s in V.WIDE_STACKS))
def test_stacks(S, k, opacity, wide):
    g, cam, lists = V.stack_case(k, opacity, wide)
    S.R.upload(g)
    seen = []
    for wm in V.WEIGHTS:
        ref = check(S, cam.to_c(0.01, 15), lists, k, SW, SH, wm, "%sstack %d weight_min %r" % ("wide " if wide else "", k, wm))
        seen.append(int((ref[0] > 0).sum()))
    assert seen[0] == k and 0 < seen[1] < k and seen[2] == 0


# ---- 2. regions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("cloud", "wide"))
def test_a_rectangle_that_cuts_tiles_and_a_painted_mask(S, case):
    if case == "cloud":
        (g, cam, lists), (h, w) = V.cloud_case(3000, 48, 64), (48, 64)
    else:
        (g, cam, lists), (h, w) = V.stack_case(300, 0.05, True), (SH, SW)
    S.R.upload(g)
    c = cam.to_c(0.01, 15)
    whole = V.reference(lists, len(g), w, h, 1.0 / 255.0)[0].sum()
    for wm in (0.0, 1.0 / 255.0):
        r = check(S, c, lists, len(g), w, h, wm, case + " rectangle", rect=V.CUT_RECT)
        assert 0 < r[0].sum() < whole or wm == 0.0
        paint = V.painted_mask(h, w)
        r = check(S, c, lists, len(g), w, h, wm, case + " painted", pixel_mask=paint)
        assert r[0].sum() > 0
        check(S, c, lists, len(g), w, h, wm, case + " painted inside a rectangle", rect=V.CUT_RECT, pixel_mask=paint)
    # a rectangle beyond the target is clamped; one pixel; one tile exactly
    check(S, c, lists, len(g), w, h, 1.0 / 255.0, case + " clamped", rect=(-5, -7, w + 10, h + 3))
    check(S, c, lists, len(g), w, h, 0.0, case + " one pixel", rect=(w // 2, h // 2, w // 2, h // 2))
    check(S, c, lists, len(g), w, h, 0.0, case + " one tile", rect=(32, 16, 47, 31))


def test_an_empty_region_writes_nothing_beyond_what_set_zeroes(S):
    g, cam, lists = V.cloud_case(3000, 48, 64)
    S.R.upload(g)
    c = cam.to_c(0.01, 15)
    n = len(g)
    zeros = want_of((np.zeros(n, np.uint32), np.zeros(n, f32), np.zeros(n, np.uint64)))
    for rect in ((10, 10, 5, 20), (10, 10, 20, 5), (64, 0, 70, 47), (0, -9, 63, -1)):
        out = Outputs(S, n)
        S.R.visibility(c, rect=rect, **out.args())
        assert_arrays(out.fetch(), zeros, "empty %r, set" % (rect,))
        out = Outputs(S, n)
        S.R.visibility(c, rect=rect, accumulate=True, **out.args())
        kept = out.fetch()
        assert all((a.view(np.uint8) == V_FILL).all() for a in kept.values()), "empty %r, accumulate: untouched" % (rect,)
    out = Outputs(S, n)                              # a mask with no pixel set: walked nowhere
    S.R.visibility(c, pixel_mask=S.array(np.zeros((48, 64), np.uint8)), **out.args())
    assert_arrays(out.fetch(), zeros, "nothing painted")


# ---- 3. the Gaussian mask ---------------------------------------------------------------------------------------------------
def test_hiding_the_nearer_half_of_a_stack_shows_the_farther_half(S):
    k = 300
    g, cam, lists = V.stack_case(k, 0.05)
    S.R.upload(g)
    c = cam.to_c(0.01, 15)
    open_ = check(S, c, lists, k, SW, SH, 1.0 / 255.0, "nothing hidden")
    assert (open_[0][:k // 2] == 0).all() and (open_[0][k - 10:] > 0).all()          # the farther half is occluded
    mask = np.ones(k, np.uint8)
    mask[k // 2:] = 0                                                            # (the depth grows with the index)
    half = check(S, c, lists, k, SW, SH, 1.0 / 255.0, "the nearer half hidden", mask=mask)
    assert (half[0][k // 2:] == 0).all(), "a hidden Gaussian is not counted"
    assert (half[0][k // 2 - 10:k // 2] > 0).all(), "... and does not occlude: the farther half is seen now"
    check(S, c, lists, k, SW, SH, 0.0, "every other one hidden", mask=(np.arange(k) % 2 * 255).astype(np.uint8))
    none = check(S, c, lists, k, SW, SH, 0.0, "all hidden", mask=np.zeros(k, np.uint8))
    assert none[0].sum() == 0


# ---- 4. SET, ACCUMULATE, NULL outputs --------------------------------------------------------------------------------------
def test_accumulate_over_two_cameras_is_the_sum_and_the_max(S):
    n, h, w = 3000, 48, 64
    g, cam0, l0 = V.cloud_case(n, h, w, 0)
    _, cam1, l1 = V.cloud_case(n, h, w, 1)
    S.R.upload(g)
    out = Outputs(S, n)
    S.R.visibility(cam0.to_c(0.01, 15), **out.args())
    S.R.visibility(cam1.to_c(0.01, 15), accumulate=True, **out.args())
    r0 = V.reference(l0, n, w, h, 1.0 / 255.0)
    both = V.reference(l1, n, w, h, 1.0 / 255.0, into=tuple(a.copy() for a in r0[:3]))
    assert (both[0] > r0[0]).any() and (both[1] > r0[1]).any()
    assert_arrays(out.fetch(), want_of(both), "two cameras")
    # ... and on top of arrays of the caller's own
    rng = np.random.default_rng(4)
    start = (rng.integers(0, 1000, n).astype(np.uint32), rng.random(n).astype(f32), rng.integers(0, 1 << 40, n).astype(np.uint64))
    out = Outputs(S, n, start=start)
    S.R.visibility(cam0.to_c(0.01, 15), weight_min=0.05, accumulate=True, **out.args())
    assert_arrays(out.fetch(), want_of(V.reference(l0, n, w, h, 0.05, into=tuple(a.copy() for a in start))), "on top of the caller's")


@pytest.mark.parametrize("names", (("pixels",), ("max_weight",), ("weight_sum",), ("pixels", "weight_sum")))
def test_a_null_output_is_left_alone(S, names):
    g, cam, lists = V.stack_case(300, 0.05, True)
    S.R.upload(g)
    check(S, cam.to_c(0.01, 15), lists, 300, SW, SH, 1.0 / 255.0, "outputs %r" % (names,), names=names)


# ---- 5. conventions, projection, exp mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ctx,oracle", (("y_down", dict(y_up=0), dict(y_up=0)), ("corner_samples", dict(sample_half=0), dict(sample_half=0)),
                                             ("y_down_corner", dict(y_up=0, sample_half=0), dict(y_up=0, sample_half=0)),
                                             ("corrected", dict(mode=MODE_CORRECTED), dict(corrected_projection=1))))
def test_conventions(name, ctx, oracle):
    n, h, w = 3000, 48, 64
    g = K.cloud(n)
    conv = O.default_conventions(**oracle)
    cam = scene_gpu.cameras(h, w)[1]
    lists = V.hit_lists(("conv", name), K.records(g, cam, conv), conv, w, h)
    with scene_gpu.session(**ctx) as s:
        s.R.upload(g)
        ref = check(s, cam.to_c(0.01, 15), lists, n, w, h, 1.0 / 255.0, name)
        assert (ref[0] > 0).sum() > 500
        check(s, cam.to_c(0.01, 15), lists, n, w, h, 0.0, name + " rectangle", rect=V.CUT_RECT)


def test_the_default_exp_mode_and_libm_exp_give_the_same_arrays():
    g, cam, lists = V.cloud_case(3000, 48, 64)
    got = []
    for mode in (0, MODE_LIBM_EXP):
        with scene_gpu.session(mode=mode) as s:
            s.R.upload(g)
            check(s, cam.to_c(0.01, 15), lists, 3000, 64, 48, 1.0 / 255.0, "mode %d" % mode)
            out = Outputs(s, 3000)
            s.R.visibility(cam.to_c(0.01, 15), weight_min=0.0, **out.args())
            got.append(out.fetch())
    assert all(np.array_equal(got[0][k], got[1][k]) for k in got[0])


# ---- 6. the resident values, a slab, no scene ----------------------------------------------------------------------------------
def test_after_a_transform_of_a_selection(S):
    n, h, w = 3000, 48, 64
    g, cam, lists = V.cloud_case(n, h, w)
    S.R.upload(g)
    sel = np.flatnonzero(g.positions[:, 0] > 0).astype(np.uint32)
    m = np.array([[1.5, 0, 0, -0.4], [0, 0.75, 0.1, 0.2], [0, 0, 1.25, 0.3]], f32)
    S.R.transform(m, index=S.array(sel), k=sel.size)
    r = S.read_all(n)
    t = splat_amd.GaussianList(r["positions"], np.ones((n, 3), f32), r["opacities"], np.zeros((n, 4), f32), r["sh"], r["cov3d"])
    assert not np.array_equal(t.positions, g.positions)
    moved = V.hit_lists(("cloud moved",), K.records(t, cam), O.default_conventions(), w, h)
    ref = check(S, cam.to_c(0.01, 15), moved, n, w, h, 1.0 / 255.0, "a selection transformed")
    assert not np.array_equal(ref[0], V.reference(lists, n, w, h, 1.0 / 255.0)[0])


def test_a_slab_on_the_context_changes_nothing():
    g, cam, lists = V.cloud_case(3000, 48, 64)
    with scene_gpu.session() as s:
        s.R.upload(g)
        s.R.set_slab(1, 2)
        check(s, cam.to_c(0.01, 15), lists, 3000, 64, 48, 1.0 / 255.0, "slab 1..2")
        img = np.zeros((48, 64), np.uint32)
        s.R.render_frame(cam.to_c(0.01, 15), img)
        assert img[16:32].any() and not img[:16].any() and not img[32:].any(), "the slab still holds for frames"


def test_no_scene_and_nothing_in_view():
    cam = K.stack_camera()
    with scene_gpu.session() as s:
        d = s.alloc(8 * 16, V_FILL)
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.n = 16
            s.R.visibility(cam.to_c(0.01, 15), pixels=d)
        assert e.value.code == _lib.ERR_NO_SCENE and "no resident scene" in str(e.value)
        assert (s.fetch(d, 8 * 16, np.uint8) == V_FILL).all(), "a refusal writes nothing"
        assert s.R.select_counts(d, d, n=0) == 0      # n == 0: fine, also without a scene
        # a scene of which the camera sees nothing: SET zeroes, nothing else
        g = K.stack(300, 0.05)
        s.R.upload(g)
        away = scene_gpu.make_camera(SH, SW, (50.0, 0.0, 5.0))
        assert not any(len(i) for i, _ in V.hit_lists(("away",), K.records(g, away), O.default_conventions(), SW, SH))
        out = Outputs(s, 300)
        s.R.visibility(away.to_c(0.01, 15), **out.args())
        assert all(not a.any() for a in out.fetch().values())


# ---- 7. frames, dropped frames, device bytes -----------------------------------------------------------------------------------
def test_frames_around_a_query_are_the_frames_without_it():
    n, h, w = 3000, 96, 128
    g = K.cloud(n, 6)
    cam = scene_gpu.make_camera(h, w)
    c = cam.to_c(0.01, 15)
    turned = scene_gpu.make_camera(h, w, yaw=0.15).to_c(0.01, 15)

    one_pass = []

    def run(s, query):
        R = s.R
        R.upload(g)
        img = np.zeros((h, w), np.uint32)
        out = Outputs(s, n)

        def frame(cc=c):
            img[:] = 0xDEADBEEF
            R.render_frame(cc, img)
            return img.copy()

        def ask(*a, **kw):                                       # what the call leaves in device_bytes()
            before = R.device_bytes()[0]
            R.visibility(*a, **kw, **out.args())
            grown.append(R.device_bytes()[0] - before)

        grown = []
        frames = [frame(), frame(turned)]                        # a frame, the query, a frame of the same camera
        one_pass.append(R.binning_mode() > 0)                    # (such frames keep depth / rectangle / visible list in registers)
        if query:
            ask(turned)
        frames.append(frame(turned))
        frames += [frame() for _ in range(STILL + 4)]            # the camera at rest: retained lists
        for _ in range(3):                                       # ... and three frames with the query between them
            if query:
                ask(c, weight_min=0.0, rect=(3, 5, 100, 90))
            frames.append(frame())
        return frames, grown, R.frames_dropped(), R.frames_retained()

    with scene_gpu.session() as a, scene_gpu.session() as b:
        fa, ha, da, ra = run(a, True)
        fb, hb, db, rb = run(b, False)
    assert fa[0].any() and len(fa) == len(fb)
    for k, (x, y) in enumerate(zip(fa, fb)):
        assert np.array_equal(x, y), "frame %d: %d pixels differ" % (k, int((x != y).sum()))
    assert np.array_equal(fa[1], fa[2]) and all(np.array_equal(fa[3], f) for f in fa[3:])
    assert da == db == 0, "splat_frames_dropped is unchanged"
    assert rb > 0, "the session without a query retains lists (the query may start a set over: time only)"
    # splat_device_bytes(): at most the first frame slot's two-pass buffers (16 bytes a Gaussian), once; temporaries are freed
    # ... exactly: a context whose frames were one-pass has no such buffers yet, one whose frames were two-pass has them already
    assert ha[0] == (16 * n if one_pass[0] else 0) and ha[1:] == [0, 0, 0] and hb == [], (ha, hb, one_pass)


# ---- 8. counts into selections -----------------------------------------------------------------------------------------------
def test_select_counts_for_every_op_and_range(S):
    n = 1000
    rng = np.random.default_rng(9)
    counts = rng.integers(0, 12, n).astype(np.uint32)
    counts[::97] = 0xFFFFFFFF
    before = (rng.random(n) < 0.5).astype(np.uint8) * 7
    dc = S.array(counts)
    for lo, hi in ((1, None), (0, 0), (3, 5), (12, None), (0, None), (0xFFFFFFFF, 0xFFFFFFFF)):
        ok = (counts >= lo) & (counts <= (0xFFFFFFFF if hi is None else hi))
        for op, want in (("set", ok), ("add", (before != 0) | ok), ("subtract", (before != 0) & ~ok), ("intersect", (before != 0) & ok)):
            ds = S.array(before)
            got = S.R.select_counts(dc, ds, at_least=lo, at_most=hi, op=op, n=n)
            sel = S.fetch(ds, n, np.uint8)
            assert np.array_equal(sel != 0, want) and got == int(want.sum()), (lo, hi, op)


def test_select_visible_with_one_camera_and_with_two(S):
    n, h, w = 3000, 48, 64
    g, cam0, l0 = V.cloud_case(n, h, w, 0)
    _, cam1, l1 = V.cloud_case(n, h, w, 1)
    S.R.upload(g)
    p0 = V.reference(l0, n, w, h, 1.0 / 255.0)[0]
    p1 = V.reference(l1, n, w, h, 1.0 / 255.0)[0]
    paint = V.painted_mask(h, w)
    ds, dp = S.alloc(n, V_FILL), S.array(paint)
    assert S.R.select_visible(cam0.to_c(0.01, 15), ds) == int((p0 > 0).sum()) == 1678
    held = S.R.device_bytes()[0]                     # (the slot's two-pass buffers exist from here on)
    assert np.array_equal(S.fetch(ds, n, np.uint8) != 0, p0 > 0)
    both = p0.astype(np.uint64) + p1
    assert S.R.select_visible([cam0.to_c(0.01, 15), cam1.to_c(0.01, 15)], ds, min_pixels=3) == int((both >= 3).sum())
    assert np.array_equal(S.fetch(ds, n, np.uint8) != 0, both >= 3) and (both >= 3).sum() > (p0 >= 3).sum()
    pp = V.reference(l0, n, w, h, 0.05, pixel_mask=paint)[0]
    got = S.R.select_visible(cam0.to_c(0.01, 15), ds, weight_min=0.05, pixel_mask=dp, op="subtract")
    assert np.array_equal(S.fetch(ds, n, np.uint8) != 0, (both >= 3) & ~(pp > 0)) and got == int(((both >= 3) & ~(pp > 0)).sum())
    assert S.R.device_bytes()[0] == held, "the counts are a temporary"



# ---- 9. the recipe: prune what the camera does not see ---------------------------------------------------------------------------
def test_pruning_what_the_camera_does_not_see():
    """select_visible at weight_min = 0, then remove(keep=True), on the 3000 cloud, where 1232 Gaussians go.

    What holds, and is asserted: the selection is the reference's; the SPLAT_MODE_LIBM_EXP frame afterwards is the oracle's frame
    of the reference's survivors, byte for byte; and its R, G and B bytes are those of the whole scene's frame -- a Gaussian that
    goes has no accepted fragment on any pixel of the view, and SPLAT_MODE_LIBM_EXP accepts exactly the query's fragments.

    What does NOT hold is the whole pixel word (the assertion the issue allowed to drop): measured on an MI355X, 49 pixels of the
    64x48 frame differ between the two scenes, in the A byte alone (e.g. 0x00090500 with all 3000, 0x0d090500 with the 1768
    survivors), and the ORACLE's own two frames differ in the same 49 pixels by the same bytes.  It is the reference's blend: a
    REJECTED fragment is drawn as (0, 0, 0, 0), which leaves the pixel's colour bytes alone but resets its alpha byte, so a
    Gaussian whose rectangle covers a pixel without contributing to it still shows in A when it is drawn last.  Pruning by
    visibility is exact in colour, not in the alpha channel the reference leaves behind."""
    n, h, w = 3000, 48, 64
    g, cam, lists = V.cloud_case(n, h, w)
    keep = V.reference(lists, n, w, h, 0.0)[0] > 0
    assert int(keep.sum()) == 1768
    survivors = splat_amd.GaussianList(*(a[keep].copy() for a in (g.positions, g.scales, g.opacities, g.rotations, g.sh, g.cov3d)))
    from helpers import oracle_camera, scene_dict
    want, _ = O.render(scene_dict(survivors), oracle_camera(cam, 0.01), nthreads=4)
    with scene_gpu.session(mode=MODE_LIBM_EXP) as s:
        s.R.upload(g)
        before = scene_gpu.frame(s.R, cam, h, w)
        ds = s.alloc(n, V_FILL)
        assert s.R.select_visible(cam.to_c(0.01, 15), ds, weight_min=0.0) == 1768
        assert np.array_equal(s.fetch(ds, n, np.uint8) != 0, keep)
        assert s.R.remove(ds, keep=True) == 1768 == s.R.n
        after = scene_gpu.frame(s.R, cam, h, w)
    assert before.any() and np.array_equal(after, want), "%d pixels differ from the oracle's frame of the survivors" % int((after != want).sum())
    rgb = np.uint32(0x00FFFFFF)
    assert np.array_equal(after & rgb, before & rgb), "%d pixels changed colour" % int(((after ^ before) & rgb != 0).sum())
    print("pixels whose alpha byte differs from the whole scene's frame:", int((after != before).sum()))
