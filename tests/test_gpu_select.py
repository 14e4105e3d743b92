"""Selections made on the GPU from the resident scene (splat_select_device, splat_selection_indices_device, -m gpu).

The reference is never the library: it is the oracle's records (O.preprocess: Pipeline::vertex restated on the CPU) plus numpy
in float32 with the operation order include/splat_hip.h states -- VOLUME ((m0 x + m1 y) + m2 z) + m3, the centre rule's
half-open comparisons against float(x0) and float(x1 + 1), the touch rule on the covered range -- and np.flatnonzero for the
indices.  Nothing here has a tolerance: the selected SET must be the reference's, the count its size.

Shapes: synthetic_scene(20000, 1) at 256 x 256 (the shape of test_preprocess_records_exact) and 3000 Gaussians at 17 x 40
(partial tiles only), from outside the cloud and from inside it; compaction from 1 byte to 2^20 + 1, the smallest mask whose
workgroup counts take the scan into a second round (a workgroup spans 4096 bytes, a round scans 256 counts)."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from oracle import oracle as O
from helpers import make_camera, oracle_camera, scene_dict, with_oracle_cov3d

pytestmark = pytest.mark.gpu
f32 = np.float32
SPAN = 4096                      # bytes of the mask per workgroup (SELECT_SPAN of splat_internal.h)
SCAN_ROUND = 256                 # workgroup counts per round of the scan (SELECT_SCAN_ROUND)
SENTINEL = 0xDEADBEEF
MODE_CORRECTED = 1


# ---- plumbing -------------------------------------------------------------------------------------------------------
class Session:
    """a Renderer and the device buffers made on it, released together (the buffers first)"""

    def __init__(self, **conventions):
        self.R = splat_amd.Renderer(**conventions)
        self._held = []

    def alloc(self, nbytes):
        R = self.R
        p = R._L.splat_device_alloc(R._h, max(int(nbytes), 4))
        assert p
        self._held.append(p)
        return p

    def put(self, a, at=None):
        """device copy of a numpy array (at: an address to write to instead of a new buffer); returns its address"""
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes) if at is None else at
        if a.nbytes:
            self.R._check(self.R._L.splat_device_upload(self.R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def get(self, p, count, dtype=np.uint8):
        out = np.zeros(count, dtype)
        if out.nbytes:
            self.R._check(self.R._L.splat_device_download(self.R._h, C.c_void_p(out.ctypes.data), C.c_void_p(p), out.nbytes))
        return out

    def release(self):
        for p in reversed(self._held):
            self.R.device_free(p)
        self._held = []

    def close(self):
        self.release()
        self.R.close()


@contextlib.contextmanager
def session(**conventions):
    s = Session(**conventions)
    try:
        yield s
    finally:
        s.close()


# the contexts: default conventions (y_up = 1, sample_half = 1, zclip on), each of the two toggled, the corrected chain
CONTEXTS = {"default": ({}, {}), "y_down": (dict(y_up=0), dict(y_up=0)), "corner_samples": (dict(sample_half=0), dict(sample_half=0)),
            "corrected": (dict(mode=MODE_CORRECTED), dict(corrected_projection=1))}


@pytest.fixture(scope="module")
def sessions():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Session(**CONTEXTS[name][0])
            assert made[name].R.config.zclip == 1
        return made[name]

    yield get
    for s in made.values():
        s.close()


def conv_of(name):
    return O.default_conventions(**CONTEXTS[name][1])


SCENES = {}


def scene(n, seed):
    if (n, seed) not in SCENES:
        SCENES[(n, seed)] = with_oracle_cov3d(splat_amd.synthetic_scene(n, seed))
    return SCENES[(n, seed)]


def copy_of(g):
    return splat_amd.GaussianList(g.positions.copy(), g.scales.copy(), g.opacities.copy(), g.rotations.copy(), g.sh.copy(), g.cov3d.copy())


def poses(h, w):
    """outside the cloud, and inside it: from there many Gaussians are behind the camera or off the target"""
    return {"outside": make_camera(h, w), "inside": make_camera(h, w, (0.3, 0.2, 0.4), 1.0, -0.2)}


# ---- the reference --------------------------------------------------------------------------------------------------
def ref_volume(pos, m, ellipsoid):
    m = np.asarray(m, f32).reshape(3, 4)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        u = [((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)]
        assert all(v.dtype == f32 for v in u)
        if ellipsoid:
            return ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) <= f32(1.0)
        return (np.abs(u[0]) <= f32(1.0)) & (np.abs(u[1]) <= f32(1.0)) & (np.abs(u[2]) <= f32(1.0))


def ref_screen(rec, W, H, rect, rule, mask):
    x0, y0, x1, y1 = rect
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    vis = rec["visible"] == 1
    if x0 > x1 or y0 > y1:
        return np.zeros(len(rec), bool)
    if rule == "touch":
        return vis & (rec["px0"] <= x1) & (rec["px1"] >= x0) & (rec["py0"] <= y1) & (rec["py1"] >= y0)
    cx, cy = rec["cx"], rec["cy"]
    with np.errstate(all="ignore"):
        hit = vis & (f32(x0) <= cx) & (cx < f32(x1 + 1)) & (f32(y0) <= cy) & (cy < f32(y1 + 1))
    if mask is not None:
        idx = np.flatnonzero(hit)
        hit[idx] = mask.reshape(H, W)[cy[idx].astype(np.int64), cx[idx].astype(np.int64)] != 0
    return hit


def reference(g, rec, W, H, box=None, ellipsoid=None, rect=None, rule="centre", pixel_mask=None, depth=None, opacity=None):
    ok = np.ones(len(g), bool)
    if box is not None:
        ok &= ref_volume(g.positions, box, False)
    if ellipsoid is not None:
        ok &= ref_volume(g.positions, ellipsoid, True)
    if rect is not None:
        ok &= ref_screen(rec, W, H, rect, rule, pixel_mask)
    with np.errstate(all="ignore"):
        if depth is not None:
            ok &= (f32(depth[0]) <= rec["depth"]) & (rec["depth"] <= f32(depth[1]))
        if opacity is not None:
            ok &= (f32(opacity[0]) <= g.opacities) & (g.opacities <= f32(opacity[1]))
    return ok


def run_select(s, n, cam_c, q, op="set", sel=None):
    """(selection bytes, count) of one query on the session's resident scene; sel: the buffer to combine with"""
    q = dict(q)
    if q.get("pixel_mask") is not None:
        q["pixel_mask"] = s.put(q["pixel_mask"])
    p = sel if sel is not None else s.put(np.full(n, 0xA5, np.uint8))     # (SET does not read it: garbage goes)
    count = s.R.select(p, cam_c, op=op, **q)
    return s.get(p, n), count


def assert_selects(s, g, rec, cam_c, q, what):
    W, H = int(cam_c.w), int(cam_c.h)
    want = reference(g, rec, W, H, **q)
    got, count = run_select(s, len(g), cam_c, q)
    assert set(np.unique(got)) <= {0, 1}, what
    bad = np.flatnonzero((got != 0) != want)
    assert bad.size == 0, "%s: %d of %d differ, first %d (want %s): record %r" % (what, bad.size, len(g), bad[0], want[bad[0]], rec[bad[0]])
    assert count == int(want.sum()), what
    return want


def affine(centre, half, skew=0.0):
    """world -> unit shape: a box / ellipsoid around `centre` with half axes `half`, sheared a little"""
    m = np.zeros((3, 4), f32)
    for k in range(3):
        m[k, k] = f32(1.0) / f32(half[k])
        m[k, 3] = -f32(centre[k]) / f32(half[k])
    m[0, 1] = f32(skew)
    m[2, 0] = f32(-skew)
    return m


def queries(g, rec, W, H):
    """every test alone (both shapes, both rules), then all four together; ranges cut through the data"""
    d = rec["depth"][np.isfinite(rec["depth"])]
    dlo, dhi = np.percentile(d, 30).astype(f32), np.percentile(d, 80).astype(f32)
    rect = (W // 4, H // 5, (3 * W) // 4, (4 * H) // 5)
    box, ell = affine((0.1, -0.1, 0.2), (0.6, 0.4, 0.5), 0.3), affine((0.0, 0.1, -0.1), (0.7, 0.5, 0.6), -0.2)
    return [("box", dict(box=box)), ("ellipsoid", dict(ellipsoid=ell)), ("centre", dict(rect=rect)),
            ("touch", dict(rect=rect, rule="touch")), ("depth", dict(depth=(dlo, dhi))), ("opacity", dict(opacity=(0.3, 0.8))),
            ("all four", dict(box=affine((0.0, 0.0, 0.0), (1.2, 1.0, 1.1), 0.1), rect=(W // 8, H // 8, W - 2, H - 2), depth=(dlo, f32(1e9)),
                              opacity=(0.1, 0.95))),
            ("all four, touch, ellipsoid", dict(ellipsoid=ell, rect=rect, rule="touch", depth=(f32(-1e9), dhi), opacity=(0.2, 1.0)))]


# ---- 1. compaction alone, no scene ------------------------------------------------------------------------------------
# one workgroup's span +- 1 (4095, 4096, 4097); 2^20 + 1 = SCAN_ROUND * SPAN + 1 bytes are 257 workgroups at offset 0 (and at 1
# and 3): the scan's second round
SIZES = (1, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, SCAN_ROUND * SPAN + 1)


@pytest.fixture(scope="module")
def bare():
    with session() as s:
        yield s


@pytest.mark.parametrize("n", SIZES)
def test_indices_are_flatnonzero_at_any_alignment(bare, n):
    s = bare
    rng = np.random.default_rng(n)
    buf = s.alloc(n + 32)
    out = s.alloc(4 * (n + 1))
    try:
        for offset in (0, 1, 3):
            for density in (0.0, 1.0, 0.5, 1e-3):
                mask = np.where(rng.random(n) < density, rng.integers(1, 256, n), 0).astype(np.uint8)      # bytes other than 0 and 1
                if density == 1.0:
                    assert mask.all()
                elif density == 0.5 and n > 64:
                    assert (mask > 1).any() and not mask.all()
                want = np.flatnonzero(mask).astype(np.uint32)
                what = "n=%d offset=%d density=%g" % (n, offset, density)
                s.put(np.full(n + 32, 0xFF, np.uint8), at=buf)          # whatever lies around the mask is nonzero: reading it would count
                s.put(mask, at=buf + offset)
                s.put(np.full(n + 1, SENTINEL, np.uint32), at=out)
                count = s.R.selection_indices(buf + offset, out, n=n, capacity=n)
                got = s.get(out, n + 1, np.uint32)
                assert count == want.size, what
                assert np.array_equal(got[:count], want), what
                assert (got[count:] == SENTINEL).all(), what
                if want.size >= 2:                                       # fewer entries than selected: a prefix, and the count stays whole
                    cap = want.size // 2
                    s.put(np.full(n + 1, SENTINEL, np.uint32), at=out)
                    assert s.R.selection_indices(buf + offset, out, n=n, capacity=cap) == want.size, what
                    got = s.get(out, cap + 1, np.uint32)
                    assert np.array_equal(got[:cap], want[:cap]) and got[cap] == SENTINEL, what
                    assert s.R.selection_indices(buf + offset, 0, n=n, capacity=0) == want.size, what      # the count alone
    finally:
        s.release()


def test_indices_refusals(bare):
    s = bare
    L, h, p = s.R._L, s.R._h, C.c_void_p
    buf, out = s.put(np.ones(16, np.uint8)), s.alloc(64)
    n = C.c_uint64(99)
    try:
        assert L.splat_selection_indices_device(h, 0, None, None, 0, C.byref(n), None) == _lib.SPLAT_OK and n.value == 0
        assert L.splat_selection_indices_device(h, 1 << 32, p(buf), p(out), 16, C.byref(n), None) == _lib.ERR_INVALID
        assert L.splat_selection_indices_device(h, 16, None, p(out), 16, C.byref(n), None) == _lib.ERR_INVALID
        assert L.splat_selection_indices_device(h, 16, p(buf), None, 16, C.byref(n), None) == _lib.ERR_INVALID
        assert L.splat_selection_indices_device(h, 16, p(buf), p(out + 2), 16, C.byref(n), None) == _lib.ERR_INVALID
        assert L.splat_selection_indices_device(h, 16, p(buf), p(out), 16, None, None) == _lib.ERR_INVALID
        assert L.splat_selection_indices_device(h, 16, p(buf), p(out), 16, C.byref(n), None) == _lib.SPLAT_OK and n.value == 16
        # a selection needs a scene
        q = _lib.SelectQuery()
        assert L.splat_select_device(h, C.byref(q), None, None, 0, p(buf), None, None) == _lib.ERR_NO_SCENE
    finally:
        s.release()


# ---- 2. every test alone, then all four together ------------------------------------------------------------------------
SHAPES = {"20000 at 256x256": (20000, 1, 256, 256), "3000 at 17x40": (3000, 6, 17, 40)}
SETTINGS = [("default", 0.01), ("default", 0.3), ("y_down", 0.01), ("corner_samples", 0.01), ("corrected", 0.01), ("corrected", 0.3)]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("ctx,lowpass", SETTINGS, ids=["%s-%g" % s for s in SETTINGS])
def test_every_test_alone_then_all_four_together(sessions, ctx, lowpass, shape):
    n, seed, h, w = SHAPES[shape]
    g = scene(n, seed)
    s = sessions(ctx)
    try:
        s.R.upload(g)
        for pose, cam in poses(h, w).items():
            rec = O.preprocess(scene_dict(g), oracle_camera(cam, lowpass), conv_of(ctx))
            vis = int((rec["visible"] == 1).sum())
            assert 0 < vis < n, "the pose is meant to see a part of the scene"
            if pose == "inside":
                assert (rec["depth"] > 0).sum() > n // 10 and (rec["depth"] < 0).sum() > n // 10      # on both sides of the camera
            for name, q in queries(g, rec, w, h):
                want = assert_selects(s, g, rec, cam.to_c(lowpass, 15), q, "%s %s %s" % (shape, pose, name))
                if shape.startswith("20000"):
                    assert 0 < want.sum() < n, "%s %s: the query is meant to cut through the scene" % (pose, name)
    finally:
        s.release()


# ---- 3. hostile rows ----------------------------------------------------------------------------------------------------
def hostile_scene(h, w):
    """3000 Gaussians and, behind them, rows chosen for what the tests do at their edges (positions for make_camera(h, w))"""
    base = scene(3000, 6)
    rows = [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (np.nan, np.nan, np.nan),      # 0-3: not finite
            (0.2, 0.1, 0.0),                                                                             # 4: zero covariance
            (0.0, 0.0, 0.0), (1.0, 0.0, 1.0), (-2.5, 0.0, 0.0), (0.0, 1.25, 0.0), (0.0, -2.5, 1.0),      # 5-9: centres on integers
            (7.0, 0.0, 0.0), (-7.0, 0.5, 0.0)]                                                           # 10-11: centre off target, quad on it
    k = len(rows)
    g = splat_amd.GaussianList(np.concatenate([base.positions, np.array([r + (1.0,) for r in rows], f32)]),
                               np.concatenate([base.scales, np.repeat(base.scales[:1], k, 0)]),
                               np.concatenate([base.opacities, np.full(k, 0.5, f32)]),
                               np.concatenate([base.rotations, np.repeat(base.rotations[:1], k, 0)]),
                               np.concatenate([base.sh, np.repeat(base.sh[:1], k, 0)]),
                               np.concatenate([base.cov3d, np.repeat(base.cov3d[:1] * f32(300.0), k, 0)]))
    g.cov3d[len(base) + 4] = 0.0
    return g, len(base)


@pytest.mark.parametrize("lowpass", [0.01, 0.0])
def test_hostile_rows(sessions, lowpass):
    h, w = 48, 64
    g, b = hostile_scene(h, w)
    cam = make_camera(h, w)
    rec = O.preprocess(scene_dict(g), oracle_camera(cam, lowpass))
    cam_c = cam.to_c(lowpass, 15)
    # the rows are what they are meant to be, by the oracle
    assert not rec["visible"][b: b + 4].any()
    if lowpass == 0.0:
        assert rec["visible"][b + 4] == 0 and rec["cov2d"][b + 4][0] == 0          # singular: det == 0
    on_int = [i for i in range(b + 5, b + 10)]
    assert all(rec["visible"][i] == 1 for i in on_int)
    assert all(rec["cx"][i] == np.floor(rec["cx"][i]) or rec["cy"][i] == np.floor(rec["cy"][i]) for i in on_int)
    assert sum(rec["cx"][i] == np.floor(rec["cx"][i]) for i in on_int) >= 3 and sum(rec["cy"][i] == np.floor(rec["cy"][i]) for i in on_int) >= 3
    left, right = b + 10, b + 11
    assert rec["visible"][left] == 1 and rec["cx"][left] < 0 and rec["px0"][left] == 0
    assert rec["visible"][right] == 1 and rec["cx"][right] >= w and rec["px1"][right] == w - 1
    s = sessions("default")
    try:
        s.R.upload(g)
        everything = (0, 0, w - 1, h - 1)
        for rule in ("centre", "touch"):
            want = assert_selects(s, g, rec, cam_c, dict(rect=everything, rule=rule), "whole target, " + rule)
            assert not want[b: b + 4].any()
            assert want[left] == (rule == "touch") and want[right] == (rule == "touch")      # touch selects them, centre does not
        # NaN fails VOLUME and DEPTH, whatever the bounds
        huge = affine((0.0, 0.0, 0.0), (1e30, 1e30, 1e30))
        for q in (dict(box=huge), dict(ellipsoid=huge), dict(depth=(-np.inf, np.inf))):
            want = assert_selects(s, g, rec, cam_c, q, "nan: %s" % list(q))
            assert not want[b] and not want[b + 3] and want[: b].all()
        assert_selects(s, g, rec, cam_c, dict(opacity=(0.5, 0.5)), "opacity on its bounds")
        # rectangle edges on the integers the centres land on: x0 <= cx is in, cx < x1 + 1 puts x1 = cx - 1 out
        for i in on_int:
            cx, cy = int(np.floor(rec["cx"][i])), int(np.floor(rec["cy"][i]))
            for rect, inside in (((cx, 0, w - 1, h - 1), True), ((0, 0, cx - 1, h - 1), False),
                                 ((0, cy, w - 1, h - 1), True), ((0, 0, w - 1, cy - 1), False), ((cx, cy, cx, cy), True)):
                want = assert_selects(s, g, rec, cam_c, dict(rect=rect), "row %d rect %r" % (i, rect))
                assert want[i] == inside, (i, rect, rec["cx"][i], rec["cy"][i])
        # rectangles partly and wholly outside the target, and an inverted one
        for rect in ((-10, -10, 40, 30), (w - 30, h - 25, w + 50, h + 50), (-(2 ** 31), -(2 ** 31), 2 ** 31 - 1, 2 ** 31 - 1)):
            for rule in ("centre", "touch"):
                assert assert_selects(s, g, rec, cam_c, dict(rect=rect, rule=rule), "%r %s" % (rect, rule)).any()
        for rect in ((w, 0, w + 10, 10), (0, -20, w - 1, -1), (-30, 0, -1, h - 1), (40, 5, 30, 10), (2 ** 31 - 1, 0, 2 ** 31 - 1, 5)):
            for rule in ("centre", "touch"):
                assert not assert_selects(s, g, rec, cam_c, dict(rect=rect, rule=rule), "%r %s" % (rect, rule)).any()
    finally:
        s.release()


# ---- 4. pixel mask ------------------------------------------------------------------------------------------------------
def test_pixel_mask(sessions):
    n, seed, h, w = SHAPES["20000 at 256x256"]
    g, s = scene(n, seed), sessions("default")
    rng = np.random.default_rng(77)
    noise = np.where(rng.random((h, w)) < 0.5, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (((xx - 150) ** 2 + (yy - 100) ** 2) <= 60 ** 2).astype(np.uint8) * np.uint8(200)
    try:
        s.R.upload(g)
        for pose, cam in poses(h, w).items():
            rec = O.preprocess(scene_dict(g), oracle_camera(cam, 0.01))
            for name, mask in (("noise", noise), ("disc", disc)):
                for rect in ((0, 0, w - 1, h - 1), (40, 30, 200, 180), (-5, -5, 2 * w, 2 * h)):
                    want = assert_selects(s, g, rec, cam.to_c(0.01, 15), dict(rect=rect, pixel_mask=mask), "%s %s %r" % (pose, name, rect))
                    unmasked = reference(g, rec, w, h, rect=rect)
                    assert 0 < want.sum() < unmasked.sum(), "the mask is meant to take a part away"
        with pytest.raises(splat_amd.SplatError) as e:           # the library's own refusal (Renderer.select refuses earlier)
            q = _lib.SelectQuery(tests=_lib.SEL_SCREEN, screen_rule=1, x1=5, y1=5)
            cam_c = poses(h, w)["outside"].to_c(0.01, 15)
            s.R._check(s.R._L.splat_select_device(s.R._h, C.byref(q), C.byref(cam_c), C.c_void_p(s.put(noise)), 0, C.c_void_p(s.alloc(n)), None, None))
        assert e.value.code == _lib.ERR_INVALID
    finally:
        s.release()


# ---- 5. ops -------------------------------------------------------------------------------------------------------------
def test_ops_are_the_boolean_algebra_of_their_set_results(sessions):
    n, seed, h, w = SHAPES["20000 at 256x256"]
    g, s = scene(n, seed), sessions("default")
    cam = make_camera(h, w)
    cam_c = cam.to_c(0.01, 15)
    rec = O.preprocess(scene_dict(g), oracle_camera(cam, 0.01))
    qa, qb = dict(rect=(60, 50, 190, 200)), dict(opacity=(0.4, 1.0), box=affine((0.0, 0.0, 0.0), (2.0, 2.0, 2.0)))
    a, b = reference(g, rec, w, h, **qa), reference(g, rec, w, h, **qb)
    assert (a & b).any() and (a & ~b).any() and (~a & b).any() and (~a & ~b).any()
    try:
        s.R.upload(g)
        sa, ca = run_select(s, n, cam_c, qa)
        sb, cb = run_select(s, n, cam_c, qb)
        assert np.array_equal(sa != 0, a) and np.array_equal(sb != 0, b) and (ca, cb) == (a.sum(), b.sum())
        seven = (sa * np.uint8(7)).astype(np.uint8)            # a selection the caller made itself: bytes other than 0 and 1
        for op, want in (("add", a | b), ("subtract", a & ~b), ("intersect", a & b)):
            got, count = run_select(s, n, cam_c, qb, op=op, sel=s.put(seven))
            assert np.array_equal(got != 0, want), op
            assert count == int(want.sum()), op
            if op in ("add", "subtract"):                       # the bytes of Gaussians that do not pass stay as they were
                assert np.array_equal(got[~b], seven[~b]), op
                assert (got[b] == (1 if op == "add" else 0)).all(), op
            else:
                assert set(np.unique(got)) <= {0, 1}
        # a count_out of NULL is fine
        q = _lib.SelectQuery()
        p = s.alloc(n)
        assert s.R._L.splat_select_device(s.R._h, C.byref(q), None, None, 0, C.c_void_p(p), None, None) == _lib.SPLAT_OK
        assert s.get(p, n).all()
    finally:
        s.release()


# ---- 6. resident values, slab -------------------------------------------------------------------------------------------
def test_the_selection_is_of_the_resident_values_and_ignores_a_slab(sessions):
    n, seed, h, w = SHAPES["20000 at 256x256"]
    g, s = scene(n, seed), sessions("default")
    cam = make_camera(h, w, yaw=math.radians(10.0))
    cam_c = cam.to_c(0.01, 15)
    rng = np.random.default_rng(5)
    e = copy_of(g)
    e.positions[:, :3] += (0.3 * rng.standard_normal((n, 3))).astype(f32)
    e.opacities[:] = rng.random(n).astype(f32)
    try:
        s.R.upload(g)
        rec_g = O.preprocess(scene_dict(g), oracle_camera(cam, 0.01))
        rec_e = O.preprocess(scene_dict(e), oracle_camera(cam, 0.01))
        name, q = queries(e, rec_e, w, h)[6]
        assert name == "all four"
        before = assert_selects(s, g, rec_g, cam_c, q, "before the edit")
        s.R.update_device(positions=s.put(e.positions), opacities=s.put(e.opacities), n=n)
        after = assert_selects(s, e, rec_e, cam_c, q, "after the edit")
        assert (before != after).sum() > n // 20, "the edit is meant to change the selection"
        # with a slab set the selection is the whole target's
        tiles_y = (h + _lib.TILE - 1) // _lib.TILE
        for name, q in queries(e, rec_e, w, h)[2:4] + [(name, q)]:
            s.R.set_slab(tiles_y // 2, tiles_y // 2 + 2)
            want = assert_selects(s, e, rec_e, cam_c, q, "slab, " + name)
            s.R.set_slab(0, -1)
            ys = rec_e["cy"][want]
            assert ((ys < 16 * (tiles_y // 2)) | (ys >= 16 * (tiles_y // 2 + 2))).sum() > want.sum() // 4, "selected outside the slab's rows"
    finally:
        s.R.set_slab(0, -1)
        s.release()


# ---- 7. the frame path is undisturbed -----------------------------------------------------------------------------------
def stage(R, cam_c, h, w):
    """(image, records, tile offsets, tile order) of one frame rendered with statistics"""
    img = np.zeros((h, w), np.uint32)
    st = R.render(cam_c, img)
    n_tiles = ((h + _lib.TILE - 1) // _lib.TILE) * ((w + _lib.TILE - 1) // _lib.TILE)
    assert st.n_pairs > 0
    off, order = R.tile_lists(n_tiles, st.n_pairs)
    return img, R.records(), off, order


def test_the_frame_path_is_undisturbed(sessions):
    n, seed, h, w = SHAPES["20000 at 256x256"]
    g, s = scene(n, seed), sessions("default")
    cam_c = make_camera(h, w).to_c(0.01, 15)
    try:
        s.R.upload(g)
        sel, idx = s.alloc(n), s.alloc(4 * n)
        stage(s.R, cam_c, h, w)                                  # (the first frame sizes storage)
        before = stage(s.R, cam_c, h, w)
        held, dropped = s.R.device_bytes()[0], s.R.frames_dropped()
        k = s.R.select(sel, cam_c, rect=(30, 30, 200, 220), opacity=(0.2, 1.0))
        assert s.R.selection_indices(sel, idx, n=n, capacity=n) == k and 0 < k < n
        assert s.R.device_bytes()[0] == held, "temporaries live for the call"
        assert s.R.frames_dropped() == dropped
        after = stage(s.R, cam_c, h, w)
        assert np.array_equal(before[0], after[0]) and before[0].any()
        assert before[1].tobytes() == after[1].tobytes()
        assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
        assert s.R.frames_dropped() == dropped
        # ... also between asynchronous frames in flight
        image = s.R.device_image(np.zeros((h, w), np.uint32))
        for _ in range(3):
            s.R.render_frame_device(cam_c, image, sync=False)
        assert s.R.select(sel, cam_c, rect=(30, 30, 200, 220), opacity=(0.2, 1.0)) == k
        s.R.render_frame_device(cam_c, image, sync=True)
        got = s.R.device_download(image, h, w)
        s.R.device_free(image)
        want = np.zeros((h, w), np.uint32)
        s.R.render_frame(cam_c, want)
        assert np.array_equal(got, want)
        s.R.sync()
    finally:
        s.release()


# ---- 8. the loop this exists for ----------------------------------------------------------------------------------------
def frames_of(R, h, w):
    out = []
    for cam in list(poses(h, w).values()) + [make_camera(h, w, yaw=math.radians(10.0))]:
        img = np.full((h, w), SENTINEL, np.uint32)
        R.render_frame(cam.to_c(0.01, 15), img)
        out.append(img)
    return out


def hidden(g, which):
    e = copy_of(g)
    e.opacities[which] = 0.0
    return e


def test_select_indices_update_is_a_fresh_upload_with_those_opacities_zeroed(sessions):
    n, seed, h, w = 3000, 6, 96, 128
    g, s = scene(n, seed), sessions("default")
    cam = make_camera(h, w)
    cam_c = cam.to_c(0.01, 15)
    rect = (40, 20, 100, 70)
    want = reference(g, O.preprocess(scene_dict(g), oracle_camera(cam, 0.01)), w, h, rect=rect, rule="touch")
    assert 0 < want.sum() < n
    try:
        s.R.upload(g)
        plain = frames_of(s.R, h, w)
        sel, idx = s.alloc(n), s.alloc(4 * n)
        k = s.R.select(sel, cam_c, rect=rect, rule="touch")
        assert s.R.selection_indices(sel, idx, n=n, capacity=n) == k == want.sum()
        assert np.array_equal(s.get(idx, k, np.uint32), np.flatnonzero(want))
        s.R.update_indexed(idx, k=k, opacities=s.put(np.zeros(k, f32)))
        got = frames_of(s.R, h, w)
        with session() as ref:
            ref.R.upload(hidden(g, want))
            for a, b in zip(got, frames_of(ref.R, h, w)):
                assert np.array_equal(a, b), "%d pixels differ" % int((a != b).sum())
        assert not np.array_equal(got[0], plain[0]), "hiding the selection is meant to show"
    finally:
        s.release()


def test_the_loop_takes_torch_tensors_written_on_a_side_stream(sessions):
    import torch
    n, seed, h, w = 3000, 6, 96, 128
    g, s = scene(n, seed), sessions("default")
    cam = make_camera(h, w)
    cam_c = cam.to_c(0.01, 15)
    yy, xx = np.mgrid[0:h, 0:w]
    lasso = (((xx - 64) ** 2 + (yy - 48) ** 2) <= 30 ** 2).astype(np.uint8)
    want = reference(g, O.preprocess(scene_dict(g), oracle_camera(cam, 0.01)), w, h, rect=(0, 0, w - 1, h - 1), pixel_mask=lasso)
    assert 0 < want.sum() < n
    s.R.upload(g)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    host = torch.from_numpy(lasso).pin_memory()
    mask = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    sel = torch.empty(n + 3, dtype=torch.bool, device=dev)[3:]              # a view that starts off every boundary
    idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
    junk = torch.zeros(16 << 20, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(10):                           # work in front of the copy: it has not run when the call is made
            junk.add_(1.0)
        mask.copy_(host, non_blocking=True)
        sel.fill_(True)
    k = s.R.select(sel, cam_c, rect=(0, 0, w - 1, h - 1), pixel_mask=mask, stream=side)
    assert k == want.sum()
    with torch.cuda.stream(side):
        sel.logical_not_()                            # the caller edits the selection itself: everything BUT the lasso
    k = s.R.selection_indices(sel, idx, stream=side)
    assert k == n - want.sum()
    assert np.array_equal(idx[:k].cpu().numpy().astype(np.uint32), np.flatnonzero(~want))
    assert (idx[k:] == -1).all()
    s.R.update_indexed(idx[:k], opacities=torch.zeros(k, dtype=torch.float32, device=dev))
    with session() as ref:
        ref.R.upload(hidden(g, ~want))
        for a, b in zip(frames_of(s.R, h, w), frames_of(ref.R, h, w)):
            assert np.array_equal(a, b), "%d pixels differ" % int((a != b).sum())
    del mask, sel, idx, junk


# ---- 9. edge sizes through the whole call -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_edge_sizes(sessions, n):
    h, w = 48, 64
    g, s = scene(n, 40 + n), sessions("default")
    cam = make_camera(h, w)
    cam_c = cam.to_c(0.01, 15)
    rec = O.preprocess(scene_dict(g), oracle_camera(cam, 0.01))
    try:
        s.R.upload(g)
        sel, idx = s.put(np.full(n + 1, 0xA5, np.uint8)), s.put(np.full(n + 1, SENTINEL, np.uint32))
        assert s.R.select(sel, None) == n                        # an empty query: all n
        assert (s.get(sel, n + 1) == [1] * n + [0xA5]).all()     # ... and not a byte more
        assert s.R.selection_indices(sel, idx, n=n, capacity=n) == n
        assert np.array_equal(s.get(idx, n + 1, np.uint32), list(range(n)) + [SENTINEL])
        for name, q in queries(g, rec, w, h):
            assert_selects(s, g, rec, cam_c, q, "n=%d %s" % (n, name))
        want = assert_selects(s, g, rec, cam_c, dict(rect=(0, 0, w - 1, h - 1), rule="touch"), "n=%d" % n)
        assert want.sum() == (rec["visible"] == 1).sum()
    finally:
        s.release()
