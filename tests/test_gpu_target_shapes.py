"""GPU tests (-m gpu) of render targets beyond 4K and on both sides of every tile-count switch of the binning launches.

How a frame's scan / layout workgroups are launched depends on its tile count m (16 x 16-pixel tiles).  The thresholds are
declared once below, with where the kernel sources define them; GEOMETRIES puts a target on each side of each of them, and
tests/test_target_shapes_table.py (no GPU) holds the table to the sources and checks that every switch is crossed.  Here each
target is held to the CPU oracle (counts, pixels, tile lists), every launch variant is forced at the same frames, moving cameras
at the thresholds are compared frame for frame with a context that has no history, the target changes inside one context, and
an 8K frame is split into slabs.  What they stand for in the reference: src/main.rs:69-78 over src/pipelines.rs:66-86 at any
window size."""
import math
import os

import numpy as np
import pytest

import splat_amd
import splat_amd.renderer
from splat_amd import _lib
from oracle import oracle as O
from helpers import scene_dict, oracle_camera, image_diff, make_camera

pytestmark = pytest.mark.gpu

TILE = 16

# ---- the tile-count switches (m = tiles of the frame or slab) -----------------------------------------------------------
# splat_kernels.hip, launch_scan: scan_bucket_kernel<1024> above, <256> at or below (unless SPLAT_SCAN_THREADS says otherwise)
SCAN_WIDE_ABOVE = 12000
# splat_kernels.hip, launch_layout: the overflow-redo chain's layout_kernel<256> at or below, <1024> above
REDO_LAYOUT_NARROW_MAX = 12000
# splat_kernels.hip, launch_scan: the moving-camera region filter of build_layout keeps two u16 per tile in 48 KB of dynamic
# LDS -- on while (4 m + 15) & ~15 <= 49152, i.e. m <= 12288
MOTION_FILTER_LDS = 49152
MOTION_FILTER_MAX = MOTION_FILTER_LDS // 4
# splat_kernels.hip, launch_scan: one byte of LDS per tile for the length classes while (m + 15) & ~15 <= 49152, else the
# scan's second pass re-reads lens[]
CLASSES_LDS = 49152
CLASSES_IN_LDS_MAX = CLASSES_LDS
# splat_api.hip, splat_upload_scene: the per-tile arrays are made for 240 x 135 tiles (3840 x 2160) at upload; ensure_bins
# makes them again for a larger target
BINS_AT_UPLOAD = 240 * 135
# splat_api.hip, build_frame_const: the ABI's largest width / height
MAX_SIDE = 65535


def tiles_of(w, h):
    return ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)


# name -> (w, h)
GEOMETRIES = {
    "2560x1200": (2560, 1200),     # 12 000: scan / redo layout 256 threads, filter on
    "2560x1216": (2560, 1216),     # 12 160: scan 1024 threads with the filter on
    "2048x1536": (2048, 1536),     # 12 288: the filter's inclusive edge
    "2400x1312": (2400, 1312),     # 12 300: the filter off
    "4096x3072": (4096, 3072),     # 49 152: classes kept in LDS
    "3840x3280": (3840, 3280),     # 49 200: classes re-read
    "7680x4320": (7680, 4320),     # 129 600: classes re-read, per-tile arrays regrown
    "7679x4319": (7679, 4319),     # 129 600, ragged
    "16x4320": (16, 4320),         # one tile column
    "5x3000": (5, 3000),           # one tile column, ragged
    "7680x16": (7680, 16),         # one tile row
    "7680x9": (7680, 9),           # one tile row, ragged
    "65535x16": (65535, 16),       # the ABI's widest: 4 096 tiles in a row
    "16x65535": (16, 65535),       # the ABI's tallest: 4 096 tiles in a column
    "1x1": (1, 1),
}

# every switch: (name, the side it takes for m) -- tests/test_target_shapes_table.py checks that both sides are covered
SWITCHES = [
    ("scan_bucket_kernel<1024> (not <256>)", lambda m: m > SCAN_WIDE_ABOVE),
    ("redo chain layout_kernel<256> (not <1024>)", lambda m: m <= REDO_LAYOUT_NARROW_MAX),
    ("motion filter fits in LDS", lambda m: ((4 * m + 15) & ~15) <= MOTION_FILTER_LDS),
    ("motion filter with 1024 scan threads", lambda m: SCAN_WIDE_ABOVE < m <= MOTION_FILTER_MAX),
    ("length classes in LDS (not re-read)", lambda m: ((m + 15) & ~15) <= CLASSES_LDS),
    ("per-tile arrays regrown after upload", lambda m: m > BINS_AT_UPLOAD),
]

LIBM_EXACT = ("2560x1216", "3840x3280", "7680x4320")      # SPLAT_MODE_LIBM_EXP frames bit for bit
THRESHOLD_GEOMETRIES = ("2560x1200", "2560x1216", "2048x1536", "2400x1312", "4096x3072", "3840x3280", "7680x4320")
MOVING_GEOMETRIES = ("2560x1216", "2048x1536", "2400x1312", "7680x4320")


def scene_size(m):
    return 150000 if m > 100000 else (100000 if m > 40000 else (60000 if m > 10000 else 40000))


def oracle_threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 8)))


# ---- shared state: scenes (cov3d computed once), one context for the oracle cases, fresh-context frames -------------------
_scenes = {}
_fresh = {}
_ctx = {}


def scene(n, dense=False, seed=None):
    key = (n, dense, seed)
    if key not in _scenes:
        g = splat_amd.synthetic_scene(n, seed if seed is not None else 1000 + n // 1000)
        if dense:                                  # as test_near_selection_renders_the_fully_sorted_frame: thousands of keys per tile
            g.positions[:, :3] *= 0.22
            g.opacities[::3] *= 0.05
        g.compute_cov3d(shared_renderer())
        _scenes[key] = g
    return _scenes[key]


def shared_renderer():
    if "R" not in _ctx:
        _ctx["R"] = splat_amd.Renderer()
        _ctx["scene"] = None
    return _ctx["R"]


def shared_with(g):
    R = shared_renderer()
    if _ctx["scene"] is not g:
        R.upload(g)
        _ctx["scene"] = g
    return R


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    if "R" in _ctx:
        _ctx["R"].close()
    _ctx.clear()
    _scenes.clear()
    _fresh.clear()


@pytest.fixture(autouse=True)
def _forget_large_fresh_frames():
    """frames above 4K (133 MB each at 8K) are kept for the test that made them only"""
    yield
    for k in [k for k, img in _fresh.items() if img.size > 3840 * 2160]:
        del _fresh[k]


def pose(w, h, yaw=0.3, pitch=0.0, pos=(0.0, 0.0, 5.0)):
    return make_camera(h, w, pos, yaw, pitch)


def fresh_frame(g, cam):
    """the frame of a context with nothing in its history but the scene and this one synchronous frame"""
    c = cam.to_c(0.01)
    key = (id(g), int(c.w), int(c.h), tuple(c.view), tuple(c.cam_pos))
    if key not in _fresh:
        r = splat_amd.Renderer()
        try:
            r.upload(g)
            img = np.zeros((int(c.h), int(c.w)), np.uint32)
            r.render_frame(c, img)
        finally:
            r.close()
        _fresh[key] = img
    return _fresh[key]


def expected_tile_lists(g, cam, tiles_x, tiles_y):
    """the oracle's tile lists: per-tile counts prefix-summed, and every list in stable depth order (ties by index)"""
    pre = O.preprocess(scene_dict(g), oracle_camera(cam, 0.01))
    glob = O.sort(g.positions, np.array(cam.to_c(0.01).view[:], np.float32))
    rank = np.empty(len(g), np.int64)
    rank[glob] = np.arange(len(g))
    v = np.nonzero(pre["visible"] == 1)[0]
    tx0, tx1 = pre["px0"][v].astype(np.int64) // TILE, pre["px1"][v].astype(np.int64) // TILE
    ty0, ty1 = pre["py0"][v].astype(np.int64) // TILE, pre["py1"][v].astype(np.int64) // TILE
    assert (tx0 >= 0).all() and (tx1 < tiles_x).all() and (ty0 >= 0).all() and (ty1 < tiles_y).all() and (tx1 >= tx0).all() and (ty1 >= ty0).all()
    nx = tx1 - tx0 + 1
    cnt = nx * (ty1 - ty0 + 1)
    total = int(cnt.sum())
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    local = np.arange(total, dtype=np.int64) - first
    nxr = np.repeat(nx, cnt)
    tile = (np.repeat(ty0, cnt) + local // nxr) * tiles_x + np.repeat(tx0, cnt) + local % nxr
    gi = np.repeat(v, cnt)
    order = gi[np.argsort(tile * len(g) + rank[gi], kind="stable")].astype(np.uint32)
    off = np.zeros(tiles_x * tiles_y + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(tile, minlength=tiles_x * tiles_y))
    return off, order


def check_against_oracle(g, cam, img, st, R, tiles_x, tiles_y, what):
    ref, ost = O.render(scene_dict(g), oracle_camera(cam, 0.01), nthreads=oracle_threads())
    h, w = img.shape
    assert st.n_visible == ost.n_visible and st.n_pairs == ost.n_tile_pairs, (what, st.n_visible, ost.n_visible, st.n_pairs, ost.n_tile_pairs)
    mx, cnt = image_diff(img, ref)
    assert mx <= 1 and cnt <= 1e-4 * w * h, (what, mx, cnt)
    # the lists of the frame just compared (often a target's first frame: its regions asked for more than the key buffer held,
    # and the buffer grows behind it)
    off, order = R.tile_lists(tiles_x * tiles_y, st.n_pairs)
    eoff, eorder = expected_tile_lists(g, cam, tiles_x, tiles_y)
    assert np.array_equal(off.astype(np.int64), eoff), (what, "tile offsets", int(np.argmax(off.astype(np.int64) != eoff)))
    assert np.array_equal(order, eorder), (what, "tile lists", int(np.argmax(order != eorder)))
    # ... and the same pose again, in regions sized from that frame
    again = np.zeros_like(img)
    st2 = R.render(cam.to_c(0.01), again)
    assert np.array_equal(again, img), (what, "second frame")
    off, order = R.tile_lists(tiles_x * tiles_y, st2.n_pairs)
    assert np.array_equal(off.astype(np.int64), eoff) and np.array_equal(order, eorder), (what, "second frame's tile lists")
    return ref


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_target_matches_oracle(name):
    """counts, pixels and tile lists at every target; SPLAT_MODE_LIBM_EXP bit for bit at 12 160, 49 200 and 129 600 tiles"""
    w, h = GEOMETRIES[name]
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    g = scene(scene_size(tiles_x * tiles_y))
    R = shared_with(g)
    cam = pose(w, h)
    img = np.zeros((h, w), np.uint32)
    st = R.render(cam.to_c(0.01), img)
    ref = check_against_oracle(g, cam, img, st, R, tiles_x, tiles_y, name)
    if w * h > 64:
        assert img.any(), name
    if name in LIBM_EXACT:
        r = splat_amd.Renderer(mode=splat_amd.MODE_LIBM_EXP)
        try:
            r.upload(g)
            exact = np.zeros((h, w), np.uint32)
            st2 = r.render(cam.to_c(0.01), exact)
            assert st2.n_pairs == st.n_pairs
            assert np.array_equal(exact, ref), (name, image_diff(exact, ref))
        finally:
            r.close()


@pytest.mark.parametrize("name", ["3840x3280", "7680x4320"])
def test_dense_target_with_long_lists_matches_oracle(name):
    """lists of more than 2048 keys at a large target: near selection (the default) against the oracle, and a selection so small
    that long tiles go through the repair launch gives the same bytes"""
    w, h = GEOMETRIES[name]
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    g = scene(50000, dense=True)
    R = shared_with(g)
    cam = pose(w, h, yaw=0.2, pos=(0.0, 0.1, 3.0))
    img = np.zeros((h, w), np.uint32)
    st = R.render(cam.to_c(0.01), img)
    assert st.max_tile_len > 2048 and st.n_near_tiles > 0, (st.max_tile_len, st.n_near_tiles)
    check_against_oracle(g, cam, img, st, R, tiles_x, tiles_y, name + " dense")
    near = R.get_option(_lib.OPT_NEAR_SELECT_KEYS)
    try:
        R.set_option(_lib.OPT_NEAR_SELECT_KEYS, 64)
        small = np.zeros((h, w), np.uint32)
        st2 = R.render(cam.to_c(0.01), small)
        assert st2.n_near_fallback > 0, "the repair path was meant to run"
        assert np.array_equal(small, img), int((small != img).sum())
    finally:
        R.set_option(_lib.OPT_NEAR_SELECT_KEYS, near)


def test_first_frame_tile_lists_are_the_oracles():
    """the tile lists of a context's very first frame at 1920 x 1080.  Its regions ask for more than the key buffer made at upload
    holds: the frame is squeezed into it, and the buffer grows behind the frame -- which used to discard the frame's keys, so that
    splat_get_tile_lists read a fresh buffer and gave every entry the index of slot 0 (the pixels were right)."""
    g = scene(20000)
    r = splat_amd.Renderer()
    try:
        r.upload(g)
        cam = pose(1920, 1080)
        st = r.render(cam.to_c(0.01), np.zeros((1080, 1920), np.uint32))
        off, order = r.tile_lists(120 * 68, st.n_pairs)
    finally:
        r.close()
    eoff, eorder = expected_tile_lists(g, cam, 120, 68)
    assert np.array_equal(off.astype(np.int64), eoff)
    assert np.array_equal(order, eorder), int((order != eorder).sum())


GARBAGE = np.uint32(0x9E3779B9)


def async_frames(r, cams, h, w):
    """every camera's cleared frame rendered asynchronously into an image of its own, all in flight together; returns the
    images (None for a frame the device skipped: its image untouched) after checking the skips were reported"""
    init = np.full((h, w), GARBAGE, np.uint32)
    imgs = [r.device_image(init) for _ in cams]
    d0 = r.frames_dropped()
    try:
        for c, p in zip(cams, imgs):
            r.render_frame_device(c.to_c(0.01), p)
        try:
            r.sync()
        except splat_amd.renderer.SplatError as e:     # (a frame that outgrew its regions: skipped, reported once)
            assert e.code == _lib.ERR_CAPACITY, e
        out = []
        for p in imgs:
            a = r.device_download(p, h, w)
            out.append(None if (a == GARBAGE).all() else a)
    finally:
        for p in imgs:
            r.device_free(p)
    assert sum(a is None for a in out) <= r.frames_dropped() - d0
    return out


def short_path(w, h):
    """rest, rest, then a creep and two steps: a moving camera's frames bin into an earlier camera's regions"""
    return [pose(w, h, yaw=0.3 + math.radians(d)) for d in (0.0, 0.0, 0.5, 1.0, 4.0, 7.0)]


@pytest.mark.parametrize("name", THRESHOLD_GEOMETRIES)
def test_every_launch_variant_gives_the_same_frames(name, monkeypatch):
    """on both sides of every threshold: the scan at 256, 512 and 1024 threads, the overflow redo on every moving frame (both
    layout launches of the redo chain), two-pass binning (scan_kernel) and count first on every moving frame -- the same bytes
    as a context without history renders for each pose"""
    w, h = GEOMETRIES[name]
    g = scene(scene_size(tiles_of(w, h)))
    cams = short_path(w, h)
    want = [fresh_frame(g, c) for c in cams]
    assert want[-1].any()
    variants = [("SPLAT_SCAN_THREADS", str(t)) for t in (256, 512, 1024)] + [
        (_lib.OPT_OVERFLOW_REDO, 2), (_lib.OPT_ONE_PASS_BINNING, 0), (_lib.OPT_COUNT_FIRST, 2)]
    for key, val in variants:
        with monkeypatch.context() as mp:
            if isinstance(key, str):
                mp.setenv(key, val)
            r = splat_amd.Renderer()
        try:
            if not isinstance(key, str):
                r.set_option(key, val)
            r.upload(g)
            first = np.zeros((h, w), np.uint32)
            r.render_frame(cams[0].to_c(0.01), first)       # (sizes the key storage: a first frame that outgrows it asynchronously is skipped)
            assert np.array_equal(first, want[0]), (name, key, val, "first")
            got = async_frames(r, cams, h, w)
            assert got[0] is not None and got[-1] is not None, (name, key)
            for k, a in enumerate(got):
                if a is not None:
                    assert np.array_equal(a, want[k]), (name, key, val, k, int((a != want[k]).sum()))
            last = np.zeros((h, w), np.uint32)
            r.render_frame(cams[-1].to_c(0.01), last)
            assert np.array_equal(last, want[-1]), (name, key, val, "synchronous")
        finally:
            r.close()


def moving_path(w, h):
    """a creeping yaw (0.5 degrees a frame), 3- and 10-degree steps, then a stretch at rest: 12 frames"""
    yaws, a = [], 0.3
    for d in (0.0, 0.5, 0.5, 0.5, 0.5, 3.0, 3.0, 10.0, 10.0, 0.0, 0.0, 0.0):
        a += math.radians(d)
        yaws.append(a)
    return [pose(w, h, yaw=y) for y in yaws]


def policy_radii(cams, n_tiles):
    """the layout radius the frame policy (splat_policy_decide, include/splat_policy.h) gives each frame of an asynchronous
    sequence behind one synchronous frame of its first pose: the host side of enqueue_frame as tests/test_frame_policy.py
    mirrors it"""
    from test_frame_policy import Driver, policy_lib
    D = Driver(policy_lib())
    D.n_tiles = n_tiles
    D.step(None, awaited=1, idle=1, cam=cams[0].to_c(0.01))
    return [int(D.step(None, cam=c.to_c(0.01)).layout_radius) for c in cams]


@pytest.mark.parametrize("name", MOVING_GEOMETRIES)
def test_moving_camera_frames_equal_fresh_contexts(name):
    """a moving camera at each threshold, twelve frames in flight: every frame the device did not skip is the frame of a context
    without history; the first frame and the last one at rest are the oracle's.  The policy sizes the regions for motion
    (layout_radius > 0) on the way, which is what turns build_layout's filter on where it fits."""
    w, h = GEOMETRIES[name]
    m = tiles_of(w, h)
    g = scene(scene_size(m))
    cams = moving_path(w, h)
    radii = policy_radii(cams, m)
    assert max(radii) > 0 and radii[-1] == 0, radii
    r = splat_amd.Renderer()
    try:
        r.upload(g)
        first = np.zeros((h, w), np.uint32)
        r.render_frame(cams[0].to_c(0.01), first)       # (a frame before the sequence: regions for its slots exist)
        got = async_frames(r, cams, h, w)
    finally:
        r.close()
    assert got[0] is not None and got[-1] is not None
    for k, a in enumerate(got):
        if a is not None:
            want = fresh_frame(g, cams[k])
            assert np.array_equal(a, want), (name, k, int((a != want).sum()))
    for k in (0, len(cams) - 1):
        ref, _ = O.render(scene_dict(g), oracle_camera(cams[k], 0.01), nthreads=oracle_threads())
        mx, cnt = image_diff(got[k], ref)
        assert mx <= 1 and cnt <= 1e-4 * w * h, (name, k, mx, cnt)


def test_target_changes_inside_one_context():
    """1080p -> 8K -> 1080p -> one tile column -> one tile row, at rest and moving, and another scene of the same size uploaded
    between two frames: every frame is a fresh context's"""
    n = 150000
    g = scene(n)
    g2 = scene(n, seed=4242)
    r = splat_amd.Renderer()
    try:
        r.upload(g)
        for w, h in ((1920, 1080), (7680, 4320), (1920, 1080), (16, 4320), (4320, 16)):
            cams = [pose(w, h, yaw=0.3 + math.radians(d)) for d in (0.0, 0.0, 1.0, 2.0, 5.0)]
            rest = np.zeros((h, w), np.uint32)
            r.render_frame(cams[0].to_c(0.01), rest)
            assert np.array_equal(rest, fresh_frame(g, cams[0])), (w, h)
            got = async_frames(r, cams, h, w)
            assert got[0] is not None and got[-1] is not None, (w, h)
            for k, a in enumerate(got):
                if a is not None:
                    assert np.array_equal(a, fresh_frame(g, cams[k])), (w, h, k)
        # another scene with the same n, between two frames of the same camera
        cam = pose(1920, 1080)
        before = np.zeros((1080, 1920), np.uint32)
        r.render_frame(cam.to_c(0.01), before)
        r.upload(g2)
        after = np.zeros((1080, 1920), np.uint32)
        r.render_frame(cam.to_c(0.01), after)
        assert np.array_equal(before, fresh_frame(g, cam))
        assert np.array_equal(after, fresh_frame(g2, cam))
        assert not np.array_equal(before, after)
        got = async_frames(r, [cam, pose(1920, 1080, yaw=0.31), cam], 1080, 1920)
        for k, c in enumerate([cam, pose(1920, 1080, yaw=0.31), cam]):
            if got[k] is not None:
                assert np.array_equal(got[k], fresh_frame(g2, c)), k
    finally:
        r.close()


def test_8k_frame_as_slabs():
    """balanced partitions of a 7680 x 4320 frame into 2, 3 and 8 tile-row slabs give the full frame byte for byte, and so does
    a slab of fewer than 12 000 tiles (20 rows of 480) while the full frame has 129 600"""
    from splat_amd import dist as sdist
    w, h = GEOMETRIES["7680x4320"]
    g = scene(scene_size(tiles_of(w, h)))
    R = shared_with(g)
    cam_c = pose(w, h).to_c(0.01)
    full = np.zeros((h, w), np.uint32)
    st = R.render(cam_c, full)
    loads = R.tile_row_loads(cam_c)
    assert len(loads) == 270 and int(loads.sum()) == st.n_pairs
    try:
        for world in (2, 3, 8):
            slabs = sdist.slab_partition_balanced(loads, world)
            parts = np.zeros_like(full)
            for s in slabs:
                R.set_slab(*s)
                R.render(cam_c, parts)
            R.set_slab(0, -1)
            assert np.array_equal(full, parts), (world, int((full != parts).sum()))
        a, b = 125, 145
        assert (b - a) * (w // TILE) < SCAN_WIDE_ABOVE
        R.set_slab(a, b)
        part = np.zeros_like(full)
        R.render(cam_c, part)
        assert np.array_equal(part[a * TILE:b * TILE], full[a * TILE:b * TILE])
        assert not part[:a * TILE].any() and not part[b * TILE:].any()
        assert part.any()
    finally:
        R.set_slab(0, -1)
