"""Retained lists on the GPU (SPLAT_OPT_RETAIN_LISTS, -m gpu): with the camera at rest one frame leaves its lists in order in
memory and the frames behind it launch the compositor alone.  Every comparison is against a second context with the option
off, byte for byte; how many frames are retained is what the decision function (tests/test_retain_decide.py drives the same
one) predicts for the sequence.

The scenes are the smallest at which every kind of tile list exists (counted with the oracle's preprocess; 328 x 200 has a
partial tile column and a partial tile row, 273 tiles):
    synthetic_scene(60000, 7)           1 empty, 1 of one key, 260 of 2..2048 keys, 11 of more (longest 3655)
    synthetic_surface_scene(60000, 7)   88 empty, 10 of one key, 168 of 2..2048 keys, 7 of more (longest 2333)"""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import scene_dict, oracle_camera, channels
from test_retain_decide import Driver, CAM_WORDS, RETAIN, STILL

pytestmark = pytest.mark.gpu

H, W = 200, 328
IMAGES = 4
_SCENES = {}


def scene(name):
    """the scene with its cov3d (computed once, on the GPU)"""
    if name not in _SCENES:
        # ("dense": the cloud with 200000 Gaussians -- its longest list passes 8192 keys, from which the frame policy keeps the
        # near selection on; the two small scenes' frames order their few long lists with the sort launches once a frame has
        # reported, so no selection exists by the time a writer does)
        g = splat_amd.synthetic_surface_scene(60000, 7) if name == "surface" else splat_amd.synthetic_scene(200000 if name == "dense" else 60000, 7)
        R = splat_amd.Renderer()
        try:
            g.compute_cov3d(R)
        finally:
            R.close()
        _SCENES[name] = g
    return _SCENES[name]


def camera(yaw_deg=0.0, h=H, w=W):
    cam = splat_amd.Camera(h, w, (0.0, 0.0, 5.0))
    if yaw_deg:
        cam.update_yaw_angle(math.radians(yaw_deg))
    cam.update_camera_pose()
    return cam


def cam_words(c, slab=(0, -1)):
    raw = bytes(c) + np.asarray(slab, np.int32).tobytes()
    raw += b"\0" * (4 * CAM_WORDS - len(raw))
    return np.frombuffer(raw, np.uint32).tolist()


@contextlib.contextmanager
def context(g, retain, mode=0, options=(), overlap=1):
    R = splat_amd.Renderer(mode=mode) if mode else splat_amd.Renderer()
    try:
        for opt, v in options:
            R.set_option(opt, v)
        R.set_option(_lib.OPT_RETAIN_LISTS, retain)
        if overlap != 1:
            R.set_frame_overlap(overlap)
        R.upload(g)
        yield R
    finally:
        R.close()


class Images:
    def __init__(self, R, n=IMAGES, h=H, w=W, fill=0):
        self.R, self.h, self.w = R, h, w
        self.ptr = [R.device_image(np.full((h, w), fill, np.uint32)) for _ in range(n)]

    def get(self, k):
        return self.R.device_download(self.ptr[k % len(self.ptr)], self.h, self.w)

    def free(self):
        for p in self.ptr:
            self.R.device_free(p)


def async_frames(R, cams, imgs, clear=True):
    """one asynchronous frame per camera into the rotating images, IMAGES in flight between two downloads; every frame downloaded"""
    out = []
    render = R.render_frame_device if clear else R.render_device
    for k0 in range(0, len(cams), len(imgs.ptr)):
        batch = cams[k0:k0 + len(imgs.ptr)]
        for j, c in enumerate(batch):
            render(c, imgs.ptr[j])
        R.sync()
        out += [imgs.get(j) for j in range(len(batch))]
    return out


def predicted(cams, **kw):
    """what the decision function says for these cameras in a row on a fresh scene (every writer clean)"""
    d = Driver(**kw)
    return [d.frame(cam_words(c)) for c in cams]


def both(g, cams, clear=True, fill=0, **kw):
    """the frames of `cams` with retention on and off, and the retaining context's counters"""
    res = []
    for retain in (1, 0):
        with context(g, retain, **kw) as R:
            imgs = Images(R, fill=fill)
            frames = async_frames(R, cams, imgs, clear)
            res.append((frames, R.frames_retained(), R.frames_dropped()))
            imgs.free()
    return res


def assert_equal_frames(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s frame %d: %d pixels differ" % (what, k, int((x != y).sum()))


@pytest.mark.parametrize("name", ["cloud", "surface"])
def test_rest(name):
    c = camera().to_c(0.01, 15)
    cams = [c] * 24
    (on, retained, dropped), (off, retained_off, _) = both(scene(name), cams)
    assert_equal_frames(on, off, name)
    assert on[0].any()
    want = predicted(cams).count(RETAIN)
    assert want == 24 - STILL - 1 > 0
    assert retained == want and retained_off == 0
    assert dropped == 0


@pytest.mark.parametrize("name", ["cloud", "surface"])
def test_path(name):
    a, b = camera().to_c(0.01, 15), camera(1.0).to_c(0.01, 15)
    cams = [a] * 8 + [b] + [a] * 11
    (on, retained, dropped), (off, _, _) = both(scene(name), cams)
    assert_equal_frames(on, off, name)
    acts = predicted(cams)
    assert acts[8] != RETAIN and acts[9] != RETAIN          # the moved frame and the frame after it are binned
    assert retained == acts.count(RETAIN) > 0 and dropped == 0


def _edit_opacity(R, g, held):
    """an in-place opacity edit by index (every third Gaussian gets another's opacity); returns the edited scene"""
    idx = np.ascontiguousarray(np.arange(0, len(g), 3), np.uint32)
    E = splat_amd.GaussianList(g.positions.copy(), g.scales.copy(), g.opacities.copy(), g.rotations.copy(), g.sh.copy(), g.cov3d.copy())
    E.opacities[idx] = g.opacities[::-1][idx] * np.float32(0.5)

    def dev(a):
        a = np.ascontiguousarray(a)
        p = R._L.splat_device_alloc(R._h, a.nbytes)
        assert p
        held.append(p)
        R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p
    R.update_indexed(dev(idx), k=len(idx), opacities=dev(E.opacities[idx]))
    return E


@pytest.mark.parametrize("change", ["edit", "upload", "slab", "option", "target"])
def test_a_change_at_rest_ends_retention(change):
    g = scene("cloud")
    c = camera().to_c(0.01, 15)
    with context(g, 1) as R:
        imgs = Images(R)
        async_frames(R, [c] * 8, imgs)
        before = R.frames_retained()
        assert before == 8 - STILL - 1
        held, slab, ref_g, ref_opts, h2, w2, c2 = [], None, g, (), H, W, c
        if change == "edit":
            ref_g = _edit_opacity(R, g, held)
        elif change == "upload":
            ref_g = g.subset(np.arange(0, len(g), 2))
            R.upload(ref_g)
        elif change == "slab":
            slab = (2, 9)
            R.set_slab(*slab)
        elif change == "option":
            ref_opts = ((_lib.OPT_EARLY_OUT_EPS, 1e-4),)
            R.set_option(*ref_opts[0])
        else:
            h2, w2 = 120, 200
            c2 = camera(h=h2, w=w2).to_c(0.01, 15)
        img = Images(R, 1, h2, w2)
        R.render_frame_device(c2, img.ptr[0], sync=True)
        assert R.frames_retained() == before, change          # the next frame is not retained
        got = img.get(0)
        with context(ref_g, 0, options=ref_opts) as F:
            if slab:
                F.set_slab(*slab)
            fimg = Images(F, 1, h2, w2)
            F.render_frame_device(c2, fimg.ptr[0], sync=True)
            want = fimg.get(0)
            fimg.free()
        assert np.array_equal(got, want), (change, int((got != want).sum()))
        # ... and the rest that follows is retained again, same frames
        more = async_frames(R, [c2] * 8, Images(R, IMAGES, h2, w2))
        assert R.frames_retained() > before and R.frames_dropped() == 0
        for k, f in enumerate(more):
            assert np.array_equal(f, want), (change, k)
        for p in held:
            R.device_free(p)


def test_in_out_image_without_the_fused_clear():
    c = camera().to_c(0.01, 15)
    # every frame blends onto what its image holds: four images, six frames each
    (on, retained, dropped), (off, _, _) = both(scene("cloud"), [c] * 24, clear=False, fill=0x40302010)
    assert_equal_frames(on, off)
    assert not np.array_equal(on[0], on[4])            # (the images really are in/out)
    assert retained == 24 - STILL - 1 and dropped == 0


def test_host_visible_frames_into_a_page_locked_image():
    c = camera().to_c(0.01, 15)
    out = []
    for retain in (1, 0):
        with context(scene("surface"), retain) as R:
            img = R.host_image(H, W)
            frames = []
            for _ in range(10):
                img[:] = 0xDEADBEEF
                R.render_frame(c, img)
                frames.append(img.copy())
            out.append((frames, R.frames_retained()))
    assert_equal_frames(out[0][0], out[1][0])
    assert out[0][1] == 10 - STILL - 1 and out[1][1] == 0


def test_statistics_of_a_retained_frame():
    """the status block of a retained frame is its own: what the compositor counts into it late (waves whose early-out bracket
    did not close) is that frame's count, not a sum over the frames before, and not what the ring entry held 32 frames ago.
    Start hints off and an early-out at transmittance 0.5 make that count large and the same on every frame."""
    c = camera().to_c(0.01, 15)
    opts = ((_lib.OPT_START_HINTS, 0), (_lib.OPT_EARLY_OUT_EPS, 0.5))
    stats = []
    for retain in (1, 0):
        with context(scene("cloud"), retain, options=opts) as R:
            imgs = Images(R)
            async_frames(R, [c] * 12, imgs)
            before = R.frames_retained()
            assert before == (12 - STILL - 1 if retain else 0)
            sts = [R.render_frame_device(c, imgs.ptr[0], sync=True, want_stats=True) for _ in range(40)]    # (more than a ring of 32)
            assert R.frames_retained() == (before + 40 if retain else 0)
            stats.append(sts)
            imgs.free()
    for a, b in zip(*stats):
        assert (a.n_visible, a.n_pairs, a.max_tile_len) == (b.n_visible, b.n_pairs, b.max_tile_len)
        assert a.n_visible > 0 and a.n_pairs > 0 and a.n_iter_blend > 0
    late = [(s.n_fallback, s.n_sort_fallback, s.n_near_fallback) for s in stats[0]]
    print("late counters of retained statistics frames:", late[:3], "reference:", [(s.n_fallback, s.n_sort_fallback, s.n_near_fallback) for s in stats[1][:3]])
    assert late[0][0] > 0, late[0]
    assert all(v == late[0] for v in late), late
    assert all(s.n_fallback == late[0][0] for s in stats[1]), "the binned frames of the same rest count the same waves"


def test_libm_exp_mode_is_the_oracle_bit_for_bit():
    g = scene("cloud")
    cam = camera()
    c = cam.to_c(0.01, 15)
    with context(g, 1, mode=splat_amd.MODE_LIBM_EXP) as R:
        imgs = Images(R)
        frames = async_frames(R, [c] * 12, imgs)
        assert R.frames_retained() == 12 - STILL - 1
        imgs.free()
    ref, _ = O.render(scene_dict(g), oracle_camera(cam, 0.01), nthreads=min(os.cpu_count() or 8, 16))
    for k in (STILL + 1, 11):
        assert np.array_equal(frames[k], ref), k


def test_fast_mode_stays_within_one_of_the_exact_frame():
    g = scene("cloud")
    c = camera().to_c(0.01, 15)
    with context(g, 0) as R:
        imgs = Images(R, 1)
        R.render_frame_device(c, imgs.ptr[0], sync=True)
        exact = imgs.get(0)
        imgs.free()
    with context(g, 1, mode=splat_amd.MODE_FAST) as R:
        imgs = Images(R)
        frames = async_frames(R, [c] * 12, imgs)
        assert R.frames_retained() == 12 - STILL - 1
        imgs.free()
    for k in range(STILL + 1, 12):
        d = np.abs(channels(frames[k]) - channels(exact))
        assert d[..., 1:].max() <= 1 and d[..., 0].max() == 0, k


@pytest.mark.parametrize("name", ["cloud", "surface", "dense"])
def test_forced_repair_inside_retained_frames(name, monkeypatch):
    """Selections of 128 keys that ignore what the walks needed before (SPLAT_DBG_SELECT_BLIND): on every BINNED frame the long
    tiles' walks run out of their selection and the tiles repair inside the compositor -- the writer's among them.  A repair
    sorts the list in place through the room its selection lay in, so the retained frames behind the writer must find the tile
    marked as in order (near_m = the list's length): they equal the reference's frames, and they have nothing left to repair
    but the tiles the writer's walks did not (each at most once).  On the two small scenes only the first frame selects (see
    scene()): there the frames are compared and the set must exist; the repair assertions are the dense scene's."""
    monkeypatch.setenv("SPLAT_DBG_SELECT_BLIND", "1")
    c = camera().to_c(0.01, 15)
    opts = ((_lib.OPT_NEAR_SELECT_KEYS, 128),)
    n_frames = STILL + 1 + 4                  # the writer is frame STILL; four retained frames behind it
    res = []
    for retain in (1, 0):
        with context(scene(name), retain, options=opts) as R:
            imgs = Images(R)
            frames, sts = [], []
            for k in range(n_frames):
                sts.append(R.render_frame_device(c, imgs.ptr[k % IMAGES], sync=True, want_stats=True))
                frames.append(imgs.get(k))
            res.append((frames, sts, R.frames_retained(), R.frames_dropped()))
            imgs.free()
    (on, st_on, retained, dropped), (off, st_off, _, _) = res
    assert_equal_frames(on, off, name)
    assert retained == 4 and dropped == 0
    print("repairs per frame, retaining:", [(s.n_near_tiles, s.n_near_fallback) for s in st_on], "reference:", [s.n_near_fallback for s in st_off])
    if name != "dense":
        return
    assert all(s.n_near_fallback > 0 for s in st_off)                   # every binned frame repairs
    writer = st_on[STILL]
    assert writer.n_near_tiles > 0 and writer.n_near_fallback > 0       # ... the writer too: the set exists over repaired tiles
    later = sum(s.n_near_fallback for s in st_on[STILL + 1:])
    assert later <= writer.n_near_tiles - writer.n_near_fallback, (later, writer.n_near_tiles, writer.n_near_fallback)


# SPLAT_OPT_PIPELINE_DEPTH 1 retains (one slot: the writer's); two-pass binning never does (include/splat_retain.h)
@pytest.mark.parametrize("opts,retains", [(((_lib.OPT_SORT_IN_COMPOSITOR, 0),), True), (((_lib.OPT_SORT_IN_COMPOSITOR, 1),), True),
                                           (((_lib.OPT_NEAR_SELECT_KEYS, 0),), True), (((_lib.OPT_PIPELINE_DEPTH, 1),), True),
                                           (((_lib.OPT_ONE_PASS_BINNING, 0),), False),
                                           (((_lib.OPT_NEAR_SELECT_KEYS, 0), (_lib.OPT_SORT_IN_COMPOSITOR, 1)), True)])
def test_orderings(opts, retains):
    c = camera().to_c(0.01, 15)
    (on, retained, dropped), (off, _, _) = both(scene("cloud"), [c] * 12, options=opts)
    assert_equal_frames(on, off, str(opts))
    assert dropped == 0
    assert retained == (12 - STILL - 1 if retains else 0), opts


def test_frame_overlap_two_never_retains():
    c = camera().to_c(0.01, 15)
    (on, retained, dropped), (off, _, _) = both(scene("cloud"), [c] * 12, overlap=2)
    assert_equal_frames(on, off)
    assert retained == 0 and dropped == 0
    assert predicted([c] * 12, overlap=2).count(RETAIN) == 0
