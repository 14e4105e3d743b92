"""Proven starts of a retained set (-m gpu): a frame composited from retained lists whose hinted walk starts exactly where a
bracketed walk of an earlier frame of the set closed goes single-state from there -- the lists are the same bytes, so the
bracket would close again.  The frame must be what the bracket gives: every comparison is against a context created with
SPLAT_DBG_PROVEN_STARTS=0 (every early-out walk bracketed, as in a binned frame), byte for byte and count for count.
SPLAT_DBG_PROVEN_STARTS=2 starts such walks from state 255 instead of 0: the proof's claim from the other end.
SPLAT_DBG_BRACKET_COUNT=1 makes a retained statistics frame report the steps walked with both states (as n_iter_scan), which
is how a test sees from outside that proofs are taken.

Scenes, target and helpers are those of test_gpu_retain_lists.py; the sequences are those of test_gpu_stage_cache.py."""
import ctypes as C
import os

import numpy as np
import pytest

import splat_amd
from oracle import oracle as O
from splat_amd import _lib
from helpers import scene_dict, oracle_camera
from test_retain_decide import STILL
from test_gpu_retain_lists import H, W, IMAGES, Images, async_frames, assert_equal_frames, camera, context, scene, _edit_opacity

pytestmark = pytest.mark.gpu

SCANS = ((_lib.OPT_START_HINTS, 0), (_lib.OPT_EARLY_OUT_EPS, 0.5))      # every frame scans and retries
REFINE_THEN = ((SCANS, 12), (((_lib.OPT_START_HINTS, 2),), 12))         # ... then hinted starts with a margin


def rest(monkeypatch, proofs, name, frames=24, mode=0, options=(), then=(), lead=0):
    """`frames` asynchronous frames at rest with SPLAT_DBG_PROVEN_STARTS=proofs (behind `lead` synchronous ones, not returned),
    then for every (options, frames) of `then` the options set and that many more; returns (every frame, frames retained,
    frames dropped)"""
    monkeypatch.setenv("SPLAT_DBG_PROVEN_STARTS", str(proofs))
    c = camera().to_c(0.01, 15)
    with context(scene(name), 1, mode=mode, options=options) as R:
        imgs = Images(R)
        for _ in range(lead):
            R.render_frame_device(c, imgs.ptr[0], sync=True)
        out = async_frames(R, [c] * frames, imgs)
        for opts, n in then:
            for o, v in opts:
                R.set_option(o, v)
            out += async_frames(R, [c] * n, imgs)
        res = (out, R.frames_retained(), R.frames_dropped())
        imgs.free()
    return res


_OFF = {}


def off(monkeypatch, name, **kw):
    """the frames with every walk bracketed: rendered once per sequence, shared, never changed"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _OFF:
        _OFF[key] = rest(monkeypatch, 0, name, **kw)
    return _OFF[key]


def on_and_off(monkeypatch, name, proofs=1, **kw):
    (on, kept, dropped), (ref, kept_off, dropped_off) = rest(monkeypatch, proofs, name, **kw), off(monkeypatch, name, **kw)
    assert_equal_frames(on, ref, name)
    assert kept == kept_off > 0 and dropped == dropped_off == 0
    return on, kept


@pytest.mark.parametrize("name", ["cloud", "surface", "dense"])
def test_frames_at_rest(name, monkeypatch):
    on, kept = on_and_off(monkeypatch, name)
    assert kept == 24 - STILL - 1 and on[0].any()
    assert_equal_frames(on, [on[0]] * 24, name)


@pytest.mark.parametrize("name", ["cloud", "dense"])
def test_a_proven_walk_from_state_255_is_the_same_frame(name, monkeypatch):
    on, kept = on_and_off(monkeypatch, name, proofs=2)
    assert kept == 24 - STILL - 1


@pytest.mark.parametrize("name", ["cloud", "dense", "surface"])
def test_libm_exp_mode_is_the_oracle_bit_for_bit(name, monkeypatch):
    """(the cloud is the issue's case; its walks take no proof -- see test_retained_frames_take_their_proofs -- so the two
    scenes whose walks do are what holds a proven walk to the oracle)"""
    on, _ = on_and_off(monkeypatch, name, mode=splat_amd.MODE_LIBM_EXP)
    ref, _ = O.render(scene_dict(scene(name)), oracle_camera(camera(), 0.01), nthreads=min(os.cpu_count() or 8, 16))
    assert_equal_frames(on, [ref] * 24, "oracle")


def probe_failures(R):
    """n_probe_fail of the last synchronous statistics frame (the debug getter; tests/test_gpu_start_refine.py)"""
    f = R._L.splat_debug_probe_failures
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]
    n = C.c_uint64()
    assert f(R._h, C.byref(n)) == 0
    return int(n.value)


def stats_sequence(monkeypatch, proofs, name, n_frames, bracket_count=False, options=()):
    """synchronous statistics frames at rest (synchronous: see test_gpu_stage_cache.py); returns their statistics (each with
    its frame's n_probe_fail as `probe_fail`) and how many were composited from retained lists"""
    monkeypatch.setenv("SPLAT_DBG_PROVEN_STARTS", str(proofs))
    if bracket_count:
        monkeypatch.setenv("SPLAT_DBG_BRACKET_COUNT", "1")
    c = camera().to_c(0.01, 15)
    with context(scene(name), 1, options=options) as R:
        imgs = Images(R)
        sts = []
        for _ in range(n_frames):
            st = R.render_frame_device(c, imgs.ptr[0], sync=True, want_stats=True)
            st.probe_fail = probe_failures(R)
            sts.append(st)
        kept = R.frames_retained()
        assert R.frames_dropped() == 0
        imgs.free()
    return sts, kept


@pytest.mark.parametrize("name", ["cloud", "dense", "surface"])
def test_a_proven_walk_takes_the_steps_a_bracketed_one_does(name, monkeypatch):
    """the window in which refinement probes: probes, retries and proofs taken and left, frame by frame"""
    n_frames = STILL + 1 + 10
    work = []
    for proofs in (1, 0):
        sts, kept = stats_sequence(monkeypatch, proofs, name, n_frames)
        assert kept == 10
        work.append([(s.n_iter_blend, s.n_fallback, s.n_near_fallback, s.probe_fail) for s in sts])
    print("(n_iter_blend, n_fallback, n_near_fallback, n_probe_fail) of the writer and the frames behind it:", work[0][STILL:])
    assert all(w[0] > 0 for w in work[0])
    assert work[0] == work[1]


@pytest.mark.parametrize("name", ["cloud", "dense", "surface"])
def test_retained_frames_take_their_proofs(name, monkeypatch):
    """40 frames: start refinement has converged, no walk probes any more.  Bracketed steps are reported in n_iter_scan.
    Measured, steps with both states / blend steps of a frame at rest with proofs off: cloud 0 / 97 999, dense 14 550 / 276 720,
    surface 2 517 / 100 206; with proofs on 0 in all three.  On the cloud no hinted walk brackets at all: no wave of that scene
    saturates within three quarters of its list, and such a walk's hint says "the whole list, without a bracket" (the same
    with the early-out at transmittance 0.5).  There is nothing for a proof to save there and nothing to be positive: the
    cloud is held to equal counts, the two scenes whose walks do start inside their lists to "positive" and "a tenth"."""
    n_frames = 40
    (on, kept), (ref, kept_off) = (stats_sequence(monkeypatch, p, name, n_frames, bracket_count=True) for p in (1, 0))
    assert kept == kept_off == n_frames - STILL - 1
    last = slice(n_frames - 4, n_frames)
    br_on, br_off = [s.n_iter_scan for s in on[last]], [s.n_iter_scan for s in ref[last]]
    print("steps with both states, last frames: proofs on", br_on, "off", br_off, "of", [s.n_iter_blend for s in ref[last]])
    if name != "cloud":
        assert all(b > 0 for b in br_off)
    assert all(10 * a < b or a == b == 0 for a, b in zip(br_on, br_off))
    assert [s.n_iter_blend for s in on] == [s.n_iter_blend for s in ref]


@pytest.mark.parametrize("name", ["cloud", "dense", "surface"])
def test_refinement_scans_and_retries(name, monkeypatch):
    """test_gpu_stage_cache.py's sequence: refinement converges, proofs left and taken (on dense and surface: the cloud's walks
    take none); then every frame scans and retries, over a table that still holds those proofs; then hinted starts with a
    margin, which match no proof"""
    on, kept = on_and_off(monkeypatch, name, frames=40, then=REFINE_THEN)
    assert kept > 40 - STILL - 1


_BRACKETED_OFF = {}


def bracketed_at_rest(R, c, imgs):
    """(steps with both states, blend steps) of one synchronous statistics frame (SPLAT_DBG_BRACKET_COUNT=1), which must be
    a retained one"""
    r0 = R.frames_retained()
    st = R.render_frame_device(c, imgs.ptr[0], sync=True, want_stats=True)
    assert R.frames_retained() == r0 + 1
    return int(st.n_iter_scan), int(st.n_iter_blend)


def bracketed_with_proofs_off(monkeypatch, name):
    """the same figures behind 40 frames at rest of a context that takes no proofs: once per scene"""
    if name not in _BRACKETED_OFF:
        monkeypatch.setenv("SPLAT_DBG_PROVEN_STARTS", "0")
        monkeypatch.setenv("SPLAT_DBG_BRACKET_COUNT", "1")
        c = camera().to_c(0.01, 15)
        with context(scene(name), 1) as R:
            imgs = Images(R)
            async_frames(R, [c] * 40, imgs)
            _BRACKETED_OFF[name] = bracketed_at_rest(R, c, imgs)
            imgs.free()
    return _BRACKETED_OFF[name]


@pytest.mark.parametrize("change", ["edit", "upload", "slab", "option", "target"])
@pytest.mark.parametrize("name", ["cloud", "dense", "surface"])
def test_proofs_are_not_trusted_across_a_change(name, change, monkeypatch):
    """40 frames at rest; on dense and surface the set's proofs are then in the table and in use, which a statistics frame
    shows (steps with both states: positive in a context that takes no proofs, under a tenth of that here; the cloud, the
    issue's case, has none either way).  Then something the lists depend on changes, and the next rest must be a fresh
    context's frame"""
    off_steps, off_blend = bracketed_with_proofs_off(monkeypatch, name)
    monkeypatch.setenv("SPLAT_DBG_PROVEN_STARTS", "1")
    monkeypatch.setenv("SPLAT_DBG_BRACKET_COUNT", "1")
    g = scene(name)
    c = camera().to_c(0.01, 15)
    with context(g, 1) as R:
        imgs = Images(R)
        async_frames(R, [c] * 40, imgs)
        assert R.frames_retained() == 40 - STILL - 1
        on_steps, on_blend = bracketed_at_rest(R, c, imgs)
        print("steps with both states before the change: proofs on %d, off %d, of %d blend steps" % (on_steps, off_steps, off_blend))
        if name != "cloud":
            assert off_steps > 0 and 10 * on_steps < off_steps
        before = R.frames_retained()
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
        imgs2 = Images(R, IMAGES, h2, w2)
        got = async_frames(R, [c2] * 12, imgs2)
        assert R.frames_retained() >= before + 12 - STILL - 1 and R.frames_dropped() == 0
        imgs2.free()
        imgs.free()
        for p in held:
            R.device_free(p)
    with context(ref_g, 0, options=ref_opts) as F:
        if slab:
            F.set_slab(*slab)
        fimg = Images(F, 1, h2, w2)
        F.render_frame_device(c2, fimg.ptr[0], sync=True)
        want = fimg.get(0)
        fimg.free()
    assert want.any()
    assert_equal_frames(got, [want] * 12, change)


def test_forced_repair_inside_retained_frames(monkeypatch):
    """test_gpu_retain_lists.py's sequence on the dense scene: tiles repair inside the writer and inside retained frames"""
    monkeypatch.setenv("SPLAT_DBG_SELECT_BLIND", "1")
    c = camera().to_c(0.01, 15)
    n_frames = STILL + 1 + 4
    res = []
    for proofs in (1, 0):
        monkeypatch.setenv("SPLAT_DBG_PROVEN_STARTS", str(proofs))
        with context(scene("dense"), 1, options=((_lib.OPT_NEAR_SELECT_KEYS, 128),)) as R:
            imgs = Images(R)
            frames, late = [], []
            for k in range(n_frames):
                s = R.render_frame_device(c, imgs.ptr[k % IMAGES], sync=True, want_stats=True)
                late.append((s.n_fallback, s.n_sort_fallback, s.n_near_tiles, s.n_near_fallback, s.n_iter_blend))
                frames.append(imgs.get(k))
            res.append((frames, late, R.frames_retained(), R.frames_dropped()))
            imgs.free()
    (on, late_on, kept, dropped), (ref, late_off, kept_off, _) = res
    assert_equal_frames(on, ref)
    print("late counters:", late_on)
    assert late_on == late_off
    assert kept == kept_off == 4 and dropped == 0
    assert late_on[STILL][3] > 0                    # the writer repairs


def test_fast_mode(monkeypatch):
    """nothing is taken in fast mode (two synchronous frames in front: see test_gpu_stage_cache.py's test_fast_mode)"""
    on, kept = on_and_off(monkeypatch, "cloud", mode=splat_amd.MODE_FAST, lead=2)
    assert kept >= 24 - STILL - 1
