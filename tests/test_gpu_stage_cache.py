"""Staging verdicts kept from one retained frame to the next (-m gpu): a frame composited from retained lists takes the masks
the frames before it left -- which records of a 64-record batch reach its wave's 8x8 block -- instead of computing them again.
A kept verdict must stage exactly the records a computed one does: every comparison is against a context created with
SPLAT_DBG_STAGE_CACHE=0 (nothing kept), byte for byte and count for count.  SPLAT_DBG_STAGE_CACHE=2 zeroes the kept masks
behind the second retained frame of a set, which is the one way to see from outside that frames really read them.

Scenes, target and helpers are those of test_gpu_retain_lists.py (empty tiles, one-key lists, lists of 2..2048 keys and longer
ones; "dense" has a near selection at the writer)."""
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


def rest(monkeypatch, cache, name, frames=24, mode=0, options=(), then=(), lead=0):
    """`frames` asynchronous frames at rest with SPLAT_DBG_STAGE_CACHE=cache (behind `lead` synchronous ones, not returned),
    then for every (options, frames) of `then` the options set and that many more; returns (every frame, frames retained,
    frames dropped)"""
    monkeypatch.setenv("SPLAT_DBG_STAGE_CACHE", str(cache))
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


def on_and_off(monkeypatch, name, **kw):
    (on, kept, dropped), (off, kept_off, dropped_off) = rest(monkeypatch, 1, name, **kw), rest(monkeypatch, 0, name, **kw)
    assert_equal_frames(on, off, name)
    assert kept == kept_off > 0 and dropped == dropped_off == 0
    return on, kept


@pytest.mark.parametrize("name", ["cloud", "surface", "dense"])
def test_frames_at_rest(name, monkeypatch):
    on, kept = on_and_off(monkeypatch, name)
    assert kept == 24 - STILL - 1 and on[0].any()
    assert_equal_frames(on, [on[0]] * 24, name)


def test_libm_exp_mode_is_the_oracle_bit_for_bit(monkeypatch):
    on, _ = on_and_off(monkeypatch, "cloud", mode=splat_amd.MODE_LIBM_EXP)
    ref, _ = O.render(scene_dict(scene("cloud")), oracle_camera(camera(), 0.01), nthreads=min(os.cpu_count() or 8, 16))
    assert_equal_frames(on, [ref] * 24, "oracle")


def test_fast_mode(monkeypatch):
    """A fast-mode frame depends on where its walks start (within one count of the exact frame), and that follows how the
    frame's long lists were ordered, which the frame policy decides from what earlier frames have reported to the host when the
    frame is enqueued: 24 asynchronous frames on a fresh context came out as three different sequences in 8 runs (4 pixels apart)
    with nothing kept and with retention off alike.  Two synchronous frames in front -- the policy has its reports -- and the 24
    asynchronous frames behind them are one sequence in 8 of 8 runs: those are compared, byte for byte."""
    on, kept = on_and_off(monkeypatch, "cloud", mode=splat_amd.MODE_FAST, lead=2)
    assert kept >= 24 - STILL - 1


@pytest.mark.parametrize("name", ["cloud", "dense"])
def test_a_kept_verdict_stages_what_a_computed_one_does(name, monkeypatch):
    """(every frame of the sequence is synchronous: how the binned frames in front of the writer order their long lists --
    and with it how many of a list's records a walk of the set meets -- follows what earlier frames have reported to the host
    by the time a frame is enqueued, which two runs of asynchronous frames do not have in common)"""
    c = camera().to_c(0.01, 15)
    n_frames = STILL + 1 + 10
    work = []
    for cache in (1, 0):
        monkeypatch.setenv("SPLAT_DBG_STAGE_CACHE", str(cache))
        with context(scene(name), 1) as R:
            imgs = Images(R)
            sts = [R.render_frame_device(c, imgs.ptr[0], sync=True, want_stats=True) for _ in range(n_frames)]
            assert R.frames_retained() == 10
            work.append([(s.n_iter_blend, s.n_fallback, s.n_near_fallback) for s in sts])
            imgs.free()
    print("(n_iter_blend, n_fallback, n_near_fallback) of the writer and the frames behind it:", work[0][STILL:])
    assert all(w[0] > 0 for w in work[0])
    assert work[0] == work[1]


def test_retained_frames_read_the_kept_masks(monkeypatch):
    (frames, kept, _) = rest(monkeypatch, 2, "cloud", frames=12)
    assert kept == 12 - STILL - 1
    for k in range(STILL + 3):                      # binned frames, the writer, the set's first two frames
        assert np.array_equal(frames[k], frames[0]), k
    wrong = [int((f != frames[0]).sum()) for f in frames[STILL + 3:]]
    print("pixels that differ once the kept masks are zeroed:", wrong)
    assert all(w > 0 for w in wrong), wrong


def test_refinement_scans_and_retries(monkeypatch):
    """40 frames let start refinement converge; then every frame scans and retries (start hints 0, early-out at
    transmittance 0.5: test_statistics_of_a_retained_frame's configuration -- such frames keep their scan's verdicts, take
    and leave none); then hinted starts that are too shallow and go deeper, where the kept batches grow within the set"""
    scans = ((_lib.OPT_START_HINTS, 0), (_lib.OPT_EARLY_OUT_EPS, 0.5))
    on, kept = on_and_off(monkeypatch, "cloud", frames=40, then=((scans, 12), (((_lib.OPT_START_HINTS, 2),), 12)))
    assert kept > 40 - STILL - 1


def test_forced_repair_inside_retained_frames(monkeypatch):
    """test_gpu_retain_lists.py's sequence on the dense scene: tiles repair inside the writer and inside retained frames"""
    monkeypatch.setenv("SPLAT_DBG_SELECT_BLIND", "1")
    c = camera().to_c(0.01, 15)
    n_frames = STILL + 1 + 4
    res = []
    for cache in (1, 0):
        monkeypatch.setenv("SPLAT_DBG_STAGE_CACHE", str(cache))
        with context(scene("dense"), 1, options=((_lib.OPT_NEAR_SELECT_KEYS, 128),)) as R:
            imgs = Images(R)
            frames, late = [], []
            for k in range(n_frames):
                s = R.render_frame_device(c, imgs.ptr[k % IMAGES], sync=True, want_stats=True)
                late.append((s.n_fallback, s.n_sort_fallback, s.n_near_tiles, s.n_near_fallback, s.n_iter_blend))
                frames.append(imgs.get(k))
            res.append((frames, late, R.frames_retained(), R.frames_dropped()))
            imgs.free()
    (on, late_on, kept, dropped), (off, late_off, kept_off, _) = res
    assert_equal_frames(on, off)
    print("late counters:", late_on)
    assert late_on == late_off
    assert kept == kept_off == 4 and dropped == 0
    assert late_on[STILL][3] > 0                    # the writer repairs


def test_walks_of_more_than_32_batches(monkeypatch):
    """no early-out: every walk takes its whole list, the longest 3655 keys = 58 batches, of which the nearest 32 are kept"""
    on, kept = on_and_off(monkeypatch, "cloud", frames=16, options=((_lib.OPT_EARLY_OUT_EPS, 0.0),))
    assert kept == 16 - STILL - 1


@pytest.mark.parametrize("change", ["edit", "upload", "slab", "option", "target"])
def test_the_next_rest_starts_from_nothing(change, monkeypatch):
    monkeypatch.setenv("SPLAT_DBG_STAGE_CACHE", "1")
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
