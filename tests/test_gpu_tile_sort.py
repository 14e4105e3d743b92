"""GPU tests (-m gpu): every route that puts a tile list in order is held to the oracle's stable sort, key for key.

The scenes of tests/sort_cases.py give each tile one list of a chosen length and chosen depth-key bits (tests/test_sort_cases_host.py
shows, by the oracle alone, that they do).  Every route below renders them with a statistics pointer and reads the lists back
(splat_get_tile_lists): offsets and order must equal the oracle's exactly -- membership, order and tie order -- in the scene's first
frame, which is binned into bootstrap regions, and in its third, whose regions were sized from the frames before; the pair count is
the number of Gaussians and no frame is dropped.  A mismatch names the tile with its length and pattern, the first wrong position
with the indices and depth bits there, and whether the list still holds the expected keys (misordered) or not (a key lost or held
twice).

    (a) defaults          lists of up to 2048 keys are sorted by their tile's compositor workgroup and written back.  The longer
                          ones are served by the near selection, whose output cannot be read back: for them the GETTER runs the sort
                          launches (sort_tiles_kernel<512, 8192>, <1024, 16384>, merge_runs_kernel, sort_list_global) behind the
                          frame -- so this route holds those launches on a near-selection frame's regions, NOT the selection, which
                          stays held by the frame's bytes only
    (b) FUSED_SORT_MAX 0, SORT_IN_COMPOSITOR 0, NEAR_SELECT_KEYS 0
                          every list through the sort launches, sort_tiles_kernel<256, 2048> included
    (c) SORT_IN_COMPOSITOR 1, NEAR_SELECT_KEYS 0
                          long lists through the compositor's partition_long_list and its global fallback
    (d) SPLAT_SORT_RADIX_MIN = 0 and = 2048, on the lists of up to 2048 keys: the radix sort at 2, 3 and 63 keys, the bitonic
                          network at 2047 and 2048
    (e) NEAR_SELECT_KEYS 0, RETAIN_LISTS 1, one camera until a frame was retained: the lists read then are still the expected ones

each with one-pass and with two-pass binning ((e): one-pass, the only path that retains).  The frames of all of them are the same
bytes, within 1 LSB of the oracle's frame (the SPLAT_MODE_LIBM_EXP frame: the oracle's bit for bit)."""
import numpy as np
import pytest

import splat_amd
import sort_cases as SC
from splat_amd import _lib as L
from helpers import image_diff

pytestmark = pytest.mark.gpu

TOL_LSB = 1          # the project's bar (tests/test_gpu_parity.py)

DEFAULTS = ((L.OPT_FUSED_SORT_MAX, 2048), (L.OPT_SORT_IN_COMPOSITOR, -1), (L.OPT_NEAR_SELECT_KEYS, 2048))
ROUTES = {
    "a": DEFAULTS,
    "b": ((L.OPT_FUSED_SORT_MAX, 0), (L.OPT_SORT_IN_COMPOSITOR, 0), (L.OPT_NEAR_SELECT_KEYS, 0)),
    "c": ((L.OPT_FUSED_SORT_MAX, 2048), (L.OPT_SORT_IN_COMPOSITOR, 1), (L.OPT_NEAR_SELECT_KEYS, 0)),
    "near64": ((L.OPT_FUSED_SORT_MAX, 2048), (L.OPT_SORT_IN_COMPOSITOR, -1), (L.OPT_NEAR_SELECT_KEYS, 64)),
}
OPTION_NAMES = {L.OPT_FUSED_SORT_MAX: "FUSED_SORT_MAX", L.OPT_SORT_IN_COMPOSITOR: "SORT_IN_COMPOSITOR", L.OPT_NEAR_SELECT_KEYS: "NEAR_SELECT_KEYS",
                L.OPT_ONE_PASS_BINNING: "ONE_PASS_BINNING", L.OPT_RETAIN_LISTS: "RETAIN_LISTS"}
BINNING = {"one-pass": 1, "two-pass": 0}
_results = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _results.clear()
    SC.forget_scenes()


def open_route(settings, one_pass, retain=0, mode=0):
    """a context with the route's options in force; skips when the environment pins one of them to something else"""
    R = splat_amd.Renderer(mode=mode) if mode else splat_amd.Renderer()
    try:
        for opt, v in tuple(settings) + ((L.OPT_ONE_PASS_BINNING, one_pass), (L.OPT_RETAIN_LISTS, retain)):
            R.set_option(opt, v)
            if R.get_option(opt) != v:
                pytest.skip("SPLAT_OPT_%s is pinned to %g by the environment, the route needs %g" % (OPTION_NAMES[opt], R.get_option(opt), v))
    except BaseException:
        R.close()
        raise
    return R


def list_mismatch(s, R, st):
    """None, or what is wrong with the lists of the frame just rendered"""
    if st.n_pairs != s.n:
        return "%s: %d pairs, %d Gaussians" % (s.name, st.n_pairs, s.n)
    off, order = R.tile_lists(s.n_tiles, int(st.n_pairs))
    eoff, eorder = s.expected()
    return SC.describe_mismatch(s, off, order, eoff, eorder)


def three_frames(s, R, one_pass):
    """three statistics frames of the scene on a context that has none yet: {frames, fallbacks, mismatch of the first and of the
    third frame's lists, dropped}"""
    R.upload(s.g)
    frames, fallbacks, wrong = [], [], []
    for k in range(3):
        img = np.zeros((s.h, s.w), np.uint32)
        st = R.render(s.cam_c(), img)
        frames.append(img)
        fallbacks.append(int(st.n_sort_fallback))
        if k != 1:
            wrong.append(list_mismatch(s, R, st))
        assert (R.binning_mode() > 0) == bool(one_pass), ("binning path", R.binning_mode(), one_pass)
    return dict(frames=frames, fallbacks=fallbacks, wrong=wrong, dropped=R.frames_dropped())


def run(scene, route, binning):
    key = (scene, route, binning)
    if key not in _results:
        s = SC.scene(scene)
        R = open_route(ROUTES[route], BINNING[binning])
        try:
            _results[key] = three_frames(s, R, BINNING[binning])
        finally:
            R.close()
        print("n_sort_fallback of %s, route (%s), %s binning, frames 1-3: %s" % (scene, route, binning, _results[key]["fallbacks"]))
    return _results[key]


@pytest.mark.parametrize("binning", list(BINNING))
@pytest.mark.parametrize("route", ["a", "b", "c"])
@pytest.mark.parametrize("scene", ["sweep", "patterns", "distinct"])
def test_route_leaves_the_oracles_lists(scene, route, binning):
    """routes (a), (b), (c): first and third frame, lists exact.  The patterns scene holds all-equal lists longer than
    sort_radix_min: its frames must count bitonic fallbacks -- the fallback ran, and its result is what was compared.  The counter
    of the scene without a single tie is printed only: a fallback there means that the lane-order assumption noted in
    radix_sort_depth did not hold, which costs time, not correctness."""
    res = run(scene, route, binning)
    for k, msg in zip((1, 3), res["wrong"]):
        assert msg is None, "route (%s), %s binning, frame %d: %s" % (route, binning, k, msg)
    assert res["dropped"] == 0
    if scene == "patterns":
        assert min(res["fallbacks"]) >= 1, res["fallbacks"]


@pytest.mark.parametrize("radix_min", [0, 2048])
@pytest.mark.parametrize("scene", ["sweep_short", "patterns_short"])
def test_radix_and_bitonic_at_every_short_length(scene, radix_min, monkeypatch):
    """route (d): SPLAT_SORT_RADIX_MIN (read when the context is made) = 0: the radix sort and its tie fix-up from 2 keys on;
    = 2048: the bitonic network up to 2047 and 2048 keys -- in the compositor's own sort (a) and in sort_tiles_kernel<256, 2048>
    (b), one-pass and two-pass.  With 2048 no list of these scenes takes the radix sort, so nothing can fall back from it: that the
    counter stays 0 over lists at ONE depth shows the variable was read."""
    s = SC.scene(scene)
    for route in ("a", "b"):
        for binning, one_pass in BINNING.items():
            with monkeypatch.context() as mp:
                mp.setenv("SPLAT_SORT_RADIX_MIN", str(radix_min))
                R = open_route(ROUTES[route], one_pass)
            try:
                res = three_frames(s, R, one_pass)
            finally:
                R.close()
            print("n_sort_fallback of %s, SPLAT_SORT_RADIX_MIN=%d, route (%s), %s binning: %s" % (scene, radix_min, route, binning, res["fallbacks"]))
            for k, msg in zip((1, 3), res["wrong"]):
                assert msg is None, "SPLAT_SORT_RADIX_MIN=%d, route (%s), %s binning, frame %d: %s" % (radix_min, route, binning, k, msg)
            assert res["dropped"] == 0
            if radix_min == 2048:
                assert max(res["fallbacks"]) == 0, res["fallbacks"]


@pytest.mark.parametrize("scene", ["sweep", "patterns"])
def test_lists_behind_a_retained_frame(scene):
    """route (e): the same camera until frames_retained() has grown; the lists read then -- the writer's, which the retained frame
    composited from -- are the expected ones, and the retained frame is the frame of route (b)"""
    s = SC.scene(scene)
    R = open_route(((L.OPT_NEAR_SELECT_KEYS, 0),), 1, retain=1)
    try:
        R.upload(s.g)
        img = st = None
        for k in range(16):
            img = np.zeros((s.h, s.w), np.uint32)
            st = R.render(s.cam_c(), img)
            if R.frames_retained() > 0:
                break
        assert R.frames_retained() > 0, "no frame of 16 at rest was retained"
        msg = list_mismatch(s, R, st)
        assert msg is None, "behind a retained frame (frame %d): %s" % (k + 1, msg)
        assert R.frames_dropped() == 0
    finally:
        R.close()
    want = run(scene, "b", "one-pass")["frames"][0]
    assert np.array_equal(img, want), int((img != want).sum())


@pytest.mark.parametrize("scene", ["sweep", "patterns"])
def test_every_route_renders_the_same_bytes(scene):
    """every exact-mode route, near selection at 2048 (route (a)) and at 64 keys: the bytes of route (b); those within 1 LSB per
    channel of the oracle's frame; the SPLAT_MODE_LIBM_EXP frame the oracle's bit for bit"""
    s = SC.scene(scene)
    base = run(scene, "b", "one-pass")["frames"][0]
    assert base.any()
    for route in ("a", "b", "c", "near64"):
        for binning in BINNING:
            res = run(scene, route, binning)
            for k, img in enumerate(res["frames"]):
                assert np.array_equal(img, base), "route (%s), %s binning, frame %d: %d pixels differ from route (b)" % (
                    route, binning, k + 1, int((img != base).sum()))
            assert res["dropped"] == 0
    ref, ost = s.oracle_frame()
    assert ost.n_tile_pairs == s.n
    mx, cnt = image_diff(base, ref)
    print("%s: %d pixels differ from the oracle's, by at most %d LSB" % (scene, cnt, mx))
    assert mx <= TOL_LSB, (mx, cnt)
    R = open_route(DEFAULTS, 1, mode=splat_amd.MODE_LIBM_EXP)
    try:
        R.upload(s.g)
        exact = np.zeros((s.h, s.w), np.uint32)
        st = R.render(s.cam_c(), exact)
        assert st.n_pairs == s.n
    finally:
        R.close()
    assert np.array_equal(exact, ref), image_diff(exact, ref)
