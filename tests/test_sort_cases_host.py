"""The scenes of tests/sort_cases.py are what they claim, by the oracle alone (no GPU): every Gaussian is visible and sits in one
tile, the per-tile counts are the intended lengths, the view depth is z bit for bit, every pattern has the key span and the
tie runs it promises, and the expected order is a permutation of each tile's members.  tests/test_gpu_tile_sort.py relies on
exactly these conditions when it compares the device's lists with the oracle's."""
import numpy as np
import pytest

import sort_cases as SC
from oracle import oracle as O
from helpers import scene_dict, oracle_camera, make_camera, with_oracle_cov3d

SCENES = ("sweep", "patterns", "distinct", "sweep_short", "patterns_short")


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    SC.forget_scenes()


_pre = {}


def preprocessed(name):
    if name not in _pre:
        s = SC.scene(name)
        _pre[name] = O.preprocess(scene_dict(s.g), oracle_camera(s.cam, SC.LOWPASS))
    return _pre[name]


def test_the_scenes_hold_the_lengths_the_issue_names():
    assert len(SC.SWEEP_LENGTHS) == 38 and SC.scene("sweep").n == 549336 and SC.scene("sweep").w == 128
    assert len(SC.PATTERNS) == 20 and len(SC.scene("patterns").cases) == 140
    assert sorted(set(n for n, _ in SC.scene("patterns").cases)) == list(SC.PATTERN_LENGTHS)
    assert max(n for n, _ in SC.scene("sweep_short").cases) == SC.FUSED_MAX == max(n for n, _ in SC.scene("patterns_short").cases)
    for a in (128, 1408, 2048, 8192, 16384, 65536):             # both sides of every length switch
        assert {a - 1, a, a + 1} <= set(SC.SWEEP_LENGTHS) or {a, a + 1} <= set(SC.SWEEP_LENGTHS), a


@pytest.mark.parametrize("name", SCENES)
def test_every_gaussian_is_visible_in_one_tile_at_its_own_depth(name):
    s = SC.scene(name)
    pre = preprocessed(name)
    assert (pre["visible"] == 1).all()
    assert np.array_equal(pre["px0"] // SC.TILE, pre["px1"] // SC.TILE) and np.array_equal(pre["py0"] // SC.TILE, pre["py1"] // SC.TILE)
    assert (pre["px0"] >= 0).all() and (pre["px1"] < s.w).all() and (pre["py0"] >= 0).all() and (pre["py1"] < s.h).all()
    assert (pre["px1"] - pre["px0"] <= 4).all() and (pre["py1"] - pre["py0"] <= 4).all()       # a few pixels whatever the depth
    assert np.array_equal(SC.bits_of(pre["depth"]), SC.bits_of(s.g.positions[:, 2]))           # depth is z, bit for bit
    assert (s.g.positions[:, 2] > 0).all()
    # the tile the builder says each case is in, and no other
    tile = (pre["py0"] // SC.TILE).astype(np.int64) * s.tiles_x + pre["px0"] // SC.TILE
    counts = np.bincount(tile, minlength=s.n_tiles)
    want = np.zeros(s.n_tiles, np.int64)
    for k, (length, _) in enumerate(s.cases):
        want[s.tile_of_case[k]] = length
        assert (tile[s.members[k]] == s.tile_of_case[k]).all(), (k, s.cases[k])
    assert np.array_equal(counts, want)
    # the original indices are spread over the tiles: a list's members are not a range
    for k, (length, _) in enumerate(s.cases):
        if length >= 64:
            assert np.diff(np.sort(s.members[k])).max() > 1, s.cases[k]


@pytest.mark.parametrize("name", SCENES)
def test_patterns_have_the_span_and_the_tie_runs_they_promise(name):
    s = SC.scene(name)
    depth = preprocessed(name)["depth"]
    for k, (length, pattern) in enumerate(s.cases):
        z = depth[s.members[k]]
        assert len(z) == length
        want = SC.intended(pattern, length)
        if want["span_bits"] is not None:
            assert SC.span_bits(z) == want["span_bits"], (s.cases[k], SC.span_bits(z))
        if want["runs"] is not None:
            assert SC.tie_runs(z) == want["runs"], (s.cases[k], SC.tie_runs(z))
        if pattern == "uniform" and length:
            b = SC.bits_of(z)
            assert b.min() >= SC.OCTAVE and b.max() < SC.OCTAVE + (1 << 23)                      # one octave: [0.25, 0.5)
        if pattern == "consecutive":
            assert np.array_equal(np.sort(SC.bits_of(z)), SC.BAND_BASE + np.arange(length, dtype=np.uint32))
        if pattern == "log":
            assert z.min() == SC.LOG_LO and z.max() == SC.LOG_HI
        if pattern == "band":
            b = SC.bits_of(z).astype(np.int64)
            inside = (b >= SC.BAND_BASE) & (b < SC.BAND_BASE + SC.BAND_WIDTH)
            far = max(1, int(round(0.002 * length)))
            assert length - far <= inside.sum() <= length and inside.sum() >= 0.99 * length, s.cases[k]
            assert z[~inside].min() >= np.float32(1e-20) and z.max() <= 1.0
            if length >= 5000:                             # the keys outside stretch the span far beyond the band
                assert SC.span_bits(z) >= 24 and (~inside).sum() >= 8, s.cases[k]
        if pattern in ("asc", "desc") and length > 1:
            d = np.diff(z[np.argsort(s.members[k])].astype(np.float64))
            assert (d >= 0).all() if pattern == "asc" else (d <= 0).all(), s.cases[k]
    if name == "distinct":
        assert all(SC.tie_runs(depth[m]) == {1: len(m)} for m in s.members)


def test_span_patterns_sit_on_both_sides_of_the_digit_widths():
    """plan_digits: V = significant bits of the span, P = ceil(V / wmax) passes of ceil(V / P) bits, wmax = 9 up to 1408 keys and 8
    above: spans of 255 / 256 / 257 are one 8-bit pass or two passes (one 9-bit pass where 512 bins fit), 511 / 512 / 513 one or
    two 9-bit passes"""
    got = {p: SC.intended(p, 2048)["span_bits"] for p in SC.PATTERNS if p.startswith("span")}
    assert got == {"span255": 8, "span256": 9, "span257": 9, "span511": 9, "span512": 10, "span513": 10}
    for n in (100, 1500, 2048, 70000):
        assert SC.intended("consecutive", n)["span_bits"] == (n - 1).bit_length()
    assert 1500 > 1408 >= 100                               # PATTERN_LENGTHS has lists with 512 bins and lists with 256


@pytest.mark.parametrize("name", SCENES)
def test_expected_order_is_a_stable_depth_sort_of_each_tiles_members(name):
    s = SC.scene(name)
    eoff, eorder = s.expected()
    assert eoff[-1] == s.n == len(eorder)
    z = s.g.positions[:, 2]
    for k, (length, _) in enumerate(s.cases):
        t = s.tile_of_case[k]
        lst = eorder[eoff[t]:eoff[t + 1]].astype(np.int64)
        assert len(lst) == length
        assert np.array_equal(np.sort(lst), np.sort(s.members[k]))                   # a permutation of the members
        if length > 1:
            dz, di = np.diff(z[lst].astype(np.float64)), np.diff(lst)
            assert (dz >= 0).all() and (di[dz == 0] > 0).all(), s.cases[k]           # ascending depth, ties by ascending index
    assert SC.describe_mismatch(s, eoff, eorder.copy(), eoff, eorder) is None


def test_a_mismatch_names_the_list_the_position_and_the_kind():
    s = SC.scene("sweep_short")
    eoff, eorder = s.expected()
    t = s.tile_of_case[[n for n, _ in s.cases].index(1025)]
    a = int(eoff[t])
    swapped = eorder.copy()
    swapped[a + 10], swapped[a + 11] = eorder[a + 11], eorder[a + 10]
    msg = SC.describe_mismatch(s, eoff, swapped, eoff, eorder)
    assert "tile %d (1025 keys, pattern uniform)" % t in msg and "from position 10 " in msg and "misordered" in msg, msg
    assert "%d@%08x" % (int(eorder[a + 10]), int(s.depth_bits[eorder[a + 10]])) in msg, msg
    dup = eorder.copy()
    dup[a + 500] = eorder[a + 3]                            # one key twice, another lost: the pair count still matches
    msg = SC.describe_mismatch(s, eoff, dup, eoff, eorder)
    assert "from position 500 " in msg and "NOT the same keys: 1 lost (first [%d])" % int(eorder[a + 500]) in msg, msg
    assert "1 held more than once (first [%d])" % int(eorder[a + 3]) in msg, msg
    short = np.array(eoff).copy()
    short[t + 1:] -= 1
    msg = SC.describe_mismatch(s, short[:], eorder, eoff, eorder)
    assert "1025 keys" in msg and "1024 keys on the device" in msg, msg


def test_expected_tile_lists_is_the_one_the_target_shape_tests_use():
    """tests/test_gpu_target_shapes.py keeps its own expected_tile_lists (low-pass 0.01): the same lists, on a scene whose
    Gaussians cover several tiles each"""
    import splat_amd
    import test_gpu_target_shapes as T
    g = with_oracle_cov3d(splat_amd.synthetic_scene(3000, 11))
    cam = make_camera(96, 160)
    off, order = SC.expected_tile_lists(g, cam, 10, 6, 0.01)
    toff, torder = T.expected_tile_lists(g, cam, 10, 6)
    assert len(order) > len(g) and np.array_equal(off, toff) and np.array_equal(order, torder)
