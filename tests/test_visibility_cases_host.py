"""The cases of tests/test_gpu_visibility.py, run through the reference alone (tests/visibility_cases.py: the oracle and numpy,
no GPU): the facts that keep the GPU comparisons from being vacuous -- how many Gaussians each scene shows as seen at every
weight_min used, that a threshold hides some and leaves some, that the long stacks stop early, that one Gaussian of a wide
stack collects from several tiles -- and that the reference's early-out walk is its full walk."""
import numpy as np
import pytest

import pick_cases as K
import visibility_cases as V

SH, SW = K.STACK_TARGET


def seen(lists, n, w, h, weight_min, **kw):
    return V.reference(lists, n, w, h, weight_min, **kw)


def test_the_3000_cloud():
    g, cam, lists = V.cloud_case(3000, 48, 64)
    assert int((K.records(g, cam)["visible"] == 1).sum()) == 2241
    assert max(len(idx) for idx, _ in lists) == 12
    counts = [int((seen(lists, 3000, 64, 48, wm)[0] > 0).sum()) for wm in V.WEIGHTS]
    assert counts == [1768, 1678, 874]


def test_the_257_cloud_on_the_target_with_partial_tiles():
    g, cam, lists = V.cloud_case(257, 24, 40)
    counts = [int((seen(lists, 257, 40, 24, wm)[0] > 0).sum()) for wm in V.WEIGHTS[:2]]
    assert counts == [105, 103]


@pytest.mark.parametrize("k,opacity,at0,at255,walked,total", ((300, 0.05, 300, 77, None, None), (5000, 0.01, 5000, 91, 6032, 23376)))
def test_the_stacks(k, opacity, at0, at255, walked, total):
    g, cam, lists = V.stack_case(k, opacity)
    p0 = seen(lists, k, SW, SH, 0.0)
    p1 = seen(lists, k, SW, SH, 1.0 / 255.0)
    assert int((p0[0] > 0).sum()) == at0 and int((p1[0] > 0).sum()) == at255
    assert p0[3] == p0[4], "weight_min 0 walks every hit"
    if walked is not None:
        assert (p1[3], p1[4]) == (walked, total)
    if k == 300:
        assert int((seen(lists, k, SW, SH, 0.05)[0] > 0).sum()) == 0            # opacity 0.05 caps alpha, so w, below 0.05
    # the seen ones are the NEAREST ones: the stack's depth grows with the index
    assert np.array_equal(np.flatnonzero(p1[0] > 0), np.arange(k - at255, k))
    assert max(len(idx) for idx, _ in lists) == k


@pytest.mark.parametrize("k,opacity,at255,most,walked,total", ((300, 0.05, 79, 208, None, None), (2100, 0.02, 93, 124, 67184, 185496)))
def test_the_wide_stacks(k, opacity, at255, most, walked, total):
    g, cam, lists = V.stack_case(k, opacity, wide=True)
    rec = K.records(g, cam)
    assert (rec["px0"].min(), rec["py0"].min(), rec["px1"].max(), rec["py1"].max()) == V.WIDE_RECT
    # every Gaussian crosses x = 32 and collects from two workgroups at least; the nearer half -- all that are seen at 1/255
    # among them -- crosses y = 16 and y = 32 too: six workgroups
    assert (rec["px0"] < 32).all() and (rec["px1"] >= 32).all()
    six = (rec["py0"] < 16) & (rec["py1"] >= 32)
    assert 0 < int(six.sum()) < k and six[k - at255:].all()
    p0 = seen(lists, k, SW, SH, 0.0)
    p1 = seen(lists, k, SW, SH, 1.0 / 255.0)
    assert int((p0[0] > 0).sum()) == k and int((p1[0] > 0).sum()) == at255
    assert int(p0[0].max()) == most and int(p1[0].max()) == most
    if walked is not None:
        assert (p1[3], p1[4]) == (walked, total)
    if k == 2100:                                    # lists just above 2048 keys in several tiles
        per_tile = {}
        for y in range(SH):
            for x in range(SW):
                t = (y // 16, x // 16)
                per_tile.setdefault(t, set()).update(lists[y * SW + x][0].tolist())
        assert sum(1 for s in per_tile.values() if len(s) > 2048) >= 2


@pytest.mark.parametrize("case", ("cloud", "stack", "wide"))
def test_the_early_out_walk_is_the_full_walk(case):
    if case == "cloud":
        (g, cam, lists), (h, w) = V.cloud_case(3000, 48, 64), (48, 64)
    else:
        (g, cam, lists), (h, w) = V.stack_case(300, 0.05, wide=case == "wide"), (SH, SW)
    for wm in V.WEIGHTS:
        full = seen(lists, len(g), w, h, wm)
        early = seen(lists, len(g), w, h, wm, early_out=True)
        for a, b in zip(full[:3], early[:3]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert full[3:] == early[3:]
        if wm > 0 and case != "cloud":
            assert early[3] < early[4], "the walk stops early"


def test_the_sums_and_the_maxima_are_consistent():
    g, cam, lists = V.cloud_case(3000, 48, 64)
    p, m, s, _, _ = seen(lists, 3000, 64, 48, 1.0 / 255.0)
    assert p.dtype == np.uint32 and m.dtype == np.float32 and s.dtype == np.uint64
    on = p > 0
    assert ((m > 0) == on).all() and ((s > 0) == on).all()
    assert (m[on] >= np.float32(1.0 / 255.0)).all() and (m <= np.float32(0.99)).all()
    assert (s <= p.astype(np.uint64) * np.uint64(1 << 24)).all()
    # a rectangle and a mask take pixels away, never add any
    pr = seen(lists, 3000, 64, 48, 1.0 / 255.0, rect=V.CUT_RECT)[0]
    pm = seen(lists, 3000, 64, 48, 1.0 / 255.0, pixel_mask=V.painted_mask(48, 64))[0]
    assert (pr <= p).all() and (pm <= p).all() and 0 < pr.sum() < p.sum() and 0 < pm.sum() < p.sum()
