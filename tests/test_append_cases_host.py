"""The numpy restatement of append and reorder (tests/append_cases.py), held without a GPU: an append leaves the resident slots
alone and orders what it adds among itself -- non-finite centres first -- and append followed by reorder ends in the order a
fresh upload of the concatenation computes.  The library's own morton_order cannot be reached without a device (its only way
out is splat_get_scene_layout, which needs a context), so the agreement with it holds by construction: every order here is
remove_cases.morton_order, which tests/test_gpu_remove.py holds to splat_upload_scene's layout and tests/test_gpu_append.py
holds to the layouts after an append and a reorder."""
import numpy as np
import pytest

import splat_amd
import append_cases as AC
import remove_cases as RC
from test_remove_cases_host import SCENES, cloud, spoiled

f32 = np.float32
PAIRS = ((1, 1), (255, 1), (255, 2), (256, 1), (257, 255), (1000, 24), (1000, 1000), (1000, 3000))


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("n,m", PAIRS)
def test_the_appended_order_is_a_permutation_that_leaves_the_resident_slots_alone(n, m, name):
    pos, extra = SCENES[name](n, 300 + n), SCENES[name](m, 400 + m)
    orig = RC.morton_order(pos)
    got = AC.appended_order(orig, extra)
    assert got.dtype == np.uint32 and len(got) == n + m
    assert np.array_equal(np.sort(got), np.arange(n + m)), "a permutation"
    assert np.array_equal(got[:n], orig), "the first n slots are untouched"
    tail = got[n:].astype(np.int64) - n
    assert np.array_equal(tail, RC.morton_order(extra)), "the tail is the new rows' own order, offset by n"
    # ... which sorts the codes of the appended positions in THEIR box, ties in row order
    codes = RC.morton_codes(extra)[tail].astype(np.int64)
    assert (np.diff(codes) >= 0).all()
    assert (np.diff(tail)[np.diff(codes) == 0] > 0).all()
    # any order of the resident part is kept, a stale one included
    stale = np.random.default_rng(n).permutation(n).astype(np.uint32)
    assert np.array_equal(AC.appended_order(stale, extra)[:n], stale)


def test_non_finite_centres_come_first_in_the_tail():
    n, m = 300, 1000
    extra = cloud(m, 5)
    bad = np.random.default_rng(6).choice(m, 40, replace=False)
    extra[bad] = f32(np.nan)
    extra[bad[:10]] = f32(np.inf)
    got = AC.appended_order(RC.morton_order(cloud(n, 4)), extra)
    head = np.sort(got[n:n + 40].astype(np.int64) - n)
    assert np.array_equal(head, np.sort(bad)), "all coordinates non-finite: code 0, in front of every finite centre of the tail"
    assert np.array_equal(got[n:n + 40].astype(np.int64) - n, head), "... in row order among themselves"


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("n,m", PAIRS)
def test_append_then_reorder_is_the_fresh_uploads_order(n, m, name):
    pos, extra = SCENES[name](n, 500 + n), SCENES[name](m, 600 + m)
    both = np.concatenate([pos, extra])
    assert np.array_equal(AC.reordered_order(both), RC.morton_order(both))
    after_append = AC.appended_order(RC.morton_order(pos), extra)
    assert AC.moved(after_append, both) == int((after_append != RC.morton_order(both)).sum())
    assert AC.moved(RC.morton_order(both), both) == 0, "a scene in order has nothing to move"


def test_an_append_from_the_same_cloud_leaves_a_scene_that_a_reorder_moves():
    pos, extra = cloud(1000, 21), cloud(100, 22)
    assert AC.moved(AC.appended_order(RC.morton_order(pos), extra), np.concatenate([pos, extra])) > 0
    p = spoiled(1000, 23)
    assert AC.moved(RC.morton_order(p), p) == 0


def test_appended_concatenates_every_field_in_row_order():
    g, e = splat_amd.synthetic_scene(100, 3), splat_amd.synthetic_scene(37, 4)
    both = AC.appended(g, e)
    assert len(both) == 137
    for f in AC.FIELDS:
        a = getattr(both, f)
        assert a.dtype == f32 and a.flags["C_CONTIGUOUS"], f
        assert np.array_equal(a[:100], getattr(g, f)) and np.array_equal(a[100:], getattr(e, f)), f
    none = RC.rows_of(e, np.zeros(0, np.int64))
    same = AC.appended(g, none)
    assert len(same) == 100 and all(np.array_equal(getattr(same, f), getattr(g, f)) for f in AC.FIELDS)


def test_bounds_volume_skips_blocks_without_a_finite_box():
    b = np.zeros((3, 8), f32)
    b[0, :6] = (0, 0, 0, 1, 2, 3)
    b[1, :6] = np.nan
    b[2, :6] = (-1, -1, -1, 1, 1, 1)
    assert AC.bounds_volume(b) == 6.0 + 8.0
