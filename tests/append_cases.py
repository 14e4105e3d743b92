"""What splat_append_gaussians_device and splat_reorder_scene_device do, restated in numpy for the tests that hold them to this
(tests/test_gpu_append.py, tests/test_gpu_append_sequences.py, tests/test_append_cases_host.py): the values after an append, what
becomes of the scene's order, and the order a reorder leaves -- all built on tests/remove_cases.py's rows_of and morton_order."""
import numpy as np

import splat_amd
import remove_cases as RC

FIELDS = RC.FIELDS


def appended(g, extra):
    """the Gaussians of g followed by those of extra: the new ones get the indices len(g) .. in row order"""
    both = splat_amd.GaussianList(*[np.concatenate([getattr(g, f), getattr(extra, f)]) for f in FIELDS])
    assert len(both) == len(g) + len(extra)
    return both


def appended_order(orig, extra_positions):
    """the scene's order (orig[slot] = original index) after an append: the resident slots as they were, behind them the new rows
    in the Morton order of their positions ALONE, numbered from len(orig)"""
    orig = np.asarray(orig, np.uint32)
    tail = RC.morton_order(extra_positions).astype(np.int64) + len(orig)
    return np.concatenate([orig, tail.astype(np.uint32)])


def reordered_order(positions):
    """the scene's order after a reorder: what a fresh upload of the resident positions computes"""
    return RC.morton_order(positions)


def moved(orig, positions):
    """how many slots a reorder finds holding another Gaussian than the new order gives them"""
    return int((np.asarray(orig, np.uint32) != reordered_order(positions)).sum())


def bounds_volume(bounds):
    """the sum of the blocks' AABB volumes in float64, over the blocks that have a finite box"""
    b = np.asarray(bounds, np.float64)
    ext = b[:, 3:6] - b[:, 0:3]
    ok = np.isfinite(ext).all(1)
    return float(ext[ok].prod(1).sum())
