"""The target geometries of tests/test_gpu_target_shapes.py against the tile-count switches of the binning launches (no GPU):
every threshold declared there is the one the kernel sources use, and every switch has a geometry on each side of it."""
import os
import re

from test_gpu_target_shapes import (GEOMETRIES, SWITCHES, THRESHOLD_GEOMETRIES, MOVING_GEOMETRIES, LIBM_EXACT, TILE, tiles_of,
                                    SCAN_WIDE_ABOVE, REDO_LAYOUT_NARROW_MAX, MOTION_FILTER_LDS, MOTION_FILTER_MAX, CLASSES_LDS,
                                    BINS_AT_UPLOAD, MAX_SIDE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "splat_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def body(text, signature):
    """the text of the function that starts at `signature`, up to the next function at column 0"""
    i = text.index(signature)
    j = re.compile(r"^\S.*\(", re.M).search(text, i + len(signature))
    return text[i:j.start() if j else len(text)]


TRIPWIRE = ("the source no longer reads as tests/test_gpu_target_shapes.py's threshold table expects.  This test matches source "
            "text: if a threshold moved, update the table and its geometries (a target on each side); if only the text was "
            "reformatted, update the pattern here -- not the kernel")


def has(text, pattern):
    assert pattern in text, "%s: %r" % (TRIPWIRE, pattern)


def test_thresholds_are_the_kernel_sources():
    k = source("splat_kernels.hip")
    scan = body(k, "void launch_scan(")
    has(scan, "m > %du ? 1024 : 256" % SCAN_WIDE_ABOVE)
    has(scan, "cls_bytes = (m + 15u) & ~15u, in_lds = cls_bytes <= %du" % CLASSES_LDS)
    has(scan, "mv_bytes = (4u * m + 15u) & ~15u")
    has(scan, "mv_bytes > %du" % MOTION_FILTER_LDS)
    layout = body(k, "void launch_layout(")
    has(layout, "redo_gate != nullptr && m <= %du" % REDO_LAYOUT_NARROW_MAX)
    has(layout, "layout_kernel<256>")
    has(layout, "layout_kernel<1024>")
    api = source("splat_api.hip")
    has(api, "ensure_bins(c, 240u * 135u)")
    assert 240 * 135 == BINS_AT_UPLOAD
    has(api, "cam->w > %d.0f || cam->h > %d.0f" % (MAX_SIDE, MAX_SIDE))
    assert MOTION_FILTER_MAX == 12288 and ((4 * MOTION_FILTER_MAX + 15) & ~15) <= MOTION_FILTER_LDS < ((4 * (MOTION_FILTER_MAX + 1) + 15) & ~15)


def test_every_switch_has_a_geometry_on_each_side():
    tiles = {name: tiles_of(w, h) for name, (w, h) in GEOMETRIES.items()}
    for what, side in SWITCHES:
        for group in (GEOMETRIES, THRESHOLD_GEOMETRIES):     # (the launch variants are forced on both sides as well)
            sides = {side(tiles[name]) for name in group}
            assert sides == {True, False}, (what, sorted(group))
        moving = {side(tiles[name]) for name in MOVING_GEOMETRIES}
        if "filter" in what:
            assert moving == {True, False}, what
    # next to the thresholds, not only on either side somewhere
    ms = set(tiles.values())
    assert {SCAN_WIDE_ABOVE, SCAN_WIDE_ABOVE + 160, MOTION_FILTER_MAX, MOTION_FILTER_MAX + 12, CLASSES_LDS, CLASSES_LDS + 48} <= ms
    assert any(m >= 4 * BINS_AT_UPLOAD for m in ms)                  # (8K: four times the tiles made at upload)
    for name in LIBM_EXACT + THRESHOLD_GEOMETRIES + MOVING_GEOMETRIES:
        assert name in GEOMETRIES


def test_lines_edges_and_the_abi_limits_are_covered():
    shapes = list(GEOMETRIES.values())
    assert (MAX_SIDE, 16) in shapes and (16, MAX_SIDE) in shapes and (1, 1) in shapes
    cols = [(w, h) for w, h in shapes if w <= TILE and h > TILE]
    rows = [(w, h) for w, h in shapes if h <= TILE and w > TILE]
    assert any(w == TILE for w, _ in cols) and any(w < TILE for w, _ in cols)       # one tile column, whole and ragged
    assert any(h == TILE for _, h in rows) and any(h < TILE for _, h in rows)
    assert any(w % TILE and h % TILE and tiles_of(w, h) > BINS_AT_UPLOAD for w, h in shapes)   # a ragged target above 4K
