"""What splat_remove_gaussians_device does, restated in numpy for the tests that hold it to this (tests/test_gpu_remove.py,
tests/test_remove_cases_host.py): which Gaussians survive a selection and what they are renumbered to, what becomes of the
scene's order, and the order a fresh upload would give -- morton_order of splat_amd/csrc/splat_scene.hip in float32."""
import numpy as np

import splat_amd

f32 = np.float32
GONE = 0xFFFFFFFF
FIELDS = ("positions", "scales", "opacities", "rotations", "sh", "cov3d")


def rows_of(g, rows):
    """the Gaussians `rows` of g, in that order, as a list of their own"""
    return splat_amd.GaussianList(*[np.ascontiguousarray(getattr(g, f)[rows]) for f in FIELDS])


def survives(sel, keep):
    """per Gaussian: does it stay?  sel: nonzero = selected; keep: the selected stay (a crop), else they go (a delete)"""
    sel = np.asarray(sel) != 0
    return sel if keep else ~sel


def index_map_of(sel, keep):
    """per old Gaussian its new index -- the rank among the survivors in original index order -- or GONE"""
    stay = survives(sel, keep)
    m = np.full(len(stay), GONE, np.uint32)
    m[stay] = np.arange(int(stay.sum()), dtype=np.uint32)
    return m


def removed(g, sel, keep=False):
    """(survivors, index_map): the Gaussians that stay, in original index order, and index_map_of"""
    stay = survives(sel, keep)
    return rows_of(g, np.flatnonzero(stay)), index_map_of(sel, keep)


def compacted_order(orig, index_map):
    """the scene's order (orig[slot] = original index) without the slots whose Gaussian went, in the new numbering"""
    m = np.asarray(index_map, np.uint32)[np.asarray(orig, np.int64)]
    return m[m != GONE]


# ---- morton_order, restated --------------------------------------------------------------------------------------------------
def spread3(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def finite_box(pos):
    """(lo[3], hi[3]) over the finite values of every axis ON ITS OWN, as morton_order takes them; +inf / -inf without one"""
    lo, hi = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
    for a in range(3):
        v = np.asarray(pos, f32)[:, a]
        v = v[np.isfinite(v)]
        if len(v):
            lo[a], hi[a] = v.min(), v.max()
    return lo, hi


def morton_codes(pos):
    pos = np.asarray(pos, f32)
    lo, hi = finite_box(pos)
    code = np.zeros(len(pos), np.uint32)
    with np.errstate(all="ignore"):
        for a in range(3):
            sc = f32(1023.0) / f32(hi[a] - lo[a]) if hi[a] > lo[a] else f32(0.0)
            v = pos[:, a]
            t = ((v - lo[a]).astype(f32) * sc).astype(f32)
            t = np.where(f32(0.0) < t, t, f32(0.0))           # std::max(0.0f, t): 0 for a NaN
            t = np.where(t < f32(1023.0), t, f32(1023.0))     # std::min(1023.0f, t)
            q = np.where(np.isfinite(v), t, f32(0.0)).astype(np.uint32)
            code |= spread3(q) << np.uint32(a)
    return code


def morton_order(pos):
    """order[slot] = original index: by code, ties in index order"""
    return np.argsort(morton_codes(pos), kind="stable").astype(np.uint32)


def extremes(pos):
    """the (up to six) Gaussians that hold the finite per-axis extremes: while they stay, the finite box stays"""
    pos = np.asarray(pos, f32)
    out = set()
    for a in range(3):
        v = pos[:, a]
        ok = np.flatnonzero(np.isfinite(v))
        if len(ok):
            out.add(int(ok[np.argmin(v[ok])]))
            out.add(int(ok[np.argmax(v[ok])]))
    return np.array(sorted(out), np.int64)
