"""What the tests of the pick share (tests/test_pick_cases_host.py, tests/test_gpu_pick.py): the reference, the scenes and the
pixel sets.

The reference is never the library.  reference_pick is made of the oracle's records (O.preprocess: Pipeline::vertex restated on
the CPU), the oracle's fragment (O.fragment_n: fragment() with glibc's expf, one call per pixel) and numpy float32 for the order
and the coverage chain -- and of nothing else.

synthetic_scene alone is too thin for the chain: at most 12 hits at any pixel of a 64x48 target for 3000 Gaussians.  The
stacked pixels come from a constructed stack: k isotropic Gaussians of scale 0.2 at (0, 0, z), z = -1 + 2 (j // 2 * 2) / k, so that
pairs share a depth, identity rotation, one opacity, seen by make_camera(48, 64): every one of them hits the two centre
pixels."""
import numpy as np

import splat_amd
from oracle import oracle as O
from helpers import make_camera, oracle_camera, scene_dict, with_oracle_cov3d

f32 = np.float32
NONE = 0xFFFFFFFF
TRUNCATED = 1
MAX_PIXELS, MAX_HITS = 256, 4096
SENTINEL = 0xA5                                  # every byte of a layer row nothing may write
RESULT = np.dtype([("n_hits", "u4"), ("flags", "u4"), ("front_index", "u4"), ("front_depth", "f4"), ("front_alpha", "f4"),
                   ("surface_index", "u4"), ("surface_depth", "f4"), ("surface_coverage", "f4")])
LAYER = np.dtype([("index", "u4"), ("depth", "f4"), ("alpha", "f4"), ("coverage", "f4")])
assert RESULT.itemsize == 32 and LAYER.itemsize == 16


# ---- the reference ------------------------------------------------------------------------------------------------------
def hits_of(rec, conv, x, y, alpha_min=0.0, mask=None):
    """(indices, depths, alphas) of the hits of pixel (x, y), nearest first: descending depth, descending index among equals"""
    off = f32(0.5) if conv.sample_half else f32(0.0)
    inside = (rec["visible"] == 1) & (rec["px0"] <= x) & (x <= rec["px1"]) & (rec["py0"] <= y) & (y <= rec["py1"])
    if mask is not None:
        inside &= np.asarray(mask) != 0
    cand = np.flatnonzero(inside)
    r = rec[cand]
    sxy = np.empty((len(cand), 2), f32)
    sxy[:, 0] = f32(x) + off
    sxy[:, 1] = f32(y) + off
    ra = np.ascontiguousarray(np.stack([r["cx"], r["cy"], r["hx"], r["hy"]], 1), f32)
    # fragment_n takes dy = cy - sy (y up); with y down dy changes sign, and with it the cross term alone: B -> -B gives the
    # same bits ((-B dx) dy = -((B dx) dy) = (B dx) (-dy), and dy dy does not see the sign)
    B = r["conic"][:, 1] if conv.y_up else -r["conic"][:, 1]
    rb = np.ascontiguousarray(np.stack([r["conic"][:, 0], B, r["conic"][:, 2], r["opacity"]], 1), f32)
    alpha, cov = O.fragment_n(sxy, ra, rb)
    assert cov.all()                             # the covered range IS the set of samples inside the rectangle
    hit = (alpha != 0) & (alpha >= f32(alpha_min))
    idx, a, d = cand[hit], alpha[hit], rec["depth"][cand[hit]]
    assert not np.isnan(d).any()
    order = np.lexsort((-idx.astype(np.int64), -d))      # primary: -depth ascending (float comparison: the zeros tie)
    return idx[order].astype(np.uint32), d[order], a[order]


def chain(alpha):
    """coverage_k after each hit: T_k = T_{k-1} * (1 - alpha_k), each operation rounded to float32"""
    out = np.empty(len(alpha), f32)
    t = f32(1.0)
    for k, a in enumerate(alpha):
        ia = f32(1.0) - f32(a)
        t = f32(t * ia)
        out[k] = f32(1.0) - t
    return out


def reference_pick(records, conv, pixels, alpha_min=0.0, coverage_min=0.5, mask=None, max_hits=1024, max_layers=0):
    """(results [P] of RESULT, layers [P, max_layers] of LAYER with every byte of a row that is not due left SENTINEL,
    hit lists: per pixel (indices, depths, alphas) nearest first)"""
    pixels = np.asarray(pixels, np.int64).reshape(-1, 2)
    res = np.zeros(len(pixels), RESULT)
    lay = np.frombuffer(bytes([SENTINEL]) * (16 * len(pixels) * max_layers), LAYER).reshape(len(pixels), max_layers).copy()
    lists = []
    for p, (x, y) in enumerate(pixels):
        idx, d, a = hits_of(records, conv, int(x), int(y), alpha_min, mask)
        lists.append((idx, d, a))
        r = res[p]
        r["n_hits"] = len(idx)
        r["front_index"], r["surface_index"] = NONE, NONE
        if len(idx) == 0:
            continue
        r["front_index"], r["front_depth"], r["front_alpha"] = idx[0], d[0], a[0]
        if len(idx) > max_hits:
            r["flags"] = TRUNCATED
            continue
        cov = chain(a)
        reach = np.flatnonzero(cov >= f32(coverage_min))
        if reach.size:
            k = reach[0]
            r["surface_index"], r["surface_depth"], r["surface_coverage"] = idx[k], d[k], cov[k]
        else:
            r["surface_coverage"] = cov[-1]
        m = min(len(idx), max_layers)
        lay[p, :m]["index"], lay[p, :m]["depth"], lay[p, :m]["alpha"], lay[p, :m]["coverage"] = idx[:m], d[:m], a[:m], cov[:m]
    return res, lay, lists


# ---- the scenes -----------------------------------------------------------------------------------------------------------
STACKS = ((5, 0.5), (300, 0.05), (5000, 0.01))
STACK_TARGET = (48, 64)                          # (h, w)
STACK_CENTRES = ((32, 24), (31, 23))             # every Gaussian of a stack hits both
STACK_EMPTY = ((0, 0), (63, 47), (40, 24))       # ... and none of them these
# from the table of the issue, checked by tests/test_pick_cases_host.py: (k, opacity) -> (front index, surface rank at 0.5, the front being rank 0)
STACK_FACTS = {(5, 0.5): (4, 1), (300, 0.05): (299, 16), (5000, 0.01): (4999, 82)}
_SCENES = {}


def stack(k, opacity):
    if ("stack", k, opacity) not in _SCENES:
        j = np.arange(k)
        pos = np.zeros((k, 4), f32)
        pos[:, 2] = (-1.0 + 2.0 * (j // 2 * 2) / k).astype(f32)
        pos[:, 3] = 1.0
        rot = np.zeros((k, 4), f32)
        rot[:, 3] = 1.0                          # (i, j, k, w): the identity
        g = splat_amd.GaussianList(pos, np.full((k, 3), 0.2, f32), np.full(k, opacity, f32), rot, np.zeros((k, 48), f32))
        _SCENES[("stack", k, opacity)] = with_oracle_cov3d(g)
    return _SCENES[("stack", k, opacity)]


def cloud(n, seed=1):
    if ("cloud", n, seed) not in _SCENES:
        _SCENES[("cloud", n, seed)] = with_oracle_cov3d(splat_amd.synthetic_scene(n, seed))
    return _SCENES[("cloud", n, seed)]


def copy_of(g):
    return splat_amd.GaussianList(g.positions.copy(), g.scales.copy(), g.opacities.copy(), g.rotations.copy(), g.sh.copy(), g.cov3d.copy())


def stack_camera():
    return make_camera(*STACK_TARGET)


def records(g, cam, conv=None):
    return O.preprocess(scene_dict(g), oracle_camera(cam, 0.01), conv or O.default_conventions())


# ---- the pixel sets -------------------------------------------------------------------------------------------------------
def pixel_set(count, w, h, seed=5):
    """the first `count` of 256 pixels of a w x h target: the four corners, the middle and its duplicate, then scattered ones
    -- every smaller set is a prefix of the largest, so one reference serves them all (a set of one: the middle)"""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (w // 2, h // 2)]
    rest = np.stack([rng.integers(0, w, MAX_PIXELS), rng.integers(0, h, MAX_PIXELS)], 1)
    base = np.concatenate([np.array(fixed, np.int64), rest])[:MAX_PIXELS].astype(np.int32)
    return np.ascontiguousarray(base[4:5] if count == 1 else base[:count])


def prefix(count):
    """where the `count` pixels of pixel_set lie in the set of 256"""
    return slice(4, 5) if count == 1 else slice(0, count)


CLOUD_SIZES = (1, 255, 256, 257, 3000)
CLOUD_TARGETS = ((48, 64), (24, 40))             # (h, w)
PIXEL_COUNTS = (1, 64, 65, 256)
ALPHA_CUTS = (0.05, 0.5)                         # on the 3000 cloud at 64x48, first camera: each leaves some hits and removes some
