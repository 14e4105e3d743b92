"""What the tests of the visibility query share (tests/test_visibility_cases_host.py, tests/test_gpu_visibility.py): the
reference, the scenes and the cached references.

The reference is never the library.  A pixel's hits and their order are tests/pick_cases.hits_of (the oracle's records, the
oracle's fragment with glibc's expf); the chain, the weights, the Q24 truncation and the accumulation are numpy float32 and
integers:  T_0 = 1, w_k = f32(T_{k-1} * alpha_k), T_k = f32(T_{k-1} * f32(1 - alpha_k)), seen when w_k >= weight_min, and per
Gaussian the count of pixels, the greatest w and the sum of int(w * 2**24).

The hits of a whole target take about 2 s on the CPU, so they are computed once per (scene, camera, conventions, mask) --
hit_lists, cached by the caller's key -- and every weight_min, rectangle and pixel mask is answered from them."""
import numpy as np

import pick_cases as K
import splat_amd
from helpers import with_oracle_cov3d
from oracle import oracle as O

f32 = np.float32
Q24 = f32(16777216.0)
WEIGHTS = (0.0, 1.0 / 255.0, 0.05)
CLOUD_SIZES = K.CLOUD_SIZES                      # 1, 255, 256, 257, 3000
CLOUD_TARGETS = K.CLOUD_TARGETS                  # (48, 64) and (24, 40): the second has partial tiles on both axes
STACKS = ((300, 0.05), (5000, 0.01))             # the second: lists beyond 2048 and 4096 keys
WIDE_STACKS = ((300, 0.05), (2100, 0.02))        # scale 0.6: rectangles x 21..42, y 13..34 -- across the tile edges x = 32, y = 16, 32
WIDE_RECT = (21, 13, 42, 34)
CUT_RECT = (20, 10, 37, 33)                      # a rectangle that cuts tiles on every side
_SCENES = {}
_HITS = {}


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def wide_stack(k, opacity):
    """pick_cases.stack with scale 0.6: every Gaussian covers parts of six tiles of the stack target"""
    if (k, opacity) not in _SCENES:
        j = np.arange(k)
        pos = np.zeros((k, 4), f32)
        pos[:, 2] = (-1.0 + 2.0 * (j // 2 * 2) / k).astype(f32)
        pos[:, 3] = 1.0
        rot = np.zeros((k, 4), f32)
        rot[:, 3] = 1.0
        g = splat_amd.GaussianList(pos, np.full((k, 3), 0.6, f32), np.full(k, opacity, f32), rot, np.zeros((k, 48), f32))
        _SCENES[(k, opacity)] = with_oracle_cov3d(g)
    return _SCENES[(k, opacity)]


def painted_mask(h, w, seed=11):
    """a pixel mask as a brush leaves it: two discs and a stroke, any nonzero byte counts"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx - w * 0.4) ** 2 + (yy - h * 0.45) ** 2 <= (h * 0.3) ** 2) | ((xx - w * 0.8) ** 2 + (yy - h * 0.7) ** 2 <= 16)
    m |= (np.abs(yy - xx * h / w) <= 1)
    out = np.where(m, np.random.default_rng(seed).integers(1, 256, (h, w)), 0).astype(np.uint8)
    assert out.any() and not out.all()
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------
def hit_lists(key, rec, conv, w, h, mask=None):
    """per pixel y * w + x of the whole target: (indices, alphas) of its hits, nearest first; cached under `key`"""
    if key not in _HITS:
        lists = []
        for y in range(h):
            for x in range(w):
                idx, _, a = K.hits_of(rec, conv, x, y, 0.0, mask)
                lists.append((idx, np.ascontiguousarray(a, f32)))
        _HITS[key] = lists
    return _HITS[key]


def region_pixels(w, h, rect=None, pixel_mask=None):
    x0, y0, x1, y1 = (0, 0, w - 1, h - 1) if rect is None else rect
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    return [(x, y) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1) if pixel_mask is None or pixel_mask[y, x] != 0]


def reference(lists, n, w, h, weight_min, rect=None, pixel_mask=None, early_out=False, into=None):
    """(pixels u32 [n], max_weight f32 [n], weight_sum u64 [n], hits walked, hits in all) over the region.
    early_out: the pixel's walk, hit by hit, stopping as soon as T < weight_min (weight_min > 0); else the whole list at once
    (np.cumprod of float32 multiplies left to right, one rounded product each: the same chain).  into: arrays to add to."""
    wm = f32(weight_min)
    pixels, maxw, wsum = into if into is not None else (np.zeros(n, np.uint32), np.zeros(n, f32), np.zeros(n, np.uint64))
    walked = total = 0
    for x, y in region_pixels(w, h, rect, pixel_mask):
        idx, a = lists[y * w + x]
        total += len(idx)
        if len(idx) == 0:
            continue
        if early_out:
            t = f32(1.0)
            for k in range(len(idx)):
                if wm > 0 and t < wm:
                    break
                walked += 1
                wk = f32(t * a[k])
                t = f32(t * f32(f32(1.0) - a[k]))
                if wk >= wm:
                    i = idx[k]
                    pixels[i] += 1
                    maxw[i] = max(maxw[i], wk)
                    wsum[i] += np.uint64(int(f32(wk * Q24)))
            continue
        t = np.cumprod(f32(1.0) - a, dtype=f32)
        before = np.concatenate([np.ones(1, f32), t[:-1]])
        wk = (before * a).astype(f32)
        seen = wk >= wm
        walked += int((before >= wm).sum()) if wm > 0 else len(idx)
        i = idx[seen]                                 # (distinct within a pixel)
        pixels[i] += 1
        maxw[i] = np.maximum(maxw[i], wk[seen])
        wsum[i] += (wk[seen] * Q24).astype(np.uint64)
    return pixels, maxw, wsum, walked, total


def cloud_case(n, h, w, ci=0):
    """(g, camera, hit lists) of pick_cases.cloud(n) under camera ci of scene_gpu.cameras(h, w), default conventions"""
    import scene_gpu
    g = K.cloud(n)
    cam = scene_gpu.cameras(h, w)[ci]
    return g, cam, hit_lists(("cloud", n, h, w, ci), K.records(g, cam), O.default_conventions(), w, h)


def stack_case(k, opacity, wide=False):
    g = wide_stack(k, opacity) if wide else K.stack(k, opacity)
    cam = K.stack_camera()
    h, w = K.STACK_TARGET
    return g, cam, hit_lists(("wide" if wide else "stack", k, opacity), K.records(g, cam), O.default_conventions(), w, h)
