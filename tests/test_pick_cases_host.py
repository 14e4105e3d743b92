"""The cases of tests/test_gpu_pick.py, run through the reference alone (tests/pick_cases.py: the oracle and numpy, no GPU):
what the GPU cases rely on is asserted here, so that none of them passes on an empty comparison -- the stacks have the hits,
ties, fronts and surface ranks they were built for, the largest exceeds the list's cap, every cloud has both hit and empty
pixels, and every alpha cut used leaves some hits and removes some."""
import numpy as np
import pytest

import pick_cases as K
import scene_gpu
from oracle import oracle as O

f32 = np.float32


@pytest.mark.parametrize("k,opacity", K.STACKS)
def test_a_stack_is_what_it_was_built_for(k, opacity):
    g = K.stack(k, opacity)
    rec = K.records(g, K.stack_camera())
    conv = O.default_conventions()
    front, rank = K.STACK_FACTS[(k, opacity)]
    res, _, lists = K.reference_pick(rec, conv, K.STACK_CENTRES + K.STACK_EMPTY, max_hits=K.MAX_HITS if k <= K.MAX_HITS else 8192)
    for p in range(len(K.STACK_CENTRES)):
        idx, d, a = lists[p]
        assert len(idx) == res[p]["n_hits"] == k
        assert int((d[1:] == d[:-1]).sum()) == k // 2                      # pairs share a depth ...
        tied = np.flatnonzero(d[1:] == d[:-1])
        assert (idx[tied] > idx[tied + 1]).all()                           # ... and the larger index comes first
        assert (d[1:] <= d[:-1]).all()
        assert res[p]["front_index"] == idx[0] == front
        assert res[p]["surface_index"] == idx[rank] and rank >= 1          # the rank counts from the front, which is rank 0:
        assert res[p]["surface_index"] != res[p]["front_index"]            # in every stack the surface lies BEHIND the front
        cov = K.chain(a)
        assert cov[rank] >= f32(0.5) and cov[rank - 1] < f32(0.5) and res[p]["surface_coverage"] == cov[rank]
    for p in range(len(K.STACK_CENTRES), len(K.STACK_CENTRES) + len(K.STACK_EMPTY)):
        assert res[p]["n_hits"] == 0 and res[p]["front_index"] == K.NONE and res[p]["surface_index"] == K.NONE


def test_the_largest_stack_exceeds_the_cap():
    k = K.STACKS[-1][0]
    assert k > K.MAX_HITS
    rec = K.records(K.stack(*K.STACKS[-1]), K.stack_camera())
    res, lay, _ = K.reference_pick(rec, O.default_conventions(), K.STACK_CENTRES + K.STACK_EMPTY[:1], max_hits=K.MAX_HITS, max_layers=2)
    for p in range(2):
        assert res[p]["flags"] == K.TRUNCATED and res[p]["n_hits"] == k and res[p]["front_index"] == k - 1
        assert res[p]["surface_index"] == K.NONE and res[p]["surface_depth"] == 0 and res[p]["surface_coverage"] == 0
    assert res[2]["flags"] == 0
    assert (lay.view(np.uint8) == K.SENTINEL).all()                        # no layer of a truncated pixel is due


def test_the_chain_never_reaches_one_and_a_tiny_threshold_is_met_at_once():
    rec = K.records(K.stack(300, 0.05), K.stack_camera())
    conv = O.default_conventions()
    res, _, lists = K.reference_pick(rec, conv, K.STACK_CENTRES, coverage_min=1.0, max_hits=300)
    assert (res["surface_index"] == K.NONE).all() and (res["surface_coverage"] > 0.99).all() and (res["surface_coverage"] < 1.0).all()
    res, _, _ = K.reference_pick(rec, conv, K.STACK_CENTRES, coverage_min=1e-6, max_hits=300)
    assert (res["surface_index"] == res["front_index"]).all()


@pytest.mark.parametrize("h,w", K.CLOUD_TARGETS)
def test_every_cloud_case_has_hit_and_empty_pixels(h, w):
    g = K.cloud(3000)
    pixels = K.pixel_set(256, w, h)
    assert len(pixels) == 256 and (pixels[4] == pixels[5]).all()
    assert {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)} <= {tuple(p) for p in pixels.tolist()}
    for cam in scene_gpu.cameras(h, w):
        rec = K.records(g, cam)
        res, _, _ = K.reference_pick(rec, O.default_conventions(), pixels)
        assert (res["n_hits"] > 0).any() and (res["n_hits"] == 0).any()
        assert (res["n_hits"] > 1).any()                                   # an order to get right


def test_every_alpha_cut_leaves_some_hits_and_removes_some():
    h, w = K.CLOUD_TARGETS[0]
    rec = K.records(K.cloud(3000), scene_gpu.cameras(h, w)[0])
    conv = O.default_conventions()
    pixels = K.pixel_set(256, w, h)
    full = K.reference_pick(rec, conv, pixels)[0]["n_hits"].sum()
    for cut in K.ALPHA_CUTS:
        left = K.reference_pick(rec, conv, pixels, alpha_min=cut)[0]["n_hits"].sum()
        assert 0 < left < full, (cut, left, full)
    rec = K.records(K.stack(5, 0.5), K.stack_camera())
    n = [K.reference_pick(rec, conv, K.STACK_CENTRES, alpha_min=a)[0]["n_hits"][0] for a in (0.0, 0.4, 0.6)]
    print(n)
    assert n[0] == 5 and n[2] == 0


def test_pixel_sets_have_their_sizes():
    for count in K.PIXEL_COUNTS:
        for h, w in K.CLOUD_TARGETS:
            p = K.pixel_set(count, w, h)
            assert p.shape == (count, 2) and (p >= 0).all() and (p[:, 0] < w).all() and (p[:, 1] < h).all()
