"""The scene handed over in device memory (splat_upload_scene_device, -m gpu): the order, the block bounds and the
packing computed on the GPU must be the host path's, bit for bit -- splat_upload_scene is the specification.  Every case
uploads the same data through the host path on one context and through the device path on another and compares what the
library keeps (splat_get_scene_layout) and what it renders.  At most two contexts are alive at any time."""
import contextlib
import math

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from helpers import make_camera
from bench import WORKLOADS, make_scene

pytestmark = pytest.mark.gpu
f32 = np.float32


@contextlib.contextmanager
def renderer():
    R = splat_amd.Renderer()
    try:
        yield R
    finally:
        R.close()


@contextlib.contextmanager
def uploaded_pair(g):
    """(A, B): g through splat_upload_scene on A, through splat_upload_scene_device on B"""
    with renderer() as A, renderer() as B:
        A.upload(g)
        d = g.to_device(B)
        try:
            d.upload()
        finally:
            d.free()
        yield A, B


def with_cov3d(g):
    with renderer() as R:
        g.compute_cov3d(R)
    return g


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_same_layout(A, B, what=""):
    oa, ba = A.scene_layout()
    ob, bb = B.scene_layout()
    assert oa.shape == ob.shape and ba.shape == bb.shape, what
    bad = np.flatnonzero(oa != ob)
    assert bad.size == 0, "%s: order differs in %d slots, first at %d (host %d, device %d)" % (what, bad.size, bad[0], oa[bad[0]], ob[bad[0]])
    nan = np.isnan(ba) & np.isnan(bb)                       # NaN matches NaN, whatever its payload
    bits = (ba.view(np.uint32) != bb.view(np.uint32)) & ~nan
    assert not bits.any(), "%s: bounds differ in %d words, first block %d: host %r device %r" % (
        what, int(bits.sum()), np.argwhere(bits)[0][0], ba[np.argwhere(bits)[0][0]], bb[np.argwhere(bits)[0][0]])
    return oa, ba


# ---- scenes ---------------------------------------------------------------------------------------------------------
def cloud():
    return splat_amd.synthetic_scene(120000, 71)


def surfaces():
    return splat_amd.synthetic_surface_scene(120000, 72)


def lattice():
    """50000 Gaussians on a 4 x 4 x 4 lattice: 64 codes, hundreds of Gaussians each -- the order among equal codes decides"""
    g = splat_amd.synthetic_scene(50000, 73)
    rng = np.random.default_rng(5)
    g.positions[:, :3] = rng.integers(0, 4, (50000, 3)).astype(f32) - f32(1.5)
    return g


def flat_axis():
    g = splat_amd.synthetic_scene(30000, 74)
    g.positions[:, 1] = f32(0.25)                           # hi == lo on this axis: its scale is 0
    return g


def non_finite():
    """NaN and +/-inf coordinates sprinkled in, signed zeros, and 300 Gaussians without any finite coordinate at the lowest
    indices: their code is 0, so they fill the first 256-slot block -- a block without a finite centre"""
    g = splat_amd.synthetic_scene(60000, 75)
    rng = np.random.default_rng(6)
    p = g.positions
    p[:, 0] = np.abs(p[:, 0])                               # (x >= 0: a block that holds a zero has it as its lower bound)
    p[:300, :3] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), (300, 3))
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        idx = rng.choice(np.arange(300, 60000), 400, replace=False)
        p[idx, rng.integers(0, 3, 400)] = f32(v)
    z = rng.choice(np.arange(300, 60000), 2000, replace=False)
    p[z[:1000], 0] = f32(0.0)
    p[z[1000:], 0] = f32(-0.0)                              # +0 and -0 compare equal and differ in a bound's bits
    return g


def nan_covariance(g):
    g.cov3d[777, 4] = np.nan
    g.cov3d[40000, 0] = np.inf
    return g


LAYOUT_SCENES = [("cloud", cloud, False), ("surfaces", surfaces, False),
                 ("n=1", lambda: splat_amd.synthetic_scene(1, 81), False), ("n=255", lambda: splat_amd.synthetic_scene(255, 82), False),
                 ("n=256", lambda: splat_amd.synthetic_scene(256, 83), False), ("n=257", lambda: splat_amd.synthetic_scene(257, 84), False),
                 ("n=65537", lambda: splat_amd.synthetic_scene(65537, 85), False),
                 ("lattice", lattice, False), ("flat axis", flat_axis, False), ("non-finite", non_finite, False),
                 ("NaN covariance", cloud, True)]


@pytest.mark.parametrize("name,make,spoil_cov", LAYOUT_SCENES, ids=[s[0] for s in LAYOUT_SCENES])
def test_layout_identity(name, make, spoil_cov):
    g = with_cov3d(make())
    if spoil_cov:
        nan_covariance(g)
    with uploaded_pair(g) as (A, B):
        orig, bounds = assert_same_layout(A, B, name)
        assert np.array_equal(np.sort(orig), np.arange(len(g), dtype=np.uint32)), "the order is not a permutation"
        # the cases are what they claim to be
        if name == "non-finite":
            assert np.isnan(bounds[0, :6]).all() and not np.isnan(bounds[1:, :6]).all(1).any()
            zero_lo = bounds[:, 0] == 0
            assert (zero_lo & np.signbit(bounds[:, 0])).any() and (zero_lo & ~np.signbit(bounds[:, 0])).any()
        if spoil_cov:
            assert np.isinf(bounds[:, 6]).sum() == 2
        if name == "lattice":
            assert len(np.unique(g.positions[:, :3], axis=0)) == 64


def frames_of(R, cams, sizes):
    out = []
    for (h, w) in sizes:
        for cam in cams(h, w):
            img = np.zeros((h, w), np.uint32)
            st = R.render_frame(cam.to_c(0.01, 15), img, want_stats=True)
            out.append((img, (st.n_visible, st.n_pairs, st.n_blocks_culled)))
    return out


def camera_walk(h, w):
    rest = make_camera(h, w)
    return [rest, rest, make_camera(h, w, yaw=math.radians(10.0)), make_camera(h, w, (0.3, 0.2, 0.4), 1.0, -0.2)]


@pytest.mark.parametrize("make", [cloud, surfaces, non_finite], ids=["cloud", "surfaces", "non-finite"])
def test_frame_identity(make):
    g = with_cov3d(make())
    with uploaded_pair(g) as (A, B):
        fa = frames_of(A, camera_walk, [(256, 256), (1080, 1920)])
        fb = frames_of(B, camera_walk, [(256, 256), (1080, 1920)])
        assert any(img.any() for img, _ in fa)
        for k, ((ia, sa), (ib, sb)) in enumerate(zip(fa, fb)):
            assert sa == sb, (k, sa, sb)
            assert np.array_equal(ia, ib), "frame %d: %d pixels differ" % (k, int((ia != ib).sum()))
        assert A.frames_dropped() == B.frames_dropped()


def test_reupload_loop():
    """five rounds of: move the Gaussians on the device, upload from there, render -- against the host path fed the same positions"""
    import torch
    g = with_cov3d(cloud())
    cam = make_camera(540, 960).to_c(0.01, 15)
    with renderer() as A, renderer() as B:
        dev = torch.device("cuda", 0)
        pos, cov, op, sh = (torch.from_numpy(a).to(dev) for a in (g.positions, g.cov3d, g.opacities, g.sh))
        gen = torch.Generator(device=dev).manual_seed(11)
        held = []
        for k in range(5):
            pos[:, :3] += 0.02 * torch.randn((len(g), 3), generator=gen, device=dev, dtype=torch.float32)
            B.upload_device(pos, cov, op, sh)              # (torch's current stream)
            ib = np.zeros((540, 960), np.uint32)
            B.render_frame(cam, ib)
            g.positions = np.ascontiguousarray(pos.cpu().numpy())
            A.upload(g)
            ia = np.zeros((540, 960), np.uint32)
            A.render_frame(cam, ia)
            assert ia.any() and np.array_equal(ia, ib), "round %d: %d pixels differ" % (k, int((ia != ib).sum()))
            assert_same_layout(A, B, "round %d" % k)
            held.append(B.device_bytes()[0])
        assert held[4] == held[0], held
        assert B.frames_dropped() == 0 and A.frames_dropped() == 0


def test_compute_cov3d_device_and_a_scene_built_on_the_device():
    rng = np.random.default_rng(21)
    n = 120000
    g = cloud()
    g.scales = np.exp(rng.normal(-4.0, 0.8, (n, 3))).astype(f32)
    g.rotations = (rng.standard_normal((n, 4)) * rng.uniform(0.2, 3.0, (n, 1))).astype(f32)       # un-normalised
    with renderer() as A, renderer() as B:
        ref = A.compute_cov3d(g.scales, g.rotations)
        d = g.to_device(B)
        try:
            d.compute_cov3d()
            got = np.zeros((n, 9), f32)
            B._check(B._L.splat_device_download(B._h, got.ctypes.data, d.cov3d, got.nbytes))
            assert same_bits(ref, got), "%d covariances differ" % int((ref.view(np.uint32) != got.view(np.uint32)).any(1).sum())
            d.upload()                                       # positions, opacities, sh as sent; cov3d as computed here
        finally:
            d.free()
        g.cov3d = ref
        A.upload(g)
        assert_same_layout(A, B, "device-built scene")
        cam = make_camera(540, 960).to_c(0.01, 15)
        ia, ib = np.zeros((540, 960), np.uint32), np.zeros((540, 960), np.uint32)
        A.render_frame(cam, ia)
        B.render_frame(cam, ib)
        assert ia.any() and np.array_equal(ia, ib)


def test_debug_getters_translate_slots_after_a_device_upload():
    g = with_cov3d(splat_amd.synthetic_scene(30000, 91))
    cam = make_camera(256, 320).to_c(0.01, 15)
    with uploaded_pair(g) as (A, B):
        got = []
        for R in (A, B):
            img = np.zeros((256, 320), np.uint32)
            st = R.render(cam, img)
            n_tiles = ((256 + _lib.TILE - 1) // _lib.TILE) * ((320 + _lib.TILE - 1) // _lib.TILE)
            off, order = R.tile_lists(n_tiles, st.n_pairs)
            got.append((img, R.records(), off, order))
        (ia, ra, oa, la), (ib, rb, ob, lb) = got
        assert np.array_equal(ia, ib) and la.size > 0
        # depth and pixel rectangle are recomputed for every Gaussian; the rest of a record is K1's, which writes none for a
        # Gaussian it culls (that memory is whatever the allocation held): compared where the frame defined it
        assert ra["depth"].tobytes() == rb["depth"].tobytes()
        seen = ra["px0"] <= ra["px1"]
        assert np.array_equal(seen, rb["px0"] <= rb["px1"]) and seen.sum() > 1000
        assert ra[seen].tobytes() == rb[seen].tobytes()
        assert np.array_equal(oa, ob) and np.array_equal(la, lb)


def test_stream_contract():
    """the buffers are still being written on a torch side stream when the call is made: the library waits, the caller does not"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    g = with_cov3d(cloud())
    n = len(g)
    with renderer() as A, renderer() as B:
        A.upload(g)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        host = [torch.from_numpy(a).pin_memory() for a in (g.positions, g.cov3d, g.opacities, g.sh)]
        bufs = [torch.full(h.shape, float("nan"), dtype=torch.float32, device=dev) for h in host]
        junk = torch.zeros(64 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):                              # work in front of the copies: they have not run when the call is made
                junk.add_(1.0)
            for b, h in zip(bufs, host):
                b.copy_(h, non_blocking=True)
        B.upload_device(*bufs, stream=side)
        assert B.n == n
        assert_same_layout(A, B, "side stream")
        cam = make_camera(256, 256).to_c(0.01, 15)
        ia, ib = np.zeros((256, 256), np.uint32), np.zeros((256, 256), np.uint32)
        A.render_frame(cam, ia)
        B.render_frame(cam, ib)
        assert ia.any() and np.array_equal(ia, ib)
        del bufs, junk


def test_device_upload_peaks_no_higher_than_the_host_upload():
    """fresh contexts, the same scene: 16 B per Gaussian of sort storage (two key and two index arrays of 4 B) plus the
    scan tables against 276 B per Gaussian of staging copies (4 + 9 + 1 + 48 floats + the order).  The caller's own
    buffers are not the library's: they live in a third party's allocations (here: another context's)."""
    g = with_cov3d(cloud())
    with renderer() as A:
        A.upload(g)
        host_peak = A.device_bytes()[1]
    with renderer() as owner, renderer() as B:
        d = g.to_device(owner)
        try:
            B.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=d.n)
        finally:
            d.free()
        now, peak = B.device_bytes()
        assert peak <= host_peak, (peak, host_peak)
        assert now <= peak


def test_errors():
    g = with_cov3d(splat_amd.synthetic_scene(1000, 95))
    cam = make_camera(64, 64).to_c(0.01, 15)
    img = np.zeros((64, 64), np.uint32)
    with renderer() as A, renderer() as B:
        d = g.to_device(B)
        try:
            before = B.device_bytes()
            with pytest.raises(splat_amd.SplatError) as e:
                B.upload_device(0, d.cov3d, d.opacities, d.sh, n=d.n)          # NULL device pointer, n > 0
            assert e.value.code == _lib.ERR_INVALID
            with pytest.raises(splat_amd.SplatError) as e:
                B.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=0xFFFFFFFF)
            assert e.value.code == _lib.ERR_INVALID
            assert B.device_bytes() == before                                      # ... before any allocation
            with pytest.raises(splat_amd.SplatError) as e:
                B.compute_cov3d_device(d.scales, 0, d.cov3d, n=d.n)
            assert e.value.code == _lib.ERR_INVALID
            # an empty scene: whatever a render answers after splat_upload_scene(n = 0) -- an error code, or a frame with
            # nothing in it -- it answers after splat_upload_scene_device(n = 0): the two paths agree
            d.upload()
            B.render_frame(cam, img)
            B.upload_device(0, 0, 0, 0, n=0)
            A.upload(g)
            A.render_frame(cam, img)
            A.upload(g.subset(np.arange(0)))
            answers = []
            for R in (A, B):
                out = np.full((64, 64), 0xDEADBEEF, np.uint32)
                try:
                    R.render_frame(cam, out)
                    code = _lib.SPLAT_OK
                except splat_amd.SplatError as err:
                    code = err.code
                answers.append((code, out))
            assert answers[0][0] == answers[1][0], (answers[0][0], answers[1][0])
            assert answers[0][0] in (_lib.SPLAT_OK, _lib.ERR_NO_SCENE), answers[0][0]
            assert np.array_equal(answers[0][1], answers[1][1])
            assert A.n == 0 and B.n == 0
            assert A.scene_layout()[0].size == 0 and B.scene_layout()[0].size == 0
        finally:
            d.free()
    with pytest.raises(TypeError):
        splat_amd.renderer._count_of(16, 4, None)                                 # plain addresses need n=


def test_c3_full_size():
    """C3 (1.5 M Gaussians, bench.WORKLOADS): the layout and one 1080p frame"""
    n, W, H, seed = WORKLOADS["C3"]
    g = make_scene("C3")
    assert len(g) == n
    with_cov3d(g)
    with uploaded_pair(g) as (A, B):
        assert_same_layout(A, B, "C3")
        cam = make_camera(H, W).to_c(0.01, 15)
        ia, ib = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
        sa = A.render_frame(cam, ia, want_stats=True)
        sb = B.render_frame(cam, ib, want_stats=True)
        assert (sa.n_visible, sa.n_pairs, sa.n_blocks_culled) == (sb.n_visible, sb.n_pairs, sb.n_blocks_culled)
        assert ia.any() and np.array_equal(ia, ib), "%d pixels differ" % int((ia != ib).sum())
