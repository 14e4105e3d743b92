"""Plumbing the GPU tests of the scene read-back and transform share (tests/test_gpu_scene_read.py,
tests/test_gpu_scene_transform.py): a Renderer with the device buffers made on it, the scenes, cameras and targets
tests/test_gpu_scene_update.py argues for, frames and stage data compared byte for byte."""
import contextlib
import ctypes as C
import math

import numpy as np

import splat_amd
from splat_amd import _lib
from helpers import make_camera, with_oracle_cov3d

f32 = np.float32
SIZES = (1, 255, 256, 257, 1000)                     # one block, a full block, a block plus one, three blocks and a partial one
TARGETS = ((96, 128), (160, 256))                    # (h, w)
FIELDS = ("positions", "cov3d", "opacities", "sh")
PER = {"positions": 4, "cov3d": 9, "opacities": 1, "sh": 48}
SENTINEL = 0xA5                                      # every byte of a buffer nothing may write: the float -2.3e-16


class Session:
    """a Renderer and the device buffers made on it, released together (the buffers first)"""

    def __init__(self, **conventions):
        self.R = splat_amd.Renderer(**conventions)
        self._held = []

    def device(self, g):
        d = g.to_device(self.R)
        self._held.append(d.free)
        return d

    def alloc(self, nbytes, fill=None):
        """nbytes of device memory, every byte `fill` when given; returns the address"""
        R = self.R
        p = R._L.splat_device_alloc(R._h, max(int(nbytes), 4))
        assert p
        self._held.append(lambda: R.device_free(p))
        if fill is not None and nbytes:
            a = np.full(int(nbytes), fill, np.uint8)
            R._check(R._L.splat_device_upload(R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def array(self, a):
        """device copy of a numpy array; returns its address"""
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.R._check(self.R._L.splat_device_upload(self.R._h, C.c_void_p(p), C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def fetch(self, p, shape, dtype=f32):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            self.R._check(self.R._L.splat_device_download(self.R._h, C.c_void_p(out.ctypes.data), C.c_void_p(p), out.nbytes))
        return out

    def read_all(self, n=None):
        """the four resident fields through read_device into sentinel-filled buffers: {field: array}"""
        n = self.R.n if n is None else n
        bufs = {f: self.alloc(4 * PER[f] * n, SENTINEL) for f in FIELDS}
        self.R.read_device(n=n, **bufs)
        return {f: self.fetch(bufs[f], (n,) if PER[f] == 1 else (n, PER[f])) for f in FIELDS}

    def close(self):
        for free in reversed(self._held):
            free()
        self._held = []
        self.R.close()


@contextlib.contextmanager
def session(**conventions):
    s = Session(**conventions)
    try:
        yield s
    finally:
        s.close()


@contextlib.contextmanager
def fresh_upload(g, **conventions):
    """the reference: a fresh Renderer that takes g through splat_upload_scene"""
    R = splat_amd.Renderer(**conventions)
    try:
        R.upload(g)
        yield R
    finally:
        R.close()


def in_view(n, seed):
    return with_oracle_cov3d(splat_amd.synthetic_scene(n, seed))


def copy_of(g, positions=None, cov3d=None):
    return splat_amd.GaussianList(g.positions.copy() if positions is None else positions, g.scales.copy(), g.opacities.copy(),
                                  g.rotations.copy(), g.sh.copy(), g.cov3d.copy() if cov3d is None else cov3d)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_same_bits(got, want, what=""):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), "%s: %d of %d words differ, first at %r" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def assert_resident(s, g, what="", w=1.0):
    """what read_device gives back is g, bit for bit (w of the positions: 1)"""
    got = s.read_all(len(g))
    want_pos = g.positions.copy()
    want_pos[:, 3] = f32(w)
    assert_same_bits(got["positions"], want_pos, what + " positions")
    for f in ("cov3d", "opacities", "sh"):
        assert_same_bits(got[f], getattr(g, f), what + " " + f)
    return got


def cameras(h, w):
    """at rest in front of the scene, turned, INSIDE the scene, and close"""
    return [make_camera(h, w), make_camera(h, w, yaw=math.radians(10.0)), make_camera(h, w, (0.3, 0.2, 0.4), 1.0, -0.2),
            make_camera(h, w, (0.0, 0.0, 3.0), pitch=0.1)]


def frame(R, cam, h, w):
    img = np.full((h, w), 0xDEADBEEF, np.uint32)
    R.render_frame(cam.to_c(0.01, 15), img)
    return img


def frames(R):
    return [frame(R, cam, h, w) for (h, w) in TARGETS for cam in cameras(h, w)]


def assert_same_frames(got, want, what=""):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s frame %d: %d pixels differ" % (what, k, int((a != b).sum()))


def stage(R, h=160, w=256):
    """(image, records, tile offsets, tile order, statistics) of one frame rendered with statistics"""
    img = np.zeros((h, w), np.uint32)
    st = R.render(make_camera(h, w).to_c(0.01, 15), img)
    n_tiles = ((h + _lib.TILE - 1) // _lib.TILE) * ((w + _lib.TILE - 1) // _lib.TILE)
    if st.n_pairs == 0:                               # (no list to fetch)
        return img, R.records(), np.zeros(n_tiles + 1, np.uint32), np.zeros(0, np.uint32), st
    off, order = R.tile_lists(n_tiles, st.n_pairs)
    return img, R.records(), off, order, st


def assert_same_stage(R, ref, what=""):
    """image, records, tile lists and the frame's counts of R are ref's"""
    (ia, ra, oa, la, sa), (ib, rb, ob, lb, sb) = stage(R), stage(ref)
    assert np.array_equal(ia, ib), what
    # depth and pixel rectangle exist for every Gaussian; the rest of a record is K1's, which writes none for a Gaussian
    # it culls: compared where the frame defined it
    assert ra["depth"].tobytes() == rb["depth"].tobytes(), what
    seen = ra["px0"] <= ra["px1"]
    assert np.array_equal(seen, rb["px0"] <= rb["px1"]), what
    assert ra[seen].tobytes() == rb[seen].tobytes(), what
    assert np.array_equal(oa, ob) and np.array_equal(la, lb), what
    assert (sa.n_visible, sa.n_singular, sa.n_pairs) == (sb.n_visible, sb.n_singular, sb.n_pairs), what
    return int(seen.sum()), la.size


def assert_bounds(got, want, what="", blocks=None):
    sel = slice(None) if blocks is None else blocks
    got, want = np.ascontiguousarray(got[sel]), np.ascontiguousarray(want[sel])
    assert got.shape == want.shape, what
    nan = np.isnan(got) & np.isnan(want)              # NaN matches NaN, whatever its payload
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), "%s: bounds differ in %d words, first block %d" % (what, int(bad.sum()), np.argwhere(bad)[0][0])


def index_sets(n, seed):
    """k = 0, 1, 300 scattered across the blocks (all n when there are fewer) and n: distinct, unsorted uint32 indices"""
    rng = np.random.default_rng(seed)
    out = [np.zeros(0, np.uint32), np.array([n // 2], np.uint32)]
    if n > 1:
        out.append(rng.permutation(n)[: min(300, n)].astype(np.uint32))
        out.append(rng.permutation(n).astype(np.uint32))
    return out
