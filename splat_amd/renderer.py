"""Thin object wrapper over the C ABI context (include/splat_hip.h)."""
import ctypes as C
import sys

import numpy as np

from . import _lib

f32 = np.float32


class SplatError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("splat error %d: %s" % (code, msg))
        self.code = code


def _fp(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _device_address(a, what, floats, device, any_dtype=False):
    """Device address of one scene buffer: an int is taken as it is; anything with data_ptr() (a torch tensor -- the
    package itself never imports torch) is checked as far as it describes itself: float32, contiguous, on the context's
    GPU, `floats` elements (None: not known yet)."""
    if isinstance(a, int):
        if a < 0:
            raise ValueError("%s: a device address is not negative" % what)
        return a
    if not hasattr(a, "data_ptr"):
        raise TypeError("%s: expected a device address (int) or an object with data_ptr(), got %s" % (what, type(a).__name__))
    dt = getattr(a, "dtype", None)
    if not any_dtype and dt is not None and str(dt).rsplit(".", 1)[-1] != "float32":
        raise TypeError("%s: float32 expected, got %s" % (what, dt))
    if hasattr(a, "is_contiguous") and not a.is_contiguous():
        raise ValueError("%s: not contiguous" % what)
    dev = getattr(a, "device", None)
    if dev is not None and hasattr(dev, "type"):
        if dev.type != "cuda":
            raise ValueError("%s: lives on %s, not on a GPU" % (what, dev))
        if dev.index is not None and dev.index != device:
            raise ValueError("%s: lives on GPU %d, the context on GPU %d" % (what, dev.index, device))
    if floats is not None and hasattr(a, "numel") and int(a.numel()) != floats:
        raise ValueError("%s: %d floats expected, got %d" % (what, floats, int(a.numel())))
    return int(a.data_ptr())


def _byte_mask_address(a, what, count, device):
    """Device address of a byte mask (a selection, a pixel mask): as _device_address, of any dtype one byte wide (uint8,
    bool) and `count` elements where it can tell."""
    p = _device_address(a, what, None, device, any_dtype=True)
    if not isinstance(a, int):
        if hasattr(a, "element_size") and int(a.element_size()) != 1:
            raise TypeError("%s: one byte per element expected, got %s" % (what, getattr(a, "dtype", None)))
        if hasattr(a, "numel") and int(a.numel()) != count:
            raise ValueError("%s: %d bytes expected, got %d" % (what, count, int(a.numel())))
    return p


def _count_of(a, per, n):
    """Gaussians in buffer `a` of `per` floats each: from its numel() unless the caller said n=."""
    if n is not None:
        return int(n)
    if isinstance(a, int) or not hasattr(a, "numel"):
        raise TypeError("n= is required with plain device addresses")
    m = int(a.numel())
    if m % per:
        raise ValueError("%d floats are not a whole number of Gaussians (%d floats each)" % (m, per))
    return m // per


def _producer_stream(stream, args):
    """The hipStream_t the caller's writes were enqueued on.  None: torch's current stream when the buffers are torch's
    (looked up only if the caller has imported torch -- this package does not), else 0 = the caller has synchronised."""
    if stream is not None:
        return int(getattr(stream, "cuda_stream", stream))
    torch = sys.modules.get("torch")
    if torch is not None:
        t = next((a for a in args if isinstance(a, torch.Tensor)), None)
        if t is not None:
            cur = torch.cuda.current_stream(t.device)
            if not int(cur.cuda_stream):
                # the legacy default stream has no handle to record an event on (NULL means "already synchronised" to
                # the library), and the context's streams do not wait for it by themselves
                cur.synchronize()
            return int(cur.cuda_stream)
    return 0


def _rotation3(rotation):
    r = np.asarray(rotation, dtype=f32)
    if r.size != 9:
        raise ValueError("rotation: 9 (3x3) numbers expected, got %d" % r.size)
    return np.ascontiguousarray(r.reshape(9), f32)


def sh_rotation_blocks(rotation):
    """splat_sh_rotation_blocks: (D1 [3,3], D2 [5,5], D3 [7,7]) float32, the blocks that bands 1-3 of a channel's sh
    coefficients (sh[3k + ch], k = 1..3 | 4..8 | 9..15) are multiplied by when the scene is turned by `rotation` (world ->
    world, anything that reshapes to 3x3, cast to float32): c'_m = sum_k D(m,k) c_k, so that eval_sh(c', R d) == eval_sh(c, d).
    Host only: needs neither a Renderer nor a GPU.  ValueError unless the matrix is orthogonal (every entry finite,
    max |R R^T - I| <= 1e-4; a reflection is fine)."""
    r = _rotation3(rotation)
    d = [np.zeros((n, n), f32) for n in (3, 5, 7)]
    L = _lib.lib()
    if L.splat_sh_rotation_blocks(_fp(r), *[_fp(a) for a in d]) != _lib.SPLAT_OK:
        raise ValueError("rotation: %s" % (L.splat_last_error(None) or b"").decode())
    return tuple(d)


LUMA = (0.2126, 0.7152, 0.0722)                      # Rec. 709 weights of linear r, g, b


def colour_matrix(saturation=1.0, tint=(1.0, 1.0, 1.0), contrast=1.0, brightness=0.0):
    """A 3x4 float32 colour map [A | t] (rgb' = A rgb + t) for Renderer.recolour, built in float64 in this order:
    1. saturation s: A = s I + (1 - s) 1 w^T with w = LUMA (0: every channel becomes the luma, 1: nothing changes);
    2. tint: A <- diag(tint) A;
    3. contrast c about 0.5: A <- c A, t <- c t + 0.5 (1 - c);
    4. brightness b: t <- t + b.
    The defaults give the identity exactly.  Host only: needs neither a Renderer nor a GPU."""
    s, c, b = float(saturation), float(contrast), float(brightness)
    tint = np.asarray(tint, np.float64).reshape(-1)
    if tint.size != 3:
        raise ValueError("tint: 3 numbers expected, got %d" % tint.size)
    A = s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), np.asarray(LUMA, np.float64))
    t = np.zeros(3)
    A = np.diag(tint) @ A
    A, t = c * A, c * t + 0.5 * (1.0 - c)
    t = t + b
    return np.concatenate([A, t[:, None]], 1).astype(f32)


class Renderer:
    """One context = one GPU = one stream.  `conventions` overrides splat_default_config fields
    (y_up, sample_half, zclip, zmin, zmax)."""

    def __init__(self, device=0, pair_capacity=0, **conventions):
        self._L = _lib.lib()
        cfg = _lib.Config()
        self._L.splat_default_config(C.byref(cfg))
        cfg.device = int(device)
        cfg.pair_capacity = int(pair_capacity)
        for k, v in conventions.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown convention %r" % k)
            setattr(cfg, k, v)
        self.config = cfg
        h = C.c_void_p()
        rc = self._L.splat_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise SplatError(rc, (self._L.splat_last_error(None) or b"").decode())
        self._h = h
        self.n = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.splat_destroy(self._h)
            self._h = None
            for p in getattr(self, "_pinned", []):
                self._L.splat_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SplatError(rc, (self._L.splat_last_error(self._h) or b"").decode())

    # ---- scene ------------------------------------------------------------------------
    def upload(self, gaussians):
        g = gaussians
        self._check(self._L.splat_upload_scene(self._h, len(g), _fp(g.positions), _fp(g.cov3d), _fp(g.opacities),
                                               _fp(g.sh)))
        self.n = len(g)

    def compute_cov3d(self, scales, rotations):
        scales = np.ascontiguousarray(scales, f32)
        rotations = np.ascontiguousarray(rotations, f32)
        n = scales.shape[0]
        out = np.zeros((n, 9), f32)
        self._check(self._L.splat_compute_cov3d(self._h, n, _fp(scales), _fp(rotations), _fp(out)))
        return out

    def upload_device(self, positions, cov3d, opacities, sh, stream=None, n=None):
        """splat_upload_scene_device: the scene from buffers that are already in this GPU's memory (layouts of upload():
        positions [n,4], cov3d [n,9], opacities [n], sh [n,48], float32).  Each one is a device address (int, with n=) or
        an object with data_ptr().  stream: the hipStream_t (or torch stream) the buffers were written on; the library
        waits for that work, not the caller.  Synchronous: the buffers are free again on return.  The frames that follow
        are those of upload() of the same data, byte for byte."""
        if hasattr(positions, "positions") and n is None:      # a DeviceGaussians (GaussianList.to_device)
            n = positions.n
        if hasattr(positions, "positions"):
            positions = positions.positions
        n = _count_of(positions, 4, n)
        dev = int(self.config.device)
        ptrs = [_device_address(a, what, per * n, dev) for a, what, per in
                ((positions, "positions", 4), (cov3d, "cov3d", 9), (opacities, "opacities", 1), (sh, "sh", 48))]
        st = _producer_stream(stream, (positions, cov3d, opacities, sh))
        self._check(self._L.splat_upload_scene_device(self._h, n, *[C.c_void_p(p) for p in ptrs], C.c_void_p(st)))
        self.n = n

    def _update_fields(self, rows, positions, cov3d, opacities, sh):
        """(mask, [four addresses]) of an in-place edit of `rows` rows: a field that is None is not named and its address 0"""
        dev = int(self.config.device)
        mask, ptrs = 0, []
        for a, what, per, bit in ((positions, "positions", 4, _lib.FIELD_POS), (cov3d, "cov3d", 9, _lib.FIELD_COV3D),
                                  (opacities, "opacities", 1, _lib.FIELD_OPACITY), (sh, "sh", 48, _lib.FIELD_SH)):
            if a is None:
                ptrs.append(0)
            else:
                mask |= bit
                ptrs.append(_device_address(a, what, per * rows, dev))
        return mask, ptrs

    def update_device(self, positions=None, cov3d=None, opacities=None, sh=None, stream=None, n=None):
        """splat_update_scene_device: the resident scene edited in place.  The fields that are not None are rewritten for all
        n Gaussians from device buffers (layouts, addresses and stream as in upload_device, indexed by original Gaussian); the
        others stay.  Nothing is freed, allocated or sorted: the scene keeps the order of its last upload, and the frames
        that follow are those of upload() of the edited arrays, byte for byte.  Synchronous; frames in flight end first and
        show the scene as it was."""
        n = self.n if n is None else int(n)
        mask, ptrs = self._update_fields(n, positions, cov3d, opacities, sh)
        st = _producer_stream(stream, (positions, cov3d, opacities, sh))
        self._check(self._L.splat_update_scene_device(self._h, n, mask, *[C.c_void_p(p) for p in ptrs], C.c_void_p(st)))

    def update_indexed(self, index, positions=None, cov3d=None, opacities=None, sh=None, stream=None, k=None):
        """splat_update_gaussians_device: the same for the k Gaussians index[0..k) (uint32 / int32 original indices in device
        memory, distinct; k= with a plain address).  The field buffers are compact: row t belongs to Gaussian index[t].  An
        index >= n raises SplatError(ERR_INVALID) with nothing applied."""
        k, pi = self._index_address(index, k)
        mask, ptrs = self._update_fields(k, positions, cov3d, opacities, sh)
        st = _producer_stream(stream, (index, positions, cov3d, opacities, sh))
        self._check(self._L.splat_update_gaussians_device(self._h, k, C.c_void_p(pi), mask, *[C.c_void_p(p) for p in ptrs],
                                                          C.c_void_p(st)))

    def read_device(self, positions=None, cov3d=None, opacities=None, sh=None, n=None):
        """splat_read_scene_device, the inverse of update_device: the resident values of the fields that are not None into the
        caller's writable device buffers (layouts and addresses as in upload_device), rows in original index order, bit for
        bit what the uploads and edits put there; positions get w = 1.  The others are not touched.  Synchronous; reads the
        scene only: the frames in flight come first and nothing kept from frame to frame is lost."""
        n = self.n if n is None else int(n)
        mask, ptrs = self._update_fields(n, positions, cov3d, opacities, sh)
        self._check(self._L.splat_read_scene_device(self._h, n, mask, *[C.c_void_p(p) for p in ptrs]))

    def _index_address(self, index, k):
        """(k, address) of k 32-bit indices in device memory: k from numel() unless given"""
        if k is None:
            if isinstance(index, int) or not hasattr(index, "numel"):
                raise TypeError("k= is required with a plain device address")
            k = int(index.numel())
        k = int(k)
        if not isinstance(index, int) and hasattr(index, "element_size") and int(index.element_size()) != 4:
            raise TypeError("index: 32-bit indices expected, got %s" % getattr(index, "dtype", None))
        return k, _device_address(index, "index", k, int(self.config.device), any_dtype=True)

    def read_indexed(self, index, positions=None, cov3d=None, opacities=None, sh=None, stream=None, k=None):
        """splat_read_gaussians_device, the inverse of update_indexed: compact rows, row t = Gaussian index[t] (uint32 / int32
        original indices in device memory, in any order, duplicates allowed; k= with a plain address).  stream: where the
        indices were written.  An index >= n raises SplatError(ERR_INVALID) with nothing written."""
        k, pi = self._index_address(index, k)
        mask, ptrs = self._update_fields(k, positions, cov3d, opacities, sh)
        st = _producer_stream(stream, (index,))
        self._check(self._L.splat_read_gaussians_device(self._h, k, C.c_void_p(pi), mask, *[C.c_void_p(p) for p in ptrs],
                                                        C.c_void_p(st)))

    def transform(self, matrix, index=None, stream=None, k=None, rotate_sh=False):
        """splat_transform_scene_device / splat_transform_gaussians_device: the affine map `matrix` (world -> world; anything
        that reshapes to 3x4 or to 4x4 with the last row 0 0 0 1, cast to float32) applied in place to the positions and
        3D covariances (A S A^T) of the whole scene, or of the Gaussians index[0..k) (as in update_indexed: distinct).
        Opacities and sh stay; sh is not rotated unless rotate_sh is true: then the linear part of `matrix` must be
        orthogonal (judged as rotate_sh judges it, BEFORE anything is applied: ValueError, nothing changed) and the transform
        is followed by rotate_sh of the same Gaussians with it.  An edit like update_device: synchronous, frames in flight end
        first, and the frames that follow are those of upload() of the mapped arrays, byte for byte."""
        m = np.asarray(matrix, dtype=f32)
        if m.size == 16:
            m = m.reshape(4, 4)
            if not np.array_equal(m[3], np.array([0, 0, 0, 1], f32)):
                raise ValueError("matrix: the last row of a 4x4 must be 0 0 0 1 (an affine map)")
            m = m[:3]
        elif m.size != 12:
            raise ValueError("matrix: 12 (3x4) or 16 (4x4) numbers expected, got %d" % m.size)
        m = np.ascontiguousarray(m.reshape(12), f32)
        r = np.ascontiguousarray(m.reshape(3, 4)[:, :3])
        if rotate_sh:
            sh_rotation_blocks(r)                                  # ValueError unless orthogonal
        if index is None:
            self._check(self._L.splat_transform_scene_device(self._h, _fp(m)))
        else:
            k, pi = self._index_address(index, k)
            st = _producer_stream(stream, (index,))
            self._check(self._L.splat_transform_gaussians_device(self._h, k, C.c_void_p(pi), _fp(m), C.c_void_p(st)))
        if rotate_sh:
            self.rotate_sh(r, index, stream, k)

    def rotate_sh(self, rotation, index=None, stream=None, k=None):
        """splat_rotate_sh_scene_device / splat_rotate_sh_gaussians_device: view-dependent colour turned by the orthogonal
        map `rotation` (world -> world; anything that reshapes to 3x3, cast to float32; a reflection is fine), in place, for
        the whole scene or for the Gaussians index[0..k) (as in transform).  Bands 1-3 of sh are multiplied by the blocks of
        sh_rotation_blocks(rotation); band 0 and every other field keep their bits, so eval_sh(sh', R d) == eval_sh(sh, d).
        A matrix that is not orthogonal (max |R R^T - I| > 1e-4, or a non-finite entry) raises SplatError(ERR_INVALID) with
        nothing applied.  An edit like update_device of sh alone."""
        r = _rotation3(rotation)
        if index is None:
            self._check(self._L.splat_rotate_sh_scene_device(self._h, _fp(r)))
            return
        k, pi = self._index_address(index, k)
        st = _producer_stream(stream, (index,))
        self._check(self._L.splat_rotate_sh_gaussians_device(self._h, k, C.c_void_p(pi), _fp(r), C.c_void_p(st)))

    # ---- selections ---------------------------------------------------------------------
    _SEL_OPS = {"set": _lib.SEL_OP_SET, "add": _lib.SEL_OP_ADD, "subtract": _lib.SEL_OP_SUBTRACT, "intersect": _lib.SEL_OP_INTERSECT}

    # ---- colour ---------------------------------------------------------------------------
    def _indices(self, index, k):
        """(k, address, address to free or 0) of 32-bit indices: device memory as _index_address takes it, or a host sequence
        of integers, which is copied into a buffer of the call's own"""
        if isinstance(index, int) or hasattr(index, "data_ptr"):
            return self._index_address(index, k) + (0,)
        host = np.ascontiguousarray(index)
        if host.size and host.dtype.kind not in "iu":
            raise TypeError("idx: integer indices expected, got %s" % host.dtype)
        if host.size and (host.min() < 0 or host.max() > 0xFFFFFFFF):
            raise ValueError("idx: indices are 32-bit and not negative")
        host = np.ascontiguousarray(host.reshape(-1), np.uint32)
        if not host.size:
            return 0, 0, 0
        p = self._L.splat_device_alloc(self._h, host.nbytes)
        if not p:
            raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"no device memory for the indices").decode())
        rc = self._L.splat_device_upload(self._h, C.c_void_p(p), C.c_void_p(host.ctypes.data), host.nbytes)
        if rc != 0:
            self.device_free(p)
            self._check(rc)
        return int(host.size), p, p

    def colours(self, cam_c, idx=None, out=None, stream=None, k=None):
        """splat_eval_colours_device: the colour each Gaussian is drawn with under cam_c -- eval_sh at the direction from
        cam_c.cam_pos, bands as cam_c.sh_dim names them, + 0.5, unclamped: the r, g, b of the records a frame of cam_c is made
        of, bit for bit, for every Gaussian, visible or not (a NaN stays a NaN).  idx=None: all n, original index order.
        Otherwise row t belongs to Gaussian idx[t]: 32-bit indices in device memory (a device address with k=, or an object
        with data_ptr()) or a host sequence of integers, in any order, duplicates allowed.  out=None: returns a numpy float32
        array [k, 3].  With out= (device memory of 3 k float32: an address or an object with data_ptr()) the call writes
        there, copies nothing down and returns out.  Reads the scene only, as select does.  An index >= n raises
        SplatError(ERR_INVALID) with nothing written."""
        if idx is None:
            k, pi, mine = self.n, 0, 0
        else:
            k, pi, mine = self._indices(idx, k)
        own = 0
        try:
            if k == 0 and idx is not None:                     # no rows: nothing is asked of the library
                return np.zeros((0, 3), f32) if out is None else out
            if out is None:
                own = po = self._L.splat_device_alloc(self._h, 12 * k)
                if not po:
                    raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"no device memory for the colours").decode())
            else:
                po = _device_address(out, "out", 3 * k, int(self.config.device))
            st = _producer_stream(stream, (idx, out))
            self._check(self._L.splat_eval_colours_device(self._h, C.byref(cam_c) if cam_c is not None else None, k,
                                                          C.c_void_p(pi) if idx is not None else None, C.c_void_p(po), C.c_void_p(st)))
            if out is not None:
                return out
            rgb = np.zeros((k, 3), f32)
            self._check(self._L.splat_device_download(self._h, C.c_void_p(rgb.ctypes.data), C.c_void_p(po), rgb.nbytes))
            return rgb
        finally:
            for p in (own, mine):
                if p:
                    self.device_free(p)

    def select_colour(self, cam_c, selection, rgb=None, tolerance=None, matrix=None, shape="ellipsoid", clamp=True, op="set",
                      stream=None):
        """splat_select_colour_device, the magic wand: which Gaussians are drawn, under cam_c, in a colour that a 3x4 map takes
        into the unit box (shape="box": |u_k| <= 1) or the unit ball (shape="ellipsoid": |u|^2 <= 1), into `selection` (as
        select takes it), combined by op.  rgb= and tolerance= (a scalar or a per-channel triple): the colours within
        `tolerance` of rgb -- colour_to_unit = [diag(1 / tolerance) | -rgb / tolerance], made in float64 and rounded to
        float32; matrix=: the map itself (3x4: a luminance band is one row of luma weights and two zero rows).  clamp: the
        colour is clamped to [0, 1] per channel first, as a frame's bytes show it.  A NaN colour never passes.  Returns how
        many Gaussians are selected after the op."""
        if shape not in ("box", "ellipsoid"):
            raise ValueError("shape: 'box' or 'ellipsoid', got %r" % (shape,))
        if op not in self._SEL_OPS:
            raise ValueError("op: one of %s, got %r" % (sorted(self._SEL_OPS), op))
        if matrix is not None:
            if rgb is not None or tolerance is not None:
                raise ValueError("matrix= or rgb= with tolerance=: one of the two")
            m = np.asarray(matrix, dtype=f32)
            if m.size != 12:
                raise ValueError("matrix: 12 (3x4) numbers expected, got %d" % m.size)
        else:
            if rgb is None or tolerance is None:
                raise ValueError("rgb= and tolerance= go together (or give matrix=)")
            c = np.asarray(rgb, np.float64).reshape(-1)
            if c.size != 3:
                raise ValueError("rgb: 3 numbers expected, got %d" % c.size)
            tol = np.asarray(tolerance, np.float64).reshape(-1)
            if tol.size not in (1, 3):
                raise ValueError("tolerance: a scalar or 3 numbers expected, got %d" % tol.size)
            tol = np.broadcast_to(tol, (3,))
            if not (tol > 0).all():
                raise ValueError("tolerance: positive numbers expected, got %r" % (tolerance,))
            m = np.concatenate([np.diag(1.0 / tol), (-c / tol)[:, None]], 1).astype(f32)
        q = _lib.ColourQuery()
        q.colour_to_unit[:] = [float(x) for x in np.ascontiguousarray(m, f32).ravel()]
        q.shape = 0 if shape == "box" else 1
        q.clamp = 1 if clamp else 0
        ps = _byte_mask_address(selection, "selection", self.n, int(self.config.device))
        st = _producer_stream(stream, (selection,))
        count = C.c_uint64()
        self._check(self._L.splat_select_colour_device(self._h, C.byref(q), C.byref(cam_c) if cam_c is not None else None,
                                                       self._SEL_OPS[op], C.c_void_p(ps), C.byref(count), C.c_void_p(st)))
        return int(count.value)

    def recolour(self, m, idx=None, stream=None, k=None):
        """splat_recolour_scene_device / splat_recolour_gaussians_device: the colour map rgb' = A rgb + t (m = [A | t]: anything
        that reshapes to 3x4, cast to float32; colour_matrix makes one) applied to what every Gaussian is drawn with, from
        every direction and at every sh_dim, by mapping its sh coefficients in place -- for the whole scene or for the
        Gaussians idx[0..k) (distinct; device memory as in update_indexed, or a host sequence of integers).  Every other field
        keeps its bits.  A non-finite entry raises SplatError(ERR_INVALID) with nothing applied.  An edit like update_device
        of sh alone."""
        a = np.asarray(m, dtype=f32)
        if a.size != 12:
            raise ValueError("m: 12 (3x4) numbers expected, got %d" % a.size)
        a = np.ascontiguousarray(a.reshape(12), f32)
        if idx is None:
            self._check(self._L.splat_recolour_scene_device(self._h, _fp(a)))
            return
        k, pi, mine = self._indices(idx, k)
        try:
            st = _producer_stream(stream, (idx,))
            self._check(self._L.splat_recolour_gaussians_device(self._h, k, C.c_void_p(pi), _fp(a), C.c_void_p(st)))
        finally:
            if mine:
                self.device_free(mine)

    def select(self, selection, cam_c=None, *, box=None, ellipsoid=None, rect=None, rule="centre", pixel_mask=None, depth=None,
               opacity=None, op="set", stream=None):
        """splat_select_device: which Gaussians of the resident scene pass every test named, into `selection` -- one byte per
        Gaussian in device memory, original index order, nonzero = selected (a device address or an object with data_ptr():
        a torch.uint8 / torch.bool tensor of n elements).  box / ellipsoid: a 3x4 row-major affine map from world space to
        the unit box / unit sphere; rect=(x0, y0, x1, y1): inclusive pixels of the target of cam_c, by rule "centre" (where
        the Gaussian's centre lands; pixel_mask: a w*h uint8 device image it must also hit) or "touch" (its covered pixels
        meet the rectangle); depth=(min, max): view-space z under cam_c; opacity=(min, max).  op: "set", "add",
        "subtract", "intersect" with what `selection` holds.  The screen test sees the very records a frame of cam_c is made
        of.  Returns how many Gaussians are selected after the op."""
        q = _lib.SelectQuery()
        if box is not None and ellipsoid is not None:
            raise ValueError("box and ellipsoid: one volume per query (combine two queries with op=)")
        vol = box if box is not None else ellipsoid
        if vol is not None:
            m = np.ascontiguousarray(vol, f32)
            if m.shape != (3, 4):
                raise ValueError("box / ellipsoid: a 3x4 array expected, got shape %r" % (m.shape,))
            q.tests |= _lib.SEL_VOLUME
            q.volume_shape = 0 if box is not None else 1
            q.world_to_unit[:] = [float(x) for x in m.ravel()]
        if rule not in ("centre", "touch"):
            raise ValueError("rule: 'centre' or 'touch', got %r" % (rule,))
        if pixel_mask is not None and rect is None:
            raise ValueError("pixel_mask: goes with rect= (the whole target: rect=(0, 0, w - 1, h - 1))")
        if rect is not None:
            if pixel_mask is not None and rule == "touch":
                raise ValueError("pixel_mask goes with rule='centre', not with 'touch'")
            q.tests |= _lib.SEL_SCREEN
            q.screen_rule = 0 if rule == "centre" else 1
            q.x0, q.y0, q.x1, q.y1 = [int(x) for x in rect]
        if depth is not None:
            q.tests |= _lib.SEL_DEPTH
            q.depth_min, q.depth_max = float(depth[0]), float(depth[1])
        if opacity is not None:
            q.tests |= _lib.SEL_OPACITY
            q.opacity_min, q.opacity_max = float(opacity[0]), float(opacity[1])
        if op not in self._SEL_OPS:
            raise ValueError("op: one of %s, got %r" % (sorted(self._SEL_OPS), op))
        if (q.tests & (_lib.SEL_SCREEN | _lib.SEL_DEPTH)) and cam_c is None:
            raise ValueError("rect= and depth= need cam_c")
        dev = int(self.config.device)
        ps = _byte_mask_address(selection, "selection", self.n, dev)
        pm = _byte_mask_address(pixel_mask, "pixel_mask", int(cam_c.w) * int(cam_c.h), dev) if pixel_mask is not None else 0
        st = _producer_stream(stream, (selection, pixel_mask))
        count = C.c_uint64()
        self._check(self._L.splat_select_device(self._h, C.byref(q), C.byref(cam_c) if cam_c is not None else None, C.c_void_p(pm),
                                                self._SEL_OPS[op], C.c_void_p(ps), C.byref(count), C.c_void_p(st)))
        return int(count.value)

    def selection_indices(self, selection, out, stream=None, n=None, capacity=None):
        """splat_selection_indices_device: the indices of the nonzero bytes of `selection` (n bytes: n= with a plain address,
        default the resident scene's n), ascending, as uint32 into `out` (device memory of `capacity` entries: capacity= with a
        plain address) -- what update_indexed takes as index.  Returns how many are selected; when that is more than
        capacity, the first `capacity` of them were written."""
        dev = int(self.config.device)
        if n is None:
            n = int(selection.numel()) if (not isinstance(selection, int) and hasattr(selection, "numel")) else self.n
        n = int(n)
        ps = _byte_mask_address(selection, "selection", n, dev)
        if capacity is None:
            if isinstance(out, int) or not hasattr(out, "numel"):
                raise TypeError("capacity= is required with a plain device address")
            capacity = int(out.numel())
        capacity = int(capacity)
        if not isinstance(out, int) and hasattr(out, "element_size") and int(out.element_size()) != 4:
            raise TypeError("out: 32-bit indices expected, got %s" % getattr(out, "dtype", None))
        po = _device_address(out, "out", None, dev, any_dtype=True)
        st = _producer_stream(stream, (selection, out))
        count = C.c_uint64()
        self._check(self._L.splat_selection_indices_device(self._h, n, C.c_void_p(ps), C.c_void_p(po), capacity, C.byref(count),
                                                           C.c_void_p(st)))
        return int(count.value)

    def remove(self, selection, keep=False, index_map=None, stream=None, n=None):
        """splat_remove_gaussians_device: the selected Gaussians taken out of the resident scene (keep=True: everything BUT
        them -- a crop), the survivors compacted on the GPU.  `selection` is select's: n bytes of device memory, original index
        order, nonzero = selected (a torch.uint8 / torch.bool tensor, or a device address; n= names another length than the
        resident scene's, which the library then refuses).  Survivors keep their relative original order and are renumbered
        by rank: from here on every index, row and selection byte means the new numbering, and self.n is the new count.
        index_map: a device buffer of n 32-bit elements that receives, per old Gaussian, its new index or 0xFFFFFFFF
        (_lib.REMOVED_INDEX) -- what carries the caller's own per-Gaussian arrays and other selections across the call; a
        DeviceGaussians (GaussianList.to_device) made before the call still holds the old rows and is stale.  Nothing is
        sorted, freed memory is given back, and the frames that follow are those of upload() of the survivors, byte for byte.
        A selection that removes nothing leaves everything kept from frame to frame in place; one that removes everything
        leaves no scene.  Synchronous; frames in flight end first and show the scene as it was.  Returns the new n."""
        dev = int(self.config.device)
        n = self.n if n is None else int(n)
        ps = _byte_mask_address(selection, "selection", n, dev)
        pm = 0
        if index_map is not None:
            if not isinstance(index_map, int) and hasattr(index_map, "element_size") and int(index_map.element_size()) != 4:
                raise TypeError("index_map: 32-bit indices expected, got %s" % getattr(index_map, "dtype", None))
            pm = _device_address(index_map, "index_map", None, dev, any_dtype=True)
            if not isinstance(index_map, int) and hasattr(index_map, "numel") and int(index_map.numel()) != n:
                raise ValueError("index_map: %d elements expected, got %d" % (n, int(index_map.numel())))
        st = _producer_stream(stream, (selection, index_map))
        n_after = C.c_uint64()
        self._check(self._L.splat_remove_gaussians_device(self._h, n, C.c_void_p(ps), _lib.REMOVE_UNSELECTED if keep else _lib.REMOVE_SELECTED,
                                                          C.c_void_p(pm), C.byref(n_after), C.c_void_p(st)))
        self.n = int(n_after.value)
        return self.n

    def append(self, positions, cov3d=None, opacities=None, sh=None, stream=None, m=None):
        """splat_append_gaussians_device: m Gaussians added to the resident scene from buffers in this GPU's memory (layouts,
        addresses and stream as in upload_device: positions [m,4], cov3d [m,9], opacities [m], sh [m,48], float32, or a
        DeviceGaussians; m= with plain addresses).  The new Gaussians get the original indices n .. n+m-1 in row order and
        every resident one keeps its index, so the caller's index lists stay good; its selections and other buffers of n
        elements do not grow with the scene.  The resident slots stay where they are and the new rows are ordered among
        themselves behind them (reorder() puts the whole scene in order); the frames that follow are those of upload() of
        the concatenated arrays, byte for byte.  With no resident scene (self.n == 0) this is upload_device.  m == 0 changes
        nothing.  Synchronous; frames in flight end first and show the scene as it was.  Returns the new n."""
        if hasattr(positions, "positions"):                    # a DeviceGaussians (GaussianList.to_device)
            d = positions
            if m is None:
                m = d.n
            cov3d = d.cov3d if cov3d is None else cov3d
            opacities = d.opacities if opacities is None else opacities
            sh = d.sh if sh is None else sh
            positions = d.positions
        for a, what in ((cov3d, "cov3d"), (opacities, "opacities"), (sh, "sh")):
            if a is None:
                raise TypeError("%s: an append names all four fields" % what)
        if m is None and (isinstance(positions, int) or not hasattr(positions, "numel")):
            raise TypeError("m= is required with plain device addresses")
        m = _count_of(positions, 4, m)
        if m < 0:
            raise ValueError("m: a count is not negative")
        dev = int(self.config.device)
        ptrs = [_device_address(a, what, per * m, dev) for a, what, per in
                ((positions, "positions", 4), (cov3d, "cov3d", 9), (opacities, "opacities", 1), (sh, "sh", 48))]
        st = _producer_stream(stream, (positions, cov3d, opacities, sh))
        if self.n == 0:
            self._check(self._L.splat_upload_scene_device(self._h, m, *[C.c_void_p(p) for p in ptrs], C.c_void_p(st)))
            self.n = m
            return self.n
        n_after = C.c_uint64()
        self._check(self._L.splat_append_gaussians_device(self._h, self.n, m, *[C.c_void_p(p) for p in ptrs], C.byref(n_after),
                                                          C.c_void_p(st)))
        self.n = int(n_after.value)
        return self.n

    def reorder(self):
        """splat_reorder_scene_device: the resident scene put into the order upload() of its current values would give it.
        Appends, indexed transforms and updates of positions, and removals leave the order of the last upload in place, which
        costs time only -- K1 culls by the bounds of 256 consecutive slots, select_neighbours is bounded by the pairs of
        such blocks within reach -- and this call takes that cost away: afterwards scene_layout() is a fresh upload's, bounds
        included, while values, indices and frames are what they were.  Returns how many slots hold another Gaussian than
        before; 0: nothing was moved and everything kept from frame to frame is still there.  Synchronous."""
        moved = C.c_uint64()
        self._check(self._L.splat_reorder_scene_device(self._h, C.byref(moved)))
        return int(moved.value)

    def duplicate(self, index, k=None, stream=None):
        """Copies of the Gaussians index[0..k) (as in read_indexed: uint32 / int32 original indices in device memory, in any
        order, duplicates allowed; k= with a plain address) appended to the resident scene: read_indexed of the four fields
        into buffers of the library's, then append.  Copy t is Gaussian first_new_index + t.  A copy ties its original in
        depth at every camera and has the higher index, so it is composited behind it.  What read_indexed refuses is refused
        here, with nothing appended, and the buffer is freed on every way out.  Returns (first_new_index, n)."""
        k, pi = self._index_address(index, k)
        first = self.n
        if k == 0:
            return first, self.n
        st = _producer_stream(stream, (index,))
        self.read_indexed(pi, stream=st, k=k)              # no field named: the library judges context, scene and k, and nothing else
        base = self._L.splat_device_alloc(self._h, 4 * 62 * k)
        if not base:
            raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"duplicate: no device memory for the rows").decode())
        try:
            pp, pc, po, ps = base, base + 16 * k, base + 52 * k, base + 56 * k        # [k,4] [k,9] [k] [k,48] float32
            self.read_indexed(pi, pp, pc, po, ps, stream=st, k=k)
            return first, self.append(pp, pc, po, ps, m=k)
        finally:
            self._L.splat_device_free(self._h, C.c_void_p(base))

    block_pairs = None         # what the most recent select_neighbours was bounded by (see there)

    def select_neighbours(self, selection, radius, *, source=None, at_least=0, at_most=None, op="set", counts=None,
                          max_block_pairs=None, stream=None):
        """splat_select_neighbours_device: a Gaussian passes when the number of OTHER Gaussians of the source set whose
        centres lie within `radius` of its own (d2 <= radius^2 in float32, on the resident centres) is in
        [at_least, at_most]; at_most=None: no upper end.  `selection`, and `op` with what it holds, are select's; `source`
        is a byte mask like a selection (None: every Gaussian is a source) and may be `selection` itself.  counts: a device
        buffer of n 32-bit elements that receives the counts (saturated at at_most + 1); selection may then be None.  The
        two recipes:
            floaters, fewer than k others within r:   select_neighbours(sel, r, at_most=k-1)
            grow a selection by r:                    select_neighbours(sel, r, source=sel, at_least=1, op="add")
        The work is bounded before it is done: the call counts the pairs of 256-Gaussian blocks whose bounds are within reach
        of each other (kept in self.block_pairs, also when the call is refused) and raises SplatError(ERR_CAPACITY), with
        nothing written, when they exceed max_block_pairs.  None: 64 per block -- a policy, not a measurement: a radius below
        a block's own extent reaches a few dozen blocks of a Morton-ordered cloud; 0: no limit.  A scene whose blocks' bounds
        overlap more than that is refused at ANY radius -- the 1.5 M Gaussian benchmark cloud has 73 pairs per block at
        radius 0 (profiles/select_neighbours.json): pass a limit there, e.g. 128 * n_blocks.  Returns how many Gaussians are
        selected after the op (counts only: how many pass)."""
        radius = float(radius)
        if not (radius >= 0.0) or radius == float("inf"):
            raise ValueError("radius: a finite number >= 0 expected, got %r" % (radius,))
        at_least = int(at_least)
        at_most = 0xFFFFFFFF if at_most is None else int(at_most)
        if not (0 <= at_least <= 0xFFFFFFFF and 0 <= at_most <= 0xFFFFFFFF):
            raise ValueError("at_least / at_most: 32-bit counts expected, got %d and %d" % (at_least, at_most))
        if at_least > at_most:
            raise ValueError("at_least (%d) is above at_most (%d): nothing could pass" % (at_least, at_most))
        if op not in self._SEL_OPS:
            raise ValueError("op: one of %s, got %r" % (sorted(self._SEL_OPS), op))
        if selection is None and counts is None:
            raise ValueError("selection and counts: at least one of the two")
        dev = int(self.config.device)
        ps = _byte_mask_address(selection, "selection", self.n, dev) if selection is not None else 0
        pq = _byte_mask_address(source, "source", self.n, dev) if source is not None else 0
        pc = 0
        if counts is not None:
            if not isinstance(counts, int) and hasattr(counts, "element_size") and int(counts.element_size()) != 4:
                raise TypeError("counts: 32-bit counts expected, got %s" % getattr(counts, "dtype", None))
            pc = _device_address(counts, "counts", None, dev, any_dtype=True)
            if not isinstance(counts, int) and hasattr(counts, "numel") and int(counts.numel()) != self.n:
                raise ValueError("counts: %d elements expected, got %d" % (self.n, int(counts.numel())))
        if max_block_pairs is None:
            max_block_pairs = 64 * ((self.n + 255) // 256)
        max_block_pairs = int(max_block_pairs)
        if max_block_pairs < 0:
            raise ValueError("max_block_pairs: not negative (0: no limit), got %d" % max_block_pairs)
        st = _producer_stream(stream, (selection, source, counts))
        count, pairs = C.c_uint64(), C.c_uint64()
        self.block_pairs = None
        rc = self._L.splat_select_neighbours_device(self._h, radius, C.c_void_p(pq), at_least, at_most, self._SEL_OPS[op], C.c_void_p(ps),
                                                    C.c_void_p(pc), max_block_pairs, C.byref(pairs), C.byref(count), C.c_void_p(st))
        if rc in (_lib.SPLAT_OK, _lib.ERR_CAPACITY):
            self.block_pairs = int(pairs.value)
        self._check(rc)
        return int(count.value)

    # the layouts of splat_pick_result and splat_pick_layer, as numpy sees them
    PICK_RESULT_DTYPE = np.dtype([("n_hits", "u4"), ("flags", "u4"), ("front_index", "u4"), ("front_depth", "f4"), ("front_alpha", "f4"),
                                  ("surface_index", "u4"), ("surface_depth", "f4"), ("surface_coverage", "f4")])
    PICK_LAYER_DTYPE = np.dtype([("index", "u4"), ("depth", "f4"), ("alpha", "f4"), ("coverage", "f4")])

    def pick(self, cam_c, pixels, *, alpha_min=0.0, coverage=0.5, mask=None, max_hits=1024, layers=0, results=None, layers_out=None,
             stream=None):
        """splat_pick_device: what lies under the pixels -- (x, y) pairs of the target of cam_c, AT MOST 256 of them: more
        raises ValueError (split the call; nothing loops silently).  A Gaussian is a hit of a pixel when the reference's
        fragment of it is accepted there with alpha >= alpha_min (glibc's expf, whatever mode the context renders in) and
        its byte in `mask` (a selection: n bytes of device memory; None: all) is nonzero.  Hits are ordered nearest first.
        Per pixel: n_hits, flags, the front hit (front_index, front_depth, front_alpha) and the surface -- the first hit at
        which the float coverage 1 - prod(1 - alpha) reaches `coverage` (surface_index, surface_depth, surface_coverage;
        index 0xFFFFFFFF when none does) -- which is what a click should select.  layers=k: also the first k hits of every
        pixel, each (index, depth, alpha, coverage).  max_hits (1..4096) bounds the list kept per pixel: a pixel with more
        hits has flags & 1 set, exact n_hits and front, no surface and no layers.
        Returns a numpy structured array of len(pixels) results (PICK_RESULT_DTYPE), or with layers=k the pair (results,
        layers [len(pixels), k] of PICK_LAYER_DTYPE; rows beyond a pixel's hits are zero).  With results= (and layers_out=
        when layers > 0) -- device tensors or addresses of 32 bytes per pixel and 16 per pixel and layer -- the call
        writes there, copies nothing down and returns None: pick -> indices -> edit stays on the GPU."""
        px = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
        if len(px) > _lib.PICK_MAX_PIXELS:
            raise ValueError("pixels: at most %d per call, got %d" % (_lib.PICK_MAX_PIXELS, len(px)))
        max_hits, layers = int(max_hits), int(layers)
        if not 1 <= max_hits <= _lib.PICK_MAX_HITS:
            raise ValueError("max_hits: 1 .. %d expected, got %d" % (_lib.PICK_MAX_HITS, max_hits))
        if not 0 <= layers <= max_hits:
            raise ValueError("layers: 0 .. max_hits (%d) expected, got %d" % (max_hits, layers))
        if (results is None) != (layers_out is None) and layers > 0:
            raise ValueError("results= and layers_out=: both or neither when layers > 0")
        q = _lib.PickQuery(float(alpha_min), float(coverage), max_hits, layers)
        dev = int(self.config.device)
        pm = _byte_mask_address(mask, "mask", self.n, dev) if mask is not None else 0
        st = _producer_stream(stream, (mask, results, layers_out))
        k = len(px)
        own = results is None
        if own:                               # one buffer of the call's own: the results, the layer rows behind them
            pr = self._L.splat_device_alloc(self._h, max(32 * k + 16 * k * layers, 4))
            if not pr:
                raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"pick: no device memory for the results").decode())
            pl = pr + 32 * k
        else:
            pr = _device_address(results, "results", None, dev, any_dtype=True)
            pl = _device_address(layers_out, "layers_out", None, dev, any_dtype=True) if layers_out is not None else 0
        try:
            self._check(self._L.splat_pick_device(self._h, C.byref(q), C.byref(cam_c), k, px.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.c_void_p(pm), C.c_void_p(pr), C.c_void_p(pl) if layers else None, C.c_void_p(st)))
            if not own:
                return None
            raw = np.zeros(32 * k + 16 * k * layers, np.uint8)
            if raw.nbytes:
                self._check(self._L.splat_device_download(self._h, C.c_void_p(raw.ctypes.data), C.c_void_p(pr), raw.nbytes))
            res = raw[:32 * k].view(self.PICK_RESULT_DTYPE).copy()
            if not layers:
                return res
            lay = raw[32 * k:].view(self.PICK_LAYER_DTYPE).reshape(k, layers).copy()
            due = np.where(res["flags"] & _lib.PICK_TRUNCATED, 0, np.minimum(res["n_hits"], layers))
            lay[np.arange(layers)[None, :] >= due[:, None]] = np.zeros((), self.PICK_LAYER_DTYPE)   # the library leaves those rows alone
            return res, lay
        finally:
            if own:
                self.device_free(pr)

    def _sized_address(self, a, what, size, count):
        """Device address of a buffer of `count` elements of `size` bytes (None: 0), checked where it describes itself."""
        if a is None:
            return 0
        if not isinstance(a, int) and hasattr(a, "element_size") and int(a.element_size()) != size:
            raise TypeError("%s: %d-byte elements expected, got %s" % (what, size, getattr(a, "dtype", None)))
        p = _device_address(a, what, None, int(self.config.device), any_dtype=True)
        if not isinstance(a, int) and hasattr(a, "numel") and int(a.numel()) != count:
            raise ValueError("%s: %d elements expected, got %d" % (what, count, int(a.numel())))
        return p

    def visibility(self, cam_c, *, weight_min=1.0 / 255.0, rect=None, pixel_mask=None, mask=None, pixels=None, max_weight=None,
                   weight_sum=None, accumulate=False, stream=None):
        """splat_visibility_device: what each Gaussian contributes to the view of cam_c, occlusion taken into account.  The
        hits of a pixel and their order are pick's (alpha_min = 0; `mask`: a selection, a Gaussian whose byte is 0 neither
        counts nor occludes); walking them nearest first with T = 1, hit k has the weight w = T * alpha and leaves
        T *= 1 - alpha, and it is SEEN at the pixel when w >= weight_min (in [0, 1); 0: every hit of the list).  Over the pixels
        of rect=(x0, y0, x1, y1) (inclusive, clamped; None: the whole target) whose byte of pixel_mask (a w*h uint8 device
        image; None: all) is nonzero, the call writes per Gaussian, original index order, into the device buffers given
        (tensors or addresses, n elements each, at least one):
            pixels      uint32   on how many pixels it is seen
            max_weight  float32  its greatest weight (0: seen nowhere)
            weight_sum  uint64   the sum of int(w * 2**24), truncating -- Q24 fixed point, bit-reproducible
        accumulate=True adds (and maxes) on top of what the buffers hold instead of zeroing them first: a loop over cameras
        leaves a Gaussian's importance over the view set on the device.  Exact in every bit.  Synchronous; frames afterwards
        are the frames they would have been (retained lists and region layouts start over: time only)."""
        weight_min = float(weight_min)
        if not (0.0 <= weight_min < 1.0):
            raise ValueError("weight_min: a number in [0, 1) expected, got %r" % (weight_min,))
        if pixels is None and max_weight is None and weight_sum is None:
            raise ValueError("pixels, max_weight, weight_sum: at least one of the three")
        w, h = int(cam_c.w), int(cam_c.h)
        x0, y0, x1, y1 = (0, 0, w - 1, h - 1) if rect is None else [int(v) for v in rect]
        q = _lib.VisibilityQuery(weight_min, x0, y0, x1, y1, _lib.VIS_ACCUMULATE if accumulate else _lib.VIS_SET)
        dev = int(self.config.device)
        pp = _byte_mask_address(pixel_mask, "pixel_mask", w * h, dev) if pixel_mask is not None else 0
        pm = _byte_mask_address(mask, "mask", self.n, dev) if mask is not None else 0
        pc = self._sized_address(pixels, "pixels", 4, self.n)
        px = self._sized_address(max_weight, "max_weight", 4, self.n)
        ps = self._sized_address(weight_sum, "weight_sum", 8, self.n)
        st = _producer_stream(stream, (pixel_mask, mask, pixels, max_weight, weight_sum))
        self._check(self._L.splat_visibility_device(self._h, C.byref(q), C.byref(cam_c), C.c_void_p(pp), C.c_void_p(pm), C.c_void_p(pc),
                                                    C.c_void_p(px), C.c_void_p(ps), C.c_void_p(st)))

    def select_counts(self, counts, selection, at_least=1, at_most=None, op="set", stream=None, n=None):
        """splat_select_counts_device: Gaussian i passes when at_least <= counts[i] <= at_most (None: no upper end), combined
        with `selection` by op as select does.  counts: n uint32 in device memory -- visibility's pixels, select_neighbours'
        counts (n= with plain addresses; default the resident scene's n).  Returns how many are selected after the op."""
        at_least = int(at_least)
        at_most = 0xFFFFFFFF if at_most is None else int(at_most)
        if not (0 <= at_least <= 0xFFFFFFFF and 0 <= at_most <= 0xFFFFFFFF):
            raise ValueError("at_least / at_most: 32-bit counts expected, got %d and %d" % (at_least, at_most))
        if at_least > at_most:
            raise ValueError("at_least (%d) is above at_most (%d): nothing could pass" % (at_least, at_most))
        if op not in self._SEL_OPS:
            raise ValueError("op: one of %s, got %r" % (sorted(self._SEL_OPS), op))
        if n is None:
            n = int(counts.numel()) if (not isinstance(counts, int) and hasattr(counts, "numel")) else self.n
        n = int(n)
        pc = self._sized_address(counts, "counts", 4, n)
        ps = _byte_mask_address(selection, "selection", n, int(self.config.device))
        st = _producer_stream(stream, (counts, selection))
        count = C.c_uint64()
        self._check(self._L.splat_select_counts_device(self._h, n, C.c_void_p(pc), at_least, at_most, self._SEL_OPS[op], C.c_void_p(ps),
                                                       C.byref(count), C.c_void_p(st)))
        return int(count.value)

    def select_visible(self, cams, selection, *, weight_min=1.0 / 255.0, min_pixels=1, rect=None, pixel_mask=None, mask=None, op="set",
                       stream=None):
        """What is SEEN: the Gaussians that visibility() finds on at least min_pixels pixels over `cams` -- one camera or a
        sequence of them, their pixel counts added up in a temporary on the device -- into `selection` by op.  rect,
        pixel_mask, mask and weight_min are visibility's and apply to every camera.
            select_visible(cam, sel, pixel_mask=lasso)                  what is seen under the lasso, not the wall behind it
            select_visible(train_cams, sel); remove(sel, keep=True)     prune what no camera sees
        Returns how many Gaussians are selected after the op."""
        if isinstance(cams, _lib.CameraC):
            cams = [cams]
        else:
            try:
                cams = list(cams)                     # any iterable of cameras: a list, a generator, an object array
            except TypeError:
                raise TypeError("cams: a camera (Camera.to_c) or an iterable of them expected, got %s" % type(cams).__name__) from None
        if not cams:
            raise ValueError("cams: at least one camera")
        for cam_c in cams:
            if not isinstance(cam_c, _lib.CameraC):
                raise TypeError("cams: every element must be a camera (Camera.to_c), got %s" % type(cam_c).__name__)
        min_pixels = int(min_pixels)
        if not 0 <= min_pixels <= 0xFFFFFFFF:
            raise ValueError("min_pixels: a 32-bit count expected, got %d" % min_pixels)
        if op not in self._SEL_OPS:
            raise ValueError("op: one of %s, got %r" % (sorted(self._SEL_OPS), op))
        _byte_mask_address(selection, "selection", self.n, int(self.config.device))
        tmp = self._L.splat_device_alloc(self._h, max(4 * self.n, 4))
        if not tmp:
            raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"select_visible: no device memory for the counts").decode())
        try:
            for k, cam_c in enumerate(cams):
                self.visibility(cam_c, weight_min=weight_min, rect=rect, pixel_mask=pixel_mask, mask=mask, pixels=tmp, accumulate=k > 0,
                                stream=stream)
            return self.select_counts(tmp, selection, at_least=min_pixels, op=op, stream=stream, n=self.n)
        finally:
            self.device_free(tmp)

    def compute_cov3d_device(self, scales, rotations, out, stream=None, n=None):
        """splat_compute_cov3d_device: kernel K0 from device buffers (scales [n,3], rotations [n,4]) into a device buffer
        (out [n,9]); arguments and stream as in upload_device.  Returns when `out` is written."""
        n = _count_of(scales, 3, n)
        dev = int(self.config.device)
        ptrs = [_device_address(a, what, per * n, dev) for a, what, per in
                ((scales, "scales", 3), (rotations, "rotations", 4), (out, "out", 9))]
        st = _producer_stream(stream, (scales, rotations, out))
        self._check(self._L.splat_compute_cov3d_device(self._h, n, *[C.c_void_p(p) for p in ptrs], C.c_void_p(st)))
        return out

    # ---- the scene from PLY rows ---------------------------------------------------------
    @staticmethod
    def _ply_layout_of(layout):
        lay = getattr(layout, "layout", layout)                 # gaussians.ply_layout()'s result, or the structure itself
        if not isinstance(lay, _lib.PlyLayout):
            raise TypeError("layout: expected a _lib.PlyLayout (or gaussians.ply_layout()'s result), got %s" % type(layout).__name__)
        return lay

    def _ply_rows(self, rows, lay):
        """device address of the vertex rows: an int, or anything with data_ptr() (a torch.uint8 tensor, say) -- of any
        dtype, at any byte address, holding at least n * stride bytes where it can tell"""
        p = _device_address(rows, "rows", None, int(self.config.device), any_dtype=True)
        if not isinstance(rows, int) and hasattr(rows, "numel") and hasattr(rows, "element_size"):
            have = int(rows.numel()) * int(rows.element_size())
            if have < int(lay.n) * int(lay.stride):
                raise ValueError("rows: %d bytes, the layout describes %d" % (have, int(lay.n) * int(lay.stride)))
        return p

    def load_ply(self, path, compute_cov3d=True):
        """The scene from a PLY file, with the work on the GPU: the payload of a binary file crosses PCIe once, as the bytes
        the file holds, and is decoded, activated, recentred and uploaded there (splat_upload_ply_device); an ascii file
        takes the host loader and upload().  compute_cov3d=False leaves cov3d zero (Gaussian::new).  The frames are those of
        load_from_ply + compute_cov3d + upload, byte for byte.  Returns the number of Gaussians."""
        import os
        so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsplat_host.so")
        if not os.path.exists(so):
            raise RuntimeError("splat_amd: %s is missing -- run __graft_entry__.build()" % so)
        H = C.CDLL(so)
        H.splat_host_load_ply_to_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        H.splat_host_load_ply_to_gpu.restype = C.c_longlong
        err = C.create_string_buffer(512)
        n = H.splat_host_load_ply_to_gpu(self._h, str(path).encode(), 1 if compute_cov3d else 0, err, 512)
        if n < 0:
            raise ValueError(err.value.decode("utf-8", "replace") or "load_ply failed")
        self.n = int(n)
        return self.n

    def upload_ply_rows(self, rows, layout, compute_cov3d=True, stream=None):
        """splat_upload_ply_device: the scene from PLY vertex rows that are already in this GPU's memory.  rows: a device
        address or an object with data_ptr(); layout: gaussians.ply_layout(path) or a _lib.PlyLayout; stream as in
        upload_device.  Synchronous: `rows` is free again on return."""
        lay = self._ply_layout_of(layout)
        p = self._ply_rows(rows, lay) if lay.n else 0
        st = _producer_stream(stream, (rows,))
        self._check(self._L.splat_upload_ply_device(self._h, C.byref(lay), C.c_void_p(p), 1 if compute_cov3d else 0, C.c_void_p(st)))
        self.n = int(lay.n)

    def decode_ply_device(self, rows, layout, positions, scales, opacities, rotations, sh, stream=None):
        """splat_decode_ply_device: PLY vertex rows in device memory -> five device buffers of the caller (positions [n,4],
        scales [n,3], opacities [n], rotations [n,4] as (i,j,k,w), sh [n,48], float32), activated and recentred as
        load_from_ply does.  Arguments and stream as in upload_device.  Returns when they are written."""
        lay = self._ply_layout_of(layout)
        n = int(lay.n)
        dev = int(self.config.device)
        ptrs = [_device_address(a, what, (per * n) if n else None, dev) for a, what, per in
                ((positions, "positions", 4), (scales, "scales", 3), (opacities, "opacities", 1), (rotations, "rotations", 4), (sh, "sh", 48))]
        p = self._ply_rows(rows, lay) if n else 0
        st = _producer_stream(stream, (rows, positions, scales, opacities, rotations, sh))
        self._check(self._L.splat_decode_ply_device(self._h, C.byref(lay), C.c_void_p(p), *[C.c_void_p(q) for q in ptrs], C.c_void_p(st)))

    def _ply_encode_layout(self, layout):
        """the layout of an encode, judged as far as Python can: what the kernel needs to own whole dwords"""
        lay = self._ply_layout_of(layout)
        if int(lay.stride) == 0 or int(lay.stride) % 4:
            raise ValueError("layout: stride %d is not a positive multiple of 4" % int(lay.stride))
        if int(lay.stride) > 65528:
            raise ValueError("layout: stride %d is above 65528 bytes (a row must fit the encoder's stage)" % int(lay.stride))
        seen = set()
        for k, name in enumerate(_lib.PLY_SLOT_NAMES):
            o = int(lay.offset[k])
            if o == -1:
                continue
            if o < 0 or o % 4 or o + 4 > int(lay.stride):
                raise ValueError("layout: offset %d of %s is not a multiple of 4 inside the row" % (o, name))
            if o in seen:
                raise ValueError("layout: offset %d of %s overlaps another property" % (o, name))
            seen.add(o)
        return lay

    def encode_ply_rows(self, rows, layout, index=None, stream=None, k=None):
        """splat_encode_ply_scene_device / splat_encode_ply_gaussians_device, the inverse of decode_ply_device: the RESIDENT
        scene written as PLY vertex rows into `rows` (writable device memory of layout.n * layout.stride bytes, 4-byte aligned: a
        device address or an object with data_ptr()).  layout: gaussians.inria_layout(n), or any _lib.PlyLayout whose stride
        and present offsets are multiples of 4 (stride <= 65528); offset -1 = not written; bytes no slot names are written
        as 0.  index=None: row t is Gaussian t (layout.n must be the scene's n); else row t is Gaussian index[t] (uint32 /
        int32 original indices in device memory, any order, duplicates allowed; k= with a plain address; layout.n must be k).
        Each covariance becomes three log scales and a unit quaternion (rot_0 >= 0), the opacity its logit; positions and
        sh keep their bits.  Through the loader the covariances and opacities come back within the error of a float64
        decomposition rounded to float32, not bit for bit; an opacity of 0 or 1 and a zero covariance come back exactly.
        Synchronous; reads the scene only, like read_device.  An index >= n raises SplatError(ERR_INVALID), nothing written."""
        lay = self._ply_encode_layout(layout)
        if index is None:
            if int(lay.n) != self.n:
                raise ValueError("layout: %d rows, the resident scene has %d Gaussians" % (int(lay.n), self.n))
            p = self._ply_rows(rows, lay) if lay.n else 0
            if p % 4:
                raise ValueError("rows: the address is not a multiple of 4")
            self._check(self._L.splat_encode_ply_scene_device(self._h, C.byref(lay), C.c_void_p(p)))
            return
        k, pi = self._index_address(index, k)
        if int(lay.n) != k:
            raise ValueError("layout: %d rows for %d indices" % (int(lay.n), k))
        p = self._ply_rows(rows, lay) if k else 0
        if p % 4:
            raise ValueError("rows: the address is not a multiple of 4")
        st = _producer_stream(stream, (index, rows))
        self._check(self._L.splat_encode_ply_gaussians_device(self._h, k, C.c_void_p(pi), C.byref(lay), C.c_void_p(p), C.c_void_p(st)))

    def save_ply(self, path, index=None, stream=None, k=None):
        """The resident scene, or its Gaussians index[0..k) (as in encode_ply_rows), into the canonical 62-float INRIA file at
        `path` (gaussians.PLY_PROPS order, binary little endian): encoded on the GPU into a temporary device buffer and
        copied down once (splat_host_save_ply_from_gpu).  What encode_ply_rows says about exactness holds; load_from_ply
        recentres on every load, so the reloaded positions are the saved ones minus their sequential-float32 mean.  Returns
        the number of rows written."""
        import os
        so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsplat_host.so")
        if not os.path.exists(so):
            raise RuntimeError("splat_amd: %s is missing -- run __graft_entry__.build()" % so)
        if index is None:
            k, pi = self.n, 0
        else:
            k, pi = self._index_address(index, k)
            # the file writer takes no stream: what wrote the indices is waited for here
            if stream is not None and hasattr(stream, "synchronize"):
                stream.synchronize()
            elif stream is not None and int(stream):
                raise ValueError("save_ply: a raw stream handle cannot be waited for here -- synchronise it and pass stream=None")
            else:
                torch = sys.modules.get("torch")
                if torch is not None and isinstance(index, torch.Tensor):
                    torch.cuda.current_stream(index.device).synchronize()
        H = C.CDLL(so)
        H.splat_host_save_ply_from_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_char_p, C.c_int]
        H.splat_host_save_ply_from_gpu.restype = C.c_longlong
        err = C.create_string_buffer(512)
        rows = H.splat_host_save_ply_from_gpu(self._h, str(path).encode(), k, C.c_void_p(pi), err, 512)
        if rows < 0:
            raise ValueError(err.value.decode("utf-8", "replace") or "save_ply failed")
        return int(rows)

    def scene_layout(self):
        """(orig, bounds) of the current scene: orig[j] = the Gaussian stored in slot j (uint32 [n]); bounds = per K1 block
        of 256 slots lo[3], hi[3], fmax, pad (float32 [ceil(n/256), 8])."""
        nb = (self.n + 255) // 256
        orig = np.zeros(self.n, np.uint32)
        bounds = np.zeros((nb, 8), f32)
        self._check(self._L.splat_get_scene_layout(self._h, orig.ctypes.data_as(C.POINTER(C.c_uint32)), self.n,
                                                   bounds.ctypes.data_as(C.POINTER(C.c_float)), nb))
        return orig, bounds

    def set_slab(self, tile_row0=0, tile_row1=-1):
        self._check(self._L.splat_set_slab(self._h, int(tile_row0), int(tile_row1)))

    def tile_row_loads(self, cam_c):
        """(Gaussian, tile) pairs per tile row of the full frame: the load estimate for slab balancing."""
        n_rows = (int(cam_c.h) + _lib.TILE - 1) // _lib.TILE
        out = np.zeros(n_rows, np.uint64)
        self._check(self._L.splat_tile_row_loads(self._h, C.byref(cam_c), out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 n_rows))
        return out

    def set_frame_overlap(self, n):
        """2: asynchronous frames to DIFFERENT device images (a swap chain) may composite side by side (include/splat_hip.h,
        splat_set_frame_overlap); 1 (default): one compositor at a time, in call order."""
        self._check(self._L.splat_set_frame_overlap(self._h, int(n)))

    def set_option(self, option, value):
        """splat_set_option: a tuning option (_lib.OPT_*) from code instead of from the environment; never changes a pixel"""
        self._check(self._L.splat_set_option(self._h, int(option), float(value)))

    def get_option(self, option):
        v = C.c_double()
        self._check(self._L.splat_get_option(self._h, int(option), C.byref(v)))
        return v.value

    def set_stream(self, stream_ptr):
        self._check(self._L.splat_set_stream(self._h, C.c_void_p(stream_ptr)))

    # ---- frames -----------------------------------------------------------------------
    def render(self, cam_c, argb, want_stats=True):
        """argb: uint32 [h,w] host array, blended in place."""
        assert argb.dtype == np.uint32 and argb.flags.c_contiguous
        assert argb.shape == (int(cam_c.h), int(cam_c.w))
        st = _lib.Stats()
        self._check(self._L.splat_render(self._h, C.byref(cam_c), argb.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         C.byref(st) if want_stats else None))
        return st

    def render_frame(self, cam_c, argb_out, want_stats=False):
        """splat_render_frame: the viewer loop's `clear; render_to_buffer` (src/main.rs:73-74) as one synchronous call; argb_out
        (uint32 [h,w], host) is written, never read.  A page-locked image (host_image / host_register) is written by the
        compositor itself."""
        assert argb_out.dtype == np.uint32 and argb_out.flags.c_contiguous
        assert argb_out.shape == (int(cam_c.h), int(cam_c.w))
        st = _lib.Stats() if want_stats else None
        self._check(self._L.splat_render_frame(self._h, C.byref(cam_c), argb_out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               C.byref(st) if want_stats else None))
        return st

    def render_device(self, cam_c, d_ptr, sync=False, want_stats=False):
        """d_ptr: device address of a w*h u32 image (e.g. torch_tensor.data_ptr())."""
        st = _lib.Stats() if want_stats else None
        self._check(self._L.splat_render_device(self._h, C.byref(cam_c), C.c_void_p(d_ptr), 1 if sync else 0,
                                                C.byref(st) if want_stats else None))
        return st

    # ---- multi-GPU, one process per GPU (form A of include/splat_hip.h "Multi-GPU") ---------
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128-byte RCCL id to hand to the other ranks"""
        L = _lib.lib()
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES)()
        rc = L.splat_comm_unique_id(buf)
        if rc != 0:
            raise SplatError(rc, "splat_comm_unique_id")
        return bytes(buf)

    def comm_init(self, unique_id, n_ranks, rank):
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self._L.splat_comm_init_rank(self._h, buf, int(n_ranks), int(rank)))

    def comm_set_slabs(self, slabs):
        flat = (C.c_int32 * (2 * len(slabs)))(*[int(v) for s in slabs for v in s])
        self._check(self._L.splat_comm_set_slabs(self._h, flat))

    def comm_loopback(self, on=True):
        """test hook: a single-rank communicator's gather sends this rank's rows through RCCL to itself"""
        self._check(self._L.splat_comm_loopback(self._h, 1 if on else 0))

    def comm_gather(self, d_ptr, w, h, root=0):
        """enqueue the gather of slab rows to `root` on the context's stream (grouped ncclSend / ncclRecv)"""
        self._check(self._L.splat_comm_gather(self._h, C.c_void_p(d_ptr), int(w), int(h), int(root)))

    # ---- device images without a HIP toolchain on the caller's side ------------------------
    def device_image(self, init):
        """Device copy of a uint32 [h,w] host image; returns its device address (free with device_free)."""
        assert init.dtype == np.uint32 and init.flags.c_contiguous
        p = self._L.splat_device_alloc(self._h, init.nbytes)
        if not p:
            raise SplatError(_lib.ERR_HIP, (self._L.splat_last_error(self._h) or b"").decode())
        self._check(self._L.splat_device_upload(self._h, C.c_void_p(p), C.c_void_p(init.ctypes.data), init.nbytes))
        return p

    def device_download(self, d_ptr, h, w):
        out = np.zeros((int(h), int(w)), np.uint32)
        self._check(self._L.splat_device_download(self._h, C.c_void_p(out.ctypes.data), C.c_void_p(d_ptr), out.nbytes))
        return out

    def device_free(self, d_ptr):
        self._L.splat_device_free(self._h, C.c_void_p(d_ptr))

    def render_frame_device(self, cam_c, d_ptr, sync=False, want_stats=False):
        """the viewer loop's frame (clear + render_to_buffer, src/main.rs:73-74) on a device image; the clear is fused
        into the compositor"""
        st = _lib.Stats() if want_stats else None
        self._check(self._L.splat_render_frame_device(self._h, C.byref(cam_c), C.c_void_p(d_ptr), 1 if sync else 0,
                                                      C.byref(st) if want_stats else None))
        return st

    def sync(self):
        """Wait for everything enqueued.  Raises SplatError(ERR_CAPACITY) once if an ASYNCHRONOUS frame was
        skipped on the device (storage has been grown: render it again)."""
        self._check(self._L.splat_sync(self._h))

    def device_bytes(self):
        """(bytes of device memory the context holds now, the most it has held)"""
        peak = C.c_uint64()
        now = int(self._L.splat_device_bytes(self._h, C.byref(peak)))
        return now, int(peak.value)

    def frames_dropped(self):
        """frames skipped on the device since the context was created (redone internally or reported)"""
        return int(self._L.splat_frames_dropped(self._h))

    def frames_retained(self):
        """frames since the context was created that were composited from retained lists (OPT_RETAIN_LISTS): the compositor
        alone, on the lists an earlier frame of the same camera left in order"""
        n = C.c_uint64()
        self._check(self._L.splat_frames_retained(self._h, C.byref(n)))
        return int(n.value)

    # ---- viewer-loop streaming (src/main.rs:69-78): cleared frame -> async copy into a host buffer
    @staticmethod
    def host_register(arr):
        """page-lock a numpy image the caller owns (splat_host_register): render() then copies it at the PCIe rate;
        call host_unregister(arr) before the array goes away"""
        rc = _lib.lib().splat_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes)
        if rc != 0:
            raise SplatError(rc, "splat_host_register")

    @staticmethod
    def host_unregister(arr):
        _lib.lib().splat_host_unregister(C.c_void_p(arr.ctypes.data))

    def host_image(self, h, w):
        """a pinned (page-locked) h x w uint32 image; keep the Renderer alive while it is in use"""
        p = self._L.splat_host_alloc(int(h) * int(w) * 4)
        if not p:
            raise MemoryError("splat_host_alloc")
        arr = np.ctypeslib.as_array((C.c_uint32 * (int(h) * int(w))).from_address(p)).reshape(int(h), int(w))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return arr

    def render_stream(self, cam_c, out):
        assert out.dtype == np.uint32 and out.flags.c_contiguous
        self._check(self._L.splat_render_stream(self._h, C.byref(cam_c), C.c_void_p(out.ctypes.data)))

    def stream_wait(self, out):
        self._check(self._L.splat_stream_wait(self._h, C.c_void_p(out.ctypes.data)))

    def timing(self, reset=True):
        ms = (C.c_double * 6)()
        frames = C.c_uint64()
        self._check(self._L.splat_get_timing(self._h, ms, C.byref(frames), 1 if reset else 0))
        names = ("preprocess", "scan", "emit", "sort", "composite", "status")
        return {k: ms[i] for i, k in enumerate(names)}, frames.value

    # ---- debug / stage parity -----------------------------------------------------------
    def records(self):
        dt = np.dtype([("cx", "f4"), ("cy", "f4"), ("hx", "f4"), ("hy", "f4"), ("conic", "f4", 3),
                       ("opacity", "f4"), ("rgb", "f4", 3), ("depth", "f4"), ("px0", "i4"), ("px1", "i4"),
                       ("py0", "i4"), ("py1", "i4")])
        assert dt.itemsize == C.sizeof(_lib.Record)
        out = np.zeros(self.n, dt)
        self._check(self._L.splat_get_records(self._h, out.ctypes.data_as(C.POINTER(_lib.Record)), self.n))
        return out

    def binning_mode(self):
        """bucket size (keys per tile) of the last frame's one-pass binning, 0 = two-pass, < 0 = no frame"""
        return int(self._L.splat_binning_mode(self._h))

    def tile_lists(self, n_tiles, n_pairs):
        off = np.zeros(n_tiles + 1, np.uint32)
        order = np.zeros(n_pairs, np.uint32)
        self._check(self._L.splat_get_tile_lists(self._h, off.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles + 1,
                                                 order.ctypes.data_as(C.POINTER(C.c_uint32)), n_pairs))
        return off, order
