"""What the sh rotation's tests share: the rotations, the blocks D_l(R) in float64 by numpy.linalg.lstsq, and the formula of
include/splat_hip.h restated in numpy float32 -- every product and every sum one float32 array operation, hence rounded
once, summed left to right:

    c'_m = (((D(m,0) c_0 + D(m,1) c_1) + D(m,2) c_2) + ...)          per channel and band, c_k = sh[3 (first + k) + ch]

The basis is eval_sh's own (oracle/splat_oracle.cpp): fifteen polynomials with float32 constants, restated here in float64.
The library sees a rotation's float32 entries, so the float64 blocks are those of the ROUNDED matrix."""
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24                                       # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -149                                   # the smallest subnormal: the absolute error of an underflowing operation
BANDS = ((1, 3), (4, 5), (9, 7))                     # (first k, n = 2l+1) of bands 1, 2, 3


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * k + (1 - math.cos(t)) * (k @ k)


ROTATIONS = {
    "identity": np.eye(3),
    "rot20": _rotation((1.0, 2.0, -0.5), 20.0),
    "rot173": _rotation((3.0, 1.0, 2.0), 173.0),
    "quarter_z": np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
    "mirror_x": np.diag([-1.0, 1.0, 1.0]),
    "rot20_f32": _rotation((1.0, 2.0, -0.5), 20.0).astype(f32),
}
PERMUTATIONS = ("identity", "quarter_z", "mirror_x")        # their blocks hold only 0 and +-1
assert np.linalg.det(ROTATIONS["mirror_x"]) < 0

_C1 = float(f32(0.4886025119029199))
_C2 = [float(f32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
_C3 = [float(f32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                               1.445305721320277, -0.5900435899266435)]
_C0 = float(f32(0.28209479177387814))


def basis(d):
    """[..., 15] float64: the functions eval_sh weighs sh[3k..3k+3) with, k = 1..15, at the directions d [..., 3]"""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-_C1 * y, _C1 * z, -_C1 * x,
                     _C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy),
                     _C3[0] * y * (3.0 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4.0 * zz - xx - yy),
                     _C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), _C3[4] * x * (4.0 * zz - xx - yy), _C3[5] * z * (xx - yy),
                     _C3[6] * x * (xx - 3.0 * yy)], -1)


def eval_sh64(sh, d):
    """eval_sh in float64: sh [k, 48], d [m, 3] -> [k, m, 3]"""
    sh = np.asarray(sh, np.float64).reshape(len(sh), 16, 3)
    Y = np.concatenate([np.full(d.shape[:-1] + (1,), _C0), basis(d)], -1)          # [m, 16]
    return np.einsum("mk,ikc->imc", Y, sh) + 0.5


def spiral(count=32):
    i = np.arange(count, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / count
    phi = (i + 0.5) * math.pi * (3.0 - math.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


def as_seen(R):
    """the matrix the library works with: the float32 entries, in float64"""
    return np.asarray(R, f32).astype(np.float64).reshape(3, 3)


def blocks_f64(R, snapped=False):
    """[D_1, D_2, D_3] in float64: B_l D_l = B_l^R in the least-squares sense over the 32 spiral directions; snapped: every
    entry at the nearest multiple of 2^-40, as the library defines its blocks before it rounds them to float32"""
    R = as_seen(R)
    d = spiral()
    B, BR = basis(d), basis(d @ R)                   # row i of d @ R is R^T d_i
    out = []
    for first, n in BANDS:
        s = slice(first - 1, first - 1 + n)
        D = np.linalg.lstsq(B[:, s], BR[:, s], rcond=None)[0]
        out.append(np.rint(D * 2.0 ** 40) / 2.0 ** 40 if snapped else D)
    return out


def lib_blocks(R):
    import splat_amd
    return splat_amd.sh_rotation_blocks(R)


def rotate_np(blocks, sh):
    """sh [k, 48] float32 with bands 1-3 multiplied by the float32 blocks, the header's way; band 0 as it is"""
    sh = np.ascontiguousarray(sh, f32)
    out = sh.copy()
    with np.errstate(all="ignore"):
        for (first, n), D in zip(BANDS, blocks):
            D = np.asarray(D, f32).reshape(n, n)
            for ch in range(3):
                c = [sh[:, 3 * (first + k) + ch] for k in range(n)]
                for m in range(n):
                    a = D[m, 0] * c[0]
                    for k in range(1, n):
                        a = a + D[m, k] * c[k]
                    assert a.dtype == f32
                    out[:, 3 * (first + m) + ch] = a
    return out


def rotated_rows(blocks, sh, rows=None):
    """sh with the rows named (all: None) rotated, the others as they are"""
    out = np.ascontiguousarray(sh, f32).copy()
    sel = slice(None) if rows is None else np.asarray(rows, np.int64)
    out[sel] = rotate_np(blocks, out[sel])
    return out


def coefficient_bound(D64, sh):
    """[k, 48] float64: what a float32 coefficient of rotate_np may be off the float64 product by.  A band's coefficient is n
    products and n - 1 sums in float32, of entries that were rounded to float32 once: (n + 3) u sum_k |D(m,k)| |c_k|, plus
    one smallest subnormal for each of the n products that may underflow.  Band 0: 0.  D64 are the SNAPPED blocks where a
    single coefficient is judged: the snap is no rounding relative to the entry -- it moves a 1e-16 of solver noise to 0, all
    of it -- so against unsnapped blocks a coefficient whose own weight is 0 would be off by noise times its neighbours,
    which no multiple of u |D| |c| covers."""
    sh = np.abs(np.asarray(sh, np.float64)).reshape(len(sh), 16, 3)
    out = np.zeros_like(sh)
    for (first, n), D in zip(BANDS, D64):
        out[:, first:first + n] = (n + 3) * U * np.einsum("mk,ikc->imc", np.abs(D), sh[:, first:first + n]) + n * TINY
    return out.reshape(len(sh), 48)


def product_f64(D64, sh):
    """[k, 48] float64: the blocks times the coefficients, in float64"""
    sh = np.asarray(sh, np.float64).reshape(len(sh), 16, 3)
    out = sh.copy()
    for (first, n), D in zip(BANDS, D64):
        out[:, first:first + n] = np.einsum("mk,ikc->imc", D, sh[:, first:first + n])
    return out.reshape(len(sh), 48)


def random_sh(k, seed):
    """[k, 48] float32: every row at a magnitude of its own between 1e-3 and 30, signed zeros among the values"""
    rng = np.random.default_rng(seed)
    sh = (rng.standard_normal((k, 48)) * 10.0 ** rng.uniform(-3.0, math.log10(30.0), (k, 1))).astype(f32)
    z = rng.random((k, 48)) < 0.03
    sh[z] = np.where(rng.random(int(z.sum())) < 0.5, f32(0.0), f32(-0.0))
    return sh


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


# ---- the probe library (tests/native/sh_rotate_probe.hip) ------------------------------------------------------------------
_PROBE = None


def probe():
    import ctypes as C
    import os
    global _PROBE
    if _PROBE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libsh_rotate_probe.so")
        assert os.path.exists(path), "%s is missing -- run __graft_entry__.build()" % path
        L = C.CDLL(path)
        fp = C.POINTER(C.c_float)
        L.sh_rotate_probe_host.argtypes = [fp, fp, fp, C.c_uint64, fp, fp]
        L.sh_rotate_probe_host.restype = None
        L.sh_rotate_probe_device.argtypes = [fp, fp, fp, C.c_uint64, fp, fp]
        L.sh_rotate_probe_device.restype = C.c_int
        _PROBE = L
    return _PROBE


def run_probe(blocks, sh, device=False):
    """sh [k, 48] with bands 1-3 through the probe's host (device=False) or device entry point; band 0 copied"""
    import ctypes as C
    fp = C.POINTER(C.c_float)
    sh = np.ascontiguousarray(sh, f32)
    k = len(sh)
    d = [np.ascontiguousarray(D, f32).ravel() for D in blocks]
    assert [a.size for a in d] == [9, 25, 49] and sh.shape == (k, 48)
    src = np.ascontiguousarray(sh[:, 3:])
    dst = np.full_like(src, np.nan)
    args = [a.ctypes.data_as(fp) for a in d] + [k, src.ctypes.data_as(fp), dst.ctypes.data_as(fp)]
    if device:
        rc = probe().sh_rotate_probe_device(*args)
        assert rc == 0, "sh_rotate_probe_device: HIP error %d" % rc
    else:
        probe().sh_rotate_probe_host(*args)
    return np.concatenate([sh[:, :3], dst], 1)
