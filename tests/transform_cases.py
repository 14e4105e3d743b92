"""What the scene transform's tests share: the matrices, and the formulas of include/splat_hip.h restated in numpy float32
-- every product and every sum one float32 array operation, hence rounded once, in the header's order.

    p'_r    = ((A(r,0) x + A(r,1) y) + A(r,2) z) + m[4r+3]
    T(r,c)  =  (A(r,0) S(0,c) + A(r,1) S(1,c)) + A(r,2) S(2,c)
    S'(r,c) =  (T(r,0) A(c,0) + T(r,1) A(c,1)) + T(r,2) A(c,2)

with A(r,k) = m[4r+k] and S(r,c) = cov[3c+r] (column-major blocks)."""
import math

import numpy as np

f32 = np.float32


def _about(pivot, lin):
    """the 3x4 map x -> lin (x - pivot) + pivot, composed in float64 and cast once"""
    lin = np.asarray(lin, np.float64)
    pivot = np.asarray(pivot, np.float64)
    return np.concatenate([lin, (pivot - lin @ pivot)[:, None]], 1).astype(f32)


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * k + (1 - math.cos(t)) * (k @ k)


MATRICES = {
    "identity": np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32),
    "rotation": _about((0.4, -0.3, 0.2), _rotation((1.0, 2.0, -0.5), 20.0)),        # 20 degrees about a pivot
    "scale": _about((0.0, 0.0, 0.0), 1.25 * np.eye(3)),
    "shear": np.array([[1.5, 0.25, 0.0, 0.1], [0.0, 0.75, -0.5, -0.2], [0.125, 0.0, 1.1, 0.05]], f32),   # non-uniform scale with shear
    "mirror": _about((0.1, 0.0, 0.0), np.diag([-1.0, 1.0, 1.0])),                   # det < 0
    "zero": np.zeros((3, 4), f32),
}
assert np.linalg.det(MATRICES["mirror"][:, :3].astype(np.float64)) < 0


def transform_np(m, pos, cov):
    """(positions', cov3d') of the rows given: pos [k, >=3] (columns beyond z are kept), cov [k, 9]; m 3x4"""
    m = np.asarray(m, f32).reshape(3, 4)
    pos = np.asarray(pos, f32)
    cov = np.asarray(cov, f32)
    out_p, out_c = pos.copy(), np.empty_like(cov)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        for r in range(3):
            out_p[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
        T = [[(m[r, 0] * cov[:, 3 * c] + m[r, 1] * cov[:, 3 * c + 1]) + m[r, 2] * cov[:, 3 * c + 2] for c in range(3)] for r in range(3)]
        for c in range(3):
            for r in range(3):
                out_c[:, 3 * c + r] = (T[r][0] * m[c, 0] + T[r][1] * m[c, 1]) + T[r][2] * m[c, 2]
    assert out_p.dtype == f32 and out_c.dtype == f32
    return out_p, out_c


def transformed(g, m, rows=None):
    """(positions, cov3d) of GaussianList g with the rows named (all: None) mapped by m, the others as they are"""
    pos, cov = g.positions.copy(), g.cov3d.copy()
    sel = slice(None) if rows is None else np.asarray(rows, np.int64)
    pos[sel], cov[sel] = transform_np(m, g.positions[sel], g.cov3d[sel])
    return pos, cov


# ---- the probe library (tests/native/transform_math_probe.hip) ----------------------------------------------------------
_PROBE = None


def probe():
    import ctypes as C
    import os
    global _PROBE
    if _PROBE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libtransform_math_probe.so")
        assert os.path.exists(path), "%s is missing -- run __graft_entry__.build()" % path
        L = C.CDLL(path)
        fp = C.POINTER(C.c_float)
        L.transform_probe_host.argtypes = [fp, C.c_uint64, fp, fp, fp, fp]
        L.transform_probe_host.restype = None
        L.transform_probe_device.argtypes = [fp, C.c_uint64, fp, fp, fp, fp]
        L.transform_probe_device.restype = C.c_int
        _PROBE = L
    return _PROBE


def run_probe(m, pos3, cov, device=False):
    """(pos3', cov') from the probe's host (device=False) or device entry point; pos3 [k,3], cov [k,9], float32"""
    import ctypes as C
    fp = C.POINTER(C.c_float)
    m = np.ascontiguousarray(m, f32).reshape(12)
    pos3, cov = np.ascontiguousarray(pos3, f32), np.ascontiguousarray(cov, f32)
    k = len(pos3)
    assert pos3.shape == (k, 3) and cov.shape == (k, 9)
    po, co = np.full_like(pos3, np.nan), np.full_like(cov, np.nan)
    args = [a.ctypes.data_as(fp) for a in (m,)] + [k] + [a.ctypes.data_as(fp) for a in (pos3, cov, po, co)]
    if device:
        rc = probe().transform_probe_device(*args)
        assert rc == 0, "transform_probe_device: HIP error %d" % rc
    else:
        probe().transform_probe_host(*args)
    return po, co


def random_gaussians(k, seed):
    """(pos3 [k,3], cov [k,9]): centres of a few units; covariance blocks of nine independent entries -- NOT symmetric, so
    that a transposed index shows -- over five decades of magnitude, with signed zeros among them"""
    rng = np.random.default_rng(seed)
    pos = (3.0 * rng.standard_normal((k, 3))).astype(f32)
    cov = (rng.standard_normal((k, 9)) * 10.0 ** rng.uniform(-4.0, 1.0, (k, 1))).astype(f32)
    z = rng.random((k, 9)) < 0.05
    cov[z] = np.where(rng.random(int(z.sum())) < 0.5, f32(0.0), f32(-0.0))
    pos[rng.random((k, 3)) < 0.02] = f32(-0.0)
    return pos, cov
