"""What the colour tools' tests share: the formulas of include/splat_hip.h restated in numpy float32 -- every product, sum,
quotient and root one float32 array operation, hence rounded once, in the stated order -- their float64 versions, the case
lists (matrices, queries, sh_dim) and the probe library.

    colours_np    d = (p - cam_pos) / sqrt((dx dx + dy dy) + dz dz);  rgb = eval_sh(sh, sh_dim, d) + 0.5      (K1's order)
    passes_np     clamp by comparisons, u_k = ((m[4k] r + m[4k+1] g) + m[4k+2] b) + m[4k+3], box / ball, a NaN fails
    recolour_np   sh'[3k+i] = (A(i,0) r + A(i,1) g) + A(i,2) b, and for k == 0 that + o_i

The basis is eval_sh's own (oracle/splat_oracle.cpp); its float64 restatement is tests/sh_rotate_cases.py's."""
import ctypes as C
import math
import os

import numpy as np

import splat_amd
from splat_amd import _lib
import sh_rotate_cases as S

f32 = np.float32
U = S.U                                              # unit roundoff of float32
TINY = S.TINY                                        # the smallest subnormal
SH_DIMS = (3, 12, 15, 48)                            # band 0 | bands 0-1 | 0-2 (the frames') | all four
OPS = ("set", "add", "subtract", "intersect")

_C0 = f32(0.28209479177387814)
_C1 = f32(0.4886025119029199)
_C2 = [f32(v) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
_C3 = [f32(v) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                        1.445305721320277, -0.5900435899266435)]
_2, _3, _4, _H = f32(2.0), f32(3.0), f32(4.0), f32(0.5)


def coefficients(sh_dim):
    """how many of the 16 coefficients eval_sh weighs at sh_dim"""
    return 16 if sh_dim > 27 else 9 if sh_dim > 12 else 4 if sh_dim > 3 else 1


# ---- float32, one rounding per operation -------------------------------------------------------------------------------------
def colours_np(pos, cam_pos, sh_dim, sh):
    """[k, 3] float32: pos [k, >= 3], cam_pos [3], sh [k, 48]"""
    pos, sh, cam = np.ascontiguousarray(pos, f32), np.ascontiguousarray(sh, f32), np.asarray(cam_pos, f32)
    c = lambda k: [sh[:, 3 * k + ch] for ch in range(3)]                      # noqa: E731
    with np.errstate(all="ignore"):
        dx, dy, dz = pos[:, 0] - cam[0], pos[:, 1] - cam[1], pos[:, 2] - cam[2]
        nrm = np.sqrt((dx * dx + dy * dy) + dz * dz)
        x, y, z = dx / nrm, dy / nrm, dz / nrm
        col = [_C0 * v for v in c(0)]
        if sh_dim > 3:
            k1, k2, k3 = _C1 * y, _C1 * z, _C1 * x
            col = [((col[ch] - k1 * c(1)[ch]) + k2 * c(2)[ch]) - k3 * c(3)[ch] for ch in range(3)]
            if sh_dim > 12:
                xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
                k = [_C2[0] * xy, _C2[1] * yz, _C2[2] * ((_2 * zz - xx) - yy), _C2[3] * xz, _C2[4] * (xx - yy)]
                for ch in range(3):
                    a = col[ch]
                    for m in range(5):
                        a = a + k[m] * c(4 + m)[ch]
                    col[ch] = a
                if sh_dim > 27:
                    k = [(_C3[0] * y) * (_3 * xx - yy), (_C3[1] * xy) * z, (_C3[2] * y) * ((_4 * zz - xx) - yy),
                         (_C3[3] * z) * ((_2 * zz - _3 * xx) - _3 * yy), (_C3[4] * x) * ((_4 * zz - xx) - yy), (_C3[5] * z) * (xx - yy),
                         (_C3[6] * x) * (xx - _3 * yy)]
                    for ch in range(3):
                        a = col[ch]
                        for m in range(7):
                            a = a + k[m] * c(9 + m)[ch]
                        col[ch] = a
        out = np.stack([v + _H for v in col], 1)
    assert out.dtype == f32
    return out


def passes_np(q, rgb):
    """[k] bool: q = (colour_to_unit [3, 4], shape "box" / "ellipsoid", clamp)"""
    m, shape, clamp = q
    m = np.ascontiguousarray(m, f32).reshape(3, 4)
    rgb = np.ascontiguousarray(rgb, f32)
    with np.errstate(all="ignore"):
        ch = [rgb[:, i] for i in range(3)]
        if clamp:
            ch = [np.where(v < 0, f32(0.0), np.where(v > 1, f32(1.0), v)).astype(f32) for v in ch]
        u = [((m[k, 0] * ch[0] + m[k, 1] * ch[1]) + m[k, 2] * ch[2]) + m[k, 3] for k in range(3)]
        assert all(a.dtype == f32 for a in u)
        if shape == "box":
            return (np.abs(u[0]) <= 1) & (np.abs(u[1]) <= 1) & (np.abs(u[2]) <= 1)
        return ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) <= 1


def offset_np(m):
    """[3] float32: o_i = (t_i + 0.5 ((A_i0 + A_i1) + A_i2) - 0.5) / C0 in float64 from the float32 entries, rounded once"""
    m = np.asarray(m, f32).reshape(3, 4).astype(np.float64)
    with np.errstate(all="ignore"):
        return (((m[:, 3] + 0.5 * ((m[:, 0] + m[:, 1]) + m[:, 2])) - 0.5) / float(_C0)).astype(f32)


def recolour_np(m, sh):
    """sh [k, 48] float32 mapped by m = [A | t] (3x4), the header's way"""
    m = np.asarray(m, f32).reshape(3, 4)
    o = offset_np(m)
    sh = np.ascontiguousarray(sh, f32)
    out = np.empty_like(sh)
    with np.errstate(all="ignore"):
        for k in range(16):
            r, g, b = sh[:, 3 * k], sh[:, 3 * k + 1], sh[:, 3 * k + 2]
            for i in range(3):
                v = (m[i, 0] * r + m[i, 1] * g) + m[i, 2] * b
                if k == 0:
                    v = v + o[i]
                assert v.dtype == f32
                out[:, 3 * k + i] = v
    return out


def recoloured_rows(m, sh, rows=None):
    """sh with the rows named (all: None) recoloured, the others as they are"""
    out = np.ascontiguousarray(sh, f32).copy()
    sel = slice(None) if rows is None else np.asarray(rows, np.int64)
    out[sel] = recolour_np(m, out[sel])
    return out


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def weights64(d, sh_dim):
    """[m, 16] float64: what eval_sh weighs the 16 coefficients with at the directions d [m, 3]; 0 beyond sh_dim's bands"""
    d = np.asarray(d, np.float64)
    Y = np.concatenate([np.full(d.shape[:-1] + (1,), float(_C0)), S.basis(d)], -1)
    Y[..., coefficients(sh_dim):] = 0.0
    return Y


def weights_abs64(d, sh_dim):
    """the same with every monomial of a polynomial taken by its absolute value: what the rounding errors of the float32
    evaluation of a weight scale with"""
    d = np.abs(np.asarray(d, np.float64))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c1, c2, c3 = float(_C1), [abs(float(v)) for v in _C2], [abs(float(v)) for v in _C3]
    Y = np.stack([np.full(x.shape, float(_C0)), c1 * y, c1 * z, c1 * x,
                  c2[0] * xy, c2[1] * yz, c2[2] * (2.0 * zz + xx + yy), c2[3] * xz, c2[4] * (xx + yy),
                  c3[0] * y * (3.0 * xx + yy), c3[1] * xy * z, c3[2] * y * (4.0 * zz + xx + yy),
                  c3[3] * z * (2.0 * zz + 3.0 * xx + 3.0 * yy), c3[4] * x * (4.0 * zz + xx + yy), c3[5] * z * (xx + yy),
                  c3[6] * x * (xx + 3.0 * yy)], -1)
    Y[..., coefficients(sh_dim):] = 0.0
    return Y


def colour64(sh, sh_dim, d):
    """eval_sh + 0.5 in float64: sh [k, 48], d [m, 3] -> [k, m, 3]"""
    sh = np.asarray(sh, np.float64).reshape(len(sh), 16, 3)
    return np.einsum("mk,ikc->imc", weights64(d, sh_dim), sh) + 0.5


def mapped64(m, rgb):
    """A rgb + t in float64 over the last axis"""
    m = np.asarray(m, f32).reshape(3, 4).astype(np.float64)
    return np.einsum("ij,...j->...i", m[:, :3], np.asarray(rgb, np.float64)) + m[:, 3]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _m(rows):
    return np.array(rows, f32)


MATRICES = {
    "identity": splat_amd.colour_matrix(),
    "grey": splat_amd.colour_matrix(saturation=0),
    "swap": _m([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]]),
    "negative": _m([[-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, -1, 1]]),
    "tinted_contrast": splat_amd.colour_matrix(saturation=0.7, tint=(1.1, 0.9, 0.8), contrast=1.3, brightness=-0.05),
    "zero_row": _m([[1, 0, 0, 0], [0, 0, 0, 0.25], [0, 0.5, 0.5, 0]]),
}
PERMUTATIONS = ("identity", "swap")                  # A holds only 0 and 1, t = 0: the offset is 0 and every value moves exactly


def ball(rgb, tolerance):
    """colour_to_unit of the colours within `tolerance` (a scalar or a triple) of rgb, as Renderer.select_colour makes it"""
    tol = np.broadcast_to(np.asarray(tolerance, np.float64).reshape(-1), (3,))
    return np.concatenate([np.diag(1.0 / tol), (-np.asarray(rgb, np.float64) / tol)[:, None]], 1).astype(f32)


def luma_band(lo, hi):
    """colour_to_unit of lo <= luma <= hi: one row of weights, two zero rows (|0| <= 1: they pass)"""
    half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    m = np.zeros((3, 4))
    m[0, :3] = np.asarray(splat_amd.renderer.LUMA) / half
    m[0, 3] = -mid / half
    return m.astype(f32)


# (centres and widths sit where a synthetic scene's colours are, so that each query passes a part of it: tests assert that)
QUERIES = {}
for _clamp in (True, False):
    _tag = "clamp" if _clamp else "raw"
    QUERIES["ball_" + _tag] = (ball((0.5, 0.5, 0.5), 0.35), "ellipsoid", _clamp)
    QUERIES["box_" + _tag] = (ball((0.45, 0.6, 0.4), (0.3, 0.25, 0.45)), "box", _clamp)
    QUERIES["luma_" + _tag] = (luma_band(0.35, 0.6), "box", _clamp)


def combine(op, old, passed):
    """the selection after `op`: old [n] uint8 (any values), passed [n] bool -> (bytes, selected)"""
    old = np.asarray(old, np.uint8)
    was = old != 0
    if op == "set":
        sel = passed
        return sel.astype(np.uint8), sel
    if op == "add":
        return np.where(passed, 1, old).astype(np.uint8), was | passed
    if op == "subtract":
        return np.where(passed, 0, old).astype(np.uint8), was & ~passed
    sel = was & passed
    return sel.astype(np.uint8), sel


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def lively_sh(base_sh, seed, scale=0.05):
    """base_sh with bands 1-3 at magnitudes of their own (a synthetic scene's higher bands are faint), band 0 as it is"""
    sh = S.random_sh(len(base_sh), seed)
    sh[:, :3] = base_sh[:, :3]
    sh[:, 3:] *= f32(scale)
    return sh


def specials(cam_pos):
    """(pos [k, 3], sh [k, 48]) rows that take the arithmetic to its corners: a Gaussian AT the camera (0 / 0: NaN from band 1
    on), +-inf and NaN coefficients, -0.0, subnormals, huge and tiny distances"""
    cam = np.asarray(cam_pos, f32)
    rng = np.random.default_rng(77)
    sh = (rng.standard_normal((12, 48)) * 0.3).astype(f32)
    pos = (rng.standard_normal((12, 3)) * 2.0).astype(f32)
    pos[0] = cam                                       # at the camera
    sh[1, 0] = np.inf
    sh[2, 7] = -np.inf
    sh[3, 30] = np.nan
    sh[4, 2] = np.nan
    sh[5, :] = f32(-0.0)
    sh[6, ::2] = f32(-0.0)
    sh[7, :] = f32(1e-42)                              # subnormal coefficients
    sh[8, 3:] = f32(-3e-45)
    pos[9] = cam + f32(1e-30)                          # dx dx underflows: a 0 norm from a non-zero offset
    pos[10] = cam + np.array([3e19, -2e19, 1e19], f32)  # dx dx overflows: an inf norm
    pos[11] = cam + np.array([1e-22, 0, 0], f32)       # dx dx is subnormal
    return pos, sh


def same_bits(a, b):
    """bit for bit, a NaN equal to a NaN whatever its sign and payload"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d words differ, first at %r: %r != %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def oracle_rgb(g, cam, sh_dim, lowpass=0.01):
    """the rgb of oracle.preprocess's records for the GaussianList g under the product camera cam: [n, 3] float32"""
    from oracle import oracle as O
    from helpers import oracle_camera, scene_dict
    return np.ascontiguousarray(O.preprocess(scene_dict(g), oracle_camera(cam, lowpass, sh_dim))["rgb"], f32)


# ---- the probe library (tests/native/colour_math_probe.hip) ------------------------------------------------------------------
_PROBE = None


def probe():
    global _PROBE
    if _PROBE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libcolour_math_probe.so")
        assert os.path.exists(path), "%s is missing -- run __graft_entry__.build()" % path
        L = C.CDLL(path)
        fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
        for side, res in (("host", None), ("device", C.c_int)):
            for name, args in (("eval", [fp, C.c_int32, C.c_uint64, fp, fp, fp]),
                               ("passes", [C.POINTER(_lib.ColourQuery), C.c_uint64, fp, bp]),
                               ("recolour", [fp, fp, C.c_uint64, fp, fp])):
                fn = getattr(L, "colour_probe_%s_%s" % (name, side))
                fn.argtypes, fn.restype = args, res
        L.colour_probe_map.argtypes, L.colour_probe_map.restype = [fp, fp, fp], C.c_int
        _PROBE = L
    return _PROBE


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _run(name, device, *args):
    rc = getattr(probe(), "colour_probe_%s_%s" % (name, "device" if device else "host"))(*args)
    assert not device or rc == 0, "colour_probe_%s_device: HIP error %d" % (name, rc)


def probe_colours(pos, cam_pos, sh_dim, sh, device=False):
    pos, sh = np.ascontiguousarray(np.asarray(pos, f32)[:, :3]), np.ascontiguousarray(sh, f32)
    cam = np.ascontiguousarray(cam_pos, f32)
    out = np.full((len(pos), 3), -7.5, f32)
    _run("eval", device, _fp(cam), int(sh_dim), len(pos), _fp(pos), _fp(sh), _fp(out))
    return out


def query_struct(q):
    m, shape, clamp = q
    s = _lib.ColourQuery()
    s.colour_to_unit[:] = [float(v) for v in np.asarray(m, f32).ravel()]
    s.shape, s.clamp = {"box": 0, "ellipsoid": 1}[shape], 1 if clamp else 0
    return s


def probe_passes(q, rgb, device=False):
    rgb = np.ascontiguousarray(rgb, f32)
    out = np.full(len(rgb), 9, np.uint8)
    _run("passes", device, C.byref(query_struct(q)), len(rgb), _fp(rgb), out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert np.isin(out, (0, 1)).all()
    return out.astype(bool)


def probe_map(m):
    """(refused, A [3, 3], o [3]) as recolour_map of the header makes them from m (3x4)"""
    m = np.ascontiguousarray(np.asarray(m, f32).reshape(12))
    a, o = np.zeros(9, f32), np.zeros(3, f32)
    refused = probe().colour_probe_map(_fp(m), _fp(a), _fp(o))
    return bool(refused), a.reshape(3, 3), o


def probe_recolour(m, sh, device=False):
    refused, a, o = probe_map(m)
    assert not refused
    sh = np.ascontiguousarray(sh, f32)
    out = np.full_like(sh, -7.5)
    _run("recolour", device, _fp(np.ascontiguousarray(a.ravel())), _fp(o), len(sh), _fp(sh), _fp(out))
    return out


def spiral32(count=32):
    """sh_rotate_cases.spiral()'s directions as float32 (what the oracle's eval_sh takes), and the same widened"""
    d = S.spiral(count).astype(f32)
    return d, d.astype(np.float64)


assert math.isclose(float(_C0), 0.28209479177387814, rel_tol=1e-7)
