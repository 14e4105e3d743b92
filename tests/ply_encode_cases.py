"""Inputs of the PLY encoder's tests (tests/test_ply_encode_math_host.py, tests/test_gpu_ply_encode.py,
tools/ply_save_probe.py --accuracy): covariance classes, opacities, and the float64 reference encoder the product's chain
is held to.  Plain numpy: no library of the project is loaded here.

A covariance is float32 R diag(s^2) R^T from seeded scales and unit quaternions, made symmetric by mirroring its upper
triangle (the half the encoder reads); rows are the scene's nine floats, S(r,c) = cov[3c + r]."""
import numpy as np

f32, f64 = np.float32, np.float64
N_CLASS = 4096
CLASSES = ("generic", "flat", "needle", "isotropic", "two_equal", "diagonal", "large", "tiny")
EDGES = ("zero", "rank1", "negative", "identity")


def rotations(q):
    """[n,3,3] float64 rotation matrices of quaternions q [n,4] = (i, j, k, w), normalised here: what compute_cov3d builds"""
    q = np.asarray(q, f64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    i, j, k, w = q.T
    R = np.empty((len(q), 3, 3), f64)
    R[:, 0, 0] = w * w + i * i - j * j - k * k; R[:, 0, 1] = 2 * (i * j - w * k); R[:, 0, 2] = 2 * (w * j + i * k)
    R[:, 1, 0] = 2 * (w * k + i * j); R[:, 1, 1] = w * w - i * i + j * j - k * k; R[:, 1, 2] = 2 * (j * k - w * i)
    R[:, 2, 0] = 2 * (i * k - w * j); R[:, 2, 1] = 2 * (w * i + j * k); R[:, 2, 2] = w * w - i * i - j * j + k * k
    return R


def _cov_of(scales, q):
    R = rotations(q).astype(f32)
    s2 = (scales.astype(f32) * scales.astype(f32))
    S = np.einsum("nrk,nk,nck->nrc", R, s2, R).astype(f32)
    iu = np.triu_indices(3, 1)
    S[:, iu[1], iu[0]] = S[:, iu[0], iu[1]]
    return np.ascontiguousarray(S.reshape(-1, 9))               # symmetric: row- and column-major are the same nine floats


def covariances(name, n=N_CLASS, seed=0):
    """[n,9] float32 of one class"""
    rng = np.random.Generator(np.random.PCG64([seed, CLASSES.index(name)]))
    mu = {"large": 5.0, "tiny": -14.0}.get(name, -4.0)
    s = np.exp(rng.standard_normal((n, 3)) * 0.8 + mu)
    q = rng.standard_normal((n, 4))
    if name == "flat":
        s[:, 2] *= 1e-3
    elif name == "needle":
        s[:, 1:] *= 1e-3
    elif name == "isotropic":
        s[:, 1] = s[:, 0]; s[:, 2] = s[:, 0]
    elif name == "two_equal":
        s[:, 1] = s[:, 0]
    elif name == "diagonal":
        q[:] = (0.0, 0.0, 0.0, 1.0)
    return _cov_of(s, q)


def edge_covariances():
    """[4,9] float32, in the order of EDGES"""
    v = np.array([0.1, 0.2, 0.3], f32)
    neg = np.array([[1.0, 1.0, 0.0], [1.0, 1.0 - 2.0 ** -20, 0.0], [0.0, 0.0, 1.0]], f32)   # det of the 2x2 block: -2^-20
    return np.ascontiguousarray(np.stack([np.zeros((3, 3), f32), np.outer(v, v).astype(f32), neg, np.eye(3, dtype=f32)]).reshape(4, 9))


def opacities(seed=0):
    """the hand-written opacities, then a seeded sweep over (0, 1)"""
    hand = np.array([0.0, np.float32(1e-45), 1.0 / 255.0, 0.5, 0.99, np.nextafter(f32(1), f32(0)), 1.0, 2.0, -1.0], f32)
    u = np.random.Generator(np.random.PCG64([seed, 99])).random(N_CLASS, dtype=f32)
    u = u[(u > 0) & (u < 1)]
    return np.concatenate([hand, u]).astype(f32)


def positive_floats(n=1 << 16, seed=0):
    """seeded positive finite float32 across the whole exponent range, subnormals among them"""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    bits = rng.integers(1, 0x7f800000, n, dtype=np.int64).astype(np.uint32)
    sub = rng.integers(1, 0x00800000, 1024, dtype=np.int64).astype(np.uint32)
    return np.concatenate([bits, sub, np.array([1, 0x007fffff, 0x00800000, 0x3f800000, 0x7f7fffff], np.uint32)]).view(f32)


def reference_encode(cov):
    """The float64 reference: numpy.linalg.eigh, a column flipped for det +1, sqrt(max(lam, 0)), np.log, Shepperd, each
    result rounded to float32 once.  -> (log scales [n,3], quaternions [n,4] as (i, j, k, w)), float32"""
    S = np.asarray(cov, f64).reshape(-1, 3, 3)
    lam, V = np.linalg.eigh(S)
    V[np.linalg.det(V) < 0, :, 2] *= -1.0
    with np.errstate(divide="ignore"):
        logs = np.log(np.sqrt(np.maximum(lam, 0.0)))
    n = len(S)
    m = lambda r, c: V[:, r, c]  # noqa: E731
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    diag = np.stack([tr, m(0, 0), m(1, 1), m(2, 2)], 1)
    br = np.argmax(diag, 1)
    q = np.empty((n, 4), f64)                                   # w i j k
    one = np.ones(n)
    cand = [np.stack([one + tr, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], 1),
            np.stack([m(2, 1) - m(1, 2), one + m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)], 1),
            np.stack([m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), one + m(1, 1) - m(0, 0) - m(2, 2), m(1, 2) + m(2, 1)], 1),
            np.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), one + m(2, 2) - m(0, 0) - m(1, 1)], 1)]
    for b in range(4):
        q[br == b] = cand[b][br == b]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1.0
    return logs.astype(f32), np.ascontiguousarray(q[:, [1, 2, 3, 0]]).astype(f32)


def relative_error(S_back, S):
    """e(S) = max |S' - S| / ||S||_F per matrix, in float64 ([n,9] each); a zero S answers 0 where S' is zero too, else inf"""
    a, b = np.asarray(S_back, f64).reshape(-1, 9), np.asarray(S, f64).reshape(-1, 9)
    num, den = np.abs(a - b).max(1), np.sqrt((b * b).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num == 0, 0.0, np.inf))
