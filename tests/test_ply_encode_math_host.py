"""The PLY encoder's arithmetic (splat_amd/csrc/splat_ply_encode_math.h), compiled for the HOST by the probe library
(tests/native/ply_encode_probe.hip) -- no GPU needed.  The logs against float64 numpy within 1 ulp, the clamps against the
loader's own activations, the quaternion against the matrix it came from, and the whole chain -- covariance -> row -> what
the loader reads back -- against a float64 numpy.linalg.eigh encoder pushed through the same loader, class by class: the
header's worst error may be at most twice the reference's.  The device compile of the same text is held to this one bit
for bit by tests/test_gpu_ply_encode.py.

Measured here (host compile, worst e(S) = max|S' - S| / ||S||_F per class, in units of 2^-24; header / reference):
see profiles/ply_save_accuracy.json, written by tools/ply_save_probe.py --accuracy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_encode_cases as E  # noqa: E402
import ply_cases as P  # noqa: E402

f32, f64 = np.float32, np.float64
IN_DT = {0: (f32, 1), 1: (f32, 1), 2: (f32, 6), 3: (f64, 9), 4: (f32, 10)}
OUT_DT = {0: (f32, 1), 1: (f32, 1), 2: (f64, 12), 3: (f32, 4), 4: (f32, 8)}


def probe():
    path = os.path.join(ROOT, "tests", "native", "libply_encode_probe.so")
    assert os.path.exists(path), "%s is missing -- run __graft_entry__.build()" % path
    L = C.CDLL(path)
    for name in ("ply_encode_probe_host", "ply_encode_probe_device"):
        fn = getattr(L, name)
        fn.argtypes, fn.restype = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p], C.c_int
    return L


def run(which, data, host=True):
    """the probe's function `which` over the rows of `data`"""
    dt, per = IN_DT[which]
    a = np.ascontiguousarray(data, dt).reshape(-1, per)
    out = np.zeros((len(a), OUT_DT[which][1]), OUT_DT[which][0])
    L = probe()
    rc = (L.ply_encode_probe_host if host else L.ply_encode_probe_device)(which, len(a), a.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


def encode_rows(cov, opacity=None, host=True):
    """ply_encode_one: (log scales [n,3], logits [n], quaternions [n,4] as (i, j, k, w))"""
    cov = np.asarray(cov, f32).reshape(-1, 9)
    op = np.full(len(cov), 0.5, f32) if opacity is None else np.asarray(opacity, f32)
    o = run(4, np.concatenate([cov, op[:, None]], 1), host)
    return o[:, 0:3].copy(), o[:, 3].copy(), o[:, 4:8].copy()


def loader_cov(logs, quat, tmp_path, name):
    """what the product reads back from a file that holds these log scales and quaternions: load_from_ply (libm expf, the
    quaternion as stored) and splat_host_cov3d (the normalisation, R S^2 R^T in f32)"""
    import splat_amd
    n = len(logs)
    raw = {"scale_%d" % a: logs[:, a] for a in range(3)}
    raw.update({"rot_0": quat[:, 3], "rot_1": quat[:, 0], "rot_2": quat[:, 1], "rot_3": quat[:, 2]})
    path = str(tmp_path / (name + ".ply"))
    splat_amd.write_ply(path, raw, n)
    g = splat_amd.load_from_ply(path)
    H = C.CDLL(os.path.join(ROOT, "splat_amd", "libsplat_host.so"))
    H.splat_host_cov3d.argtypes, H.splat_host_cov3d.restype = [C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_void_p], None
    out = np.zeros((n, 9), f32)
    H.splat_host_cov3d(n, g.scales.ctypes.data, g.rotations.ctypes.data, out.ctypes.data)
    return out


def ulps(a, b):
    """distance in float32 steps between finite values of the same sign region"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_probe_library_is_built():
    probe()


def test_ply_log_is_within_one_ulp_of_float64():
    lam = np.concatenate([E.positive_floats()] + [E.covariances(c).ravel() for c in ("generic", "large", "tiny")])
    lam = lam[(lam > 0) & np.isfinite(lam)].astype(f32)
    got = run(0, lam).ravel()
    ref = (0.5 * np.log(lam.astype(f64))).astype(f32)
    d = ulps(got, ref)
    print("ply_log: %d arguments, %d differ from float64's rounding, worst %d ulp" % (len(lam), int((d > 0).sum()), int(d.max())))
    assert d.max() <= 1


def test_ply_logit_is_within_one_ulp_of_float64():
    o = E.opacities()
    o = o[(o > 0) & (o < 1)]
    got = run(1, o).ravel()
    d64 = o.astype(f64)
    ref = np.log(d64 / (1.0 - d64)).astype(f32)
    d = ulps(got, ref)
    print("ply_logit: %d arguments, %d differ from float64's rounding, worst %d ulp" % (len(o), int((d > 0).sum()), int(d.max())))
    assert np.isfinite(got).all() and d.max() <= 1


def test_the_clamps_are_exact_and_the_loader_reads_them_as_0_and_1():
    lo = run(1, np.array([0.0, -0.0, -1.0, -np.inf], f32)).ravel()
    hi = run(1, np.array([1.0, 2.0, np.inf], f32)).ravel()
    assert (lo == f32(-104.0)).all() and (hi == f32(104.0)).all()
    assert np.isnan(run(1, np.array([np.nan], f32))).all() and np.isnan(run(0, np.array([np.nan], f32))).all()
    assert (run(0, np.array([0.0, -0.0, -1e-30, -np.inf], f32)).ravel() == f32(-104.0)).all()
    # the smallest subnormal and the float below 1 stay finite and inside the clamps
    edge = run(1, np.array([1e-45, np.nextafter(f32(1), f32(0))], f32)).ravel()
    assert np.isfinite(edge).all() and f32(-104.0) < edge[0] < 0 < edge[1] < f32(104.0)
    # the loader's activations of the clamps (the ply_math probe's host compile): expf, sigmoid
    bits = [P.bits_of(-104.0), P.bits_of(104.0)]
    assert P.run(0, True, bits=bits[:1]).view(f32)[0] == f32(0.0)
    s = P.run(1, True, bits=bits).view(f32)
    assert s[0] == f32(0.0) and s[1] == f32(1.0)


def test_ply_quat_is_a_unit_quaternion_with_w_not_negative_that_rebuilds_its_matrix():
    rng = np.random.default_rng(5)
    q = rng.standard_normal((4096, 4))
    q[:8] = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 0, 0), (0, 1, 1, 0), (1, 0, 1, 0), (-1, 0, 0, 0)]   # half turns: w == 0
    R = E.rotations(q)
    V = np.ascontiguousarray(R.transpose(0, 2, 1)).reshape(-1, 9)      # V[3c + r]
    got = run(3, V)
    assert got.dtype == f32
    norm = np.sqrt((got.astype(f64) ** 2).sum(1))
    assert np.abs(norm - 1.0).max() <= 2.0 ** -23
    assert (got[:, 3] >= 0).all()
    half = got[:8]
    first = np.array([h[:3][np.flatnonzero(h[:3])[0]] for h in half[got[:8, 3] == 0]])
    assert len(first) >= 7 and (first > 0).all()
    back = E.rotations(got)
    print("ply_quat: worst |V' - V| %.3g (bound 2^-22 = %.3g)" % (np.abs(back - R).max(), 2.0 ** -22))
    assert np.abs(back - R).max() <= 2.0 ** -22


def test_ply_eig3_reconstructs_its_matrix_with_a_proper_rotation():
    cov = np.concatenate([E.covariances(c, 512) for c in E.CLASSES] + [E.edge_covariances()])
    c6 = cov[:, [0, 3, 6, 4, 7, 8]]
    o = run(2, c6)
    lam, V = o[:, :3], o[:, 3:].reshape(-1, 3, 3).transpose(0, 2, 1)   # V[n, r, c]
    assert np.abs(np.linalg.det(V) - 1.0).max() < 1e-12
    assert np.abs(np.einsum("nrk,nck->nrc", V, V) - np.eye(3)).max() < 1e-12
    S = cov.astype(f64).reshape(-1, 3, 3)
    back = np.einsum("nrk,nk,nck->nrc", V, lam, V)
    scale = np.maximum(np.sqrt((S * S).sum((1, 2))), 1e-300)
    assert (np.abs(back - S).max((1, 2)) / scale).max() < 1e-13


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """per class: (worst e of the header's chain, worst e of the float64 reference's), through the loader"""
    tmp = tmp_path_factory.mktemp("ply_encode")
    out = {}
    for name in E.CLASSES + ("edges",):
        S = E.edge_covariances() if name == "edges" else E.covariances(name)
        logs, _, quat = encode_rows(S)
        rlogs, rquat = E.reference_encode(S)
        ours, ref = loader_cov(logs, quat, tmp, name), loader_cov(rlogs, rquat, tmp, name + "_ref")
        out[name] = (S, ours, ref)
    return out


@pytest.mark.parametrize("name", E.CLASSES)
def test_the_chain_is_within_twice_the_float64_reference_through_the_loader(chain, name):
    S, ours, ref = chain[name]
    e, r = E.relative_error(ours, S).max(), E.relative_error(ref, S).max()
    print("%-10s worst e: header %.2f, float64 eigh reference %.2f (units of 2^-24)" % (name, e * 2 ** 24, r * 2 ** 24))
    assert np.isfinite(ours).all()
    assert e <= 2.0 * r


def test_the_edge_cases_come_back(chain):
    S, ours, ref = chain["edges"]
    e, r = E.relative_error(ours, S), E.relative_error(ref, S)
    print("edges %r: header %r, reference %r (units of 2^-24)" % (E.EDGES, list(e * 2 ** 24), list(r * 2 ** 24)))
    zero = E.EDGES.index("zero")
    assert (ours[zero] == 0).all() and not np.signbit(ours[zero]).any()            # exactly zero
    assert (e[1:] <= 2.0 * r[1:]).all()
    logs, _, _ = encode_rows(S)
    assert (logs[zero] == f32(-104.0)).all()
    assert (logs[E.EDGES.index("rank1")] == f32(-104.0)).sum() >= 1 and (logs[E.EDGES.index("negative")] == f32(-104.0)).sum() == 1
    assert (logs[E.EDGES.index("identity")] == 0).all()
