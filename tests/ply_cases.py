"""Shared by tests/test_ply_math_host.py, tests/test_ply_device_abi.py and tests/test_gpu_ply_device.py: the handle of the
PLY activation probe (tests/native/libply_math_probe.so, built by splat_amd/csrc/Makefile from
tests/native/ply_math_probe.hip), the argument sets both compiles are held to, and a PLY writer that can produce every
property list the tests need.  Nothing here knows what the code under test should return."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_PATH = os.path.join(HERE, "native", "libply_math_probe.so")
CHUNK = 1 << 26
f32 = np.float32

# glibc's expf thresholds (e_expf.c) and the argument whose result is the smallest normal float
OFLOW = f32(float.fromhex("0x1.62e42ep6"))          # above: +inf      (88.7228...)
UFLOW = f32(float.fromhex("-0x1.9fe368p6"))         # below: +0        (-103.972...)
NORMAL_EDGE = f32(-87.33654)                        # expf ~ 2^-126: results below are subnormal

_PROBE = None


def probe():
    """The probe library; a missing one is a failure (build() makes it), never a skip."""
    global _PROBE
    if _PROBE is None:
        assert os.path.exists(PROBE_PATH), "%s is missing: make -C splat_amd/csrc all builds it" % PROBE_PATH
        L = C.CDLL(PROBE_PATH)
        L.ply_probe_device.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ply_probe_host.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.ply_probe_host.restype = None
        _PROBE = L
    return _PROBE


def run(which, host, first=0, n=0, step=1, bits=None):
    """bits of expf_libm_full (which = 0) / sigmoid_libm (1) for the floats with bits first + i * step, or for `bits`"""
    if bits is not None:
        bits = np.ascontiguousarray(bits, np.uint32)
        n = bits.size
    out = np.empty(n, np.uint32)
    src = bits.ctypes.data if bits is not None else None
    if host:
        probe().ply_probe_host(which, first, step, src, n, out.ctypes.data, 16)
    else:
        rc = probe().ply_probe_device(which, first, step, src, n, out.ctypes.data)
        assert rc == 0, "ply_probe_device: HIP error %d" % rc
    return out


def bits_of(x):
    return int(np.asarray(x, f32).view(np.uint32))


def around(x, radius=1 << 16):
    """the 2 * radius + 1 bit patterns centred on float x (clipped to one sign's patterns)"""
    b = bits_of(x)
    lo, hi = max(b - radius, b & 0x80000000), min(b + radius, (b & 0x80000000) | 0x7FFFFFFF)
    return np.arange(lo, hi + 1, dtype=np.uint32)


def same_bits(a, b):
    """equal as uint32, NaN matching NaN"""
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return (a == b) | (np.isnan(a.view(f32)) & np.isnan(b.view(f32)))


def sigmoid_reference(O, bits):
    """numpy's float32 1 / (1 + e) with e = glibc's expf(-v) (the oracle library's): IEEE add and divide"""
    e = O.expf_n(bits=np.ascontiguousarray(bits, np.uint32) ^ np.uint32(0x80000000)).view(f32)
    with np.errstate(all="ignore"):
        return (f32(1.0) / (f32(1.0) + e)).astype(f32).view(np.uint32)


# ---- PLY files of any property list ----------------------------------------------------------------------------------
NP_TYPES = {"uchar": "u1", "char": "i1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4",
            "double": "<f8"}


def write_ply_props(path, props, n, values, fmt="binary_little_endian", seed=0):
    """props: [(type, name)] in file order (names may repeat); values: name -> array for the float properties the test
    cares about (the LAST occurrence of a repeated name gets it); everything else is seeded noise.  Returns the
    structured dtype of a row (fields f0, f1, ... in file order)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype([("f%d" % k, NP_TYPES[t]) for k, (t, _) in enumerate(props)])
    data = np.zeros(n, dt)
    last = {name: k for k, (_, name) in enumerate(props)}
    for k, (t, name) in enumerate(props):
        col = "f%d" % k
        if t == "float" and name in values and last[name] == k:
            data[col] = values[name]
        elif t in ("float", "double"):
            data[col] = rng.standard_normal(n)
        else:
            data[col] = rng.integers(0, 100, n)
    with open(path, "wb") as f:
        f.write(("ply\nformat %s 1.0\nelement vertex %d\n" % (fmt, n)).encode())
        for t, name in props:
            f.write(("property %s %s\n" % (t, name)).encode())
        f.write(b"end_header\n")
        if fmt == "ascii":
            for row in data:
                f.write((" ".join(repr(float(v)) if isinstance(v, (np.floating, float)) else str(int(v)) for v in row) + "\n").encode())
        else:
            data.tofile(f)
    return dt


def expected_offsets(props, dt):
    """name -> byte offset by the loader's rules, from the numpy dtype: float32 properties only, the last of a name wins"""
    out = {}
    for k, (t, name) in enumerate(props):
        if t == "float":                     # (a property of another type is skipped over: it feeds nothing)
            out[name] = dt.fields["f%d" % k][1]
    return out
