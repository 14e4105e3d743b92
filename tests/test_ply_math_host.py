"""The PLY decoder's activations (expf_libm_full and sigmoid_libm of splat_amd/csrc/splat_device_math.h), compiled for
the HOST by the probe library (tests/native/ply_math_probe.hip), against glibc's expf as the oracle library calls it -- no
GPU needed.  The device compile of the same text is held to the same reference by tests/test_gpu_ply_device.py.

Wall time: a minute or two on 16 threads (2.2e9 arguments, each through both)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_cases as P  # noqa: E402
from oracle import oracle as O  # noqa: E402

f32 = np.float32
NEG104, POS89 = P.bits_of(-104.0), P.bits_of(89.0)
SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,           # +-0, +-inf, +-FLT_MAX
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)   # NaNs, quiet and signalling


def chunks(first, last, size=P.CHUNK):
    b = first
    while b <= last:
        n = min(size, last - b + 1)
        yield b, n
        b += n


def test_probe_library_is_built():
    P.probe()


def test_the_band_holds_what_it_is_meant_to_hold():
    # both thresholds and the whole band of subnormal results lie inside [-104, 89]
    assert f32(-104.0) < P.UFLOW < P.NORMAL_EDGE < 0 < P.OFLOW < f32(89.0)
    e = O.expf_n(bits=[P.bits_of(P.UFLOW), P.bits_of(np.nextafter(P.UFLOW, f32(-200))), P.bits_of(P.OFLOW),
                       P.bits_of(np.nextafter(P.OFLOW, f32(200)))]).view(f32)
    assert e[0] > 0 and e[1] == 0 and np.isfinite(e[2]) and np.isinf(e[3])
    sub = O.expf_n(bits=P.around(P.NORMAL_EDGE, 64)).view(f32)
    tiny = np.finfo(f32).tiny
    assert (sub < tiny).any() and (sub >= tiny).any()


def test_host_expf_libm_full_is_glibc_expf_on_every_float_from_minus_104_to_89():
    wrong, total = [], 0
    for lo, hi in ((0x80000000, NEG104), (0x00000000, POS89)):
        for first, n in chunks(lo, hi):
            got, ref = P.run(0, True, first, n), O.expf_n(first, n)
            total += n
            wrong += [(hex(first + i), hex(got[i]), hex(ref[i])) for i in np.flatnonzero(got != ref)[:100]]
    print("expf_libm_full != expf at %d of %d arguments (bits, ours, expf): %r" % (len(wrong), total, wrong[:20]))
    assert total == (NEG104 - 0x80000000 + 1) + (POS89 + 1)
    assert not wrong, "%d arguments differ from expf (bits, ours, expf): %r" % (len(wrong), wrong[:8])


def test_host_expf_libm_full_outside_the_band_and_on_the_special_values():
    rng = np.random.default_rng(31)
    below = rng.integers(NEG104 + 1, 0xFF7FFFFF, 1 << 20, dtype=np.uint32, endpoint=True)
    above = rng.integers(POS89 + 1, 0x7F7FFFFF, 1 << 20, dtype=np.uint32, endpoint=True)
    got, ref = P.run(0, True, bits=below), O.expf_n(bits=below)
    assert (got == ref).all() and (got == 0).all()                     # +0, every one
    got, ref = P.run(0, True, bits=above), O.expf_n(bits=above)
    assert (got == ref).all() and (got == 0x7F800000).all()            # +inf
    got, ref = P.run(0, True, bits=SPECIAL), O.expf_n(bits=SPECIAL)
    assert P.same_bits(got, ref).all(), (got, ref)
    assert list(got[:6]) == [0x3F800000, 0x3F800000, 0x7F800000, 0x00000000, 0x7F800000, 0x00000000]
    assert np.isnan(got[6:].view(f32)).all()                           # NaN stays NaN


def test_host_sigmoid_is_the_ieee_expression_around_glibc_expf():
    sweep = np.arange(1 << 24, dtype=np.uint32) * np.uint32(256)       # every 256th of all 2^32 patterns
    sets = [sweep, SPECIAL] + [P.around(x) for x in (P.OFLOW, -P.OFLOW, P.UFLOW, -P.UFLOW)]
    for bits in sets:
        got, ref = P.run(1, True, bits=bits), P.sigmoid_reference(O, bits)
        bad = np.flatnonzero(~P.same_bits(got, ref))
        assert bad.size == 0, "%d arguments differ, first bits 0x%08x: ours 0x%08x reference 0x%08x" % (
            bad.size, bits[bad[0]], got[bad[0]], ref[bad[0]])
    # the stride form of the probe is the array form
    assert (P.run(1, True, first=0, n=1 << 12, step=256) == P.run(1, True, bits=sweep[:1 << 12])).all()
    s = P.run(1, True, bits=[P.bits_of(0.0), 0x7F800000, 0xFF800000]).view(f32)
    assert s[0] == f32(0.5) and s[1] == f32(1.0) and s[2] == f32(0.0)
