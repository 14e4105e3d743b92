"""The compositor's plain-C++ device functions (splat_amd/csrc/splat_device_math.h), compiled for the HOST by the probe
library, against references that share no code with them -- no GPU needed.  The device compile of the same text is held
to the same references by tests/test_gpu_device_math.py.

Wall time: about a minute on 16 threads (the exhaustive exponential sweep is most of it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_math_cases as K  # noqa: E402
from oracle import oracle as O  # noqa: E402


def test_probe_library_is_built():
    K.probe()


def test_host_exp_libm_is_glibc_expf_on_every_argument():
    """Every one of the 1 118 699 521 arguments.  (This is the test that found exp_libm's reduction residual one product
    rounding away from glibc's FMA build: bits 0xc27c65d9, 0x11fa2992 against expf's 0x11fa2993, host and device alike.)"""
    # every float in [-87, -0], and +0
    wrong = []
    for first, n in K.chunks(K.NEG_FIRST, K.NEG_LAST):
        got, ref = K.host_exp_libm(first, n), O.expf_n(first, n)
        wrong += [(hex(first + i), hex(got[i]), hex(ref[i])) for i in np.flatnonzero(got != ref)[:100]]
    print("exp_libm != expf at %d arguments (bits, exp_libm, expf): %r" % (len(wrong), wrong[:20]))
    assert not wrong, "%d arguments differ from expf (bits, exp_libm, expf): %r" % (len(wrong), wrong[:8])
    assert K.host_exp_libm(bits=[0])[0] == O.expf_n(bits=[0])[0] == np.float32(1).view(np.uint32)
    # NaN stays NaN
    nan = K.host_exp_libm(bits=[0x7FC00000, 0xFFC00000, 0x7F800001]).view(np.float32)
    assert np.isnan(nan).all()
    # below -87 the function returns expf(-87) BY DESIGN (the clamp), not expf(x): -inf, -FLT_MAX, 2^20 arguments
    e87 = O.expf_n(bits=[K.NEG_LAST])[0]
    low = np.concatenate([K.below_minus_87(), np.array([0xFF800000], np.uint32)])
    assert (K.host_exp_libm(bits=low) == e87).all()
    assert (O.expf_n(bits=low) < e87).all()          # ... where expf itself keeps falling: the clamp is visible


def test_host_reject_threshold_margin_for_every_opacity():
    # every float opacity in [2^-20, 4]: the threshold lies below log(1 / (255 op)) by 1e-3 up to float32 rounding --
    # at least 5e-4 (it never rejects a fragment that could be accepted: the margin exceeds the rounding of the logf
    # and of the quotient, ~1e-6 at these magnitudes) and at most 2e-3 (it still rejects something)
    lo, hi = np.float32(2.0 ** -20).view(np.uint32), np.float32(4.0).view(np.uint32)
    dmin, dmax = np.inf, -np.inf
    for first, n in K.chunks(int(lo), int(hi), 1 << 25):
        thr = K.host_reject_threshold(first, n).astype(np.float64)
        op = np.arange(first, first + n, dtype=np.uint32).view(np.float32).astype(np.float64)
        d = -np.log(255.0 * op) - thr
        dmin, dmax = min(dmin, d.min()), max(dmax, d.max())
    print("reject_threshold: log(1/(255 op)) - threshold in [%.6g, %.6g]" % (dmin, dmax))
    assert 5e-4 <= dmin and dmax <= 2e-3, (dmin, dmax)
    # the sentinels: nothing can be accepted at opacity <= 0 (alpha <= 0 < 1/255); NaN opacity keeps every record
    s = K.host_reject_threshold(bits=np.array([0.0, -0.0, -1.0, -np.inf, np.nan], np.float32).view(np.uint32))
    assert (s[:4] == np.float32(3.0e38)).all() and s[4] == np.float32(-3.0e38)


def test_host_any_sample_covered_against_brute_force():
    c, h, lo, hi, off, cnt = K.cover_cases()
    assert c.size > 40000          # the full cross product of the listed sets
    ref = K.cover_reference(c, h, lo, cnt)
    assert 0.2 < ref.mean() < 0.8                      # both verdicts are well populated
    got = K.cover(c, h, lo, hi, off, host=True)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, [(c[i], h[i], lo[i], hi[i], off[i], got[i], ref[i]) for i in bad[:5]]


def test_host_div255_is_the_ieee_quotient():
    out = np.empty(256, np.float32)
    K.probe().probe_host_div255(out.ctypes.data)
    assert (out.view(np.uint32) == (np.arange(256, dtype=np.float32) / np.float32(255.0)).view(np.uint32)).all()


def test_fragment_cases_populate_every_branch():
    # what tests/test_gpu_device_math.py asserts before it trusts its comparison, checked here with the oracle alone
    sxy, ra, rb = K.fragment_cases(1 << 20)
    alpha, cov = O.fragment_n(sxy, ra, rb)
    shares = K.fragment_branch_shares(sxy, ra, rb, alpha, cov)
    print(shares)
    assert min(shares.values()) >= 0.01, shares
    # the constructed opacities land ON the thresholds: alpha exactly 1/255 (accepted) and one place below (rejected) both occur
    assert (alpha == K.T255).sum() > 1000 and (alpha == np.float32(0.99)).sum() > 1000
