"""The compositor's device functions (splat_amd/csrc/splat_device_math.h), each run alone on the GPU by the probe library
(tests/native/device_math_probe.hip) and held to a reference that shares no code with it: glibc's expf and the committed
oracle's fragment() / blend() (oracle/splat_oracle.cpp), numpy in float64, brute force.  Exhaustive where the input space
allows it -- every float in [-87, -0] for the exponentials, all 256 states for blend() -- and built to sit on the branches
where it does not.  One process, one probe handle; a missing probe library fails.

may_contribute is NOT here: lifted out of the compositor into the header it compiled to commuted multiplies (same
results, different instructions), so it stays a lambda of the kernel, and a copy would test nothing.

What was measured goes to profiles/device_math_sweep.json (SPLAT_DEVICE_MATH_SWEEP=<path> writes it)."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_math_cases as K  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = {}


def _record(key, value):
    SWEEP[key] = value
    path = os.environ.get("SPLAT_DEVICE_MATH_SWEEP")
    if path:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            head = ""
        with open(path, "w") as f:
            json.dump(dict(commit=head or os.environ.get("SPLAT_COMMIT", "working tree"), **SWEEP), f, indent=1, sort_keys=True)


def _same_bits(a, b):
    """equal as uint32, NaN matching NaN"""
    af, bf = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(af) & np.isnan(bf))


def test_probe_sees_a_gpu():
    import ctypes
    n = ctypes.c_int(0)
    assert K.probe().probe_device_count(ctypes.byref(n)) == 0 and n.value >= 1


def test_exp_libm_is_glibc_expf_on_every_argument():
    """Every one of the 1 118 699 521 arguments.  (This is the test that found exp_libm's reduction residual one product
    rounding away from glibc's FMA build: bits 0xc27c65d9, 0x11fa2992 against expf's 0x11fa2993, host and device alike.)"""
    # a.  every float in [-87, -0] and +0: the device result IS expf's, as uint32
    wrong = []
    for first, n in K.chunks(K.NEG_FIRST, K.NEG_LAST):
        got, ref = K.dev_exp(1, first, n), O.expf_n(first, n)
        wrong += [(hex(first + i), hex(got[i]), hex(ref[i])) for i in np.flatnonzero(got != ref)[:100]]
    print("exp_libm != expf at %d arguments (bits, exp_libm, expf): %r" % (len(wrong), wrong[:20]))
    assert not wrong, "%d arguments differ from expf (bits, exp_libm, expf): %r" % (len(wrong), wrong[:8])
    assert K.dev_exp(1, bits=[0])[0] == O.expf_n(bits=[0])[0]
    assert np.isnan(K.dev_exp(1, bits=[0x7FC00000, 0xFFC00000, 0x7F800001]).view(np.float32)).all()
    # below -87: expf(-87) by design (the clamp; the opacity precondition of splat_upload_scene is what makes it harmless)
    e87 = O.expf_n(bits=[K.NEG_LAST])[0]
    low = np.concatenate([K.below_minus_87(), np.array([0xFF800000], np.uint32)])
    assert (K.dev_exp(1, bits=low) == e87).all()
    # the host compile of the same text gives the same bits there
    assert (K.host_exp_libm(bits=low) == e87).all()


def _ulp_stats(args):
    first, dev, ref = args
    x = np.arange(first, first + dev.size, dtype=np.uint32).view(np.float32).astype(np.float64)
    t = np.exp(x)
    ulp = np.spacing(t.astype(np.float32)).astype(np.float64)
    err = np.abs(dev.view(np.float32).astype(np.float64) - t) / ulp
    eref = np.abs(ref.view(np.float32).astype(np.float64) - t) / ulp
    i = int(err.argmax())
    return float(err[i]), first + i, float(eref.max())


def test_exp_neg_is_within_one_last_place_of_expf_on_every_argument():
    # b.  The claim (README, the kernel's comment): the exponential's last place is the only thing the default mode rounds
    # differently -- so exp_neg differs from expf by at most ONE unit in the last place, everywhere on [-87, -0].
    rng = np.random.default_rng(21)
    ops = np.concatenate([np.array([1.0, 0.99, 0.5], np.float32), K.T255.reshape(1),
                          K.nextafter32(K.T255, True).reshape(1), K.nextafter32(K.T255, False).reshape(1),
                          (K.T255.view(np.uint32) + np.array([2, 3], np.uint32)).view(np.float32),
                          rng.uniform(1.0 / 255, 1.0, 56).astype(np.float32)])[:64]
    assert ops.size == 64
    # arguments where an accept flip is possible at all: within 1e-3 of log(1 / (255 op)) -- given the one-unit bound
    # asserted below, op * e moves by ~1e-7 relative, a window of 1e-3 in the argument is ten thousand times that
    xt = -np.log(255.0 * ops.astype(np.float64))
    w_lo = np.minimum(xt + 1e-3, -0.0).astype(np.float32).view(np.uint32).astype(np.int64)      # smaller magnitude = smaller bits
    w_hi = (xt - 1e-3).astype(np.float32).view(np.uint32).astype(np.int64)
    hist = {-1: 0, 0: 0, 1: 0}
    worst, worst_bits, worst_ref = 0.0, 0, 0.0
    flips = np.zeros(64, np.int64)
    t255_bits = int(K.T255.view(np.uint32))
    with ThreadPoolExecutor(8) as pool:
        for first, n in K.chunks(K.NEG_FIRST, K.NEG_LAST):
            dev, ref = K.dev_exp(0, first, n), O.expf_n(first, n)
            d = dev.view(np.int32) - ref.view(np.int32)            # all results are normal, positive floats here
            over = np.flatnonzero(np.abs(d) > 1)
            assert over.size == 0, "%d arguments off by more than one unit, first bits 0x%08x: exp_neg 0x%08x expf 0x%08x" % (
                over.size, first + over[0], dev[over[0]], ref[over[0]])
            for v in (-1, 0, 1):
                hist[v] += int((d == v).sum())
            step = 1 << 22
            for e, b, r in pool.map(_ulp_stats, [(first + s, dev[s:s + step], ref[s:s + step]) for s in range(0, n, step)]):
                if e > worst:
                    worst, worst_bits = e, b
                worst_ref = max(worst_ref, r)
            # accept flips: only where the two exponentials differ
            idx = np.flatnonzero(d != 0)
            mb = idx.astype(np.int64) + first
            for j, op in enumerate(ops):
                if xt[j] - 1e-3 > 0:
                    continue
                i0, i1 = np.searchsorted(mb, [w_lo[j], w_hi[j] + 1])
                if i0 == i1:
                    continue
                ed, er = dev[idx[i0:i1]].view(np.float32), ref[idx[i0:i1]].view(np.float32)
                pd, pr = (op * ed).astype(np.float32), (op * er).astype(np.float32)
                acc_d = ~(np.minimum(np.float32(0.99), pd) < K.T255)
                acc_r = ~(np.minimum(np.float32(0.99), pr) < K.T255)
                fl = acc_d != acc_r
                flips[j] += int(fl.sum())
                # what the one-unit bound implies: a flip needs op * expf(x) within 2 ulps of 1/255
                assert (np.abs(pr[fl].view(np.int32).astype(np.int64) - t255_bits) <= 2).all(), (float(op), pr[fl][:4])
    total = sum(hist.values())
    assert total == K.NEG_LAST - K.NEG_FIRST + 1
    print("exp_neg - expf in units of the last place: %r of %d; worst error vs float64 exp: %.4f ulp at x = %r (expf's worst: %.4f ulp)"
          % (hist, total, worst, float(np.uint32(worst_bits).view(np.float32)), worst_ref))
    print("accept flips per opacity:", dict(zip([float(o) for o in ops], flips.tolist())))
    _record("exp_neg", dict(arguments=total, minus_one=hist[-1], equal=hist[0], plus_one=hist[1],
                            worst_ulp_vs_float64=worst, worst_argument=float(np.uint32(worst_bits).view(np.float32)),
                            worst_argument_bits="0x%08x" % worst_bits, expf_worst_ulp_vs_float64=worst_ref,
                            accept_flips={"%.9g" % float(o): int(f) for o, f in zip(ops, flips)},
                            accept_flips_total=int(flips.sum())))


def test_packed_exp_neg_is_the_scalar_exp_neg():
    # c.  both components of exp_neg2 == exp_neg bit for bit: the whole of [-87, -0], then 2^24 arbitrary bit patterns
    for first, n in K.chunks(K.NEG_FIRST, K.NEG_LAST):
        s = K.dev_exp(0, first, n)
        for which in (2, 3):
            bad = np.flatnonzero(~_same_bits(K.dev_exp(which, first, n), s))
            assert bad.size == 0, (which, "0x%08x" % (first + bad[0]))
    rng = np.random.default_rng(22)
    bits = np.concatenate([rng.integers(0, 1 << 32, (1 << 24) - 8, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x80000001, 0x7F7FFFFF], np.uint32)])
    s = K.dev_exp(0, bits=bits)
    for which in (2, 3):
        bad = np.flatnonzero(~_same_bits(K.dev_exp(which, bits=bits), s))
        assert bad.size == 0, (which, "0x%08x" % bits[bad[0]])


def _fragment(sxy, ra, rb, libm, pair):
    n = sxy.shape[0]
    alpha, cov = np.empty(n, np.float32), np.empty(n, np.uint8)
    rc = K.probe().probe_fragment(n, sxy.ctypes.data, ra.ctypes.data, rb.ctypes.data, libm, pair, alpha.ctypes.data, cov.ctypes.data)
    assert rc == 0, "probe_fragment: HIP error %d" % rc
    return alpha, cov


def test_fragment_alpha_is_the_reference_fragment():
    # d.  2^22 tuples built to sit on the branches (tests/device_math_cases.py)
    sxy, ra, rb = K.fragment_cases(1 << 22)
    ref, rcov = O.fragment_n(sxy, ra, rb)
    shares = K.fragment_branch_shares(sxy, ra, rb, ref, rcov)
    print(shares)
    assert min(shares.values()) >= 0.01, shares                # every branch is populated, by the oracle's account
    # with the libm exponential: the oracle's alpha bit for bit, the same coverage
    a1, c1 = _fragment(sxy, ra, rb, 1, 0)
    bad = np.flatnonzero((a1.view(np.uint32) != ref.view(np.uint32)) | (c1 != rcov))
    assert bad.size == 0, [(sxy[i], ra[i], rb[i], a1[i], ref[i], c1[i], rcov[i]) for i in bad[:3]]
    # with exp_neg: what one unit in the exponential's last place allows, and nothing else
    a0, c0 = _fragment(sxy, ra, rb, 0, 0)
    assert (c0 == rcov).all()
    t = int(K.T255.view(np.uint32))
    acc0, accr = a0 != 0, ref != 0
    flip = np.flatnonzero(acc0 != accr)
    both = np.where(acc0, a0, ref)                              # the alpha of whichever side accepted
    assert (np.abs(both[flip].view(np.int32).astype(np.int64) - t) <= 2).all(), [(rb[i], a0[i], ref[i]) for i in flip[:3]]
    m = acc0 & accr
    assert (np.abs(a0[m].view(np.int32).astype(np.int64) - ref[m].view(np.int32)) <= 2).all()
    capped = m & (ref == np.float32(0.99)) & (a0 == np.float32(0.99))
    off_cap = m & ((ref == np.float32(0.99)) != (a0 == np.float32(0.99)))
    assert capped.sum() > 1000
    # (one side capped, the other not: only within 2 ulps below 0.99)
    assert (np.abs(np.minimum(a0, ref)[off_cap].view(np.int32).astype(np.int64) - int(np.float32(0.99).view(np.uint32))) <= 2).all()
    print("exp_neg vs libm fragment: %d accept flips, %d alphas differ of %d accepted by both" % (flip.size, int((a0[m] != ref[m]).sum()), int(m.sum())))
    # c.  the packed fragment is the scalar one, both components
    for pair in (1, 2):
        ap, _ = _fragment(sxy, ra, rb, 0, pair)
        bad = np.flatnonzero(~_same_bits(ap.view(np.uint32), a0.view(np.uint32)))
        assert bad.size == 0, (pair, [(sxy[i], ra[i], rb[i], ap[i], a0[i]) for i in bad[:3]])


def test_blend_channel_is_the_reference_blend_for_every_state():
    # e.  all 256 states x (0, every alpha in [1/255, 1/255 + 2^-12] and [0.99 - 2^-12, 0.99], 2^16 seeded between) x 21 colours
    dev255 = np.empty(256, np.float32)
    assert K.probe().probe_div255(dev255.ctypes.data) == 0
    assert (dev255.view(np.uint32) == (np.arange(256, dtype=np.float32) / np.float32(255.0)).view(np.uint32)).all()
    alphas = K.blend_alphas(1 << 16)
    colours = K.blend_colours()
    assert alphas.size > (1 << 19) + 4096 + (1 << 16) and colours.size == 21
    step = 1 << 16
    for c3 in range(0, 21, 3):                                  # the oracle blends three channels at a time
        cs = colours[c3:c3 + 3]
        for s in range(0, alphas.size, step):
            al = np.ascontiguousarray(alphas[s:s + step])
            ref = O.blend_n(al, np.ascontiguousarray(np.broadcast_to(cs, (al.size, 3)), dtype=np.float32))
            assert ((ref >> 24) == (ref[:, :1] >> 24)).all()
            for ch, shift in enumerate((16, 8, 0)):
                col = np.full(al.size, cs[ch], np.float32)
                want = ((ref >> shift) & 255).astype(np.uint8)
                outs = []
                for pair in (0, 1, 2):
                    out = np.empty((al.size, 256), np.uint8)
                    rc = K.probe().probe_blend(al.size, al.ctypes.data, col.ctypes.data, pair, out.ctypes.data)
                    assert rc == 0, "probe_blend: HIP error %d" % rc
                    outs.append(out)
                bad = np.argwhere(outs[0] != want)
                assert bad.size == 0, "alpha %r colour %r state %d: device %d, reference %d" % (
                    al[bad[0][0]], cs[ch], bad[0][1], outs[0][tuple(bad[0])], want[tuple(bad[0])])
                # the two lemmas of the early-outs, on the DEVICE bytes: monotone in the state, never expanding
                dd = np.diff(outs[0].astype(np.int16), axis=1)
                assert dd.min() >= 0 and dd.max() <= 1, (cs[ch], int(dd.min()), int(dd.max()))
                # c.  blend_channel2 == blend_channel, both components
                assert (outs[1] == outs[0]).all() and (outs[2] == outs[0]).all(), cs[ch]


def test_any_sample_covered_against_brute_force():
    # f.  blocks x centres x half extents, the full cross product; device and host compile
    c, h, lo, hi, off, cnt = K.cover_cases()
    ref = K.cover_reference(c, h, lo, cnt)
    for host in (False, True):
        got = K.cover(c, h, lo, hi, off, host=host)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (host, [(c[i], h[i], lo[i], hi[i], off[i], got[i], ref[i]) for i in bad[:5]])
