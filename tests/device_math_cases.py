"""Shared by tests/test_device_math_host.py and tests/test_gpu_device_math.py: the handle of the probe library
(tests/native/libdevice_math_probe.so, built by splat_amd/csrc/Makefile from tests/native/device_math_probe.hip) and the
input sets that both files use.  Nothing here knows what the functions under test should return."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (SPLAT_DEVICE_MATH_PROBE: another build of the probe, e.g. of a deliberately broken header, to see these tests fail)
PROBE_PATH = os.environ.get("SPLAT_DEVICE_MATH_PROBE") or os.path.join(HERE, "native", "libdevice_math_probe.so")

# every float in [-87, -0]: the bit patterns 0x80000000 .. 0xC2AE0000
NEG_FIRST, NEG_LAST = 0x80000000, 0xC2AE0000
CHUNK = 1 << 26
T255 = np.float32(1.0) / np.float32(255.0)

_PROBE = None


def probe():
    """The probe library; a missing one is a failure (build() makes it), never a skip."""
    global _PROBE
    if _PROBE is None:
        assert os.path.exists(PROBE_PATH), "%s is missing: make -C splat_amd/csrc all builds it" % PROBE_PATH
        L = C.CDLL(PROBE_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.probe_device_count.argtypes = [C.POINTER(C.c_int)]
        L.probe_exp.argtypes = [i32, u32, vp, u64, vp]
        L.probe_blend.argtypes = [u64, vp, vp, i32, vp]
        L.probe_div255.argtypes = [vp]
        L.probe_fragment.argtypes = [u64, vp, vp, vp, i32, i32, vp, vp]
        L.probe_cover.argtypes = [u64, vp, vp, vp, vp, vp, vp]
        L.probe_host_exp_libm.argtypes = [u32, vp, u64, vp, i32]
        L.probe_host_reject_threshold.argtypes = [u32, vp, u64, vp, i32]
        L.probe_host_cover.argtypes = [u64, vp, vp, vp, vp, vp, vp, i32]
        L.probe_host_div255.argtypes = [vp]
        for f in ("probe_host_exp_libm", "probe_host_reject_threshold", "probe_host_cover", "probe_host_div255"):
            getattr(L, f).restype = None
        _PROBE = L
    return _PROBE


def chunks(first, last, size=CHUNK):
    """(first bit pattern, count) pieces of the inclusive range [first, last]"""
    b = first
    while b <= last:
        n = min(size, last - b + 1)
        yield b, n
        b += n


def _p(a):
    assert a.flags.c_contiguous
    return a.ctypes.data


def host_exp_libm(first=0, n=0, bits=None, nthreads=16):
    if bits is not None:
        bits = np.ascontiguousarray(bits, np.uint32)
        n = bits.size
    out = np.empty(n, np.uint32)
    probe().probe_host_exp_libm(first, _p(bits) if bits is not None else None, n, _p(out), nthreads)
    return out


def host_reject_threshold(first=0, n=0, bits=None, nthreads=16):
    if bits is not None:
        bits = np.ascontiguousarray(bits, np.uint32)
        n = bits.size
    out = np.empty(n, np.float32)
    probe().probe_host_reject_threshold(first, _p(bits) if bits is not None else None, n, _p(out), nthreads)
    return out


def dev_exp(which, first=0, n=0, bits=None):
    """which: 0 exp_neg, 1 exp_libm, 2 / 3 exp_neg2 component x / y"""
    if bits is not None:
        bits = np.ascontiguousarray(bits, np.uint32)
        n = bits.size
    out = np.empty(n, np.uint32)
    rc = probe().probe_exp(which, first, _p(bits) if bits is not None else None, n, _p(out))
    assert rc == 0, "probe_exp: HIP error %d" % rc
    return out


def cover(c, h, lo, hi, off, host):
    n = c.size
    out = np.empty(n, np.uint8)
    a = [np.ascontiguousarray(v, np.float32) for v in (c, h, lo, hi, off)]
    if host:
        probe().probe_host_cover(n, *[_p(v) for v in a], _p(out), 16)
    else:
        for s in range(0, n, CHUNK):
            e = min(n, s + CHUNK)
            rc = probe().probe_cover(e - s, *[_p(v[s:e]) for v in a], _p(out[s:e]))
            assert rc == 0, "probe_cover: HIP error %d" % rc
    return out


def below_minus_87(n=1 << 20, seed=11):
    """n arguments below -87: its neighbours, a dense run next to it, seeded ones down to -FLT_MAX"""
    rng = np.random.default_rng(seed)
    near = np.arange(NEG_LAST + 1, NEG_LAST + 1 + n // 2, dtype=np.uint32)
    far = rng.integers(NEG_LAST + 1, 0xFF7FFFFF, n - n // 2 - 2, dtype=np.uint32, endpoint=True)
    return np.concatenate([near, far, np.array([0xFF7FFFFF, 0xC2D00000], np.uint32)])       # -FLT_MAX, -104


def nextafter32(x, up):
    x = np.asarray(x, np.float32)
    return np.nextafter(x, np.float32(np.inf if up else -np.inf), dtype=np.float32)


def cover_cases():
    """The full cross product of blocks x centres x half extents for any_sample_covered (arguments as the compositor
    passes them: lo / hi are the block's first and last SAMPLE, off already added).  Returns c, h, lo, hi, off, count."""
    C_, H_, LO, HI, OFF, CNT = [], [], [], [], [], []
    big = np.float32(3.0e38)
    for lo_px in (0, 8, 4088, 16376):
        for width in range(1, 9):
            for off in (0.0, 0.5):
                s = (np.arange(width, dtype=np.float32) + np.float32(lo_px) + np.float32(off)).astype(np.float32)
                mids = (s[:-1] + np.float32(0.5)).astype(np.float32)
                cs = np.concatenate([s, nextafter32(s, True), nextafter32(s, False),
                                     mids, nextafter32(mids, True), nextafter32(mids, False),
                                     np.array([s[0] - 1, s[0] - 0.5, s[-1] + 0.5, s[-1] + 1, s[0] - 1000, s[-1] + 1000, -1e30, 1e30,
                                               -np.inf, np.inf, np.nan], np.float32)])
                for c in cs:
                    d = np.abs(s - c).astype(np.float32) if np.isfinite(c) else np.zeros(0, np.float32)   # exact distances, f32 as the kernel forms them
                    d = d[np.isfinite(d)]
                    hs = np.concatenate([np.array([0.0, -1.0, 0.5, 1e30, np.inf, np.nan], np.float32),
                                         d, nextafter32(d, True), nextafter32(d, False)])
                    C_.append(np.full(hs.size, c, np.float32)); H_.append(hs)
                    LO.append(np.full(hs.size, s[0], np.float32)); HI.append(np.full(hs.size, s[-1], np.float32))
                    OFF.append(np.full(hs.size, off, np.float32)); CNT.append(np.full(hs.size, width, np.int32))
    del big
    return tuple(np.concatenate(v) for v in (C_, H_, LO, HI, OFF, CNT))


def cover_reference(c, h, lo, cnt):
    """brute force, float32: any(|lo + k - c| <= h for k in 0 .. cnt-1)"""
    any_ = np.zeros(c.size, bool)
    with np.errstate(invalid="ignore"):
        for k in range(8):
            s = (lo + np.float32(k)).astype(np.float32)
            any_ |= (k < cnt) & (np.abs((s - c).astype(np.float32)) <= h)
    return any_.astype(np.uint8)


def blend_colours():
    """the colours of tests/test_oracle_kat.py's monotonicity lemma: in range, out of range, what K1 stores for +-inf / NaN"""
    rng = np.random.default_rng(5)
    fmax = np.finfo(np.float32).max
    return np.concatenate([np.array([0.0, 1.0, 0.5, -0.25, 1.75, 1e30, -1e30, fmax, -fmax], np.float32),
                           rng.uniform(-0.2, 1.2, 12).astype(np.float32)])


def blend_alphas(n_seeded=1 << 16):
    """0, every float in [1/255, 1/255 + 2^-12] and [0.99 - 2^-12, 0.99], n_seeded in between"""
    rng = np.random.default_rng(6)
    a0 = T255.view(np.uint32)
    a1 = np.float32(T255 + np.float32(2.0 ** -12)).view(np.uint32)
    b1 = np.float32(0.99).view(np.uint32)
    b0 = np.float32(np.float32(0.99) - np.float32(2.0 ** -12)).view(np.uint32)
    lo = np.arange(a0, a1 + 1, dtype=np.uint32).view(np.float32)
    hi = np.arange(b0, b1 + 1, dtype=np.uint32).view(np.float32)
    mid = rng.uniform(lo[-1], hi[0], n_seeded).astype(np.float32)
    return np.concatenate([np.zeros(1, np.float32), lo, mid, hi])


def fragment_cases(n=1 << 22, seed=3):
    """Tuples (sample, record) that sit ON the branches of fragment(): samples on the rectangle's edge and a last place
    either side, power of -0 / +0 / just above 0, opacity * e on 0.99 and on 1/255 and their neighbours (opacity built
    from glibc's expf of the tuple's power: the oracle's own exponential), hostile opacities, NaN samples.
    Returns sxy[n,2], ra[n,4] (cx cy hx hy), rb[n,4] (A B C opacity)."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    f32 = np.float32
    cx = rng.uniform(0, 4096, n).astype(f32); cy = rng.uniform(0, 4096, n).astype(f32)
    sx = (np.floor(rng.uniform(0, 4096, n)) + 0.5).astype(f32); sy = (np.floor(rng.uniform(0, 4096, n)) + 0.5).astype(f32)
    kind = rng.integers(0, 16, n)
    # centres within a few pixels of the sample, so that power is a usable exponent
    near = kind != 15
    cx = np.where(near, (sx + rng.normal(0, 2.0, n)).astype(f32), cx); cy = np.where(near, (sy + rng.normal(0, 2.0, n)).astype(f32), cy)
    dx = (sx - cx).astype(f32); dy = (cy - sy).astype(f32)
    hx = (np.abs(dx) + rng.uniform(0, 4, n)).astype(f32); hy = (np.abs(dy) + rng.uniform(0, 4, n)).astype(f32)
    # conics: positive definite, moderate
    s1 = rng.uniform(0.5, 6.0, n); s2 = rng.uniform(0.5, 6.0, n); th = rng.uniform(0, np.pi, n)
    c_, s_ = np.cos(th), np.sin(th)
    A = (c_ * c_ / s1 ** 2 + s_ * s_ / s2 ** 2).astype(f32); Cc = (s_ * s_ / s1 ** 2 + c_ * c_ / s2 ** 2).astype(f32)
    B = (c_ * s_ * (1 / s1 ** 2 - 1 / s2 ** 2)).astype(f32)
    op = rng.uniform(1.0 / 255, 1.0, n).astype(f32)
    # kinds 0..2: the rectangle's edge: |dx| == hx exactly, one last place inside, one last place outside (x or y)
    for k, fn in ((0, lambda v: v), (1, lambda v: nextafter32(v, True)), (2, lambda v: nextafter32(v, False))):
        m = kind == k
        onx = m & (rng.integers(0, 2, n) == 0)
        hx = np.where(onx, fn(np.abs(dx)), hx).astype(f32); hy = np.where(m & ~onx, fn(np.abs(dy)), hy).astype(f32)
    # kinds 3, 4: power > 0 -- non-definite conics (K1's low-pass-0 case): from far above 0 down to the smallest positive
    m = (kind == 3) | (kind == 4)
    A = np.where(m, -A * rng.choice([1.0, 1e-3, 1e-10, 1e-30, 1e-38], n).astype(f32), A).astype(f32)
    Cc = np.where(m, -Cc * rng.choice([1.0, 1e-3, 1e-10, 1e-30, 1e-38], n).astype(f32), Cc).astype(f32)
    B = np.where(m, 0, B).astype(f32)
    # kind 5: power exactly -0 / +0: the sample on the centre, or a zero conic of either sign
    m = kind == 5
    z = rng.integers(0, 3, n)
    cx = np.where(m & (z == 0), sx, cx); cy = np.where(m & (z == 0), sy, cy)
    A = np.where(m & (z == 1), 0.0, A).astype(f32); Cc = np.where(m & (z == 1), 0.0, Cc).astype(f32); B = np.where(m & (z == 1), 0.0, B).astype(f32)
    A = np.where(m & (z == 2), -0.0, A).astype(f32); Cc = np.where(m & (z == 2), -0.0, Cc).astype(f32); B = np.where(m & (z == 2), -0.0, B).astype(f32)
    # the tuple's power as fragment() forms it (float32, in this order), and glibc's exponential of it
    dx = (sx - cx).astype(f32); dy = (cy - sy).astype(f32)
    with np.errstate(all="ignore"):
        power = (f32(-0.5) * ((A * dx * dx).astype(f32) + (Cc * dy * dy).astype(f32)).astype(f32) - ((B * dx).astype(f32) * dy).astype(f32)).astype(f32)
        e = O.expf_n(bits=power.view(np.uint32)).view(f32)
        # kinds 6..8: opacity * e on 1/255, kinds 9..11: on 0.99; the quotient, then -3 .. +3 last places around it
        for k0, target in ((6, T255), (9, f32(0.99))):
            # (exponents of -87 and above only: below it the quotient leaves the opacities splat_upload_scene's
            # precondition admits, ~2.4e35, where exp_libm's clamp shows -- measured: 7 of 2^22 tuples, alpha 0.214 vs 1/255)
            m = (kind >= k0) & (kind < k0 + 3) & (e > 0) & np.isfinite(e) & (power >= f32(-87.0))
            q = (target / e).astype(f32)
            step = rng.integers(-3, 4, n)
            qb = (q.view(np.int32) + step.astype(np.int32)).view(f32)
            op = np.where(m & np.isfinite(q), qb, op).astype(f32)
    # kind 12: hostile opacities
    m = kind == 12
    op = np.where(m, rng.choice(np.array([0.0, -0.0, -1.0, -1e30, 1.5, 255.0, 1e30, np.inf, -np.inf, np.nan], f32), n), op).astype(f32)
    # kind 13: samples off the target (NaN coordinates)
    m = kind == 13
    sx = np.where(m & (rng.integers(0, 2, n) == 0), np.nan, sx).astype(f32); sy = np.where(m & np.isfinite(sx), np.nan, sy).astype(f32)
    # kind 14: plain tuples (accepted, uncapped or capped by chance); kind 15: far away (coverage rejects)
    sxy = np.ascontiguousarray(np.stack([sx, sy], 1), f32)
    ra = np.ascontiguousarray(np.stack([cx, cy, hx, hy], 1), f32)
    rb = np.ascontiguousarray(np.stack([A, B, Cc, op], 1), f32)
    return sxy, ra, rb


def fragment_branch_shares(sxy, ra, rb, alpha, cov):
    """shares of the five outcomes, from the oracle's outputs (alpha, cov) and the inputs alone"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        dx = (sxy[:, 0] - ra[:, 0]).astype(f32); dy = (ra[:, 1] - sxy[:, 1]).astype(f32)
        power = (f32(-0.5) * ((rb[:, 0] * dx * dx).astype(f32) + (rb[:, 2] * dy * dy).astype(f32)).astype(f32) - ((rb[:, 1] * dx).astype(f32) * dy).astype(f32)).astype(f32)
    c = cov != 0
    n = float(len(alpha))
    return dict(uncovered=(~c).sum() / n, positive_power=(c & (power > 0)).sum() / n,
                below_threshold=(c & ~(power > 0) & (alpha == 0)).sum() / n,
                capped=(c & (alpha == f32(0.99))).sum() / n, accepted=(c & (alpha > 0) & (alpha < f32(0.99))).sum() / n)
