"""A PLY loaded on the GPU (splat_decode_ply_device / splat_upload_ply_device, -m gpu).  The host loader is the
specification, bit for bit: every comparison is against splat_amd.load_from_ply (then compute_cov3d and upload), never
against the code under test.  The activations are held to glibc's expf on the device compile as well.

Sizes.  ply_decode_kernel takes 256 rows per workgroup at the strides used here (248, 251, 253: 64 KiB of staging holds
more than 256 of them), recentre_sum_kernel walks chunks of 2048 positions.  n = 255 / 256 / 257 is one less than, equal
to and one more than a decode workgroup's rows; 4097 is one more than two chunks of the sum; 1 and 65537 are the ends."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ply_cases as P  # noqa: E402

import splat_amd  # noqa: E402
from splat_amd import _lib  # noqa: E402
from splat_amd.gaussians import PLY_PROPS  # noqa: E402
from helpers import make_camera  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_head.ply")
INRIA = [("float", p) for p in PLY_PROPS]
FIELDS = (("positions", 4), ("scales", 3), ("opacities", 1), ("rotations", 4), ("sh", 48))


@contextlib.contextmanager
def renderer():
    R = splat_amd.Renderer()
    try:
        yield R
    finally:
        R.close()


@pytest.fixture(scope="module")
def R():
    with renderer() as r:
        yield r


# ---- the device compile of expf_libm_full and the sigmoid ------------------------------------------------------------
def math_sets():
    inf = np.arange(0x7F800000 - (1 << 16), 0x7F800000 + (1 << 16) + 1, dtype=np.uint32)     # ... +inf, then NaNs
    sets = [P.around(x) for x in (0.0, -0.0, P.OFLOW, -P.OFLOW, P.UFLOW, P.NORMAL_EDGE)] + [inf, inf | np.uint32(0x80000000)]
    n = -(-(1 << 32) // 251)
    sets.append(np.arange(n, dtype=np.uint32) * np.uint32(251))                               # every 251st of all 2^32 patterns
    assert int(sets[-1][-1]) + 251 >= 1 << 32 and n > 17_000_000
    return sets


@pytest.mark.parametrize("which", [0, 1], ids=["expf_libm_full", "sigmoid"])
def test_device_activations_are_glibc_bit_for_bit(which):
    for bits in math_sets():
        got = np.concatenate([P.run(which, False, bits=bits[s:s + P.CHUNK]) for s in range(0, bits.size, P.CHUNK)])
        ref = O.expf_n(bits=bits) if which == 0 else P.sigmoid_reference(O, bits)
        nan_in = np.isnan(bits.view(f32))
        assert np.isnan(got.view(f32))[nan_in].all(), "NaN did not stay NaN"
        bad = np.flatnonzero(~P.same_bits(got, ref))
        assert bad.size == 0, "%d of %d arguments differ, first bits 0x%08x: device 0x%08x glibc 0x%08x" % (
            bad.size, bits.size, bits[bad[0]], got[bad[0]], ref[bad[0]])
    # the sets are what they claim: results on both sides of both thresholds and of the normal / subnormal boundary
    e = O.expf_n(bits=P.around(P.UFLOW)).view(f32)
    assert (e == 0).any() and (e > 0).any()
    e = O.expf_n(bits=P.around(P.OFLOW)).view(f32)
    assert np.isinf(e).any() and np.isfinite(e).any()
    e = O.expf_n(bits=P.around(P.NORMAL_EDGE)).view(f32)
    assert (e < np.finfo(f32).tiny).any() and (e >= np.finfo(f32).tiny).any()


# ---- decode identity -------------------------------------------------------------------------------------------------
def decode_on_device(R, path, shift=0):
    """the file's payload placed `shift` bytes into a device allocation -> decode_ply_device -> the five arrays"""
    pl = splat_amd.ply_layout(path)
    assert pl.binary
    n = pl.n
    payload = np.fromfile(path, np.uint8, count=pl.payload_bytes, offset=pl.payload_offset)
    assert payload.size == pl.payload_bytes == n * pl.stride
    held = []

    def alloc(nbytes):
        p = R._L.splat_device_alloc(R._h, max(nbytes, 4))
        assert p
        held.append(p)
        return p
    try:
        d_rows = alloc(payload.size + 8)
        if payload.size:
            R._check(R._L.splat_device_upload(R._h, C.c_void_p(d_rows + shift), C.c_void_p(payload.ctypes.data), payload.size))
        outs = [alloc(4 * per * n) for _, per in FIELDS]
        R.decode_ply_device(d_rows + shift, pl, *outs)
        got = {}
        for (name, per), p in zip(FIELDS, outs):
            a = np.zeros(n * per, f32)
            if a.size:
                R._check(R._L.splat_device_download(R._h, C.c_void_p(a.ctypes.data), C.c_void_p(p), a.nbytes))
            got[name] = a
    finally:
        for p in held:
            R.device_free(p)
    return got


def assert_same_arrays(got, g, what, nan_equal=False):
    for name, per in FIELDS:
        ref = np.ascontiguousarray(getattr(g, name)).reshape(-1)
        assert got[name].shape == ref.shape, (what, name)
        same = P.same_bits(got[name], ref) if nan_equal else (got[name].view(np.uint32) == ref.view(np.uint32))
        bad = np.flatnonzero(~same)
        assert bad.size == 0, "%s: %s differs in %d of %d floats, first at Gaussian %d component %d: device %r (0x%08x) host %r (0x%08x)" % (
            what, name, bad.size, ref.size, bad[0] // per, bad[0] % per, got[name][bad[0]], got[name].view(np.uint32)[bad[0]],
            ref[bad[0]], ref.view(np.uint32)[bad[0]])


def inria_file(tmp_path, n, seed):
    path = str(tmp_path / ("inria_%d.ply" % n))
    splat_amd.write_ply(path, splat_amd.synthetic_raw(n, seed), n)
    return path


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 65537])
def test_decode_identity_stride_248_aligned(R, tmp_path, n):
    path = inria_file(tmp_path, n, 100 + n % 97)
    assert splat_amd.ply_layout(path).stride == 248
    assert_same_arrays(decode_on_device(R, path), splat_amd.load_from_ply(path), "n=%d" % n)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_decode_identity_payload_at_odd_device_addresses(R, tmp_path, shift):
    path = inria_file(tmp_path, 4097, 7)
    assert_same_arrays(decode_on_device(R, path, shift), splat_amd.load_from_ply(path), "shift %d" % shift)


def strided_props(stride):
    """uchar properties before and between the floats: 251 = 248 + 3, 253 = 248 + 5"""
    extra = stride - 248
    props = [("uchar", "red")] + INRIA[:5] + [("uchar", "green")] + INRIA[5:30] + [("uchar", "blue")] + INRIA[30:]
    props += [("uchar", "pad%d" % k) for k in range(extra - 3)]
    if extra > 3:                                            # the pads go between floats as well
        props = props[:40] + props[-(extra - 3):] + props[40:-(extra - 3)]
    return props


@pytest.mark.parametrize("stride,n", [(251, 257), (251, 4097), (253, 256), (253, 4097)])
def test_decode_identity_odd_strides(R, tmp_path, stride, n):
    props = strided_props(stride)
    path = str(tmp_path / "odd.ply")
    dt = P.write_ply_props(path, props, n, splat_amd.synthetic_raw(n, 11), seed=stride)
    pl = splat_amd.ply_layout(path)
    assert pl.stride == stride == dt.itemsize and pl.layout.offset[0] == 1 and len(pl.offsets()) == 59
    assert len({o % 4 for o in pl.offsets().values()}) >= 2  # floats at more than one misalignment within a row
    for shift in (0, 3):
        assert_same_arrays(decode_on_device(R, path, shift), splat_amd.load_from_ply(path), "stride %d n %d shift %d" % (stride, n, shift))


def test_decode_identity_shuffled_property_order(R, tmp_path):
    props = [INRIA[k] for k in np.random.default_rng(5).permutation(len(INRIA))]
    path = str(tmp_path / "shuffled.ply")
    P.write_ply_props(path, props, 4097, splat_amd.synthetic_raw(4097, 12))
    assert_same_arrays(decode_on_device(R, path), splat_amd.load_from_ply(path), "shuffled")


@pytest.mark.parametrize("lacking", [("rot_",), ("scale_",), ("opacity",), ("rot_", "scale_", "opacity"), ("rot_0", "scale_1", "f_dc_", "y")],
                         ids=["no rot", "no scale", "no opacity", "none of the three", "single members"])
def test_decode_identity_absent_properties_keep_the_defaults(R, tmp_path, lacking):
    props = [p for p in INRIA if not any(p[1].startswith(s) for s in lacking)]
    path = str(tmp_path / "lacking.ply")
    P.write_ply_props(path, props, 257, splat_amd.synthetic_raw(257, 13))
    g = splat_amd.load_from_ply(path)
    got = decode_on_device(R, path)
    assert_same_arrays(got, g, "lacking %r" % (lacking,))
    # the defaults are Gaussian::new's: a scale of 0 (not exp(0)), an opacity of 0, the identity quaternion
    if "scale_" in lacking:
        assert not got["scales"].any()
    if "opacity" in lacking:
        assert not got["opacities"].any()
    if "rot_" in lacking:
        assert (got["rotations"].reshape(-1, 4) == np.array([0, 0, 0, 1], f32)).all()
    if "rot_0" in lacking:
        assert (got["rotations"].reshape(-1, 4)[:, 3] == 1).all() and (got["scales"].reshape(-1, 3)[:, 1] == 0).all()


def test_decode_identity_xyz_only(R, tmp_path):
    path = str(tmp_path / "xyz.ply")
    P.write_ply_props(path, INRIA[:3], 4097, splat_amd.synthetic_raw(4097, 14))
    assert splat_amd.ply_layout(path).stride == 12
    assert_same_arrays(decode_on_device(R, path), splat_amd.load_from_ply(path), "xyz only")


def test_decode_identity_rows_longer_than_the_staging_buffer(R, tmp_path):
    # a stride above 64 KiB: the decode reads global memory directly (its other flavour), one byte off alignment
    props = [("uchar", "tag")] + INRIA + [("float", "junk%d" % k) for k in range(16400)]
    path = str(tmp_path / "wide.ply")
    P.write_ply_props(path, props, 5, splat_amd.synthetic_raw(5, 15))
    assert splat_amd.ply_layout(path).stride == 1 + 248 + 4 * 16400 > 65536
    assert_same_arrays(decode_on_device(R, path, 2), splat_amd.load_from_ply(path), "wide rows")


def test_decode_identity_golden_head_and_the_oracle_as_second_witness(R):
    g = splat_amd.load_from_ply(GOLDEN)
    got = decode_on_device(R, GOLDEN)
    assert_same_arrays(got, g, "c1_head")
    o = O.load_ply(GOLDEN)                                   # the oracle's reader: shares no code with either loader
    for name, key in (("positions", "pos4"), ("scales", "scales"), ("opacities", "opacity"), ("rotations", "rot"), ("sh", "sh")):
        assert np.array_equal(got[name].view(np.uint32), np.ascontiguousarray(o[key], f32).reshape(-1).view(np.uint32)), name


def test_hostile_values(R, tmp_path):
    n = 20000
    rng = np.random.default_rng(41)
    raw = splat_amd.synthetic_raw(n, 16)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, P.OFLOW, np.nextafter(P.OFLOW, f32(200)), np.nextafter(P.OFLOW, f32(0)),
                        P.UFLOW, np.nextafter(P.UFLOW, f32(-200)), np.nextafter(P.UFLOW, f32(0)), P.NORMAL_EDGE, 88.0, -88.0,
                        np.finfo(f32).max, -np.finfo(f32).max], f32)
    for name in ("scale_0", "scale_1", "scale_2", "opacity"):
        v = rng.uniform(-110.0, 95.0, n).astype(f32)
        if name == "opacity":                                # the sigmoid's expf sees -v: half of the logits mirrored, so that
            v[n // 2:] = -v[n // 2:]                         # it, too, meets arguments from -110 to 95
        where = rng.choice(n, 40 * special.size, replace=False)
        v[where] = np.tile(special, 40)
        raw[name] = v
    raw["x"][rng.choice(n, 50, replace=False)] = np.nan      # x: the mean is NaN, every x is
    raw["y"][rng.choice(n, 50, replace=False)] = np.inf      # y: the mean is +inf; inf - inf = NaN, finite - inf = -inf
    raw["z"][rng.choice(n, 50, replace=False)] = f32(-0.0)
    path = str(tmp_path / "hostile.ply")
    splat_amd.write_ply(path, raw, n)
    g = splat_amd.load_from_ply(path)
    assert np.isnan(g.positions[:, 0]).all() and np.isinf(g.positions[:, 1]).any() and np.isnan(g.positions[:, 1]).any()
    assert np.isfinite(g.positions[:, 2]).all()
    assert np.isinf(g.scales).any() and (g.scales == 0).any() and ((g.scales > 0) & (g.scales < np.finfo(f32).tiny)).any()
    assert np.isnan(g.scales).any() and np.isnan(g.opacities).any() and (g.opacities == 0).any() and (g.opacities == 1).any()
    assert_same_arrays(decode_on_device(R, path), g, "hostile", nan_equal=True)


# ---- the sum really is sequential ------------------------------------------------------------------------------------
def alternating_positions(n=60000, seed=1):
    rng = np.random.default_rng(seed)
    mags = np.tile(np.array([1e8, -1e8, 1.0, -1.0, 1e-3], f32), (n + 4) // 5)[:n]
    return np.stack([rng.permutation(mags) for _ in range(3)], 1).astype(f32)


def mean_sequential(p):
    return (np.cumsum(p, axis=0, dtype=f32)[-1] / f32(len(p))).astype(f32)


def mean_pairwise(p):
    return (np.array([np.sum(np.ascontiguousarray(p[:, a]), dtype=f32) for a in range(3)], f32) / f32(len(p))).astype(f32)


def mean_block_tree(p, block=256):
    n = len(p)
    q = np.zeros(((n + block - 1) // block * block, 3), f32)
    q[:n] = p
    q = q.reshape(-1, block, 3)
    w = block
    while w > 1:
        w //= 2
        q = (q[:, :w] + q[:, w:2 * w]).astype(f32)
    return (np.cumsum(q[:, 0], axis=0, dtype=f32)[-1] / f32(n)).astype(f32)


def test_the_sum_is_one_sequential_chain_per_axis(R, tmp_path):
    n = 60000
    p = alternating_positions(n)
    seq, pair, tree = mean_sequential(p), mean_pairwise(p), mean_block_tree(p)
    # precondition: on this input a pairwise sum and a per-256-block tree give OTHER bits on every axis -- a parallel
    # reduction on the device could not pass
    assert (seq.view(np.uint32) != pair.view(np.uint32)).all(), (seq, pair)
    assert (seq.view(np.uint32) != tree.view(np.uint32)).all(), (seq, tree)
    path = str(tmp_path / "alternating.ply")
    splat_amd.write_ply(path, dict(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy()), n)
    got = decode_on_device(R, path)["positions"].reshape(n, 4)
    want = (p - seq).astype(f32)
    bad = np.flatnonzero((got[:, :3].view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, "the device mean is not the sequential one (%r): %d positions differ, first %d: device %r, sequential %r" % (
        seq, bad.size, bad[0], got[bad[0], :3], want[bad[0]])
    assert (got[:, 3] == 1).all()
    g = splat_amd.load_from_ply(path)
    assert np.array_equal(g.positions.view(np.uint32), got.view(np.uint32))          # the host loader agrees with numpy's cumsum


# ---- the whole chain -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ply_chain")
    out = {}
    for name, make, seed in (("cloud", splat_amd.synthetic_raw, 71), ("surfaces", splat_amd.synthetic_surface_raw, 72)):
        out[name] = str(d / (name + ".ply"))
        splat_amd.write_ply(out[name], make(120000, seed), 120000)
    out["c1_head"] = GOLDEN
    return out


def host_path(A, path, compute_cov3d=True):
    g = splat_amd.load_from_ply(path)
    if compute_cov3d:
        g.compute_cov3d(A)
    A.upload(g)
    return g


def assert_same_layout(A, B, what):
    oa, ba = A.scene_layout()
    ob, bb = B.scene_layout()
    assert oa.shape == ob.shape and ba.shape == bb.shape, what
    assert np.array_equal(oa, ob), "%s: order differs in %d slots" % (what, int((oa != ob).sum()))
    assert P.same_bits(ba, bb).all(), "%s: bounds differ in %d words" % (what, int((~P.same_bits(ba, bb)).sum()))


def frame(R_, h=256, w=256):
    img = np.zeros((h, w), np.uint32)
    st = R_.render_frame(make_camera(h, w).to_c(0.01, 15), img, want_stats=True)
    return img, (st.n_visible, st.n_pairs)


def assert_same_frame(A, B, what, expect_pixels=True):
    (ia, sa), (ib, sb) = frame(A), frame(B)
    assert sa == sb, (what, sa, sb)
    assert np.array_equal(ia, ib), "%s: %d pixels differ" % (what, int((ia != ib).sum()))
    if expect_pixels:
        assert ia.any(), what


@pytest.mark.parametrize("compute_cov3d", [1, 0], ids=["cov3d", "zero cov3d"])
@pytest.mark.parametrize("scene", ["cloud", "surfaces", "c1_head"])
def test_load_ply_is_the_host_path(chain_files, scene, compute_cov3d):
    path = chain_files[scene]
    with renderer() as A, renderer() as B:
        g = host_path(A, path, bool(compute_cov3d))
        assert B.load_ply(path, compute_cov3d=bool(compute_cov3d)) == len(g) == B.n
        assert_same_layout(A, B, scene)
        assert_same_frame(A, B, scene, expect_pixels=bool(compute_cov3d))
        assert A.frames_dropped() == B.frames_dropped()


def test_upload_ply_rows_from_a_torch_tensor_written_on_a_side_stream(chain_files):
    import torch
    path = chain_files["cloud"]
    pl = splat_amd.ply_layout(path)
    payload = np.fromfile(path, np.uint8, count=pl.payload_bytes, offset=pl.payload_offset)
    with renderer() as A, renderer() as B:
        host_path(A, path)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(device=dev)
        src = torch.from_numpy(payload).pin_memory()
        rows = torch.full((payload.size,), 0xFF, dtype=torch.uint8, device=dev)       # (all-ones floats are NaNs)
        junk = torch.zeros(64 << 20, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):                              # work in front of the copy: it has not run when the call is made
                junk.add_(1.0)
            rows.copy_(src, non_blocking=True)
            B.upload_ply_rows(rows, pl)                      # no stream given: torch's current one, which is `side`; no synchronise
        assert B.n == pl.n
        assert_same_layout(A, B, "side stream")
        assert_same_frame(A, B, "side stream")
        del rows, junk


def test_an_ascii_ply_takes_the_host_loader(tmp_path):
    n = 500
    path = str(tmp_path / "ascii.ply")
    P.write_ply_props(path, INRIA, n, splat_amd.synthetic_raw(n, 17), fmt="ascii")
    assert not splat_amd.ply_layout(path).binary
    with renderer() as A, renderer() as B:
        host_path(A, path)
        assert B.load_ply(path) == n
        assert_same_layout(A, B, "ascii")
        assert_same_frame(A, B, "ascii")


def test_load_ply_leaves_no_temporaries_behind(chain_files):
    path = chain_files["surfaces"]
    with renderer() as A:
        host_path(A, path)
        host_now = A.device_bytes()[0]
    with renderer() as B:
        B.load_ply(path)
        assert B.device_bytes()[0] == host_now
        B.load_ply(path)                                     # ... and a second load replaces the scene, it does not add to it
        assert B.device_bytes()[0] == host_now


def test_errors_on_a_live_context(R, tmp_path):
    path = inria_file(tmp_path, 300, 18)
    pl = splat_amd.ply_layout(path)
    # every non-NULL pointer below is this one real allocation, large enough for the largest output (sh) and the rows
    buf = R._L.splat_device_alloc(R._h, 300 * 48 * 4)
    assert buf
    before = R.device_bytes()[0]

    def spoiled(**kw):
        lay = _lib.PlyLayout.from_buffer_copy(pl.layout)
        for k, v in kw.items():
            if k == "offset":
                lay.offset[v[0]] = v[1]
            else:
                setattr(lay, k, v)
        return lay
    for lay in (spoiled(stride=0), spoiled(offset=(3, -2)), spoiled(offset=(3, 245)), spoiled(n=0xFFFFFFFF)):
        for call in (lambda: R.upload_ply_rows(buf, lay), lambda: R.decode_ply_device(buf, lay, buf, buf, buf, buf, buf)):
            with pytest.raises(splat_amd.SplatError) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(splat_amd.SplatError) as e:
        R.upload_ply_rows(0, pl)                             # NULL rows, n > 0
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(splat_amd.SplatError) as e:
        R.decode_ply_device(buf, pl, buf, 0, buf, buf, buf)
    assert e.value.code == _lib.ERR_INVALID
    assert R.device_bytes()[0] == before                     # ... all of it before any allocation
    with pytest.raises(TypeError):
        R.upload_ply_rows(buf, "not a layout")
    R.device_free(buf)
    # n == 0: as splat_upload_scene_device with n == 0
    cam = make_camera(64, 64).to_c(0.01, 15)
    answers = []
    with renderer() as A, renderer() as B:
        A.upload_device(0, 0, 0, 0, n=0)
        B.upload_ply_rows(0, spoiled(n=0))
        for X in (A, B):
            out = np.full((64, 64), 0xDEADBEEF, np.uint32)
            try:
                X.render_frame(cam, out)
                code = _lib.SPLAT_OK
            except splat_amd.SplatError as err:
                code = err.code
            answers.append((code, out))
        assert answers[0][0] == answers[1][0] and np.array_equal(answers[0][1], answers[1][1])
        assert A.n == 0 and B.n == 0
