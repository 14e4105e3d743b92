"""The resident scene saved as PLY rows on the GPU (splat_encode_ply_scene_device, splat_encode_ply_gaussians_device,
Renderer.encode_ply_rows / save_ply; -m gpu).  The rows the kernel writes are the rows the HOST compile of
splat_ply_encode_math.h gives for the resident values, bit for bit, in every layout; bytes no slot names are 0 and bytes
outside the rows keep what they held; the indexed form gathers; a round trip through the device decoder returns sh and
positions bit for bit and covariances and opacities within the float64 reference's error (the bounds of
tests/test_ply_encode_math_host.py); a save follows the edits and changes nothing a frame depends on.

Sizes: n = 1, 255, 256, 257, 700 -- at stride 248 a workgroup takes 256 rows (700: three workgroups and a partial tail), at
stride 300 it takes 218, so the block boundaries fall elsewhere."""
import ctypes as C
import os

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from splat_amd.gaussians import PLY_PROPS, inria_layout
from helpers import image_diff, make_camera
import ply_encode_cases as E
from scene_gpu import SENTINEL, TARGETS, assert_same_bits, in_view, session
from test_ply_encode_math_host import encode_rows, run
from test_retain_decide import STILL

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIZES = (1, 255, 256, 257, 700)
GUARD = 64                                            # sentinel bytes in front of and behind the rows


def case_scene(n, seed):
    """n Gaussians in view whose covariances cycle through every class and edge case and whose opacities through the
    hand-written ones and the sweep"""
    g = in_view(n, seed)
    cov = np.concatenate([E.edge_covariances()] + [E.covariances(c, max(1, (n + 7) // 8), seed) for c in E.CLASSES])
    op = E.opacities(seed)
    g.cov3d = np.ascontiguousarray(cov[np.arange(n) % len(cov)])
    g.opacities = np.ascontiguousarray(op[np.arange(n) % len(op)])
    return g


def slot_values(pos, cov, op, sh):
    """[n, 59] float32: what each slot of a row holds for these resident values, by the HOST compile of the header"""
    logs, logit, quat = encode_rows(cov, op)
    out = np.zeros((len(op), _lib.PLY_SLOTS), f32)
    out[:, _lib.PLY_SLOT_POS:_lib.PLY_SLOT_POS + 3] = pos[:, :3]
    out[:, _lib.PLY_SLOT_SCALE:_lib.PLY_SLOT_SCALE + 3] = logs
    out[:, _lib.PLY_SLOT_OPACITY] = logit
    out[:, _lib.PLY_SLOT_ROT:_lib.PLY_SLOT_ROT + 4] = quat
    out[:, _lib.PLY_SLOT_SH:] = sh
    return out


def rows_of(values, lay):
    """[n, stride] uint8: the slots laid into zeroed rows"""
    n = len(values)
    rows = np.zeros((n, int(lay.stride)), np.uint8)
    for k in range(_lib.PLY_SLOTS):
        o = int(lay.offset[k])
        if o >= 0:
            rows[:, o:o + 4] = np.ascontiguousarray(values[:, k]).view(np.uint8).reshape(n, 4)
    return rows


def layouts(n):
    inria = inria_layout(n)
    padded = inria_layout(n)
    padded.stride = 300
    shuffled = inria_layout(n)
    perm = np.random.default_rng(11).permutation(62)
    for k in range(_lib.PLY_SLOTS):
        shuffled.offset[k] = 4 * int(perm[inria.offset[k] // 4])
    no_shape = inria_layout(n)
    for k in list(range(_lib.PLY_SLOT_SCALE, _lib.PLY_SLOT_SCALE + 3)) + list(range(_lib.PLY_SLOT_ROT, _lib.PLY_SLOT_ROT + 4)):
        no_shape.offset[k] = -1
    pos_only = _lib.PlyLayout()
    pos_only.n, pos_only.stride = n, 12
    for k in range(_lib.PLY_SLOTS):
        pos_only.offset[k] = 4 * k if k < 3 else -1
    return {"inria": inria, "padded": padded, "shuffled": shuffled, "no_shape": no_shape, "pos_only": pos_only}


def encode(s, lay, index=None, k=None):
    """encode_ply_rows into a sentinel-filled buffer with guards: ([rows, stride] uint8, the guards untouched)"""
    rows = int(lay.n)
    nbytes = rows * int(lay.stride)
    p = s.alloc(GUARD + nbytes + GUARD, SENTINEL)
    s.R.encode_ply_rows(p + GUARD, lay, index=index, k=k)
    raw = s.fetch(p, (GUARD + nbytes + GUARD,), np.uint8)
    assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + nbytes:] == SENTINEL).all(), "bytes outside [0, n * stride) were written"
    return raw[GUARD:GUARD + nbytes].reshape(rows, int(lay.stride))


def assert_same_rows(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bytes differ, first at row %d byte %d" % (what, len(bad), bad[0][0], bad[0][1])


# ---- 1. the two compiles of the header ------------------------------------------------------------------------------------
def test_the_device_compile_of_the_header_is_the_host_compile_bit_for_bit():
    cov = np.concatenate([E.edge_covariances()] + [E.covariances(c, 512) for c in E.CLASSES])
    op = E.opacities()[np.arange(len(cov)) % len(E.opacities())]
    one = np.concatenate([cov, op[:, None]], 1)
    V = run(2, cov[:, [0, 3, 6, 4, 7, 8]])[:, 3:]
    for which, data in ((0, np.concatenate([E.positive_floats(), np.array([0, -1, np.nan, np.inf], f32)])), (1, np.concatenate([E.opacities(), np.array([np.nan], f32)])),
                        (2, cov[:, [0, 3, 6, 4, 7, 8]]), (3, V), (4, one)):
        host, dev = run(which, data, host=True), run(which, data, host=False)
        assert host.tobytes() == dev.tobytes(), "function %d: %d values differ" % (which, int((host.view(np.uint8) != dev.view(np.uint8)).any(-1).sum()))


# ---- 2. the kernel's rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_the_rows_are_the_host_compiles_rows_bit_for_bit_in_every_layout(n):
    g = case_scene(n, 4100 + n)
    values = slot_values(g.positions, g.cov3d, g.opacities, g.sh)
    with session() as s:
        s.R.upload(g)
        for name, lay in layouts(n).items():
            got = encode(s, lay)
            assert_same_rows(got, rows_of(values, lay), "%s, n=%d" % (name, n))
            if name == "inria":
                assert (got[:, 12:24] == 0).all()                           # nx ny nz
                assert got.view("<f4")[:, :3].tobytes() == g.positions[:, :3].tobytes()
            if name == "padded":
                assert (got[:, 248:] == 0).all()
        # a layout of another n is refused, by the wrapper and by the library, with nothing written
        wrong = inria_layout(n + 1)
        p = s.alloc((n + 1) * 248, SENTINEL)
        with pytest.raises(ValueError):
            s.R.encode_ply_rows(p, wrong)
        with pytest.raises(splat_amd.SplatError) as e:                      # the library says the same
            s.R._check(s.R._L.splat_encode_ply_scene_device(s.R._h, C.byref(wrong), C.c_void_p(p)))
        assert e.value.code == _lib.ERR_INVALID and "layout->n" in str(e.value)
        assert (s.fetch(p, ((n + 1) * 248,), np.uint8) == SENTINEL).all()


def test_an_empty_scene_and_a_scene_whose_cov3d_was_left_zero():
    with session() as s:
        s.R.encode_ply_rows(0, inria_layout(0))                             # no scene: nothing to write, no error
        assert s.R.save_ply(os.devnull) == 0
        g = in_view(300, 77)
        g.cov3d[:] = 0                                                      # compute_cov3d=False
        s.R.upload(g)
        got = encode(s, inria_layout(300)).view("<f4")
        lay = inria_layout(300)
        for k in range(3):
            assert (got[:, lay.offset[_lib.PLY_SLOT_SCALE + k] // 4] == f32(-104.0)).all()
        assert (got[:, lay.offset[_lib.PLY_SLOT_ROT + 3] // 4] == f32(1.0)).all()       # rot_0 = w: the identity


# ---- 3. by index ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (257, 700))
def test_indexed_rows_are_the_whole_scenes_rows_gathered(n):
    g = case_scene(n, 4300 + n)
    rng = np.random.default_rng(n)
    with session() as s:
        s.R.upload(g)
        for name in ("inria", "padded"):
            whole = encode(s, layouts(n)[name])
            idx = rng.integers(0, n, 3 * n // 2).astype(np.uint32)          # random order, duplicates among them
            idx[:4] = (n - 1, 0, n - 1, 0)
            lay = layouts(len(idx))[name]
            got = encode(s, lay, index=s.array(idx), k=len(idx))
            assert_same_rows(got, whole[idx], "%s, n=%d indexed" % (name, n))
        # k == 0 writes nothing
        p = s.alloc(1024, SENTINEL)
        s.R.encode_ply_rows(p, inria_layout(0), index=s.array(np.zeros(1, np.uint32)), k=0)
        assert (s.fetch(p, (1024,), np.uint8) == SENTINEL).all()
        # an index >= n: refused, nothing written
        bad = np.array([0, 1, n, 2], np.uint32)
        p = s.alloc(4 * 248, SENTINEL)
        with pytest.raises(splat_amd.SplatError) as e:
            s.R.encode_ply_rows(p, inria_layout(4), index=s.array(bad), k=4)
        assert e.value.code == _lib.ERR_INVALID and "index" in str(e.value)
        assert (s.fetch(p, (4 * 248,), np.uint8) == SENTINEL).all()


# ---- 4. the round trip on the device ---------------------------------------------------------------------------------------
def decode(s, rows, lay):
    """decode_ply_device + compute_cov3d_device of device rows: positions, scales, opacities, rotations, sh, cov3d"""
    n = int(lay.n)
    per = (("positions", 4), ("scales", 3), ("opacities", 1), ("rotations", 4), ("sh", 48))
    bufs = {f: s.alloc(4 * k * n, SENTINEL) for f, k in per}
    s.R.decode_ply_device(rows, lay, *[bufs[f] for f, _ in per])
    cov = s.alloc(36 * n)
    s.R.compute_cov3d_device(bufs["scales"], bufs["rotations"], cov, n=n)
    out = {f: s.fetch(bufs[f], (n,) if k == 1 else (n, k)) for f, k in per}
    out["cov3d"] = s.fetch(cov, (n, 9))
    return out


def test_round_trip_through_the_device_decoder_against_the_float64_reference():
    n_class = E.N_CLASS
    cov = np.concatenate([E.covariances(c) for c in E.CLASSES] + [E.edge_covariances()])
    n = len(cov)
    g = in_view(n, 4500)
    g.cov3d = np.ascontiguousarray(cov)
    op = E.opacities()
    g.opacities = np.ascontiguousarray(op[np.arange(n) % len(op)])
    lay = inria_layout(n)
    with session() as s:
        s.R.upload(g)
        p = s.alloc(n * 248, SENTINEL)
        s.R.encode_ply_rows(p, lay)
        back = decode(s, p, lay)
        resident = s.read_all(n)
        # the float64 reference's rows through the same decode
        rlogs, rquat = E.reference_encode(cov)
        d64 = g.opacities.astype(f64)
        with np.errstate(divide="ignore", invalid="ignore"):
            rlogit = np.log(d64 / (1.0 - d64)).astype(f32)
        values = np.zeros((n, _lib.PLY_SLOTS), f32)
        values[:, :3], values[:, 3:6], values[:, 6], values[:, 7:11], values[:, 11:] = g.positions[:, :3], rlogs, rlogit, rquat, g.sh
        ref = decode(s, s.array(rows_of(values, lay)), lay)
    assert_same_bits(back["sh"], resident["sh"], "sh")
    pos = resident["positions"].copy()
    pos[:, :3] -= (np.cumsum(pos[:, :3], axis=0, dtype=f32)[-1] / f32(n)).astype(f32)      # the loader's recentring
    assert_same_bits(back["positions"], pos, "positions, recentred")
    # opacities: the clamps exactly, the others within twice the reference's worst error
    o = resident["opacities"]
    assert (back["opacities"][o <= 0] == 0).all() and (back["opacities"][o >= 1] == 1).all()
    inner = (o > 0) & (o < 1)
    eo, ro = np.abs(back["opacities"][inner].astype(f64) - o[inner]).max(), np.abs(ref["opacities"][inner].astype(f64) - o[inner]).max()
    print("opacity: worst |o' - o| header %.3g, float64 reference %.3g" % (eo, ro))
    assert eo <= 2.0 * ro
    for c, name in enumerate(E.CLASSES + ("edges",)):
        sl = slice(c * n_class, min((c + 1) * n_class, n))
        e, r = E.relative_error(back["cov3d"][sl], resident["cov3d"][sl]), E.relative_error(ref["cov3d"][sl], resident["cov3d"][sl])
        print("%-10s worst e: kernel %.2f, float64 eigh reference %.2f (units of 2^-24)" % (name, e.max() * 2 ** 24, r.max() * 2 ** 24))
        assert np.isfinite(back["cov3d"][sl]).all()
        assert e.max() <= 2.0 * r.max(), name
    zero = len(E.CLASSES) * n_class + E.EDGES.index("zero")
    assert (back["cov3d"][zero] == 0).all()


# ---- 5. a save follows the edits ---------------------------------------------------------------------------------------------
def edited(s, n):
    """three edits on three disjoint selections: opacity 0, a turn with its sh, a reflection with its sh; -> the deleted indices"""
    gone = np.arange(0, n, 5, dtype=np.uint32)
    s.R.update_indexed(s.array(gone), opacities=s.array(np.zeros(len(gone), f32)), k=len(gone))
    a = 0.7
    turn = np.array([[np.cos(a), -np.sin(a), 0, 0.25], [np.sin(a), np.cos(a), 0, -0.5], [0, 0, 1, 0.125]], f32)
    turned = np.arange(1, n, 5, dtype=np.uint32)
    s.R.transform(turn, index=s.array(turned), k=len(turned), rotate_sh=True)
    mirror = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
    mirrored = np.arange(2, n, 5, dtype=np.uint32)
    s.R.transform(mirror, index=s.array(mirrored), k=len(mirrored), rotate_sh=True)
    return gone


def test_after_edits_the_rows_follow_the_resident_values():
    n = 700
    g = in_view(n, 4700)
    lay = inria_layout(n)
    with session() as s:
        s.R.upload(g)
        before = encode(s, lay)
        assert_same_rows(before, rows_of(slot_values(g.positions, g.cov3d, g.opacities, g.sh), lay), "as uploaded")
        gone = edited(s, n)
        now = s.read_all(n)
        after = encode(s, lay)
        assert_same_rows(after, rows_of(slot_values(now["positions"], now["cov3d"], now["opacities"], now["sh"]), lay), "as edited")
        changed = (after != before).any(1)
        assert changed[0::5].all() and changed[1::5].all() and changed[2::5].all() and not changed[3::5].any() and not changed[4::5].any()
        assert (after.view("<f4")[gone, lay.offset[_lib.PLY_SLOT_OPACITY] // 4] == f32(-104.0)).all()


def test_save_ply_of_the_survivors_loads_and_renders(tmp_path):
    n, (h, w) = 700, (64, 64)
    g = in_view(n, 4900)
    path = str(tmp_path / "saved.ply")
    cam = make_camera(h, w)
    with session() as s:
        R = s.R
        R.upload(g)
        gone = edited(s, n)
        whole = encode(s, inria_layout(n))
        sel = s.alloc(n, 0)
        count = R.select(sel, opacity=(1e-30, 2.0))
        assert count == n - len(gone)
        idx = s.alloc(4 * n, SENTINEL)
        assert R.selection_indices(sel, idx, n=n, capacity=n) == count
        assert R.save_ply(path, index=idx, k=count) == count
        original = np.zeros((h, w), np.uint32)
        R.render_frame(cam.to_c(0.01, 15), original)
        now = s.read_all(n)
    survivors = np.setdiff1d(np.arange(n), gone)
    # the file: the canonical header, then exactly the surviving rows in ascending order
    data = open(path, "rb").read()
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % count + b"".join(b"property float %s\n" % p.encode() for p in PLY_PROPS) + b"end_header\n"
    assert data[:len(head)] == head and len(data) == len(head) + count * 248
    assert data[len(head):] == whole[survivors].tobytes()
    pl = splat_amd.ply_layout(path)
    assert pl.n == count and pl.stride == 248 and list(pl.layout.offset) == list(inria_layout(count).offset)
    back = splat_amd.load_from_ply(path)
    assert len(back) == count and (back.opacities > 0).all()
    assert_same_bits(back.sh, now["sh"][survivors], "sh of the file")
    mean = (np.cumsum(now["positions"][survivors, :3], axis=0, dtype=f32)[-1] / f32(count)).astype(f32)
    assert_same_bits(back.positions[:, :3], now["positions"][survivors, :3] - mean, "positions of the file, recentred")
    kept = splat_amd.GaussianList(now["positions"][survivors], np.zeros((count, 3), f32), now["opacities"][survivors],
                                  np.zeros((count, 4), f32), now["sh"][survivors], now["cov3d"][survivors])
    with session() as s2:
        s2.R.upload(kept)                                                   # what was saved, as the scene held it
        fresh = np.zeros((h, w), np.uint32)
        s2.R.render_frame(cam.to_c(0.01, 15), fresh)
        assert s2.R.load_ply(path) == count
        shift = np.array([[1, 0, 0, mean[0]], [0, 1, 0, mean[1]], [0, 0, 1, mean[2]]], f32)
        s2.R.transform(shift)                                               # (back where the saved scene stood)
        reloaded = np.zeros((h, w), np.uint32)
        s2.R.render_frame(cam.to_c(0.01, 15), reloaded)
    assert reloaded.any()
    for what, ref in (("the edited scene, its opacity-0 Gaussians still resident", original), ("a fresh upload of the resident survivors", fresh)):
        worst, px = image_diff(ref, reloaded)
        print("save and reload against %s: %d of %d pixels differ, by at most %d (not asserted: nobody has derived a bound)" % (what, px, h * w, worst))


# ---- 6. a save changes nothing ---------------------------------------------------------------------------------------------
def test_a_save_changes_nothing_a_frame_depends_on(tmp_path):
    n, (h, w) = 700, TARGETS[1]
    g = in_view(n, 5100)
    cam = make_camera(h, w).to_c(0.01, 15)
    lay = inria_layout(n)
    with session() as s:
        R = s.R
        R.upload(g)
        img = R.host_image(h, w)

        def rest_frame():
            img[:] = 0xDEADBEEF
            R.render_frame(cam, img)
            return img.copy()

        rest = [rest_frame() for _ in range(STILL + 4)]
        assert rest[0].any() and all(np.array_equal(rest[0], f) for f in rest)
        retained = R.frames_retained()
        assert retained > 0, "the camera is at rest: its frames are meant to come from retained lists by now"
        rows = s.alloc(n * 248, SENTINEL)
        idx = np.arange(0, n, 3, dtype=np.uint32)
        dropped = R.frames_dropped()
        R.encode_ply_rows(rows, lay)
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 1
        R.encode_ply_rows(rows, inria_layout(len(idx)), index=s.array(idx), k=len(idx))
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 2
        assert R.save_ply(str(tmp_path / "rest.ply")) == n
        assert np.array_equal(rest_frame(), rest[0]) and R.frames_retained() == retained + 3
        assert R.frames_dropped() == dropped
        # ... nor do asynchronous frames in flight lose anything: the save comes behind them
        images = [R.device_image(np.full((h, w), 0xDEADBEEF, np.uint32)) for _ in range(3)]
        try:
            for p in images:
                R.render_frame_device(cam, p, sync=False)
            R.encode_ply_rows(rows, lay)
            for p in images:
                assert np.array_equal(R.device_download(p, h, w), rest[0])
        finally:
            for p in images:
                R.device_free(p)
