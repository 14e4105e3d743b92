"""The device scene order and the mask scan beyond one round of their tables (-m gpu): scenes of 262 144 to 1 052 673 Gaussians
and masks of up to 2 101 249 bytes, on both sides of the sizes at which scene_box_kernel takes a second row per thread,
radix_scan_kernel a second round of a digit's row (and radix_scatter_kernel reads the table from column 256 on), and
mask_scan_kernel a second round of span counts -- tests/scene_large_cases.py derives the sizes from the constants, and
tests/test_scene_large_cases_host.py shows on the CPU that the cases would catch a lost carry and a box that misses a trip.

Nothing here has a tolerance: orders, index maps and indices are numpy's (remove_cases.morton_order, np.flatnonzero, ...),
floats are compared as bits with NaN matching NaN, and layouts and frames are those of the host upload, the specification.
Every buffer a call writes starts filled with 0xA5 between guard bytes.  At most two contexts are alive at any time, and a
test's device buffers go with its session."""
import numpy as np
import pytest

import splat_amd
from splat_amd.gaussians import PLY_PROPS, inria_layout
from helpers import make_camera
import append_cases as AC
import remove_cases as RC
import scene_large_cases as L
from scene_gpu import FIELDS, PER, TARGETS, assert_bounds, assert_same_bits, fresh_upload, session
from test_gpu_device_upload import assert_same_layout

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, SENTINEL = L.GUARD, L.SENTINEL
FILL32 = 0xA5A5A5A5


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def guarded(s, nbytes):
    """a device buffer of nbytes between two guards, every byte the sentinel: (address of the buffer, fetch(count, dtype)), the
    fetch checking the guards"""
    base = s.alloc(nbytes + 2 * GUARD, SENTINEL)
    assert base % 16 == 0

    def fetch(count, dtype=f32):
        raw = s.fetch(base, (nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + nbytes:] == SENTINEL).all(), "a guard byte was written"
        return raw[GUARD:GUARD + count * np.dtype(dtype).itemsize].view(dtype).copy()

    return base + GUARD, fetch


def put_mask(s, mask, head):
    """the mask's bytes at a device address whose low four bits are `head`, guard bytes (nonzero: a kernel that read beyond
    mask[0..n) would count them) around it; returns the address"""
    mask = np.ascontiguousarray(mask, np.uint8)
    base = s.alloc(len(mask) + 2 * GUARD + 16, SENTINEL)
    assert base % 16 == 0
    p = base + GUARD + head
    s.R._check(s.R._L.splat_device_upload(s.R._h, p, mask.ctypes.data, mask.nbytes))
    assert p % 16 == head
    return p


def assert_fields(s, g, what):
    """read_device of the resident scene into guarded, sentinel-filled buffers gives g's four fields, bit for bit (w = 1)"""
    n = len(g)
    assert s.R.n == n, what
    bufs = {f: guarded(s, 4 * PER[f] * n) for f in FIELDS}
    s.R.read_device(n=n, **{f: bufs[f][0] for f in FIELDS})
    for f in FIELDS:
        got = bufs[f][1](PER[f] * n).reshape((n,) if PER[f] == 1 else (n, PER[f]))
        assert_same_bits(got, getattr(g, f), "%s %s" % (what, f))


def assert_order(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d slots hold another Gaussian, first slot %d (%d, want %d)" % (what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])


def assert_permutation(orig, what):
    assert len(orig) and np.array_equal(np.bincount(orig, minlength=len(orig)), np.ones(len(orig), np.int64)), what + ": the order is not a permutation"


def upload_from_device(s, g):
    d = s.device(g)
    s.R.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=len(g))
    assert s.R.n == len(g)


def frames_with_counts(R):
    """one frame per target: [(image, (n_visible, n_pairs, n_blocks_culled))]"""
    out = []
    for h, w in TARGETS:
        img = np.full((h, w), 0xDEADBEEF, np.uint32)
        st = R.render_frame(make_camera(h, w).to_c(0.01, 15), img, want_stats=True)
        out.append((img, (st.n_visible, st.n_pairs, st.n_blocks_culled)))
    return out


# ---- the order, every scene-order case --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.ORDER_NAMES)
def test_device_order_is_morton_order(name):
    g = L.scene(name)
    with session() as s:
        upload_from_device(s, g)
        orig, _ = s.R.scene_layout()
        assert_order(orig, L.order(name), name)
        assert_permutation(orig, name)
        if name not in L.TWINS:
            return
        with fresh_upload(g) as A:
            assert_same_layout(A, s.R, name)
            fa, fb = frames_with_counts(A), frames_with_counts(s.R)
            for k, ((ia, sa), (ib, sb)) in enumerate(zip(fa, fb)):
                print(name, "target", TARGETS[k], "visible, pairs, blocks culled:", sa, sb)
                assert sa == sb, (name, k, sa, sb)
                assert ia.any() and np.array_equal(ia, ib), "%s frame %d: %d pixels differ" % (name, k, int((ia != ib).sum()))
            print(name, "frames dropped:", A.frames_dropped(), s.R.frames_dropped())
            assert A.frames_dropped() == 0 and s.R.frames_dropped() == 0


# ---- the other three entry points of the same sort -----------------------------------------------------------------------------------
def test_upload_ply_rows_is_the_host_loaders_scene(tmp_path):
    n = L.SORT + 1
    rows = L.ply_rows(n)
    path = str(tmp_path / "large.ply")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n)
        for p in PLY_PROPS:
            f.write(("property float %s\n" % p).encode())
        f.write(b"end_header\n")
        rows.tofile(f)
    with session() as s, session() as a:
        g = splat_amd.load_from_ply(path)                     # the host path: the loader, compute_cov3d, splat_upload_scene
        assert len(g) == n
        g.compute_cov3d(a.R)
        a.R.upload(g)
        s.R.upload_ply_rows(s.array(rows), inria_layout(n))
        assert s.R.n == n
        orig, _ = assert_same_layout(a.R, s.R, "ply rows")
        assert_order(orig, RC.morton_order(g.positions), "ply rows")
        assert_fields(s, g, "ply rows")


def test_reorder_after_every_position_changed():
    g = L.scene("sort+1")
    n = len(g)
    edited = L.scene_of(L.second_positions(n))
    with session() as s:
        R = s.R
        R.upload(g)
        orig, _ = R.scene_layout()
        assert_order(orig, L.order("sort+1"), "host upload")
        R.update_device(positions=s.array(edited.positions), n=n)
        want = AC.moved(orig, edited.positions)
        moved = R.reorder()
        print("reorder moved", moved, "of", n)
        assert moved == want > n // 2
        with fresh_upload(edited) as ref:
            got, _ = assert_same_layout(ref, R, "reordered")
        assert_order(got, AC.reordered_order(edited.positions), "reordered")
        assert_fields(s, edited, "reordered")
        held = R.device_bytes()[0]
        assert R.reorder() == 0, "a second reorder finds nothing to move"
        assert R.device_bytes()[0] == held
        assert_order(R.scene_layout()[0], got, "after the second reorder")


def test_append_a_tail_beyond_a_scan_round_then_reorder():
    """257 resident Gaussians, SORT + 1 appended: the new rows are sorted on their own, behind the resident slots"""
    A, E = L.small_scene(), L.scene("sort+1")
    n, m = len(A), len(E)
    both = AC.appended(A, E)
    assert L.sort_scan_rounds(m) == 2 and L.sort_scan_rounds(n + m) == 2
    with session() as s:
        R = s.R
        R.upload(A)
        orig_a, bounds_a = R.scene_layout()
        d = s.device(E)
        assert R.append(d.positions, d.cov3d, d.opacities, d.sh, m=m) == n + m == R.n
        orig, bounds = R.scene_layout()
        assert_order(orig, AC.appended_order(orig_a, E.positions), "appended")
        assert_permutation(orig, "appended")
        assert bounds[:n // 256].tobytes() == bounds_a[:n // 256].tobytes(), "the block wholly below the seam keeps its bits"
        assert_bounds(bounds, L.block_bounds(both.positions, both.cov3d, orig), "appended")
        assert_fields(s, both, "appended")
        want = AC.moved(orig, both.positions)
        moved = R.reorder()
        print("reorder moved", moved, "of", n + m)
        assert moved == want > 0
        with fresh_upload(both) as ref:
            assert_same_layout(ref, R, "appended, reordered")
        assert_fields(s, both, "appended, reordered")


def test_append_a_few_rows_to_a_scene_beyond_a_scan_round():
    """SORT + 1 resident Gaussians, 257 appended: every whole block keeps its bounds, the seam block and the new ones are made again"""
    A, E = L.scene("sort+1"), L.small_scene()
    n, m = len(A), len(E)
    both = AC.appended(A, E)
    whole = n // 256
    with session() as s:
        R = s.R
        R.upload(A)
        orig_a, bounds_a = R.scene_layout()
        assert_order(orig_a, L.order("sort+1"), "host upload")
        d = s.device(E)
        assert R.append(d.positions, d.cov3d, d.opacities, d.sh, m=m) == n + m == R.n
        orig, bounds = R.scene_layout()
        assert_order(orig, AC.appended_order(orig_a, E.positions), "appended")
        assert whole == (256 * L.SORT_ITEMS) and bounds.shape[0] == (n + m + 255) // 256 > whole + 1
        assert bounds[:whole].tobytes() == bounds_a[:whole].tobytes(), "the blocks wholly below the seam keep their bits"
        assert_bounds(bounds[whole:], L.block_bounds(both.positions, both.cov3d, orig)[whole:], "the seam block and the new ones")
        assert_fields(s, both, "appended")


# ---- the mask scan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", L.PATTERNS)
@pytest.mark.parametrize("head,n", L.MASK_CASES)
def test_selection_indices_are_flatnonzero(head, n, pattern):
    mask = L.mask_bytes(head, n, pattern)
    want = np.flatnonzero(mask).astype(np.uint32)
    what = "head %d n %d %s" % (head, n, pattern)
    with session() as s:
        p = put_mask(s, mask, head)
        out, fetch = guarded(s, 4 * n)
        count = s.R.selection_indices(p, out, n=n, capacity=n)
        got = fetch(n, np.uint32)
        assert count == want.size > 0, what
        bad = np.flatnonzero(got[:count] != want)
        assert bad.size == 0, "%s: %d of %d indices differ, first at %d (%d, want %d)" % (what, bad.size, count, bad[0], got[bad[0]], want[bad[0]])
        assert (np.diff(got[:count].astype(np.int64)) > 0).all(), what + ": ascending"
        assert (got[count:] == FILL32).all(), what + ": entries behind the count keep the fill"
        # room for one fewer: a prefix, nothing at or behind the capacity, and the count stays whole
        cap = count - 1
        out, fetch = guarded(s, 4 * n)
        assert s.R.selection_indices(p, out, n=n, capacity=cap) == count, what
        got = fetch(n, np.uint32)
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == FILL32).all(), what + ": capacity = count - 1"


@pytest.mark.parametrize("which", L.REMOVE_SELECTIONS)
@pytest.mark.parametrize("keep", [False, True], ids=["delete", "crop"])
@pytest.mark.parametrize("head", [0, 15])
def test_remove_beyond_a_round_of_the_mask_scan(head, keep, which):
    g = L.remove_scene()
    n = len(g)
    sel = L.remove_selection(which)
    want, want_map = RC.removed(g, sel, keep)
    what = "%s %s, mask at +%d" % (which, "kept" if keep else "deleted", head)
    assert L.mask_scan_rounds(head, n) == 2 and 0 < len(want) < n
    with session() as s:
        R = s.R
        R.upload(g)
        orig_a, _ = R.scene_layout()
        p = put_mask(s, np.where(sel, L.NONZERO[np.arange(n) % 4], 0), head)
        pm, fetch_map = guarded(s, 4 * n)
        got = R.remove(p, keep=keep, index_map=pm, n=n)
        print(what, "->", got)
        assert got == len(want) == R.n, what
        got_map = fetch_map(n, np.uint32)
        bad = np.flatnonzero(got_map != want_map)
        assert bad.size == 0, "%s: the map differs for %d Gaussians, first %d (%d, want %d)" % (what, bad.size, bad[0], got_map[bad[0]], want_map[bad[0]])
        orig, bounds = R.scene_layout()
        assert_order(orig, RC.compacted_order(orig_a, want_map), what)
        assert_fields(s, want, what)
        with fresh_upload(want) as ref:
            ref_orig, ref_bounds = ref.scene_layout()
        assert_order(orig, ref_orig, what + ": the order a fresh upload of the survivors computes")
        assert_bounds(bounds, ref_bounds, what)
