"""Scenes that give every tile-list sort route lists of chosen length and chosen depth-key bits, and what the oracle says their
lists are (no GPU here; tests/test_sort_cases_host.py holds the scenes to their claims, tests/test_gpu_tile_sort.py renders them).

How one list is controlled.  A splat_amd.Camera whose pose is never updated keeps identity view and projection matrices
(tests/test_gpu_parity.py, test_identity_matrices_when_pose_never_updated), so a position IS its NDC and its view depth is its z,
bit for bit.  With cov3d = 0 and low-pass 0.3 every Gaussian is a splat of a few pixels whatever its depth; put at the centre of a
16 x 16 tile it lands in that tile alone.  So one tile is one list, its length the number of Gaussians put there, its depth keys
the f32 bit patterns written into z (depth_key of a positive float is its bits with the sign bit set: differences of bit patterns
are differences of keys).  The original indices are a random permutation across the tiles: within a tile x and y are equal, the
Morton slots differ from the original indices, and ties are settled through `orig`.  Opacities of 0.01..0.2 make the walks go a few
hundred keys deep, so the nearest part of every order shows in the frame's bytes too.

The switches the lengths sit around (splat_kernels.hip): sort_radix_min = 128 (bitonic network up to it); 1408 keys (the LDS
workspace of sort_list_in_lds<256, 2048> has room for 512-bin histograms up to it: 9-bit digits, 8 above); 2048 / 8192 / 16384 (the
size classes of the sort launches and the compositor's own limit); 16385..65536 (four runs of 16384 + merge_runs_kernel: 32769 and
49153 merge a full run with a run of one key); beyond 65536 (sort_list_global); and the compositor's partition_long_list (parts of
at most 1792 keys, at most 62 of them: 70000 and 100000 go past that)."""
import os

import numpy as np

import splat_amd
from oracle import oracle as O
from helpers import scene_dict, oracle_camera

f32 = np.float32
TILE = 16
LOWPASS = 0.3

SWEEP_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1407, 1408, 1409, 2047, 2048, 2049,
                 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32769, 49153, 65535, 65536, 65537, 70000, 100000)
PATTERN_LENGTHS = (100, 1500, 2048, 5000, 16384, 20000, 70000)
PATTERNS = ("one", "levels2", "levels3", "levels7", "levels300", "span255", "span256", "span257", "span511", "span512", "span513",
            "consecutive", "ties2_3", "ties8", "ties13", "ties40", "log", "band", "asc", "desc")
DISTINCT_LENGTHS = (129, 1500, 2048, 5000, 16384, 20000, 70000)
FUSED_MAX = 2048                       # the longest list a compositor workgroup sorts in its LDS

OCTAVE = 0x3E800000                    # bits of 0.25: [0.25, 0.5) is the 2^23 patterns from here
BAND_BASE = 0x3E900000                 # where the narrow patterns sit (0.28125)
BAND_WIDTH = 300                       # ulps
LOG_LO, LOG_HI = f32(1e-30), f32(1.0)


def bits_of(z):
    return np.ascontiguousarray(z, f32).view(np.uint32)


def _floats(bits):
    return np.ascontiguousarray(bits, np.uint32).view(f32)


def _distinct_bits(rng, k):
    """k distinct bit patterns of the octave [0.25, 0.5), in random order"""
    got = np.zeros(0, np.int64)
    while got.size < k:
        got = np.unique(np.concatenate([got, rng.integers(0, 1 << 23, k + k // 4 + 16)]))
    return (OCTAVE + rng.permutation(got)[:k]).astype(np.uint32)


def _runs(n, lengths):
    """run lengths that add up to n: `lengths` in turn, the last one cut"""
    out, k = [], 0
    while n > 0:
        r = min(lengths[k % len(lengths)], n)
        out.append(r)
        n -= r
        k += 1
    return out


def _span_offsets(n, span, rng):
    """n offsets in 0..span with both ends present (n >= 2): all distinct while span + 1 >= n, else every offset in turn"""
    if n < 2:
        return np.zeros(n, np.int64)
    if span + 1 >= n:
        inner = rng.permutation(np.arange(1, span))[:n - 2]
        return rng.permutation(np.concatenate([[0, span], inner]))
    return rng.permutation(np.arange(n) % (span + 1))


def pattern_depths(pattern, n, rng):
    """the f32 depths of one list of n keys, in the order its members get them (asc / desc: by ascending original index)"""
    if n == 0:
        return np.zeros(0, f32)
    if pattern in ("uniform", "asc", "desc"):
        z = _floats(OCTAVE + rng.integers(0, 1 << 23, n).astype(np.uint32))
        return z if pattern == "uniform" else (np.sort(z) if pattern == "asc" else np.sort(z)[::-1].copy())
    if pattern == "one":
        return np.full(n, f32(0.25))
    if pattern.startswith("levels"):
        k = min(int(pattern[6:]), n)
        return _floats(_distinct_bits(rng, k)[rng.permutation(np.arange(n) % k)])
    if pattern.startswith("span"):
        return _floats((BAND_BASE + _span_offsets(n, int(pattern[4:]), rng)).astype(np.uint32))
    if pattern == "consecutive":
        z = _floats(BAND_BASE + np.arange(n, dtype=np.uint32))      # n patterns in a row: each one np.nextafter of the one before
        assert np.array_equal(z[1:], np.nextafter(z[:-1], f32(1.0)))
        return z[rng.permutation(n)]
    if pattern.startswith("ties"):
        runs = _runs(n, {"ties2_3": (2, 3), "ties8": (8,), "ties13": (13,), "ties40": (40,)}[pattern])
        return _floats(np.repeat(_distinct_bits(rng, len(runs)), runs)[rng.permutation(n)])
    if pattern == "log":
        z = np.exp(rng.uniform(np.log(float(LOG_LO)), 0.0, n)).astype(f32)
        z = np.clip(z, LOG_LO, LOG_HI)
        z[0] = LOG_LO
        if n > 1:
            z[1] = LOG_HI
        return z[rng.permutation(n)]
    if pattern == "band":
        far = max(1, int(round(0.002 * n)))
        z = _floats((BAND_BASE + rng.integers(0, BAND_WIDTH, n)).astype(np.uint32)).copy()
        z[:far] = np.exp(rng.uniform(np.log(1e-20), 0.0, far)).astype(f32)
        return z[rng.permutation(n)]
    raise ValueError(pattern)


def intended(pattern, n):
    """what the pattern promises about a list of n keys: {"span_bits": significant bits of (largest - smallest depth key) or None,
    "runs": {tie-run length: how many} or None}"""
    if n == 0:
        return {"span_bits": 0, "runs": {}}
    if pattern == "one":
        return {"span_bits": 0, "runs": {n: 1}}
    if pattern.startswith("levels"):
        k = min(int(pattern[6:]), n)
        q, r = divmod(n, k)
        runs = {}
        if r:
            runs[q + 1] = r
        if k - r:
            runs[q] = k - r
        return {"span_bits": None, "runs": runs}
    if pattern.startswith("span") or pattern == "consecutive":
        span = int(pattern[4:]) if pattern.startswith("span") else n - 1
        if n < 2:
            return {"span_bits": 0, "runs": {1: n}}
        if span + 1 >= n:
            return {"span_bits": int(span).bit_length(), "runs": {1: n}}
        q, r = divmod(n, span + 1)
        runs = {q: span + 1 - r}
        if r:
            runs[q + 1] = r
        return {"span_bits": int(span).bit_length(), "runs": runs}
    if pattern.startswith("ties"):
        runs = {}
        for r in _runs(n, {"ties2_3": (2, 3), "ties8": (8,), "ties13": (13,), "ties40": (40,)}[pattern]):
            runs[r] = runs.get(r, 0) + 1
        return {"span_bits": None, "runs": runs}
    if pattern == "log":
        return {"span_bits": 30 if n > 1 else 0, "runs": None}
    if pattern in ("uniform", "asc", "desc"):
        return {"span_bits": 23 if n >= 63 else None, "runs": None}        # (the octave has 2^23 patterns; 63 draws span half of it)
    return {"span_bits": None, "runs": None}


def tie_runs(z):
    """{run length: how many} of equal depths in z"""
    if len(z) == 0:
        return {}
    _, counts = np.unique(bits_of(z), return_counts=True)
    lengths, many = np.unique(counts, return_counts=True)
    return {int(a): int(b) for a, b in zip(lengths, many)}


def span_bits(z):
    b = bits_of(z).astype(np.int64)
    return int(b.max() - b.min()).bit_length() if len(b) else 0


class SortScene:
    """cases[k] = (length, pattern) sits in tile column k % tiles_x, row k // tiles_x counted from the BOTTOM of the image (NDC y
    points up): the device's tile tile_of_case[k].  g: the GaussianList (cov3d zero); cam: the camera without a pose."""

    def __init__(self, name, cases, side, seed):
        self.name, self.cases = name, list(cases)
        self.h = self.w = side
        self.tiles_x = self.tiles_y = side // TILE
        self.n_tiles = self.tiles_x * self.tiles_y
        assert side % TILE == 0 and len(self.cases) <= self.n_tiles
        rng = np.random.default_rng(seed)
        n = sum(c[0] for c in self.cases)
        self.n = n
        perm = rng.permutation(n)
        pos = np.zeros((n, 4), f32)
        pos[:, 3] = 1.0
        self.tile_of_case, self.members = [], []
        at = 0
        for k, (length, pattern) in enumerate(self.cases):
            tx, ty = k % self.tiles_x, k // self.tiles_x
            self.tile_of_case.append((self.tiles_y - 1 - ty) * self.tiles_x + tx)
            who = perm[at:at + length]
            at += length
            if pattern in ("asc", "desc"):
                who = np.sort(who)
            pos[who, 0] = f32(((TILE * tx + 8) / side - 0.5) * 2)
            pos[who, 1] = f32(((TILE * ty + 8) / side - 0.5) * 2)
            pos[who, 2] = pattern_depths(pattern, length, rng)
            self.members.append(who)
        self.case_of_tile = {t: k for k, t in enumerate(self.tile_of_case)}
        rot = np.zeros((n, 4), f32)
        rot[:, 3] = 1.0
        sh = np.zeros((n, 48), f32)
        sh[:, :3] = rng.normal(0.0, 1.0, (n, 3)).astype(f32)
        self.g = splat_amd.GaussianList(pos, np.ones((n, 3), f32), rng.uniform(0.01, 0.2, n).astype(f32), rot, sh)
        self.cam = splat_amd.Camera(side, side, (0.0, 0.0, 5.0))          # no update_camera_pose(): identity matrices
        self.depth_bits = bits_of(pos[:, 2])
        self._expected = None
        self._oracle_frame = None

    def cam_c(self):
        return self.cam.to_c(LOWPASS)

    def expected(self):
        """(offsets, order) of the oracle's lists, computed once; read-only"""
        if self._expected is None:
            off, order = expected_tile_lists(self.g, self.cam, self.tiles_x, self.tiles_y, LOWPASS)
            off.setflags(write=False)
            order.setflags(write=False)
            self._expected = (off, order)
        return self._expected

    def oracle_frame(self):
        """(frame, statistics) of the oracle, computed once; read-only"""
        if self._oracle_frame is None:
            ref, ost = O.render(scene_dict(self.g), oracle_camera(self.cam, LOWPASS), nthreads=oracle_threads())
            ref.setflags(write=False)
            self._oracle_frame = (ref, ost)
        return self._oracle_frame

    def what(self, tile):
        k = self.case_of_tile.get(int(tile))
        return "tile %d (no case)" % tile if k is None else "tile %d (%d keys, pattern %s)" % (tile, self.cases[k][0], self.cases[k][1])


def oracle_threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 8)))


_SCENES = {}


def _side_for(n_cases):
    side = TILE
    while (side // TILE) ** 2 < n_cases:
        side += TILE
    return side


def scene(name):
    """"sweep": one list per length of SWEEP_LENGTHS, depths uniform over the octave [0.25, 0.5) (a 23-bit span, with the birthday
    ties that come with it), on 128 x 128.  "patterns": every length of PATTERN_LENGTHS with every pattern of PATTERNS.  "distinct":
    lists without a single tie (consecutive bit patterns).  "sweep_short" / "patterns_short": their lists of up to 2048 keys.
    Built once per process."""
    if name not in _SCENES:
        if name == "sweep":
            s = SortScene(name, [(n, "uniform") for n in SWEEP_LENGTHS], 128, 101)
        elif name == "sweep_short":
            s = SortScene(name, [(n, "uniform") for n in SWEEP_LENGTHS if n <= FUSED_MAX], 128, 102)
        elif name == "patterns":
            cases = [(n, p) for n in PATTERN_LENGTHS for p in PATTERNS]
            s = SortScene(name, cases, _side_for(len(cases)), 103)
        elif name == "patterns_short":
            cases = [(n, p) for n in PATTERN_LENGTHS if n <= FUSED_MAX for p in PATTERNS]
            s = SortScene(name, cases, _side_for(len(cases)), 104)
        elif name == "distinct":
            s = SortScene(name, [(n, "consecutive") for n in DISTINCT_LENGTHS], 64, 105)
        else:
            raise KeyError(name)
        _SCENES[name] = s
    return _SCENES[name]


def forget_scenes():
    _SCENES.clear()


def expected_tile_lists(g, cam, tiles_x, tiles_y, lowpass=0.01):
    """the oracle's tile lists: per-tile counts prefix-summed, and every list in stable depth order (ties by index).  The function
    of the same name in tests/test_gpu_target_shapes.py with the low-pass as an argument (that module stays as it is;
    tests/test_sort_cases_host.py holds the two to each other)."""
    pre = O.preprocess(scene_dict(g), oracle_camera(cam, lowpass))
    glob = O.sort(g.positions, np.array(cam.to_c(lowpass).view[:], np.float32))
    rank = np.empty(len(g), np.int64)
    rank[glob] = np.arange(len(g))
    v = np.nonzero(pre["visible"] == 1)[0]
    tx0, tx1 = pre["px0"][v].astype(np.int64) // TILE, pre["px1"][v].astype(np.int64) // TILE
    ty0, ty1 = pre["py0"][v].astype(np.int64) // TILE, pre["py1"][v].astype(np.int64) // TILE
    assert (tx0 >= 0).all() and (tx1 < tiles_x).all() and (ty0 >= 0).all() and (ty1 < tiles_y).all() and (tx1 >= tx0).all() and (ty1 >= ty0).all()
    nx = tx1 - tx0 + 1
    cnt = nx * (ty1 - ty0 + 1)
    total = int(cnt.sum())
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    local = np.arange(total, dtype=np.int64) - first
    nxr = np.repeat(nx, cnt)
    tile = (np.repeat(ty0, cnt) + local // nxr) * tiles_x + np.repeat(tx0, cnt) + local % nxr
    gi = np.repeat(v, cnt)
    order = gi[np.argsort(tile * len(g) + rank[gi], kind="stable")].astype(np.uint32)
    off = np.zeros(tiles_x * tiles_y + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(tile, minlength=tiles_x * tiles_y))
    return off, order


def describe_mismatch(s, off, order, eoff, eorder):
    """None when the lists (off, order) of scene s are the expected ones; else which list is wrong, where and how: the tile with its
    length and pattern, the first wrong position with the depth bits and indices there, and whether the list holds the expected
    keys at all (a misordered list) or not (a lost or duplicated key)"""
    off = np.asarray(off).astype(np.int64)
    eoff = np.asarray(eoff).astype(np.int64)
    if off.shape != eoff.shape or order.shape != eorder.shape:
        return "%s: %d offsets and %d entries, expected %d and %d" % (s.name, off.size, order.size, eoff.size, eorder.size)
    if not np.array_equal(off, eoff):
        t = int(np.argmax(off != eoff))
        t = max(t - 1, 0)                                  # the list in front of the first wrong offset has the wrong length
        return "%s: %s has %d keys on the device, %d expected" % (s.name, s.what(t), int(off[t + 1] - off[t]), int(eoff[t + 1] - eoff[t]))
    bad = order != eorder
    if not bad.any():
        return None
    tiles = np.unique(np.searchsorted(eoff, np.nonzero(bad)[0], side="right") - 1)
    t = int(tiles[0])
    a, b = int(eoff[t]), int(eoff[t + 1])
    got, want = order[a:b], eorder[a:b]
    p = int(np.argmax(got != want))
    same = np.array_equal(np.sort(got), np.sort(want))
    if same:
        how = "the same keys in another order (misordered)"
    else:
        lost = np.setdiff1d(want, got)
        vals, cnts = np.unique(got, return_counts=True)
        twice = vals[cnts > 1]
        foreign = np.setdiff1d(got, want)
        how = "NOT the same keys: %d lost (first %s), %d held more than once (first %s), %d that do not belong (first %s)" % (
            lost.size, lost[:3].tolist(), twice.size, twice[:3].tolist(), foreign.size, foreign[:3].tolist())

    def at(lst, q):
        if not 0 <= q < len(lst):
            return "-"
        i = int(lst[q])
        return "%d@%08x" % (i, int(s.depth_bits[i])) if i < s.n else "%d@?" % i
    lo, hi = max(p - 1, 0), min(p + 3, b - a)
    return ("%s: %s is wrong from position %d (%d of its entries differ; %d lists differ in all: tiles %s): index@depth-bits on the "
            "device %s, expected %s; %s" % (s.name, s.what(t), p, int((got != want).sum()), tiles.size, tiles[:8].tolist(),
                                           [at(got, q) for q in range(lo, hi)], [at(want, q) for q in range(lo, hi)], how))
