"""The caller's view of a resident scene, kept in numpy, and random programs of scene operations (CPU only; replayed on the
GPU by tests/test_gpu_scene_sequences.py, checked on the model alone by tests/test_scene_model_host.py).

Model holds what a caller who made every call would expect to be resident: the four fields as float32 arrays (in a
GaussianList), the scene's order, and two selection masks A and B of the caller's own.  Every operation is one method, made of
the restatements the per-operation tests already hold the library to -- imported from them, not copied:
transform_cases.transformed, sh_rotate_cases.lib_blocks / rotated_rows, remove_cases.removed / compacted_order /
morton_order, test_gpu_scene_update.block_bounds_np / spoil, test_gpu_select.reference (over the oracle's records),
test_gpu_select_neighbours.within / ref_counts / ref_pass / ref_op / ref_block_pairs, pick_cases.reference_pick, and for PLY
rows the host compile of the encoder (test_gpu_ply_encode.slot_values / rows_of) and the host loader.

program(seed, n0, length) draws a list of steps -- plain dicts with every argument -- from numpy.random.default_rng(seed) and
the model's own state, never from a device: the same list can be run on the model with no GPU.  The EDIT KINDS (EDIT_KINDS)
are walked along a window of a cyclic sequence in which every ordered pair of them occurs once (pair_cycle), so that a handful
of seeds covers all 49 pairs; steps of other kinds lie in between.  Programs that start with DENSE_MIN Gaussians or more end
with a dense scene (tile lists of more than 2048 keys), a camera at rest and an indexed sh rotation."""
import os
import tempfile

import numpy as np

import splat_amd
from splat_amd.gaussians import PLY_PROPS, inria_layout
from oracle import oracle as O
from helpers import oracle_camera, scene_dict
import pick_cases as K
import remove_cases as RC
import scene_gpu
import sh_rotate_cases as SR
import transform_cases as T
from scene_gpu import FIELDS, TARGETS, in_view
from test_gpu_ply_encode import rows_of, slot_values
from test_gpu_scene_update import block_bounds_np, spoil
from test_gpu_select import affine, reference as select_reference
from test_gpu_select_neighbours import ref_block_pairs, ref_counts, ref_op, ref_pass, within
from test_retain_decide import STILL

f32 = np.float32
UNBOUNDED = 0xFFFFFFFF
EDIT_KINDS = ("upload", "update", "update_indexed", "transform_indexed", "rotate_sh_indexed", "remove_compacting", "frames_rest")
INDEXED_EDITS = ("update_indexed", "transform_indexed", "rotate_sh_indexed")
MATRICES = tuple(k for k in T.MATRICES if k != "zero")         # "zero" takes the scene out of view for good: only before a re-upload
ORTHOGONAL = ("identity", "rotation", "mirror")                # the entries of T.MATRICES whose linear part rotate_sh accepts
ROTATIONS = tuple(SR.ROTATIONS)
OPS = ("set", "add", "subtract", "intersect")
OFFSETS = (0, 1, 3)                                            # where put_mask of tests/test_gpu_remove.py places a mask
DENSE_MIN = 2500                                               # Gaussians a dense scene needs for a tile list of more than 2048 keys
REST_FRAMES = STILL + 2
HINTS = "an edit while the near selection holds hints"                                        # the writer's frame is number STILL + 1: the next one is retained


def camera(ti, ci):
    h, w = TARGETS[ti]
    return scene_gpu.cameras(h, w)[ci]


def pair_cycle(k=len(EDIT_KINDS)):
    """a cyclic sequence of k*k symbols 0..k-1 in which every ordered pair (a, b) is adjacent exactly once (de Bruijn, n = 2)"""
    a, seq = [0] * (2 * k), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    assert len(seq) == k * k
    return seq


class _Layout:
    """what ref_block_pairs asks a Renderer for, answered by the model"""

    def __init__(self, model):
        self.m = model

    def scene_layout(self):
        return self.m.orig, self.m.bounds()


class Model:
    def __init__(self):
        self.g = None
        self.n = 0
        self.orig = np.zeros(0, np.uint32)
        self.A = np.zeros(0, np.uint8)
        self.B = np.zeros(0, np.uint8)
        self.scene_id = 0                            # counts installed scenes: uploads and compacting removals
        self._bounds = None
        self._records = {}

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _touched(self, layout=True):
        if layout:
            self._bounds = None
        self._records = {}

    def _install(self, g, orig):
        self.g, self.n, self.orig = g, len(g), np.ascontiguousarray(orig, np.uint32)
        self.scene_id += 1
        self._touched()

    def bounds(self):
        if self._bounds is None:
            self._bounds = block_bounds_np(self.g.positions, self.g.cov3d, self.orig)
        return self._bounds

    def blocks(self):
        return (self.n + 255) // 256

    def records(self, ti, ci):
        if (ti, ci) not in self._records:
            self._records[(ti, ci)] = K.records(self.g, camera(ti, ci))
        return self._records[(ti, ci)]

    def mask(self, name):
        return self.A if name == "A" else self.B

    def finite(self):
        return bool(np.isfinite(self.g.positions).all() and np.isfinite(self.g.cov3d).all())

    def state_bytes(self):
        if self.n == 0:
            return b"empty"
        return b"".join(np.ascontiguousarray(a).tobytes() for a in
                        (self.g.positions, self.g.cov3d, self.g.opacities, self.g.sh, self.orig, self.A, self.B, self.bounds()))

    def oracle_frame(self, ti, ci):
        return O.render(scene_dict(self.g), oracle_camera(camera(ti, ci), 0.01), nthreads=8)[0]

    def block_pairs(self, radius):
        return ref_block_pairs(_Layout(self), radius)

    # ---- the scenes the steps name ---------------------------------------------------------------------------------------
    @staticmethod
    def source(n, seed, spoiled=False, dense=False):
        g = in_view(n, seed)
        if dense:                                    # every Gaussian over the tiles at the middle of the target: tile lists of
            g.positions[:, :3] *= f32(0.02)          # more than 2048 keys, for which the near selection keeps hints
        return spoil(g) if spoiled else g

    def ply_rows(self):
        """the model's values as rows of the canonical INRIA layout, by the host compile of the encoder"""
        g = self.g
        return rows_of(slot_values(g.positions, g.cov3d, g.opacities, g.sh), inria_layout(self.n))

    @staticmethod
    def loaded_from_rows(rows):
        """what the loader makes of such rows: activations, recentring, and the covariances of the decoded shapes"""
        n = len(rows)
        fd, path = tempfile.mkstemp(suffix=".ply")
        try:
            with os.fdopen(fd, "wb") as f:
                f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n)
                for p in PLY_PROPS:
                    f.write(("property float %s\n" % p).encode())
                f.write(b"end_header\n")
                f.write(np.ascontiguousarray(rows).tobytes())
            g = splat_amd.load_from_ply(path)
        finally:
            os.unlink(path)
        g.cov3d = O.compute_cov3d(g.scales, g.rotations)
        return g

    # ---- one method per operation; each returns what the call is expected to give back -----------------------------------------
    def apply(self, step):
        return getattr(self, "do_" + step["kind"])(step)

    def do_upload(self, s):
        out = {}
        if s["variant"] == "ply_rows":
            out["rows"] = self.ply_rows()
            g = self.loaded_from_rows(out["rows"])
        else:
            g = self.source(s["n"], s["seed"], s["spoiled"], s["dense"])
        assert len(g) == s["n"]
        self._install(g, RC.morton_order(g.positions))
        self.A, self.B = np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        return out

    def do_update(self, s):
        src = self.source(self.n, s["seed"])
        for f in s["fields"]:
            getattr(self.g, f)[...] = getattr(src, f)
        self._touched()
        return {}

    def do_update_indexed(self, s):
        src, idx = self.source(self.n, s["seed"]), s["index"].astype(np.int64)
        for f in s["fields"]:
            getattr(self.g, f)[idx] = getattr(src, f)[idx]
        self._touched()
        return {"rows": {f: np.ascontiguousarray(getattr(src, f)[idx]) for f in s["fields"]}}

    def do_transform(self, s):
        m = T.MATRICES[s["matrix"]]
        rows = None if s["index"] is None else s["index"].astype(np.int64)
        self.g.positions, self.g.cov3d = T.transformed(self.g, m, rows)
        if s["rotate_sh"]:
            self.g.sh = SR.rotated_rows(SR.lib_blocks(np.ascontiguousarray(m[:, :3])), self.g.sh, rows)
        self._touched()
        return {}

    def do_rotate_sh(self, s):
        rows = None if s["index"] is None else s["index"].astype(np.int64)
        self.g.sh = SR.rotated_rows(SR.lib_blocks(SR.ROTATIONS[s["rotation"]]), self.g.sh, rows)
        self._touched(layout=False)
        return {}

    def removal_mask(self, s):
        return self.mask(s["mask"]).copy() if isinstance(s["mask"], str) else s["mask"]

    def do_remove(self, s):
        sel = self.removal_mask(s)
        E, index_map = RC.removed(self.g, sel, s["keep"])
        out = {"n_out": len(E), "index_map": index_map, "n_before": self.n}
        if len(E) == self.n:
            return out
        if len(E) == 0:
            self.g, self.n, self.orig = None, 0, np.zeros(0, np.uint32)
            self.A, self.B = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
            self._touched()
            return out
        stay = index_map != RC.GONE
        self.A, self.B = self.A[stay].copy(), self.B[stay].copy()          # the caller carries its masks across with the map
        self._install(E, RC.compacted_order(self.orig, index_map))
        return out

    def do_select(self, s):
        h, w = TARGETS[s["ti"]]
        rec = self.records(s["ti"], s["ci"])
        passes = select_reference(self.g, rec, w, h, **s["query"])
        new, count = ref_op(self.mask(s["into"]), passes, s["op"])
        setattr(self, s["into"], new)
        return {"bytes": new, "count": count}

    def do_selection_indices(self, s):
        return {"indices": np.flatnonzero(self.mask(s["of"])).astype(np.uint32)}

    def do_select_neighbours(self, s):
        adj = within(self.g.positions, s["radius"])
        source = self.mask(s["into"]) if s["source_is_selection"] else None
        c = ref_counts(adj, source, s["at_most"])
        new, count = ref_op(self.mask(s["into"]), ref_pass(c, s["at_least"], s["at_most"]), s["op"])
        setattr(self, s["into"], new)
        return {"bytes": new, "count": count, "counts": c.astype(np.uint32), "block_pairs": self.block_pairs(s["radius"])}

    def do_neighbours_refused(self, s):
        return {"block_pairs": self.block_pairs(s["radius"])}

    def do_pick(self, s):
        res, lay, _ = K.reference_pick(self.records(s["ti"], s["ci"]), O.default_conventions(), s["pixels"], max_layers=s["layers"])
        return {"results": res, "layers": lay}

    def do_read(self, s):
        return {}

    def do_read_indexed(self, s):
        idx = s["index"].astype(np.int64)
        rows = {f: np.ascontiguousarray(getattr(self.g, f)[idx]) for f in s["fields"]}
        if "positions" in rows:
            rows["positions"][:, 3] = f32(1.0)
        return {"rows": rows}

    def do_encode(self, s):
        return {}

    def do_frames(self, s):
        return {}


# ---- the program generator ----------------------------------------------------------------------------------------------------
def _indices(rng, n, how):
    """distinct, unsorted indices: k = 0, 1, some, n"""
    k = {"none": 0, "one": 1, "some": max(1, min(n, int(rng.integers(2, max(3, n // 3 + 1))))), "all": n}[how]
    return rng.permutation(n)[:k].astype(np.uint32)


def _field_subset(rng):
    while True:
        pick = [f for f in FIELDS if rng.random() < 0.5]
        if pick:
            return tuple(pick)


def _query(rng, model, ti, ci):
    h, w = TARGETS[ti]
    kind = ("box", "ellipsoid", "centre", "touch", "depth", "opacity")[int(rng.integers(6))]
    if kind in ("box", "ellipsoid"):
        centre, half = rng.uniform(-0.5, 0.5, 3), rng.uniform(0.8, 2.5, 3)
        return kind, {kind: affine(centre, half, float(rng.uniform(-0.3, 0.3)))}
    if kind in ("centre", "touch"):
        x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
        rect = (x0, y0, int(rng.integers(x0, w)), int(rng.integers(y0, h)))
        return kind, dict(rect=rect, rule=kind)
    if kind == "depth":
        d = model.records(ti, ci)["depth"]
        d = d[np.isfinite(d)]
        lo, hi = (np.percentile(d, 25), np.percentile(d, 75)) if len(d) else (0.0, 1.0)
        return kind, dict(depth=(f32(lo), f32(hi)))
    lo = float(rng.uniform(0.0, 0.5))
    return kind, dict(opacity=(lo, lo + float(rng.uniform(0.2, 0.5))))


def _removal_mask(rng, model, want):
    """(name, mask or "A" / "B", keep) for a removal whose outcome is `want`: "compacting", "crossing" (compacting, and fewer
    blocks afterwards), "nothing" or "everything" -- drawn, tried on the model, drawn again"""
    n = model.n
    for _ in range(64):
        keep = bool(rng.integers(2))
        name = ("A", "B", "random 1 %", "random 50 %", "random 99 %", "leaves 1", "leaves 255", "leaves 256", "leaves 257")[int(rng.integers(9))]
        if want == "nothing":
            name, mask = "removes nothing", (np.ones(n, np.uint8) if keep else np.zeros(n, np.uint8))
        elif want == "everything":
            name, mask = "removes everything", (np.zeros(n, np.uint8) if keep else np.ones(n, np.uint8))
        elif name in ("A", "B"):
            mask = name
        elif name.startswith("random"):
            mask = (rng.random(n) < int(name.split()[1]) / 100.0).astype(np.uint8)
        else:
            left = int(name.split()[1])
            if left >= n:
                continue
            stay = np.zeros(n, bool)
            stay[rng.permutation(n)[:left]] = True
            mask = (stay if keep else ~stay).astype(np.uint8)
        sel = model.mask(mask) if isinstance(mask, str) else mask
        n2 = int(RC.survives(sel, keep).sum())
        ok = {"nothing": n2 == n, "everything": n2 == 0, "compacting": 0 < n2 < n,
              "crossing": 0 < n2 and (n2 + 255) // 256 < (n + 255) // 256}[want]
        if ok:
            return name, mask, keep
    raise AssertionError("no %s removal of %d Gaussians found" % (want, n))


def program(seed, n0, length=24):
    """[step]: every step a dict with its kind, its arguments and, from the model the generator runs beside it, `edit` (its
    EDIT KIND, or None), `ends_frames` (does the call end the frames in flight and what the scheduler learnt), `n_before` and
    `n_after`"""
    rng = np.random.default_rng(seed)
    model = Model()
    steps = []
    state = {"crossed": False, "uploads": 0}

    def emit(step, edit=None, ends_frames=None):
        step["edit"] = edit
        step["n_before"] = model.n
        step["ends_frames"] = (edit is not None and edit != "frames_rest") if ends_frames is None else ends_frames
        model.apply(step)
        step["n_after"] = model.n
        steps.append(step)

    def upload(n=None, dense=None):
        first, given = state["uploads"] == 0, n is not None
        state["uploads"] += 1
        if first:
            n = n0
        if n is None:
            # until a removal has crossed a block boundary the scene stays at more than one block
            sizes = [k for k in ((257, n0 // 2 + 1, n0) if not state["crossed"] else (1, 255, 256, 257, n0 // 2 + 1, n0)) if k <= n0]
            n = int(sizes[int(rng.integers(len(sizes)))])
        variant = ("host", "device", "ply_rows", "ply_rows")[int(rng.integers(4))]
        if variant == "ply_rows" and (first or given or model.n == 0 or not model.finite()):
            variant = ("host", "device")[int(rng.integers(2))]
        if variant == "ply_rows":
            n = model.n
        emit(dict(kind="upload", variant=variant, n=n, seed=int(rng.integers(1 << 30)), spoiled=bool(variant == "host" and n >= 8 and rng.random() < 0.34),
                  dense=bool((rng.random() < 0.5 or dense) and variant != "ply_rows" and n >= DENSE_MIN)), edit="upload")

    def indexed_edit(kind, how=None):
        how = how or ("one", "some", "all")[int(rng.integers(3))]
        idx = _indices(rng, model.n, how)
        edit = kind if len(idx) else None
        if kind == "update_indexed":
            emit(dict(kind=kind, index=idx, fields=_field_subset(rng), seed=int(rng.integers(1 << 30))), edit=edit)
        elif kind == "transform_indexed":
            name = MATRICES[int(rng.integers(len(MATRICES)))]
            emit(dict(kind="transform", matrix=name, index=idx, rotate_sh=bool(name in ORTHOGONAL and rng.random() < 0.5)), edit=edit)
        else:
            emit(dict(kind="rotate_sh", rotation=ROTATIONS[int(rng.integers(len(ROTATIONS)))], index=idx), edit=edit)

    def indexed_read():
        idx = rng.integers(0, model.n, int(rng.integers(1, model.n + 1))).astype(np.uint32)      # duplicates allowed
        if rng.random() < 0.5:
            emit(dict(kind="read_indexed", index=idx, fields=_field_subset(rng)))
        else:
            emit(dict(kind="encode", index=idx))

    def removal(want):
        name, mask, keep = _removal_mask(rng, model, want)
        compacting = want in ("compacting", "crossing")
        if compacting and (int(RC.survives(model.mask(mask) if isinstance(mask, str) else mask, keep).sum()) + 255) // 256 < model.blocks():
            state["crossed"] = True
        emit(dict(kind="remove", name=name, mask=mask, keep=keep, offset=OFFSETS[int(rng.integers(3))], with_map=bool(rng.random() < 0.7)),
             edit="remove_compacting" if compacting else None, ends_frames=want != "nothing")

    def frames_rest():
        emit(dict(kind="frames", variant="rest", ti=int(rng.integers(2)), ci=0), edit="frames_rest")

    def filler():
        ti, ci = int(rng.integers(2)), int(rng.integers(4))
        which = ("select", "select", "select", "selection_indices", "floaters", "grow", "refused", "pick", "pick", "read", "read_indexed", "encode",
                 "no indices", "transform", "rotate_sh", "tour")[int(rng.integers(16))]
        into = "AB"[int(rng.integers(2))]
        if which == "select":
            name, q = _query(rng, model, ti, ci)
            emit(dict(kind="select", name=name, query=q, ti=ti, ci=ci, into=into, op=OPS[int(rng.integers(4))]))
        elif which == "selection_indices":
            emit(dict(kind="selection_indices", of=into))
        elif which in ("floaters", "grow"):
            spread = float(np.nanstd(np.where(np.isfinite(model.g.positions[:, :3]), model.g.positions[:, :3], np.nan))) if model.n > 1 else 1.0
            spread = spread if np.isfinite(spread) and spread > 0 else 1.0
            while True:                                        # the default limit is never what stops it: judged on the model
                radius = float(f32(spread * rng.uniform(0.05, 0.5)))
                if model.block_pairs(radius) <= 64 * model.blocks():
                    break
            if which == "floaters":
                emit(dict(kind="select_neighbours", radius=radius, into=into, source_is_selection=False, at_least=0, at_most=int(rng.integers(4)),
                          op=OPS[int(rng.integers(4))]))
            else:
                emit(dict(kind="select_neighbours", radius=radius, into=into, source_is_selection=True, at_least=1, at_most=UNBOUNDED, op="add"))
        elif which == "refused":
            radius = float(f32(rng.uniform(0.1, 2.0)))
            pairs = model.block_pairs(radius)
            if pairs >= 2:                                     # (a limit of pairs - 1 >= 1: 0 would mean "no limit")
                emit(dict(kind="neighbours_refused", radius=radius, into=into, max_block_pairs=pairs - 1))
        elif which == "pick":
            h, w = TARGETS[ti]
            k = int(rng.integers(1, 9))
            px = np.stack([rng.integers(w // 4, (3 * w) // 4, k), rng.integers(h // 4, (3 * h) // 4, k)], 1).astype(np.int32)
            px[0] = (w // 2, h // 2)
            emit(dict(kind="pick", pixels=px, layers=(0, 3)[int(rng.integers(2))], ti=ti, ci=ci))
        elif which == "read":
            emit(dict(kind="read", fields=_field_subset(rng)))
        elif which == "read_indexed":
            indexed_read()
        elif which == "encode":
            emit(dict(kind="encode", index=None))
        elif which == "no indices":
            indexed_edit(INDEXED_EDITS[int(rng.integers(3))], "none")
        elif which == "transform":
            name = MATRICES[int(rng.integers(len(MATRICES)))]
            emit(dict(kind="transform", matrix=name, index=None, rotate_sh=bool(name in ORTHOGONAL and rng.random() < 0.5)), ends_frames=True)
        elif which == "rotate_sh":
            emit(dict(kind="rotate_sh", rotation=ROTATIONS[int(rng.integers(len(ROTATIONS)))], index=None), ends_frames=True)
        else:
            emit(dict(kind="frames", variant="tour"))

    # the edit kinds: a window of the pair cycle, then whatever this program still lacks
    cycle = pair_cycle()
    at = int(rng.integers(len(cycle)))
    window = max(6, length // 2 - 1)
    chain = [EDIT_KINDS[cycle[(at + j) % len(cycle)]] for j in range(window)]
    if "frames_rest" not in chain[:-1]:
        chain += ["frames_rest", INDEXED_EDITS[int(rng.integers(3))]]
    if "remove_compacting" not in chain:
        chain.append("remove_compacting")
    later_uploads = [j for j, e in enumerate(chain) if e == "upload"]
    empties_before = later_uploads[int(rng.integers(len(later_uploads)))] if later_uploads else len(chain)
    nothing_before = int(rng.integers(len(chain)))
    gaps = max(0, length - len(chain) - (4 if n0 < DENSE_MIN else 8))       # how many fillers the length leaves room for

    upload()
    indexed_read() if rng.random() < 0.5 else indexed_edit(INDEXED_EDITS[int(rng.integers(3))])
    for j, kind in enumerate(chain + [None]):
        after_install = steps[-1]["edit"] in ("upload", "remove_compacting")
        if not after_install and rng.random() < gaps / float(len(chain)):
            filler()
        if j == nothing_before:
            removal("nothing")
        if j == empties_before:
            if rng.random() < 0.5:                              # the one place for the matrix that takes everything out of view
                idx = None if rng.random() < 0.5 else _indices(rng, model.n, "some")
                emit(dict(kind="transform", matrix="zero", index=idx, rotate_sh=False), ends_frames=True)
            removal("everything")
            if kind != "upload":
                upload()
                indexed_read()
        if kind is None:
            break
        if kind == "upload":
            upload()
        elif kind == "update":
            emit(dict(kind="update", fields=_field_subset(rng), seed=int(rng.integers(1 << 30))), edit="update")
        elif kind in INDEXED_EDITS:
            indexed_edit(kind)
        elif kind == "frames_rest":
            frames_rest()
        else:
            if model.n < 2:
                upload(min(n0, 257))
            removal("compacting" if state["crossed"] or model.blocks() < 2 else "crossing")
        # an indexed call is the first call behind an upload and behind a compacting removal: the inverse order is made, and made
        # again for another n
        next_is_indexed = j + 1 < len(chain) and chain[j + 1] in INDEXED_EDITS and j + 1 not in (nothing_before, empties_before)
        if kind in ("upload", "remove_compacting") and not next_is_indexed:
            indexed_read()
    if n0 >= DENSE_MIN:
        # where tile lists are long the near selection learns from a camera at rest: an edit that moves nothing arrives then, and
        # what was learnt must go all the same
        upload(n0, dense=True)
        indexed_read()
        frames_rest()
        indexed_edit("rotate_sh_indexed")
    return steps


def is_indexed_call(step):
    """does the step hand the library a non-empty index list (the calls that need the inverse order)?"""
    return step.get("index") is not None and len(step["index"]) > 0


def dense_at(steps, i):
    """is the scene of step i a dense upload that nothing has moved or thinned since?"""
    last = max(j for j in range(i) if steps[j]["kind"] == "upload")
    return steps[last]["dense"] and not any(t["kind"] in ("transform", "remove", "update", "update_indexed") and t["ends_frames"] for t in steps[last:i])


def events(steps):
    """{event: [step numbers]} of the things every program must contain (tests/test_scene_model_host.py)"""
    found = {"indexed call first after an upload": [], "indexed call first after a compacting removal": [],
             "a removal crosses a block boundary": [], "a removal of nothing": [], "a removal of everything, then an upload": [],
             "an edit while retention runs": [], "an edit while the near selection holds hints": []}
    at_rest = False
    long_lists = False                               # a camera has rested on a dense scene: the near selection has hints
    for i, s in enumerate(steps):
        if s["kind"] == "upload":
            long_lists = False
        if s["kind"] == "frames" and s["variant"] == "rest" and s["n_before"] >= DENSE_MIN and dense_at(steps, i):
            long_lists = True
        if s["ends_frames"] and long_lists:
            found["an edit while the near selection holds hints"].append((i, s["edit"]))
            long_lists = False
        before = steps[i - 1] if i else None
        if before is not None and is_indexed_call(s):
            if before["kind"] == "upload":
                found["indexed call first after an upload"].append(i)
            if before["edit"] == "remove_compacting":
                found["indexed call first after a compacting removal"].append(i)
        if s["kind"] == "remove":
            if 0 < s["n_after"] and (s["n_after"] + 255) // 256 < (s["n_before"] + 255) // 256:
                found["a removal crosses a block boundary"].append(i)
            if s["n_after"] == s["n_before"]:
                found["a removal of nothing"].append(i)
            if s["n_after"] == 0 and i + 1 < len(steps) and steps[i + 1]["kind"] == "upload":
                found["a removal of everything, then an upload"].append(i)
        if s["kind"] == "frames":
            at_rest = s["variant"] == "rest"
        elif s["ends_frames"]:
            if at_rest:
                found["an edit while retention runs"].append(i)
            at_rest = False
    return found


def assert_state(s, model, what=""):
    """what a session `s` holds is the model's: the count, the four fields bit for bit, the order and the block bounds.  (s: a
    scene_gpu.Session, or anything with R.n, R.scene_layout() and read_all(n).)"""
    assert s.R.n == model.n, "%s: n is %d, the model's %d" % (what, s.R.n, model.n)
    orig, bounds = s.R.scene_layout()
    assert np.array_equal(orig, model.orig), "%s: the scene's order is not the model's" % what
    if model.n == 0:
        return
    scene_gpu.assert_resident(s, model.g, what)
    scene_gpu.assert_bounds(bounds, model.bounds(), what)


def edit_pairs(steps):
    """[(kind, kind)]: the edit kinds of a program, each with the one that follows it"""
    kinds = [s["edit"] for s in steps if s["edit"] is not None]
    return list(zip(kinds, kinds[1:]))
