"""Append and reorder among the other scene operations, held step by step to the numpy model (tests/scene_model.py with the two
operations added; -m gpu).  The programs are FIXED and written out below: in them an append and a reorder each stand directly
before and directly after each of the seven edit kinds of scene_model.EDIT_KINDS, and next to each other in both orders.  They
are replayed by tests/test_gpu_scene_sequences.py's Replay, unchanged but for the two new steps: after EVERY step the four
resident fields, n, the scene's order and the block bounds are the model's bit for bit and no frame was dropped, the first
frame behind an edit is binned and is the fresh upload's, and at every frames step frames, records, tile lists and counts are
those of a FRESH Renderer that took the model's arrays through splat_upload_scene.  The caller's masks A and B grow by m zero
bytes at an append.  Nothing here has a tolerance."""
import numpy as np
import pytest

import append_cases as AC
import scene_model as M
from scene_gpu import session
from test_gpu_scene_sequences import Replay, brief

MODE_LIBM_EXP = 2


# ---- the model and the replay, with the two operations ---------------------------------------------------------------------------
class Model(M.Model):
    def do_append(self, s):
        m = s["m"]
        out = {"n_out": self.n + m}
        if m == 0:
            return out
        extra = self.source(m, s["seed"], s["spoiled"])
        order = AC.appended_order(self.orig, extra.positions)
        self.A = np.concatenate([self.A, np.zeros(m, np.uint8)])       # the caller's masks grow with the scene: nothing new is selected
        self.B = np.concatenate([self.B, np.zeros(m, np.uint8)])
        self._install(AC.appended(self.g, extra), order)
        return out

    def do_reorder(self, s):
        want = AC.reordered_order(self.g.positions)
        moved = int((want != self.orig).sum())
        if moved:
            self._install(self.g, want)
        return {"moved": moved}


class AppendReplay(Replay):
    def __init__(self, s, mode):
        super().__init__(s, mode)
        self.model = Model()

    def run_append(self, step, out, n, what):
        m = step["m"]
        if m == 0:
            got = self.measured(lambda: self.R.append(0, 0, 0, 0, m=0), n, False)
        else:
            d = self.s.device(M.Model.source(m, step["seed"], step["spoiled"]))
            got = self.R.append(d) if step["whole"] else self.R.append(d.positions, d.cov3d, d.opacities, d.sh, m=m)
        assert got == out["n_out"] == self.R.n, "%s: n is %d after the append, the model has %d" % (what, got, out["n_out"])
        if m:
            self.new_masks()
        else:
            for name in "AB":
                self.assert_mask(name, what)

    def run_reorder(self, step, out, n, what):
        held = self.R.device_bytes()[0]
        moved = self.R.reorder()
        assert moved == out["moved"], "%s: %d slots moved, the model has %d" % (what, moved, out["moved"])
        if moved == 0:
            assert self.R.device_bytes()[0] == held, what + ": a reorder that moves nothing is a read"
        for name in "AB":                                              # indices do not change: the caller's masks stay good
            self.assert_mask(name, what)


# ---- the programs -----------------------------------------------------------------------------------------------------------------
def every(k, first=0):
    """n -> the indices first, first + k, ... below n, descending (distinct, unsorted as far as the library can tell)"""
    return lambda n: np.arange(first, n, k, dtype=np.uint32)[::-1].copy()


def mask_every(k):
    return lambda n: (np.arange(n) % k == 0).astype(np.uint8)


def append(m, seed, spoiled=False, whole=False):
    return dict(kind="append", m=m, seed=seed, spoiled=spoiled, whole=whole)


REORDER = dict(kind="reorder")
TOUR = dict(kind="frames", variant="tour")
# one step of each edit kind, in EDIT_KINDS' order; a function of n where the arguments depend on it
EDITS = {
    "upload": lambda n0: dict(kind="upload", variant="device", n=n0, seed=31, spoiled=False, dense=False),
    "update": lambda n0: dict(kind="update", fields=("positions", "sh"), seed=32),
    "update_indexed": lambda n0: dict(kind="update_indexed", index=every(3, 1), fields=("positions", "cov3d", "opacities"), seed=33),
    "transform_indexed": lambda n0: dict(kind="transform", matrix="shear", index=every(4), rotate_sh=False),
    "rotate_sh_indexed": lambda n0: dict(kind="rotate_sh", rotation="rot20", index=every(2, 1)),
    "remove_compacting": lambda n0: dict(kind="remove", name="every third", mask=mask_every(3), keep=False, offset=1, with_map=True),
    "frames_rest": lambda n0: dict(kind="frames", variant="rest", ti=1, ci=0),
}
assert tuple(EDITS) == M.EDIT_KINDS


def chain(n0, kinds, sizes, spoiled_first, spoil_appends=True):
    """upload, append, then for every kind K: K, reorder, K, append -- append -> K, K -> reorder, reorder -> K, K -> append --
    and at the end reorder, append, reorder: the two next to each other in both orders.  sizes: the m of every append in turn."""
    sizes = iter(sizes)
    steps = [dict(kind="upload", variant="host", n=n0, seed=30, spoiled=spoiled_first, dense=False),
             append(next(sizes), 40, whole=True)]
    for j, kind in enumerate(kinds):
        steps += [EDITS[kind](n0), REORDER, EDITS[kind](n0), append(next(sizes), 41 + j, spoiled=spoil_appends and j % 2 == 1, whole=j % 2 == 0)]
    return steps + [REORDER, append(next(sizes), 60), REORDER, TOUR, append(0, 0), TOUR]


# (1000 + 24 and 257 + 255 end on a block boundary, 255 + 1 fills a block, + 2 crosses into the next, 256 + 1 opens one)
PROGRAMS = {
    "n257-first-half": chain(257, M.EDIT_KINDS[:4], (255, 1, 300, 24, 2, 100), True),
    "n257-second-half": chain(257, M.EDIT_KINDS[4:], (1, 257, 24, 255, 100), False),
    "n1000-first-half": chain(1000, M.EDIT_KINDS[:4], (24, 1000, 1, 255, 300, 100), False),
    "n1000-second-half": chain(1000, M.EDIT_KINDS[4:], (300, 24, 1000, 1, 100), True),
    # Replay.finish holds the last frame of a MODE_LIBM_EXP program to the ORACLE's frame of the model's arrays.  The oracle and the
    # library part ways on Gaussians without a finite centre -- a fresh splat_upload_scene of such arrays included: 220 and 470
    # pixels of the frames the two programs above end with -- so the programs that end at the oracle keep to finite rows; the
    # others hold those rows to a fresh upload, as every per-operation module does.
    "n257-second-half-finite": chain(257, M.EDIT_KINDS[4:], (1, 257, 24, 255, 100), False, spoil_appends=False),
    "n1000-first-half-finite": chain(1000, M.EDIT_KINDS[:4], (24, 1000, 1, 255, 300, 100), False, spoil_appends=False),
}
LIBM = ("n257-second-half-finite", "n1000-first-half-finite")
CASES = [(name, 0) for name in PROGRAMS if name not in LIBM] + [(name, MODE_LIBM_EXP) for name in LIBM]


def program(name):
    """the steps of PROGRAMS[name] in scene_model.program()'s format: the arguments that depend on n made from the model's n, and
    `edit`, `ends_frames`, `n_before` and `n_after` from the model the steps are run on here"""
    model, steps = Model(), []
    for spec in PROGRAMS[name]:
        step = {k: (v(model.n) if callable(v) else v) for k, v in spec.items()}
        kind = step["kind"]
        step["n_before"] = model.n
        out = model.apply(step)
        step["n_after"] = model.n
        # `role`: where the step stands in the program; `edit`: what it did -- an append of nothing and a reorder of a scene in
        # order (directly behind an upload) are reads
        if kind == "append":
            step["role"], changed = ("append" if step["m"] else None), step["m"] > 0
        elif kind == "reorder":
            step["role"], changed = "reorder", out["moved"] > 0
        elif kind == "frames":
            step["role"], changed = ("frames_rest" if step["variant"] == "rest" else None), False
        else:
            step["role"], changed = {"transform": "transform_indexed", "rotate_sh": "rotate_sh_indexed", "remove": "remove_compacting"}.get(kind, kind), True
            assert kind != "remove" or 0 < step["n_after"] < step["n_before"], "the removals of these programs compact"
        step["edit"] = step["role"] if changed or kind == "frames" else None
        step["ends_frames"] = changed
        steps.append(step)
    return steps


def test_the_programs_put_both_calls_before_and_after_every_edit_kind():
    """(no GPU is used: the programs are run on the model alone)"""
    pairs, moving = set(), 0
    for name in PROGRAMS:
        steps = program(name)
        roles = [s["role"] for s in steps]
        pairs |= set(zip(roles, roles[1:]))
        moving += sum(s["edit"] == "reorder" for s in steps)
        assert all(s["edit"] == "reorder" or steps[i - 1]["kind"] in ("upload", "reorder") for i, s in enumerate(steps) if s["kind"] == "reorder"), \
            name + ": a reorder moves something unless the scene has just been put in order"
    assert moving >= 20
    for new in ("append", "reorder"):
        for kind in M.EDIT_KINDS:
            assert (new, kind) in pairs and (kind, new) in pairs, (new, kind)
    assert ("append", "reorder") in pairs and ("reorder", "append") in pairs
    steps = program("n257-first-half")
    assert [s["n_after"] for s in steps if s["kind"] == "append"][0] == 512


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", CASES, ids=["%s%s" % (n, "-libm_exp" if m else "") for n, m in CASES])
def test_a_fixed_program_stays_the_models(name, mode):
    steps = program(name)
    with session(mode=mode) as s:
        replay = AppendReplay(s, mode)
        edits = []
        for i, step in enumerate(steps):
            what = "%s, step %d (%s)" % (name, i, step["kind"])
            try:
                replay.run(i, step, what)
            except Exception as e:
                raise AssertionError("%s failed: %s\n  arguments: %r\n  the two edits before it: %r\n  the steps so far: %s" % (
                    what, e, brief(step), edits[-2:], " ".join(t["kind"] for t in steps[:i + 1]))) from e
            if step["edit"] is not None:
                edits.append(step["edit"])
        replay.finish("%s, after the last step" % name)
        assert s.R.frames_dropped() == 0
