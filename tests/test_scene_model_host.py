"""The programs tests/test_gpu_scene_sequences.py replays on the GPU, run here on the model alone (tests/scene_model.py; no
GPU): what is asserted are conditions on the INPUTS of that test -- that the committed (seed, n0) programs between them put
every edit kind directly behind every other, that each of them contains the state changes the sequence test exists for, that
its indices are in range and its scene stays in view -- and that the model is deterministic.  The last test shows, with the
perturbation on the EXPECTED side, that the per-step comparison of the sequence test flags an order that was not compacted."""
import numpy as np
import pytest

import remove_cases as RC
import scene_model as M
from scene_gpu import FIELDS, PER

f32 = np.float32
LENGTH = 24
# (seed, n0): chosen so that the pair coverage below holds; 4097 bytes of mask are one SELECT_SPAN plus one
PROGRAMS = ((1, 257), (2, 257), (11, 257), (18, 257), (1, 1000), (2, 1000), (12, 1000), (21, 1000), (1, 4097), (2, 4097), (3, 4097), (6, 4097))
IDS = ["seed%d-n%d" % p for p in PROGRAMS]
_MADE = {}


def steps_of(seed, n0):
    if (seed, n0) not in _MADE:
        _MADE[(seed, n0)] = M.program(seed, n0, LENGTH)
    return _MADE[(seed, n0)]


def frozen(v):
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, dict):
        return tuple((k, frozen(v[k])) for k in sorted(v))
    if isinstance(v, (tuple, list)):
        return tuple(frozen(x) for x in v)
    return repr(v)


def run(steps, frames=False):
    """the program on a new model: ([state bytes after each step], [(step, was the oracle's frame non-empty)])"""
    model, states, seen = M.Model(), [], []
    for i, s in enumerate(steps):
        out = model.apply(s)
        states.append(model.state_bytes() + repr(frozen(out)).encode())
        assert model.n == s["n_after"]
        if frames and s["kind"] == "frames":
            ti, ci = (s["ti"], s["ci"]) if s["variant"] == "rest" else (1, 0)
            seen.append((i, bool(model.oracle_frame(ti, ci).any())))
    return states, seen


def test_every_ordered_pair_of_edit_kinds_occurs():
    count = {}
    for seed, n0 in PROGRAMS:
        for pair in M.edit_pairs(steps_of(seed, n0)):
            count[pair] = count.get(pair, 0) + 1
    print("\n%-20s" % "first \\ then" + "".join("%19s" % k for k in M.EDIT_KINDS))
    for a in M.EDIT_KINDS:
        print("%-20s" % a + "".join("%19d" % count.get((a, b), 0) for b in M.EDIT_KINDS))
    missing = [(a, b) for a in M.EDIT_KINDS for b in M.EDIT_KINDS if (a, b) not in count]
    assert not missing, "no program has %r" % (missing,)
    assert {n0 for _, n0 in PROGRAMS} == {257, 1000, 4097}
    # ... and an indexed sh rotation, which moves nothing, arrives while the near selection holds hints of a dense scene's frames
    held = [(p, at) for p in PROGRAMS for at in M.events(steps_of(*p))[M.HINTS]]
    print("edits while the near selection holds hints: %r" % (held,))
    assert any(kind == "rotate_sh_indexed" for _, (_, kind) in held)


@pytest.mark.parametrize("seed,n0", PROGRAMS, ids=IDS)
def test_the_program_contains_what_the_sequence_test_is_for(seed, n0):
    steps = steps_of(seed, n0)
    found = M.events(steps)
    print("\nseed %d, n0 %d: %d steps: %s" % (seed, n0, len(steps), " ".join(s["kind"] for s in steps)))
    for name, at in found.items():
        print("  %-48s at %s" % (name, at))
    for name, at in found.items():
        # (tile lists of more than 2048 keys take a scene of thousands: what rests on them is asked of the programs together)
        assert at or name == M.HINTS, "seed %d, n0 %d: %s does not occur" % (seed, n0, name)
    assert abs(len(steps) - LENGTH) <= 8
    assert steps[0]["kind"] == "upload" and steps[0]["n"] == n0
    for i, s in enumerate(steps):
        assert s["n_before"] <= n0 and s["n_after"] <= n0
        if s.get("index") is not None:
            assert s["index"].dtype == np.uint32 and (s["index"] < s["n_before"]).all(), "step %d" % i
            if s["kind"] not in ("read_indexed", "encode"):
                assert len(np.unique(s["index"])) == len(s["index"]), "step %d: the indices of an edit are distinct" % i
        if s["kind"] == "transform" and s["matrix"] == "zero":      # only as the last edit before a re-upload
            rest = [t for t in steps[i + 1:] if t["ends_frames"] or t["kind"] == "frames"]
            assert rest and (rest[0]["kind"] == "upload" or (rest[0]["kind"] == "remove" and rest[0]["n_after"] == 0)), "step %d" % i
        if s["kind"] in ("select_neighbours", "neighbours_refused"):
            assert np.isfinite(s["radius"]) and s["radius"] >= 0


@pytest.mark.parametrize("seed,n0", PROGRAMS, ids=IDS)
def test_the_model_is_deterministic_and_the_scene_stays_in_view(seed, n0):
    steps = steps_of(seed, n0)
    again = M.program(seed, n0, LENGTH)
    assert frozen(steps) == frozen(again), "the generator gives the same program twice"
    first, seen = run(steps, frames=True)
    second, _ = run(again)
    assert first == second, "two runs of the program give identical bytes"
    print("\nseed %d, n0 %d: frames steps (step, the oracle's frame is not empty): %s" % (seed, n0, seen))
    assert seen and 3 * sum(ok for _, ok in seen) >= 2 * len(seen)


# ---- the comparison itself: an order that was not compacted is flagged -----------------------------------------------------------
class Resident:
    """what the sequence test asks a session for, answered from arrays: the stand-in for a context on a box without a GPU"""

    def __init__(self, fields, orig, bounds):
        self.fields, self.orig, self.bounds_ = fields, orig, bounds
        self.R = self
        self.n = len(orig)

    def scene_layout(self):
        return self.orig.copy(), self.bounds_.copy()

    def read_all(self, n):
        assert n == self.n
        out = {f: self.fields[f].copy() for f in FIELDS}
        out["positions"][:, 3] = f32(1.0)
        return out


def resident_of(model):
    return Resident({f: getattr(model.g, f) for f in FIELDS}, model.orig, model.bounds())


def test_the_per_step_comparison_flags_an_order_that_was_not_compacted():
    model = M.Model()
    model.apply(dict(kind="upload", variant="host", n=1000, seed=11, spoiled=False, dense=False))
    order_before = model.orig.copy()
    before = resident_of(model)
    M.assert_state(before, model, "as uploaded")
    gone = (np.random.default_rng(12).random(1000) < 0.4).astype(np.uint8)
    out = model.apply(dict(kind="remove", mask=gone, keep=False))
    truth = resident_of(model)                                   # a library that did everything right
    M.assert_state(truth, model, "after the removal")
    assert all(truth.fields[f].shape[0] == out["n_out"] and truth.fields[f].size == out["n_out"] * PER[f] for f in FIELDS)
    # the expected side with an order that drops the slots of what went but keeps the OLD numbering
    stay = out["index_map"] != RC.GONE
    stale = M.Model()
    stale.g, stale.n, stale.A, stale.B = model.g, model.n, model.A, model.B
    stale.orig = order_before[stay[order_before]]
    assert stale.orig.shape == model.orig.shape and not np.array_equal(stale.orig, model.orig)
    with pytest.raises(AssertionError, match="order"):
        M.assert_state(truth, stale, "stale numbering")
    # ... with the order of a fresh upload instead of the compacted one: the bounds are other blocks' bounds
    fresh = M.Model()
    fresh.g, fresh.n, fresh.A, fresh.B = model.g, model.n, model.A, model.B
    fresh.orig = RC.morton_order(model.g.positions)
    if not np.array_equal(fresh.orig, model.orig):
        with pytest.raises(AssertionError):
            M.assert_state(truth, fresh, "fresh order")
    # ... and with values that were not compacted at all: n and every field say so
    with pytest.raises(AssertionError, match="n is"):
        M.assert_state(before, model, "nothing removed")
