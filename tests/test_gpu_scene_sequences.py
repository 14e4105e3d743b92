"""Random sequences of scene operations on one context, held step by step to the numpy model (tests/scene_model.py; -m gpu).

Every (seed, n0) program of tests/test_scene_model_host.py -- which shows on the CPU what these programs contain -- is replayed
on a scene_gpu.session().  Nothing here has a tolerance.  After EVERY step the four resident fields, n, the scene's order and
the block bounds are the model's bit for bit, what the call returned is what the model says, the bytes around every output
buffer are untouched, a call that only reads has left device_bytes() where it was (but for the inverse order, once per scene)
and no frame was dropped; behind an edit in place what the near selection learnt from the old values is gone (need_hint of
splat_debug_near_state: the one place where a missing scene_edited shows -- stale hints cost time, not pixels; the programs
of 4097 Gaussians end with a dense scene, a camera at rest and an indexed sh rotation for it).  At every frames step and at the end, frames, records, tile lists and counts are those of a FRESH
Renderer that took the model's arrays through splat_upload_scene.  One program per size also runs with mode = MODE_LIBM_EXP,
where its last frame is the oracle's frame of the model's arrays.

What this does not cover stays with the per-operation modules: indices out of range, side streams and torch tensors, frames
in flight under set_frame_overlap.

A failure names the seed, the step, its kind and arguments and the two edit kinds before it; `-k seed5-n1000` replays one
program, which stops at its first failing step."""
import ctypes as C

import numpy as np
import pytest

import splat_amd
from splat_amd import _lib
from splat_amd.gaussians import inria_layout
import pick_cases as K
import scene_model as M
import sh_rotate_cases as SR
import transform_cases as T
from scene_gpu import (PER, SENTINEL, TARGETS, assert_same_bits, assert_same_frames, assert_same_stage, frame, frames, fresh_upload,
                       session)
from test_gpu_ply_encode import assert_same_rows, encode
from test_gpu_remove import put_mask
from test_scene_model_host import IDS, LENGTH, PROGRAMS

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_LIBM_EXP = 2
GUARD = 16                                           # sentinel bytes in front of and behind every output buffer
WORD = 0xA5A5A5A5
LIBM = tuple(next(p for p in PROGRAMS if p[1] == n0) for n0 in (257, 1000, 4097))
CASES = [(seed, n0, 0) for seed, n0 in PROGRAMS] + [(seed, n0, MODE_LIBM_EXP) for seed, n0 in LIBM]
CASE_IDS = list(IDS) + ["seed%d-n%d-libm_exp" % p for p in LIBM]


def brief(step):
    """the step's arguments, arrays by shape"""
    return {k: ("%s%r" % (v.dtype, v.shape) if isinstance(v, np.ndarray) else v) for k, v in step.items()}


class Replay:
    """one program on one context, the model beside it"""

    def __init__(self, s, mode):
        self.s, self.R, self.mode = s, s.R, mode
        self.model = M.Model()
        self.masks = {}                              # "A", "B": device address of the caller's n bytes, GUARD sentinel bytes around
        self.images = {}
        self.inverse_of = None                       # the scene (model.scene_id) whose inverse order has been made
        self.rest = None                             # (ti, ci) while a camera is at rest and retention runs
        self.emptied = False

    # ---- plumbing -----------------------------------------------------------------------------------------------------------
    def guarded(self, nbytes):
        return self.s.alloc(nbytes + 2 * GUARD, SENTINEL) + GUARD

    def fetch_guarded(self, p, count, dtype, what):
        """`count` elements at p, the guards around them checked"""
        nbytes = count * np.dtype(dtype).itemsize
        raw = self.s.fetch(p - GUARD, (nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + nbytes:] == SENTINEL).all(), "%s: bytes around the buffer were written" % what
        return raw[GUARD:GUARD + nbytes].view(dtype).copy()

    def new_masks(self):
        """the caller's masks, as the model holds them now, in buffers of the new n (A at an odd address, B at an even one)"""
        for name, skew in (("A", 1), ("B", 2)):
            a = self.model.mask(name)
            p = self.s.alloc(len(a) + 2 * GUARD + skew, SENTINEL) + GUARD + skew
            if len(a):
                self.R._check(self.R._L.splat_device_upload(self.R._h, p, a.ctypes.data, a.nbytes))
            self.masks[name] = p

    def assert_mask(self, name, what):
        got = self.fetch_guarded(self.masks[name], self.model.n, np.uint8, what)
        want = self.model.mask(name)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d of %d selection bytes differ, first %d: %d, want %d" % (what, bad.size, len(want), bad[0], got[bad[0]], want[bad[0]])

    def index(self, step):
        return None if step["index"] is None else self.s.array(step["index"])

    def measured(self, call, n, may_make_inverse):
        """call(), which may not change what the context holds -- but for the inverse order, made once per scene by its first
        call with indices (4 n bytes and a byte per block)"""
        before = self.R.device_bytes()[0]
        got = call()
        grew = self.R.device_bytes()[0] - before
        if grew:
            nb = (n + 255) // 256
            assert may_make_inverse and self.inverse_of != self.model.scene_id, "device_bytes() moved by %d over the call" % grew
            assert 4 * n + nb <= grew <= 4 * n + nb + 64, "device_bytes() grew by %d, the inverse of %d Gaussians is %d" % (grew, n, 4 * n + nb)
            self.inverse_of = self.model.scene_id
        return got

    def rest_frame(self, ti, ci):
        h, w = TARGETS[ti]
        if ti not in self.images:
            self.images[ti] = self.R.host_image(h, w)
        img = self.images[ti]
        img[:] = 0xDEADBEEF
        self.R.render_frame(M.camera(ti, ci).to_c(0.01, 15), img)
        return img.copy()

    def hints(self):
        """what the near selection has learnt from the frames so far (splat_debug_near_state's need_hint: written for tile lists
        of more than 2048 keys), or None before the first frame"""
        for h, w in TARGETS:
            m = ((h + _lib.TILE - 1) // _lib.TILE) * ((w + _lib.TILE - 1) // _lib.TILE)
            lens, near, need = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(4 * m, np.uint32)
            if self.R._L.splat_debug_near_state(self.R._h, *[C.c_void_p(a.ctypes.data) for a in (lens, near, need)], C.c_uint(m)) == _lib.SPLAT_OK:
                return need
        return None

    def fresh(self):
        return fresh_upload(self.model.g, mode=self.mode)

    # ---- the steps --------------------------------------------------------------------------------------------------------------
    def run(self, i, step, what):
        s, R, model = self.s, self.R, self.model
        n = model.n
        out = model.apply(step)
        assert model.n == step["n_after"] and n == step["n_before"]
        in_place = step["ends_frames"] and step["kind"] in ("update", "update_indexed", "transform", "rotate_sh")
        learnt = self.hints() if in_place else None
        getattr(self, "run_" + step["kind"])(step, out, n, what)
        if learnt is not None:
            # an edit in place forgets what the scheduler learnt from the old values: seen here where a debug entry point shows it
            print("%s: the near selection held hints for %d waves" % (what, int((learnt != 0).sum())))
            assert not self.hints().any(), "%s: the near selection's hints outlive the edit" % what
        M.assert_state(s, model, what)
        assert R.frames_dropped() == 0, what
        if step["ends_frames"] and self.rest is not None:
            ti, ci = self.rest
            self.rest = None
            if model.n:
                # the first frame behind an edit is binned, not retained, and is the fresh upload's
                retained = R.frames_retained()
                got = self.rest_frame(ti, ci)
                assert R.frames_retained() == retained, "%s: the frame after an edit is binned, not retained" % what
                with self.fresh() as ref:
                    assert np.array_equal(got, frame(ref, M.camera(ti, ci), *TARGETS[ti])), "%s: the first frame after the edit" % what

    def run_upload(self, step, out, n, what):
        s, R, g = self.s, self.R, self.model.g
        if step["variant"] == "host":
            R.upload(g)
        elif step["variant"] == "device":
            d = s.device(M.Model.source(step["n"], step["seed"], step["spoiled"], step["dense"]))
            R.upload_device(d.positions, d.cov3d, d.opacities, d.sh, n=step["n"])
        else:
            R.upload_ply_rows(s.array(out["rows"]), inria_layout(step["n"]))
        assert R.n == step["n"], what
        self.new_masks()
        if self.emptied:                             # behind a removal of everything an upload behaves as on a new context
            self.emptied = False
            with self.fresh() as ref:
                assert_same_frames(frames(R), frames(ref), what + ": an upload after the scene went")
                assert_same_stage(R, ref, what + ": an upload after the scene went")

    def run_update(self, step, out, n, what):
        d = self.s.device(M.Model.source(n, step["seed"]))
        self.measured(lambda: self.R.update_device(n=n, **{f: getattr(d, f) for f in step["fields"]}), n, False)

    def run_update_indexed(self, step, out, n, what):
        rows = {f: self.s.array(out["rows"][f]) for f in step["fields"]}
        idx = self.index(step)
        self.measured(lambda: self.R.update_indexed(idx, k=len(step["index"]), **rows), n, len(step["index"]) > 0)

    def run_transform(self, step, out, n, what):
        idx = self.index(step)
        k = None if idx is None else len(step["index"])
        self.measured(lambda: self.R.transform(T.MATRICES[step["matrix"]], idx, k=k, rotate_sh=step["rotate_sh"]), n, bool(k))

    def run_rotate_sh(self, step, out, n, what):
        idx = self.index(step)
        k = None if idx is None else len(step["index"])
        self.measured(lambda: self.R.rotate_sh(SR.ROTATIONS[step["rotation"]], idx, k=k), n, bool(k))

    def run_remove(self, step, out, n, what):
        s, R = self.s, self.R
        mask = self.masks[step["mask"]] if isinstance(step["mask"], str) else put_mask(s, step["mask"], step["offset"])
        pm = self.guarded(4 * n) if step["with_map"] else None
        held = R.device_bytes()[0]
        got = R.remove(mask, keep=step["keep"], index_map=pm, n=n)
        assert got == out["n_out"] == R.n, "%s: %d Gaussians left, the model has %d" % (what, got, out["n_out"])
        if pm is not None:                           # the map read back is the model's: then both sides carry their masks across with it
            assert np.array_equal(self.fetch_guarded(pm, n, np.uint32, what), out["index_map"]), what + ": the index map"
        if got == n:
            assert R.device_bytes()[0] == held, what + ": a removal of nothing is a read"
            for name in "AB":
                self.assert_mask(name, what)
        elif got == 0:
            self.no_scene(what)
        else:
            self.new_masks()

    def no_scene(self, what):
        """every scene operation answers SPLAT_ERR_NO_SCENE, or is the documented no-op"""
        s, R = self.s, self.R
        self.emptied, self.masks = True, {}
        assert R.n == 0 and R.scene_layout()[0].size == 0, what
        buf, cam_c = s.alloc(256, 0), M.camera(0, 0).to_c(0.01, 15)
        idx = s.array(np.zeros(1, np.uint32))
        calls = {"read_device": lambda: R.read_device(n=0), "update_device": lambda: R.update_device(n=0),
                 "read_indexed": lambda: R.read_indexed(idx, opacities=buf, k=1), "update_indexed": lambda: R.update_indexed(idx, opacities=buf, k=1),
                 "transform": lambda: R.transform(T.MATRICES["rotation"]), "transform by index": lambda: R.transform(T.MATRICES["rotation"], idx, k=1),
                 "rotate_sh": lambda: R.rotate_sh(SR.ROTATIONS["rot20"]), "rotate_sh by index": lambda: R.rotate_sh(SR.ROTATIONS["rot20"], idx, k=1),
                 "select": lambda: R.select(buf, opacity=(0.0, 1.0)), "select_neighbours": lambda: R.select_neighbours(buf, 0.5),
                 "pick": lambda: R.pick(cam_c, [(0, 0)], results=buf), "remove": lambda: R.remove(put_mask(s, np.ones(4, bool)), n=4),
                 "encode by index": lambda: R.encode_ply_rows(buf, inria_layout(1), idx, k=1)}
        for name, call in calls.items():
            with pytest.raises(splat_amd.SplatError) as e:
                call()
            assert e.value.code == _lib.ERR_NO_SCENE, "%s: %s without a scene answers %d" % (what, name, e.value.code)
        R.encode_ply_rows(0, inria_layout(0))        # the documented no-op: nothing to write, no error
        assert (s.fetch(buf, (256,), np.uint8) == 0).all() and R.n == 0, what

    def run_select(self, step, out, n, what):
        cam_c = M.camera(step["ti"], step["ci"]).to_c(0.01, 15)
        count = self.measured(lambda: self.R.select(self.masks[step["into"]], cam_c, op=step["op"], **step["query"]), n, False)
        assert count == out["count"], "%s: %d selected, the model has %d" % (what, count, out["count"])
        for name in "AB":
            self.assert_mask(name, what)

    def run_selection_indices(self, step, out, n, what):
        po = self.guarded(4 * n)
        count = self.measured(lambda: self.R.selection_indices(self.masks[step["of"]], po, n=n, capacity=n), n, False)
        want = out["indices"]
        got = self.fetch_guarded(po, n, np.uint32, what)
        assert count == len(want) and np.array_equal(got[:count], want) and (got[count:] == WORD).all(), what
        assert (np.diff(got[:count].astype(np.int64)) > 0).all(), what + ": ascending"

    def run_select_neighbours(self, step, out, n, what):
        sel = self.masks[step["into"]]
        pc = self.guarded(4 * n)
        count = self.measured(lambda: self.R.select_neighbours(sel, step["radius"], source=sel if step["source_is_selection"] else None,
                                                               at_least=step["at_least"], at_most=None if step["at_most"] == M.UNBOUNDED else step["at_most"],
                                                               op=step["op"], counts=pc), n, False)
        assert self.R.block_pairs == out["block_pairs"], what
        got = self.fetch_guarded(pc, n, np.uint32, what)
        bad = np.flatnonzero(got != out["counts"])
        assert bad.size == 0, "%s: %d of %d counts differ, first %d: %d, want %d" % (what, bad.size, n, bad[0], got[bad[0]], out["counts"][bad[0]])
        assert count == out["count"], what
        for name in "AB":
            self.assert_mask(name, what)

    def run_neighbours_refused(self, step, out, n, what):
        pc = self.guarded(4 * n)

        def call():
            with pytest.raises(splat_amd.SplatError) as e:
                self.R.select_neighbours(self.masks[step["into"]], step["radius"], counts=pc, max_block_pairs=step["max_block_pairs"])
            return e.value.code

        assert self.measured(call, n, False) == _lib.ERR_CAPACITY, what
        assert self.R.block_pairs == out["block_pairs"] == step["max_block_pairs"] + 1, what
        assert (self.fetch_guarded(pc, n, np.uint32, what) == WORD).all(), what + ": nothing written"
        for name in "AB":
            self.assert_mask(name, what)

    def run_pick(self, step, out, n, what):
        P, L = len(step["pixels"]), step["layers"]
        pr, pl = self.guarded(32 * P), (self.guarded(16 * P * L) if L else None)
        cam_c = M.camera(step["ti"], step["ci"]).to_c(0.01, 15)
        assert self.measured(lambda: self.R.pick(cam_c, step["pixels"], layers=L, results=pr, layers_out=pl), n, False) is None
        got = self.fetch_guarded(pr, P, K.RESULT, what)
        for p in range(P):
            assert got[p].tobytes() == out["results"][p].tobytes(), "%s: pixel %d: got %r, want %r" % (what, p, got[p], out["results"][p])
        if L:                                        # rows that are not due keep the fill (K.SENTINEL is the guards' byte)
            lay = self.fetch_guarded(pl, P * L, K.LAYER, what).reshape(P, L)
            assert lay.tobytes() == out["layers"].tobytes(), what + ": the layers"

    def run_read(self, step, out, n, what):
        bufs = {f: self.guarded(4 * PER[f] * n) for f in step["fields"]}
        self.measured(lambda: self.R.read_device(n=n, **bufs), n, False)
        for f in step["fields"]:
            want = getattr(self.model.g, f).copy()
            if f == "positions":
                want[:, 3] = f32(1.0)
            assert_same_bits(self.fetch_guarded(bufs[f], PER[f] * n, f32, what), want.ravel(), what + " " + f)

    def run_read_indexed(self, step, out, n, what):
        k = len(step["index"])
        bufs = {f: self.guarded(4 * PER[f] * k) for f in step["fields"]}
        idx = self.index(step)
        self.measured(lambda: self.R.read_indexed(idx, k=k, **bufs), n, True)
        for f in step["fields"]:
            assert_same_bits(self.fetch_guarded(bufs[f], PER[f] * k, f32, what), out["rows"][f].ravel(), what + " " + f)

    def run_encode(self, step, out, n, what):
        # no numpy restatement of the encoder: the rows are those of a twin that took the model's arrays through a fresh upload
        k = n if step["index"] is None else len(step["index"])
        lay = inria_layout(k)
        idx = self.index(step)
        p = self.guarded(k * int(lay.stride))
        self.measured(lambda: self.R.encode_ply_rows(p, lay, index=idx, k=None if idx is None else k), n, True)
        got = self.fetch_guarded(p, k * int(lay.stride), np.uint8, what).reshape(k, int(lay.stride))
        with session(mode=self.mode) as twin:
            twin.R.upload(self.model.g)
            want = encode(twin, lay, index=None if idx is None else twin.array(step["index"]), k=None if idx is None else k)
        assert_same_rows(got, want, what)

    def run_frames(self, step, out, n, what):
        R = self.R
        with self.fresh() as ref:
            assert_same_stage(R, ref, what)
            if step["variant"] == "tour":
                assert_same_frames(frames(R), frames(ref), what)
                self.rest = None
                return
            ti, ci = step["ti"], step["ci"]
            want = frame(ref, M.camera(ti, ci), *TARGETS[ti])
        retained = R.frames_retained()
        for k in range(M.REST_FRAMES):
            assert np.array_equal(self.rest_frame(ti, ci), want), "%s: frame %d at rest is not the fresh upload's" % (what, k)
        assert R.frames_retained() > retained, "%s: %d frames at rest and none composited from retained lists" % (what, M.REST_FRAMES)
        self.rest = (ti, ci)

    def finish(self, what):
        R, model = self.R, self.model
        with self.fresh() as ref:
            assert_same_frames(frames(R), frames(ref), what)
            assert_same_stage(R, ref, what)
        if self.mode == MODE_LIBM_EXP:               # the model tied to the reference without any device code in between
            h, w = TARGETS[1]
            assert np.array_equal(frame(R, M.camera(1, 0), h, w), model.oracle_frame(1, 0)), what + ": the oracle's frame of the model's arrays"


@pytest.mark.parametrize("seed,n0,mode", CASES, ids=CASE_IDS)
def test_a_random_program_stays_the_models(seed, n0, mode):
    steps = M.program(seed, n0, LENGTH)
    with session(mode=mode) as s:
        replay = Replay(s, mode)
        edits = []
        for i, step in enumerate(steps):
            what = "seed %d, n0 %d, step %d (%s)" % (seed, n0, i, step["kind"])
            try:
                replay.run(i, step, what)
            except Exception as e:
                raise AssertionError("%s failed: %s\n  arguments: %r\n  the two edits before it: %r\n  the steps so far: %s" % (
                    what, e, brief(step), edits[-2:], " ".join(t["kind"] for t in steps[:i + 1]))) from e
            if step["edit"] is not None:
                edits.append(step["edit"])
        replay.finish("seed %d, n0 %d, after the last step" % (seed, n0))
        assert s.R.frames_dropped() == 0
