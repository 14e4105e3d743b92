"""Start refinement at rest, the policy's side, driven without a GPU.

A camera at rest lets the compositor's waves test a shallower start than the one that closed their bracket last frame
(composite_tile, phase A): splat_policy_decide says per frame whether they do, in splat_policy_decision::refine (bits 16..31
a tag of the camera at rest, bit 31 always set; bits 0..15 the frame number, which alternates the probing half of the tiles).
A camera that moves gets another tag, which makes every wave's probe state fresh again without clearing anything.
SPLAT_OPT_START_REFINE 0 reaches the policy as the SPLAT_POLICY_NO_REFINE flag of knobs.start_hints."""
import ctypes as C
import math
import os
import re

import pytest

from splat_amd import _lib
from test_frame_policy import Knobs, State, Input, RING, PROJ, yaw_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STILL = 3                       # SPLAT_POLICY_STILL_FRAMES


class Decision(C.Structure):
    _fields_ = [("cam_hash", C.c_uint64), ("cam_delta", C.c_float), ("cam_jumped", C.c_int32), ("start_hints_mode", C.c_int32),
                ("start_light", C.c_int32), ("early_min", C.c_int32), ("hint_radius", C.c_int32), ("count_first", C.c_int32),
                ("moved", C.c_int32), ("redo", C.c_int32), ("ring_kind", C.c_int32), ("solo", C.c_int32), ("comp_sorts", C.c_int32),
                ("near_cap", C.c_uint32), ("select_grid", C.c_uint32), ("grid_big", C.c_uint32), ("grid_mid", C.c_uint32),
                ("grid_long", C.c_uint32), ("pair_walk", C.c_int32), ("use_large_list", C.c_int32), ("layout_radius", C.c_int32),
                ("refine", C.c_uint32), ("next", State)]


@pytest.fixture(scope="module")
def L():
    lib = C.CDLL(_lib.LIB_PATH)          # loads without a GPU
    lib.splat_policy_decide.restype = C.c_int
    lib.splat_policy_decide.argtypes = [C.POINTER(Knobs), C.POINTER(State), C.POINTER(Input), C.POINTER(Decision)]
    lib.splat_policy_default_knobs.restype = None
    lib.splat_policy_default_knobs.argtypes = [C.POINTER(Knobs)]
    lib.splat_policy_struct_sizes.restype = None
    lib.splat_policy_struct_sizes.argtypes = [C.POINTER(C.c_uint64)]
    return lib


def no_refine_flag():
    hdr = open(os.path.join(ROOT, "include", "splat_policy.h")).read()
    return int(re.search(r"#define SPLAT_POLICY_NO_REFINE (\d+)", hdr).group(1))


class Path:
    """a camera path through the policy: one frame per step(), the state carried as enqueue_frame carries it"""

    def __init__(self, L, start_hints=None, refine=True):
        self.L, self.k, self.st, self.frame = L, Knobs(), State(), 0
        L.splat_policy_default_knobs(self.k)
        if start_hints is not None:
            self.k.start_hints = start_hints
        if not refine:
            self.k.start_hints |= no_refine_flag()

    def step(self, angle):
        self.frame += 1
        i = Input()
        i.view[:] = list(yaw_view(angle))
        i.proj[:] = list(PROJ)
        i.w, i.h, i.htanx, i.htany, i.focal = 1920.0, 1080.0, 1.7778, 1.0, 540.0
        i.cam[:] = [0.0, 0.0, 5.0]
        i.lowpass = 0.01
        i.tile_row0, i.n_tile_rows = 0, 68
        i.frame_idx, i.ring_entry, i.one_pass = self.frame, (self.frame - 1) % RING, 1
        i.layout_valid, i.n_tiles, i.has_keys2 = 1, 8160, 1
        d, d2 = Decision(), Decision()
        assert self.L.splat_policy_decide(self.k, self.st, i, d) == 0
        assert self.L.splat_policy_decide(self.k, self.st, i, d2) == 0 and bytes(d) == bytes(d2)      # pure
        self.st = State.from_buffer_copy(d.next)
        return d


def test_the_decision_mirror_is_the_librarys(L):
    sizes = (C.c_uint64 * 4)()
    L.splat_policy_struct_sizes(sizes)
    assert sizes[3] == C.sizeof(Decision)
    assert no_refine_flag() & 3 == 0           # (a flag beside the option's values 0..2)


def test_the_policy_refines_only_at_rest(L):
    p = Path(L)
    for k in range(12):
        d = p.step(0.3)
        assert (d.refine != 0) == (d.start_hints_mode == 1) == (k >= STILL), (k, d.refine, d.start_hints_mode)
        if d.refine:
            assert d.refine >> 31 == 1 and d.refine & 0xffff == p.frame & 0xffff
    # slow motion (mode 2), a fast pan (scan), a jump: no probing; at rest again: probing again
    for a in (0.3 + math.radians(0.2), 0.3 + math.radians(0.6), 0.3 + math.radians(3.0), 1.5):
        d = p.step(a)
        assert d.start_hints_mode != 1 and d.refine == 0, (a, d.start_hints_mode, d.refine)
    modes = [p.step(1.5) for _ in range(6)]
    assert [d.refine != 0 for d in modes] == [False, False, True, True, True, True]


def test_the_tag_is_the_cameras_so_a_camera_change_resets_probe_state(L):
    p = Path(L)
    tags = []
    for a in (0.3, 0.7, 0.3):                  # rest, move and rest elsewhere, back to the first pose
        ds = [p.step(a) for _ in range(8)][STILL:]
        t = {d.refine >> 16 for d in ds}
        assert len(t) == 1, t                  # one tag through a rest ...
        tags.append(t.pop())
        assert len({d.refine & 3 for d in ds}) == 4                    # ... and the frame number rides along (the probing half of the tiles alternates)
    assert tags[0] != tags[1]                  # another camera: the waves' probe words no longer match -> fresh steps
    assert tags[0] == tags[2]                  # (the same pose again: the probe state of that pose still describes its lists)


def test_the_option_turns_refinement_off(L):
    on, off = Path(L), Path(L, refine=False)
    for k in range(10):
        a, b = on.step(0.3), off.step(0.3)
        # everything but the refinement is the same decision
        assert a.start_hints_mode == b.start_hints_mode and a.early_min == b.early_min and a.hint_radius == b.hint_radius
        assert b.refine == 0
        assert (a.refine != 0) == (k >= STILL)
    # the flag does not change what the hints option means: 1 = at rest only, 0 = scan every frame
    one, zero = Path(L, start_hints=1), Path(L, start_hints=0)
    one_off = Path(L, start_hints=1, refine=False)
    for k in range(6):
        d1, d0, d1o = one.step(0.3), zero.step(0.3), one_off.step(0.3)
        assert d1.start_hints_mode == d1o.start_hints_mode == (1 if k >= STILL else 0)
        assert d0.start_hints_mode == 0 and d0.refine == 0 and d1o.refine == 0
        assert (d1.refine != 0) == (k >= STILL)
    for k in range(6):
        a = math.radians(0.2) * k
        assert one.step(a).start_hints_mode == 0 and one_off.step(a).start_hints_mode == 0    # (no slow-motion mode at 1)


def test_the_option_follows_the_header():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert int(re.search(r"#define SPLAT_OPT_START_REFINE (\d+)", hdr).group(1)) == _lib.OPT_START_REFINE
