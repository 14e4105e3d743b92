"""Retained lists: the decision (include/splat_retain.h, splat_retain.cpp) driven through scripted camera sequences on a box
without a GPU.  The scheduler (enqueue_frame) calls splat_retain_decide once per frame and then only launches what it says:
bin (0), bin as the writer (1), composite from the writer's lists (2)."""
import ctypes as C
import os
import re
import struct

import pytest

from splat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "splat_retain.h")).read()
CAM_WORDS = int(re.search(r"#define SPLAT_RETAIN_CAM_WORDS (\d+)", HDR).group(1))
BIN, WRITER, RETAIN = (int(re.search(r"#define SPLAT_RETAIN_%s (\d+)" % n, HDR).group(1)) for n in ("BIN", "WRITER", "RETAIN"))
STILL = int(re.search(r"#define SPLAT_POLICY_STILL_FRAMES (\d+)", open(os.path.join(ROOT, "include", "splat_policy.h")).read()).group(1))


class State(C.Structure):
    _fields_ = [("have_cam", C.c_uint32), ("same_run", C.c_uint32), ("writer", C.c_uint32), ("pad_", C.c_uint32),
                ("epoch", C.c_uint64), ("last_cam", C.c_uint32 * CAM_WORDS)]


class Input(C.Structure):
    _fields_ = [("cam", C.c_uint32 * CAM_WORDS), ("epoch", C.c_uint64), ("still_frames", C.c_uint32), ("enabled", C.c_int32),
                ("overlap", C.c_int32), ("one_pass", C.c_int32), ("writer_arrived", C.c_uint32), ("writer_overflow", C.c_uint32),
                ("writer_redone", C.c_uint32), ("pad_", C.c_uint32)]


class Decision(C.Structure):
    _fields_ = [("action", C.c_int32), ("ended", C.c_int32), ("wait_for_writer", C.c_int32), ("pad_", C.c_int32), ("next", State)]


def _fn():
    L = _lib.lib()
    L.splat_retain_decide.restype = C.c_int
    L.splat_retain_decide.argtypes = [C.POINTER(State), C.POINTER(Input), C.POINTER(Decision)]
    L.splat_retain_struct_sizes.restype = None
    L.splat_retain_struct_sizes.argtypes = [C.POINTER(C.c_uint64)]
    return L


def camera(yaw_bits=0):
    """48 words: a view matrix whose entry 2 is 0.25 with `yaw_bits` added to its mantissa, and other plausible words"""
    w = [0] * CAM_WORDS
    for k in range(32):
        w[k] = struct.unpack("<I", struct.pack("<f", 1.0 if k % 5 == 0 else 0.0))[0]
    w[2] = struct.unpack("<I", struct.pack("<f", 0.25))[0] + yaw_bits
    w[32], w[33] = struct.unpack("<II", struct.pack("<ff", 328.0, 200.0))
    w[44], w[45] = 0, 0xffffffff        # the slab: rows 0 .. -1 (all)
    return w


class Driver:
    """the scheduler's side: carries the state, counts still frames as the frame policy does (same camera as the last frame),
    reports every writer's status as `writer_status` says"""

    def __init__(self, enabled=1, overlap=1, one_pass=1, writer_status=(1, 0, 0)):
        self.L = _fn()
        self.st = State()
        self.enabled, self.overlap, self.one_pass, self.writer_status = enabled, overlap, one_pass, writer_status
        self.epoch = 0
        self.prev, self.still = None, 0

    def bump(self):
        self.epoch += 1
        self.still, self.prev = 0, None      # (reset_policy: the frame policy forgets its camera too)

    def frame(self, cam):
        self.still = min(self.still + 1, 1000) if cam == self.prev else 0
        self.prev = list(cam)
        i = Input()
        i.cam[:] = cam
        i.epoch, i.still_frames, i.enabled, i.overlap, i.one_pass = self.epoch, self.still, self.enabled, self.overlap, self.one_pass
        i.writer_arrived, i.writer_overflow, i.writer_redone = self.writer_status
        d = Decision()
        assert self.L.splat_retain_decide(C.byref(self.st), C.byref(i), C.byref(d)) == 0
        again = Decision()          # pure: the same arguments give the same decision
        assert self.L.splat_retain_decide(C.byref(self.st), C.byref(i), C.byref(again)) == 0
        assert bytes(d) == bytes(again)
        self.st = d.next
        self.last = d
        return d.action


def test_struct_sizes_are_the_librarys():
    sizes = (C.c_uint64 * 3)()
    _fn().splat_retain_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(State), C.sizeof(Input), C.sizeof(Decision)]
    assert _fn().splat_retain_decide(None, None, None) == -1


def test_identical_cameras_writer_then_retained():
    d = Driver()
    acts = [d.frame(camera()) for _ in range(12)]
    # frame 0 has no predecessor; frames 1..STILL are at rest for 1..STILL frames; frame STILL writes; the rest are retained
    assert acts == [BIN] * STILL + [WRITER] + [RETAIN] * (12 - STILL - 1)


def test_one_mantissa_bit_of_one_view_entry_bins():
    d = Driver()
    for _ in range(STILL + 3):
        last = d.frame(camera())
    assert last == RETAIN
    assert d.frame(camera(yaw_bits=1)) == BIN          # the moved frame
    assert d.frame(camera()) == BIN                    # ... and the frame after it, back on the first pose
    acts = [d.frame(camera()) for _ in range(STILL + 1)]
    assert acts == [BIN] * (STILL - 1) + [WRITER, RETAIN]


def test_the_slab_words_are_part_of_the_camera():
    d = Driver()
    for _ in range(STILL + 2):
        d.frame(camera())
    other = camera()
    other[45] = 7
    assert d.frame(other) == BIN


def test_epoch_bump_at_rest_bins_and_needs_the_still_count_again():
    d = Driver()
    for _ in range(STILL + 3):
        last = d.frame(camera())
    assert last == RETAIN
    d.bump()
    acts = [d.frame(camera()) for _ in range(STILL + 2)]
    assert acts == [BIN] * STILL + [WRITER, RETAIN]
    # ... also when only the epoch changes and the policy's still count runs on (a key buffer made again)
    d.epoch += 1
    acts = [d.frame(camera()) for _ in range(STILL + 2)]
    assert acts == [BIN] * STILL + [WRITER, RETAIN]


def test_the_policys_still_count_gates_too():
    d = Driver()
    d.frame(camera())
    for _ in range(6):
        d.still = -1                # (the policy keeps saying "first frame of this camera": its hash state was reset)
        assert d.frame(camera()) == BIN


@pytest.mark.parametrize("kw", [dict(overlap=2), dict(enabled=0), dict(one_pass=0)])
def test_never(kw):
    d = Driver(**kw)
    assert [d.frame(camera()) for _ in range(3 * STILL + 4)] == [BIN] * (3 * STILL + 4)


def test_switching_off_at_rest_ends_the_set():
    d = Driver()
    for _ in range(STILL + 3):
        d.frame(camera())
    d.enabled = 0
    assert d.frame(camera()) == BIN
    d.enabled = 1
    assert d.frame(camera()) == WRITER          # (the camera never moved: the next frame may write again)
    assert d.frame(camera()) == RETAIN


@pytest.mark.parametrize("status", [(0, 0, 0), (1, 2, 0), (1, 3, 0), (1, 0, 1)])
def test_a_writer_that_did_not_arrive_overflowed_or_was_redone_establishes_no_set(status):
    d = Driver(writer_status=status)
    acts = [d.frame(camera()) for _ in range(STILL + 6)]
    assert RETAIN not in acts
    assert acts[:STILL + 1] == [BIN] * STILL + [WRITER]
    # a clean writer later on does
    d.writer_status = (1, 0, 0)
    acts = [d.frame(camera()) for _ in range(3)]
    assert acts[-1] == RETAIN and acts.count(RETAIN) >= 2


def test_a_writer_whose_status_has_not_arrived_asks_the_scheduler_to_wait():
    """... and only then: the scheduler waits for the writer's frame when wait_for_writer is set, and asks again"""
    d = Driver(writer_status=(0, 0, 0))
    waits = []
    for _ in range(STILL + 2):
        d.frame(camera())
        waits.append(d.last.wait_for_writer)
    assert waits == [0] * (STILL + 1) + [1]          # the frame behind the writer
    assert d.last.action != RETAIN
    d = Driver(writer_status=(1, 2, 0))              # arrived and overflowed: nothing to wait for
    for _ in range(STILL + 3):
        d.frame(camera())
        assert d.last.wait_for_writer == 0
    d = Driver(writer_status=(0, 0, 0))              # another camera behind the writer: nothing to wait for either
    for _ in range(STILL + 1):
        d.frame(camera())
    d.frame(camera(yaw_bits=1))
    assert d.last.wait_for_writer == 0
