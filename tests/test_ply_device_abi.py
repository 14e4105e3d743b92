"""The device PLY loader as far as it shows without a GPU: the two entry points exist and refuse bad arguments before they
touch HIP, every mirror of the ABI names them under version 7, the gfx950 code object holds the new kernels without spills
or scratch and within 80 KiB of LDS, and ply_layout reads a header the way a numpy structured dtype does."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402
import ply_cases as P  # noqa: E402

import splat_amd  # noqa: E402
from splat_amd import _lib  # noqa: E402
from splat_amd.gaussians import PLY_PROPS  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_decode_ply_device", "splat_upload_ply_device")
KERNELS = ("splat::ply_decode_kernel<true>", "splat::ply_decode_kernel<false>", "splat::recentre_sum_kernel", "splat::recentre_sub_kernel")
LDS_MAX = 80 * 1024


def test_the_library_exports_the_two_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def good_layout(n=4):
    lay = _lib.PlyLayout()
    lay.n, lay.stride = n, 248
    for k in range(_lib.PLY_SLOTS):
        lay.offset[k] = 4 * k
    return lay


def call_both(ctx, lay, rows=16, out=16):
    L = _lib.lib()
    p = C.c_void_p
    lp = C.byref(lay) if lay is not None else None
    return (L.splat_decode_ply_device(ctx, lp, p(rows), p(out), p(out), p(out), p(out), p(out), None),
            L.splat_upload_ply_device(ctx, lp, p(rows), 1, None))


def test_a_null_context_is_refused_before_any_device_work():
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    assert call_both(None, good_layout()) == (_lib.ERR_INVALID, _lib.ERR_INVALID)


def spoil(**kw):
    lay = good_layout()
    for k, v in kw.items():
        if k == "offset":
            lay.offset[v[0]] = v[1]
        else:
            setattr(lay, k, v)
    return lay


BAD = [("stride 0", dict(stride=0), "stride"), ("offset -2", dict(offset=(5, -2)), "below -1"),
       ("offset + 4 > stride", dict(offset=(58, 245)), "beyond its row"), ("offset == stride", dict(offset=(0, 248)), "beyond its row"),
       ("2^32 - 1 vertices", dict(n=0xFFFFFFFF), "too many")]


@pytest.mark.parametrize("what,kw,reason", BAD, ids=[b[0] for b in BAD])
def test_each_invalid_layout_is_refused_before_any_device_work(what, kw, reason):
    # the layout is judged before the context is looked at, so that it can be judged here: the reason a call without a
    # context leaves behind (splat_last_error(NULL)) is the layout's fault, not the missing context
    L = _lib.lib()
    assert call_both(None, good_layout()) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL context" in L.splat_last_error(None)
    p, bad = C.c_void_p, spoil(**kw)
    assert L.splat_decode_ply_device(None, C.byref(bad), p(16), p(16), p(16), p(16), p(16), p(16), None) == _lib.ERR_INVALID
    assert reason.encode() in L.splat_last_error(None), L.splat_last_error(None)
    call_both(None, good_layout())                                               # (the reason is "NULL context" again)
    assert L.splat_upload_ply_device(None, C.byref(bad), p(16), 1, None) == _lib.ERR_INVALID
    assert reason.encode() in L.splat_last_error(None), L.splat_last_error(None)


def test_a_null_layout_is_refused():
    L = _lib.lib()
    assert call_both(None, None) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL layout" in L.splat_last_error(None)
    # offset == stride - 4 is the last one a row holds
    assert call_both(None, spoil(offset=(58, 244))) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL context" in L.splat_last_error(None)


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "#define SPLAT_ABI_VERSION 7\n" in hdr
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert "#define SPLAT_PLY_SLOTS 59\n" in hdr and _lib.PLY_SLOTS == 59 and len(_lib.PLY_SLOT_NAMES) == 59
    assert C.sizeof(_lib.PlyLayout) == 8 + 4 + 4 * 59 + 0 and C.sizeof(_lib.PlyLayout) % 8 == 0


def test_the_mirrors_name_both():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


@pytest.mark.parametrize("name", KERNELS)
def test_the_new_kernels_have_no_spills_no_scratch_and_lds_within_80_kib(kernels, name):
    assert name in kernels, (name, sorted(kernels))
    md = kernels[name][1]
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".group_segment_fixed_size"] <= LDS_MAX, md
    assert md[".max_flat_workgroup_size"] == 256, md


# ---- ply_layout ------------------------------------------------------------------------------------------------------
def check_layout(path, props, dt, n, binary=True):
    pl = splat_amd.ply_layout(path)
    assert pl.n == n == pl.layout.n and pl.binary == binary
    want = {k: v for k, v in P.expected_offsets(props, dt).items() if k in _lib.PLY_SLOT_NAMES}
    assert pl.offsets() == want
    for k, name in enumerate(_lib.PLY_SLOT_NAMES):
        assert pl.layout.offset[k] == want.get(name, -1), name
    if binary:
        assert pl.stride == dt.itemsize
        size = os.path.getsize(path)
        assert pl.payload_bytes == n * dt.itemsize and pl.payload_offset + pl.payload_bytes == size
        # the numpy reading of the same rows finds the same floats at those offsets
        rows = np.fromfile(path, dtype=dt, offset=pl.payload_offset)
        raw = np.fromfile(path, dtype=np.uint8, offset=pl.payload_offset).reshape(n, dt.itemsize)
        last = {name: k for k, (t, name) in enumerate(props) if t == "float"}
        for name, off in want.items():
            assert np.array_equal(raw[:, off:off + 4].copy().view("<f4")[:, 0].view(np.uint32), rows["f%d" % last[name]].view(np.uint32))
    return pl


INRIA = [("float", p) for p in PLY_PROPS]


def test_ply_layout_of_the_golden_head():
    path = os.path.join(ROOT, "tests", "golden", "c1_head.ply")
    pl = splat_amd.ply_layout(path)
    g = splat_amd.load_from_ply(path)
    assert pl.binary and pl.n == len(g) and pl.stride == 4 * len(PLY_PROPS) == 248
    dt = np.dtype([(p, "<f4") for p in PLY_PROPS])
    assert pl.offsets() == {name: dt.fields[name][1] for name in _lib.PLY_SLOT_NAMES}
    assert pl.payload_offset + pl.payload_bytes == os.path.getsize(path)


def test_ply_layout_shuffled_order(tmp_path):
    props = [INRIA[k] for k in np.random.default_rng(3).permutation(len(INRIA))]
    dt = P.write_ply_props(str(tmp_path / "s.ply"), props, 7, {})
    pl = check_layout(str(tmp_path / "s.ply"), props, dt, 7)
    assert pl.stride == 248 and sorted(pl.offsets().values()) != list(pl.offsets().values())


def test_ply_layout_with_uchar_properties_interleaved(tmp_path):
    props = [("uchar", "red")] + INRIA[:3] + [("uchar", "green"), ("uchar", "blue")] + INRIA[3:]
    dt = P.write_ply_props(str(tmp_path / "u.ply"), props, 5, {})
    pl = check_layout(str(tmp_path / "u.ply"), props, dt, 5)
    assert pl.stride == 251 and pl.layout.offset[0] == 1 and any(o % 4 for o in pl.offsets().values())


def test_ply_layout_a_double_named_x_is_absent(tmp_path):
    props = [("double", "x")] + INRIA[1:]
    dt = P.write_ply_props(str(tmp_path / "d.ply"), props, 5, {})
    pl = check_layout(str(tmp_path / "d.ply"), props, dt, 5)
    assert pl.layout.offset[0] == -1 and pl.layout.offset[1] == 8 and pl.stride == 252


def test_ply_layout_of_a_duplicated_name_the_last_wins(tmp_path):
    props = INRIA + [("float", "opacity"), ("float", "x")]
    dt = P.write_ply_props(str(tmp_path / "dup.ply"), props, 5, {})
    pl = check_layout(str(tmp_path / "dup.ply"), props, dt, 5)
    assert pl.layout.offset[_lib.PLY_SLOT_OPACITY] == 248 and pl.layout.offset[0] == 252 and pl.stride == 256


def test_ply_layout_of_an_ascii_file(tmp_path):
    dt = P.write_ply_props(str(tmp_path / "a.ply"), INRIA, 3, {}, fmt="ascii")
    pl = check_layout(str(tmp_path / "a.ply"), INRIA, dt, 3, binary=False)
    assert pl.payload_offset > 0


def test_ply_layout_errors(tmp_path):
    with pytest.raises(ValueError):
        splat_amd.ply_layout(str(tmp_path / "missing.ply"))
