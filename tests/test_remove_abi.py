"""splat_remove_gaussians_device as far as it shows without a GPU: the library exports it, what it can judge of its arguments
is refused before the context is looked at (so before any device work), every mirror of the ABI names it and its two modes
under version 7, the gfx950 code object holds the three new kernels with 256 threads and neither spills nor scratch, and
Renderer.remove refuses what it can judge by itself."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

import splat_amd  # noqa: E402
from splat_amd import _lib  # noqa: E402
from test_select_abi import FakeTensor  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = "splat_remove_gaussians_device"
KERNELS = ("splat::index_map_kernel", "splat::slot_keep_count_kernel", "splat::compact_scene_kernel")
REUSED = ("splat::mask_count_kernel", "splat::mask_scan_kernel", "splat::plane_bounds_kernel")
CONSTANTS = (("SELECTED", 0), ("UNSELECTED", 1))


def test_the_library_exports_the_entry_point():
    assert hasattr(C.CDLL(LIB), NEW)
    assert [s[0] for s in _lib.SYMBOLS].count(NEW) == 1


def remove(ctx, n=100, sel=16, mode=0, index_map=None, n_out=True):
    out = C.c_uint64(0xABCD)
    rc = _lib.lib().splat_remove_gaussians_device(ctx, n, C.c_void_p(sel) if sel else None, mode, C.c_void_p(index_map) if index_map else None,
                                                  C.byref(out) if n_out else None, None)
    assert out.value == 0xABCD, "a refused call writes nothing"
    return rc


def refused(why, **kw):
    """(this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)"""
    assert remove(None, **kw) == _lib.ERR_INVALID
    got = _lib.lib().splat_last_error(None)
    assert why.encode() in got, got


def test_every_refusal_names_its_argument_before_the_context_is_looked_at():
    refused("n_out", n_out=False)
    refused("mode", mode=2)
    refused("mode", mode=0xFFFFFFFF)
    for off in (1, 2, 3):
        refused("d_index_map_out", index_map=4096 + off)
    refused("d_selection", sel=0)
    refused("d_selection", sel=0, n=1)
    # ... in that order, and what is fine as far as the arguments go ends at the missing context
    refused("n_out", n_out=False, mode=7, sel=0)
    refused("mode", mode=7, sel=0, index_map=4097)
    refused("NULL context")
    refused("NULL context", mode=1, index_map=4096)
    refused("NULL context", sel=17)                                  # a selection lies at any byte address
    refused("NULL context", sel=0, n=0)                              # no bytes, no pointer needed


def test_the_mirrors_name_it_and_both_modes():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        assert NEW + "(" in open(os.path.join(ROOT, *rel)).read(), rel
    for name, value in CONSTANTS:
        assert getattr(_lib, "REMOVE_" + name) == value
        assert re.search(r"#define SPLAT_REMOVE_%s +%du " % (name, value), hdr), name
        assert "pub const SPLAT_REMOVE_%s: u32 = %d;" % (name, value) in ffi, name
    assert _lib.REMOVED_INDEX == 0xFFFFFFFF
    # the C++ mirror, named like its neighbours, and the Python one
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "splat_amd", "csrc", "host", "splat_host.cpp")).read()
    assert "uint64_t remove_gaussians_device(splat_ctx* ctx" in hpp and "uint64_t remove_gaussians_device(splat_ctx* ctx" in cpp
    assert "SPLAT_REMOVE_SELECTED" in hpp and "SPLAT_REMOVE_UNSELECTED" in hpp
    assert callable(splat_amd.Renderer.remove)
    # declared with the scene calls, and named in the note on what version 7 gained
    assert hdr.index("int splat_pick_device(") < hdr.index("int " + NEW + "(") < hdr.index("int splat_get_scene_layout(")
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    assert NEW in note and "SPLAT_REMOVE_" in note
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    # the ctypes signature is the header's: seven arguments, the sixth a pointer to the count
    args = [s for s in _lib.SYMBOLS if s[0] == NEW][0][2]
    assert len(args) == 7 and args[1] is C.c_uint64 and args[3] is C.c_uint32 and args[5] == C.POINTER(C.c_uint64)
    decl = re.search(r"int %s\(([^)]*)\)" % NEW, hdr).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "n", "d_selection", "mode", "d_index_map_out", "n_out",
                                                                            "producer_stream"]


def test_the_documents_say_what_a_caller_must_know():
    for rel in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "remove" in open(os.path.join(ROOT, rel)).read(), rel
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "stale" in integ and "splat_multi_ctx" in integ
    assert "R.remove(sel)" in open(os.path.join(ROOT, "README.md")).read()


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_the_new_kernels_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS + REUSED:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS)
def test_256_threads_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    print(name, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"])
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md


def test_the_gather_holds_a_gaussian_in_registers(kernels):
    """sixteen float4 planes in flight per lane are 64 VGPRs; with addresses and ranks the kernel stays within 128, which is
    four waves a SIMD -- 1024 lanes' loads in flight per CU"""
    md = kernels["splat::compact_scene_kernel"][1]
    assert 64 <= md[".vgpr_count"] <= 128, md[".vgpr_count"]


# ---- Renderer.remove, as far as it judges its arguments itself ------------------------------------------------------------
@pytest.fixture
def R():
    """a Renderer without a context: whatever reaches the library comes back as SplatError(ERR_INVALID, "NULL context")"""
    r = splat_amd.Renderer.__new__(splat_amd.Renderer)
    r._L, r._h, r.n, r.config = _lib.lib(), None, 100, _lib.Config()
    return r


def test_renderer_remove_rejects_what_it_can_judge(R):
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.remove(FakeTensor(99))                                     # a wrong length
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.remove(FakeTensor(101), keep=True)
    with pytest.raises(TypeError, match="one byte"):
        R.remove(FakeTensor(100, itemsize=4))                        # a wrong dtype
    with pytest.raises(TypeError, match="data_ptr"):
        R.remove(np.zeros(100, np.uint8))                            # a host array
    with pytest.raises(ValueError, match="not contiguous"):
        R.remove(FakeTensor(100, contiguous=False))
    with pytest.raises(TypeError, match="32-bit"):
        R.remove(FakeTensor(100), index_map=FakeTensor(100, itemsize=8))
    with pytest.raises(ValueError, match="100 elements expected"):
        R.remove(FakeTensor(100), index_map=FakeTensor(99, itemsize=4))
    # ... and a call it has nothing against reaches the library, which has no context here; n stays what it was
    for kw in ({}, {"keep": True}, {"index_map": FakeTensor(100, itemsize=4), "stream": 0}):
        with pytest.raises(splat_amd.SplatError) as e:
            R.remove(FakeTensor(100), **kw)
        assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    assert R.n == 100
