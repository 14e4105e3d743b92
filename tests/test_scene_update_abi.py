"""The in-place scene edit as far as it shows without a GPU: the two entry points exist and refuse a NULL context before they
touch HIP, every mirror of the ABI names them under version 7, and the gfx950 code object holds the new kernels (inverse
order, index check, masked repack in both forms, bounds from the planes) with 256 threads, at most 64 VGPRs, and neither
spills nor scratch."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

from splat_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_update_scene_device", "splat_update_gaussians_device")
KERNELS = ("splat::inverse_order_kernel", "splat::index_check_kernel", "splat::repack_kernel<false>", "splat::repack_kernel<true>",
           "splat::plane_bounds_kernel")


def test_the_library_exports_both_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def test_a_null_context_is_refused_before_any_device_work():
    L = _lib.lib()
    p = C.c_void_p
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    assert L.splat_update_scene_device(None, 4, 15, p(16), p(16), p(16), p(16), None) == _lib.ERR_INVALID
    assert L.splat_update_gaussians_device(None, 4, p(16), 15, p(16), p(16), p(16), p(16), None) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    # ... also when there is nothing to do
    assert L.splat_update_scene_device(None, 4, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.splat_update_gaussians_device(None, 0, None, 15, None, None, None, None, None) == _lib.ERR_INVALID


def test_the_field_bits():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for name, bit in (("POS", 1), ("COV3D", 2), ("OPACITY", 4), ("SH", 8)):
        assert getattr(_lib, "FIELD_" + name) == bit
        assert "#define SPLAT_FIELD_%s %d " % (name, bit) in hdr
        assert "pub const SPLAT_FIELD_%s: u32 = %d;" % (name, bit) in ffi


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()


def test_the_mirrors_name_both():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    assert "splat_multi_" in open(os.path.join(ROOT, "include", "splat_hip.h")).read().split("SPLAT_FIELD_SH 8")[1].split("splat_update_scene_device(")[0]


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_the_new_kernels_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS)
def test_256_threads_at_most_64_vgprs_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256 and md[".vgpr_count"] <= 64, md
