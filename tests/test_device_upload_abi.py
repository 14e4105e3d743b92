"""The device-resident scene upload as far as it shows without a GPU: the three entry points exist and refuse a NULL
context before they touch HIP, every mirror of the ABI names them under version 7, and the gfx950 code object holds the new
kernels (scene box, Morton codes, the radix sort's histogram / scan / scatter, block bounds) without spills or scratch and
small enough in LDS to share a CU."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

from splat_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_upload_scene_device", "splat_compute_cov3d_device", "splat_get_scene_layout")
KERNELS = ("splat::scene_box_kernel", "splat::scene_box_final_kernel", "splat::morton_code_kernel", "splat::radix_hist_kernel",
           "splat::radix_scan_kernel", "splat::radix_scatter_kernel", "splat::block_bounds_kernel")
# MI355X: 160 KiB of LDS per CU, workgroups per CU <= floor(160 KiB / LDS per workgroup): two workgroups share a CU while
# each declares at most 80 KiB
LDS_FOR_TWO_WORKGROUPS = 160 * 1024 // 2


def test_the_library_exports_the_three_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def test_a_null_context_is_refused_before_any_device_work():
    L = _lib.lib()
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    assert L.splat_upload_scene_device(None, 4, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == _lib.ERR_INVALID
    assert L.splat_compute_cov3d_device(None, 4, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), None) == _lib.ERR_INVALID
    orig = (C.c_uint32 * 4)()
    bounds = (C.c_float * 8)()
    assert L.splat_get_scene_layout(None, orig, 4, bounds, 1) == _lib.ERR_INVALID


def test_abi_version_is_seven_everywhere():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "#define SPLAT_ABI_VERSION 7\n" in hdr
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in ffi


def test_the_mirrors_name_all_three():
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


def test_the_new_kernels_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS)
def test_no_spills_no_scratch_and_lds_for_two_workgroups_per_cu(kernels, name):
    md = kernels[name][1]
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".group_segment_fixed_size"] <= LDS_FOR_TWO_WORKGROUPS, md
    # 256 threads each, and registers that leave the wave slots to the LDS and the 32-wave cap: at most 64 VGPRs = 8 waves / SIMD
    assert md[".max_flat_workgroup_size"] == 256 and md[".vgpr_count"] <= 64, md
