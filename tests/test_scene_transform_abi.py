"""The scene read-back and transform as far as they show without a GPU: the four entry points exist and refuse a NULL context
before they touch HIP, every mirror of the ABI names them under version 7, and the gfx950 code object holds both flavours
of both kernels (unpack, transform) with 256 threads, at most 64 VGPRs, and neither spills nor scratch."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

from splat_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_read_scene_device", "splat_read_gaussians_device", "splat_transform_scene_device", "splat_transform_gaussians_device")
KERNELS = ("splat::unpack_kernel<false>", "splat::unpack_kernel<true>", "splat::transform_kernel<false>", "splat::transform_kernel<true>")


def test_the_library_exports_the_four_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def test_a_null_context_is_refused_before_any_device_work():
    L = _lib.lib()
    p = C.c_void_p
    m = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    assert L.splat_read_scene_device(None, 4, 15, p(16), p(16), p(16), p(16)) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    assert L.splat_read_gaussians_device(None, 4, p(16), 15, p(16), p(16), p(16), p(16), None) == _lib.ERR_INVALID
    assert L.splat_transform_scene_device(None, m) == _lib.ERR_INVALID
    assert L.splat_transform_gaussians_device(None, 4, p(16), m, None) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    # ... also when there is nothing to do
    assert L.splat_read_scene_device(None, 4, 0, None, None, None, None) == _lib.ERR_INVALID
    assert L.splat_read_gaussians_device(None, 0, None, 15, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.splat_transform_gaussians_device(None, 0, None, m, None) == _lib.ERR_INVALID


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()


def test_the_mirrors_name_all_four():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    for name in NEW:
        assert name in hpp and name.replace("splat_", "", 1) + "(" in hpp, name
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    doc = hdr.split("int splat_selection_indices_device(")[1].split("int splat_transform_gaussians_device(")[0]
    assert "NOT rotated" in doc and "splat_multi_" in doc and "splat_device_bytes()" in doc


def test_the_python_surface_exists():
    import splat_amd
    for name in ("read_device", "read_indexed", "transform"):
        assert callable(getattr(splat_amd.Renderer, name))
    from splat_amd.gaussians import DeviceGaussians
    assert callable(DeviceGaussians.pull)


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_both_flavours_of_both_kernels_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS)
def test_256_threads_at_most_64_vgprs_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256 and md[".vgpr_count"] <= 64, md
