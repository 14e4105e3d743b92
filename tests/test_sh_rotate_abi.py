"""The sh rotation as far as it shows without a GPU: the three entry points exist and refuse a NULL context before they touch
HIP, every mirror of the ABI names them under version 7, the Python surface is there, and the gfx950 code object holds both
flavours of rotate_sh_kernel with 256 threads, at most 128 VGPRs, and neither spills nor scratch -- the 45 coefficients of a
Gaussian live in registers."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

from splat_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_sh_rotation_blocks", "splat_rotate_sh_scene_device", "splat_rotate_sh_gaussians_device")
KERNELS = ("splat::rotate_sh_kernel<false>", "splat::rotate_sh_kernel<true>")


def test_the_library_exports_the_three_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def test_a_null_context_or_matrix_is_refused_before_any_device_work():
    L = _lib.lib()
    p = C.c_void_p
    r = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    assert L.splat_rotate_sh_scene_device(None, r) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    assert L.splat_rotate_sh_gaussians_device(None, 4, p(16), r, None) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    # ... also when there is nothing to do, and without a matrix
    assert L.splat_rotate_sh_gaussians_device(None, 0, None, r, None) == _lib.ERR_INVALID
    assert L.splat_rotate_sh_scene_device(None, None) == _lib.ERR_INVALID
    assert L.splat_rotate_sh_gaussians_device(None, 4, p(16), None, None) == _lib.ERR_INVALID


def test_the_blocks_need_neither_a_context_nor_a_gpu():
    import splat_amd
    d = splat_amd.sh_rotation_blocks(np.eye(3))
    assert [a.shape for a in d] == [(3, 3), (5, 5), (7, 7)] and all(a.dtype == np.float32 for a in d)
    assert all(np.array_equal(a, np.eye(len(a), dtype=np.float32)) for a in d)


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()


def test_the_mirrors_name_all_three():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    for name in NEW:
        assert name in hpp and name.replace("splat_", "", 1) + "(" in hpp, name
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    # declared after the transforms, whose comment still says what they leave undone; the version comment names the three
    doc = hdr.split("int splat_transform_gaussians_device(")[1].split("int splat_rotate_sh_gaussians_device(")[0]
    for name in NEW[:2]:
        assert "int " + name + "(" in doc, name
    assert "orthogonal" in doc and "splat_multi_" in doc and "0 * inf" in doc
    assert "NOT rotated" in hdr.split("int splat_selection_indices_device(")[1].split("int splat_transform_gaussians_device(")[0]
    added = hdr.split("Added under version 7")[1].split("*/")[0]
    for name in NEW:
        assert name in added, name


def test_the_python_surface_exists():
    import splat_amd
    assert callable(splat_amd.sh_rotation_blocks)
    assert callable(splat_amd.Renderer.rotate_sh)
    assert list(inspect.signature(splat_amd.Renderer.rotate_sh).parameters) == ["self", "rotation", "index", "stream", "k"]
    par = inspect.signature(splat_amd.Renderer.transform).parameters
    assert list(par)[:5] == ["self", "matrix", "index", "stream", "k"] and par["rotate_sh"].default is False


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_both_flavours_of_the_kernel_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS)
def test_256_threads_at_most_128_vgprs_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256 and md[".vgpr_count"] <= 128, md
