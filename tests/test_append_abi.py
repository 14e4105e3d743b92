"""splat_append_gaussians_device and splat_reorder_scene_device as far as they show without a GPU: the library exports them,
what the append can judge of its arguments is refused before the context is looked at (so before any device work) and in the
documented order, every mirror of the ABI names both under version 7, the gfx950 code object holds the three new kernels with
256 threads and neither spills nor scratch, and Renderer.append / reorder / duplicate refuse what they can judge by themselves."""
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
APPEND, REORDER = "splat_append_gaussians_device", "splat_reorder_scene_device"
KERNELS = ("splat::grow_scene_kernel", "splat::pack_append_kernel", "splat::permute_scene_kernel")
REUSED = ("splat::pack_scene_kernel", "splat::plane_bounds_kernel", "splat::radix_scatter_kernel", "splat::unpack_kernel<false>",
          "splat::inverse_order_kernel", "splat::order_moved_kernel")
LIMIT = 0xFFFFFFFF


def test_the_library_exports_both_entry_points():
    for name in (APPEND, REORDER):
        assert hasattr(C.CDLL(LIB), name), name
        assert [s[0] for s in _lib.SYMBOLS].count(name) == 1, name


def append(ctx, n=100, m=10, pos=4096, cov=8192, op=12288, sh=16384, n_out=True):
    out = C.c_uint64(0xABCD)
    rc = _lib.lib().splat_append_gaussians_device(ctx, n, m, *[C.c_void_p(p) if p else None for p in (pos, cov, op, sh)],
                                                  C.byref(out) if n_out else None, None)
    assert out.value == 0xABCD, "a refused call writes nothing, not even *n_out"
    return rc


def refused(why, **kw):
    """(this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)"""
    assert append(None, **kw) == _lib.ERR_INVALID
    got = _lib.lib().splat_last_error(None)
    assert why.encode() in got, got


def test_every_refusal_names_its_argument_before_the_context_is_looked_at():
    refused("n_out", n_out=False)
    refused("n + m", n=LIMIT - 10, m=10)
    refused("n + m", n=LIMIT, m=0)
    refused("n + m", n=0, m=LIMIT)
    refused("n + m", n=1, m=2 ** 64 - 1)                             # the sum is judged, not its low 64 bits
    refused("n + m", n=2 ** 64 - 1, m=2 ** 64 - 1)
    refused("d_pos4", pos=0)
    refused("d_cov3d", cov=0)
    refused("d_opacity", op=0)
    refused("d_sh", sh=0)
    # ... in that order, and what is fine as far as the arguments go ends at the missing context
    refused("n_out", n_out=False, n=LIMIT, pos=0)
    refused("n + m", n=LIMIT - 1, m=1, pos=0, sh=0)
    refused("d_pos4", pos=0, cov=0, op=0, sh=0)
    refused("d_cov3d", cov=0, op=0, sh=0)
    refused("d_opacity", op=0, sh=0)
    refused("NULL context")
    refused("NULL context", n=LIMIT - 11, m=10)                      # n + m = 0xFFFFFFFE: the last count an index can number
    refused("NULL context", m=0, pos=0, cov=0, op=0, sh=0)           # no rows, no pointers needed
    refused("NULL context", pos=4097)                                # alignment is the kernels' to need, as in an upload
    # the reorder has nothing to judge but the context
    moved = C.c_uint64(0xABCD)
    assert _lib.lib().splat_reorder_scene_device(None, C.byref(moved)) == _lib.ERR_INVALID and moved.value == 0xABCD
    assert b"NULL context" in _lib.lib().splat_last_error(None)
    assert _lib.lib().splat_reorder_scene_device(None, None) == _lib.ERR_INVALID


def test_the_mirrors_name_both_calls():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in (APPEND, REORDER):
            assert name + "(" in text, (rel, name)
    # the C++ mirror, named like its neighbours, and the Python one
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "splat_amd", "csrc", "host", "splat_host.cpp")).read()
    for decl in ("uint64_t append_gaussians_device(splat_ctx* ctx", "uint64_t reorder_scene_device(splat_ctx* ctx"):
        assert decl in hpp and decl in cpp, decl
    for method in ("append", "reorder", "duplicate"):
        assert callable(getattr(splat_amd.Renderer, method)), method
    # declared directly after the removal, in this order, and named in the note on what version 7 gained
    at = [hdr.index("int " + name + "(") for name in ("splat_remove_gaussians_device", APPEND, REORDER)]
    assert at == sorted(at)
    between = hdr[at[0]:at[2]]
    assert len(re.findall(r"^int splat_\w+\(", between, re.M)) == 2, "nothing is declared between the removal and the two"
    assert hdr.index("int splat_pick_device(") < at[0] and at[2] < hdr.index("int splat_get_scene_layout(")
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    assert APPEND in note and REORDER in note
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    # the ctypes signatures are the header's
    args = [s for s in _lib.SYMBOLS if s[0] == APPEND][0][2]
    assert len(args) == 9 and args[1] is C.c_uint64 and args[2] is C.c_uint64 and args[7] == C.POINTER(C.c_uint64)
    decl = re.search(r"int %s\(([^)]*)\)" % APPEND, hdr).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "n", "m", "d_pos4", "d_cov3d", "d_opacity", "d_sh", "n_out",
                                                                            "producer_stream"]
    args = [s for s in _lib.SYMBOLS if s[0] == REORDER][0][2]
    assert len(args) == 2 and args[1] == C.POINTER(C.c_uint64)
    decl = re.search(r"int %s\(([^)]*)\)" % REORDER, hdr).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in decl.split("/*")[0].split(",")] == ["ctx", "moved_out"]


def test_the_documents_say_what_a_caller_must_know():
    for rel in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "append" in text and "reorder" in text, rel
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("splat_decode_ply_device", "splat_compute_cov3d_device", "stale", "splat_multi_ctx"):
        assert word in integ[integ.index(APPEND + "("):], word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "R.append(" in readme and "R.reorder()" in readme


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_the_new_kernels_are_in_the_gfx950_code_object(kernels):
    for name in KERNELS + REUSED:
        assert name in kernels, (name, sorted(kernels))


@pytest.mark.parametrize("name", KERNELS + ("splat::order_moved_kernel",))
def test_256_threads_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    print(name, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"])
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md


@pytest.mark.parametrize("name", ("splat::grow_scene_kernel", "splat::permute_scene_kernel"))
def test_the_copies_hold_a_gaussian_in_registers(kernels, name):
    """sixteen float4 planes per lane are 64 VGPRs; with addresses the kernels stay within 128, which is four waves a SIMD, as
    compact_scene_kernel does"""
    md = kernels[name][1]
    assert 64 <= md[".vgpr_count"] <= 128, md[".vgpr_count"]


# ---- Renderer.append / reorder / duplicate, as far as they judge their arguments themselves -----------------------------------
@pytest.fixture
def R():
    """a Renderer without a context: whatever reaches the library comes back as SplatError(ERR_INVALID, "NULL context")"""
    r = splat_amd.Renderer.__new__(splat_amd.Renderer)
    r._L, r._h, r.n, r.config = _lib.lib(), None, 100, _lib.Config()
    return r


def floats(numel, contiguous=True):
    t = FakeTensor(numel, contiguous=contiguous, itemsize=4)
    t.dtype = "torch.float32"
    return t


def rows(m, **other):
    """four fake float32 tensors of m rows; other: {field: tensor} in place of the right one"""
    t = dict(positions=floats(4 * m), cov3d=floats(9 * m), opacities=floats(m), sh=floats(48 * m))
    t.update(other)
    return [t[f] for f in ("positions", "cov3d", "opacities", "sh")]


def test_renderer_append_rejects_what_it_can_judge(R):
    with pytest.raises(ValueError, match="whole number of Gaussians"):
        R.append(*rows(10, positions=floats(41)))
    with pytest.raises(ValueError, match="90 floats expected"):
        R.append(*rows(10, cov3d=floats(91)))
    with pytest.raises(ValueError, match="10 floats expected"):
        R.append(*rows(10, opacities=floats(9)))
    with pytest.raises(ValueError, match="480 floats expected"):
        R.append(*rows(10, sh=floats(48)))
    with pytest.raises(TypeError, match="float32 expected"):
        R.append(*rows(10, sh=FakeTensor(480, itemsize=4)))          # 32 bits wide, and not float32
    with pytest.raises(ValueError, match="not contiguous"):
        R.append(*rows(10, sh=floats(480, contiguous=False)))
    with pytest.raises(TypeError, match="data_ptr"):
        R.append(rows(10)[0], np.zeros((10, 9), np.float32), *rows(10)[2:])      # a host array
    with pytest.raises(TypeError, match="m= is required"):
        R.append(np.zeros((10, 4), np.float32), *rows(10)[1:])       # ... which says nothing a device buffer would
    with pytest.raises(TypeError, match="m= is required"):
        R.append(4096, 8192, 12288, 16384)                           # plain addresses say nothing of their length
    with pytest.raises(TypeError, match="all four fields"):
        R.append(floats(40))
    with pytest.raises(ValueError, match="not negative"):
        R.append(4096, 8192, 12288, 16384, m=-1)
    # ... and a call it has nothing against reaches the library, which has no context here; n stays what it was
    for call in (lambda: R.append(*rows(10)), lambda: R.append(4096, 8192, 12288, 16384, m=3, stream=0), lambda: R.append(*rows(0)),
                 lambda: R.reorder()):
        with pytest.raises(splat_amd.SplatError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    assert R.n == 100
    # with no resident scene an append is an upload: that call's answer to a missing context
    R.n = 0
    with pytest.raises(splat_amd.SplatError) as e:
        R.append(*rows(10))
    assert e.value.code == _lib.ERR_INVALID and R.n == 0


def test_renderer_duplicate_rejects_what_it_can_judge(R):
    with pytest.raises(TypeError, match="k= is required"):
        R.duplicate(4096)
    with pytest.raises(TypeError, match="32-bit"):
        R.duplicate(FakeTensor(10, itemsize=8))
    with pytest.raises(ValueError, match="not contiguous"):
        R.duplicate(FakeTensor(10, itemsize=4, contiguous=False))
    assert R.duplicate(FakeTensor(0, itemsize=4)) == (100, 100)      # nothing to copy: nothing is asked of the library
    # ... and a call it has nothing against reaches the library before anything is allocated
    for kw in ({}, {"stream": 0}):
        with pytest.raises(splat_amd.SplatError) as e:
            R.duplicate(FakeTensor(10, itemsize=4), **kw)
        assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    with pytest.raises(splat_amd.SplatError) as e:
        R.duplicate(4096, k=3)
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    assert R.n == 100
