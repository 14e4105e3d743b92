"""The selection by neighbourhood as far as it shows without a GPU: the library exports the entry point, a bad argument is
refused before the context is looked at (so before any device work) with a reason that names the argument, every mirror of
the ABI names the call under version 7, the gfx950 code object holds the new kernels with 256 threads and neither spills nor
scratch, and Renderer.select_neighbours refuses what it can judge by itself."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

import splat_amd  # noqa: E402
from splat_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NAME = "splat_select_neighbours_device"
KERNELS = ("splat::nb_block_pairs_kernel", "splat::nb_count_kernel<false>", "splat::nb_count_kernel<true>", "splat::nb_apply_kernel")
UNBOUNDED = 0xFFFFFFFF


def read(*rel):
    return open(os.path.join(ROOT, *rel)).read()


def test_the_library_exports_the_entry_point():
    assert hasattr(C.CDLL(LIB), NAME)
    names = [s[0] for s in _lib.SYMBOLS]
    # next to the other two selection symbols
    assert names[names.index("splat_select_device"):][:3] == ["splat_select_device", "splat_selection_indices_device", NAME]


def call(ctx=None, radius=1.0, source=None, count_min=0, count_max=UNBOUNDED, op=0, sel=16, counts=None, limit=0):
    p = C.c_void_p
    return _lib.lib().splat_select_neighbours_device(ctx, radius, p(source) if source else None, count_min, count_max, op,
                                                     p(sel) if sel else None, p(counts) if counts else None, limit, None, None, None)


def refused(why, **kw):
    """(this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)"""
    assert call(None, **kw) == _lib.ERR_INVALID
    got = _lib.lib().splat_last_error(None)
    assert why.encode() in got, got
    if why != "NULL context":
        assert b"context" not in got, got


def test_a_bad_argument_is_refused_before_the_context_is_looked_at():
    refused("radius", radius=float("nan"))
    refused("radius", radius=-1.0)
    refused("radius", radius=-1e-45)
    refused("radius", radius=float("inf"))
    refused("radius", radius=float("-inf"))
    refused("radius", radius=1.9e19)                          # finite, its square is not (f32 max is 3.4e38)
    refused("radius", radius=3.4e38)
    refused("count_min", count_min=1, count_max=0)
    refused("count_min", count_min=UNBOUNDED, count_max=UNBOUNDED - 1)
    refused("op", op=4)
    refused("op", op=0x80000000)
    refused("op", op=4, sel=None, counts=16)                 # (not used by a counts-only call, refused all the same)
    refused("d_selection", sel=None, counts=None)
    refused("d_counts_out", sel=None, counts=None)
    refused("d_counts_out", counts=18)
    refused("d_counts_out", sel=None, counts=17)


def test_a_faultless_call_ends_at_the_null_context():
    refused("NULL context")
    refused("NULL context", radius=0.0)
    refused("NULL context", radius=-0.0)
    refused("NULL context", radius=1.8e19)                    # its square is finite
    refused("NULL context", count_min=3, count_max=3, op=3, source=17, sel=17, counts=16, limit=5)
    refused("NULL context", source=16, sel=16, op=1, count_min=1)      # a selection grown in place
    refused("NULL context", sel=None, counts=32)               # counts only


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in read("include", "splat_hip.h")
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in read("rust", "src", "ffi.rs")


def test_the_mirrors_name_the_call():
    for rel in (("include", "splat_hip.h"), ("rust", "src", "ffi.rs"), ("INTEGRATION.md",)):
        assert NAME + "(" in read(*rel), rel
    for rel in (("include", "splat_host.hpp"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = read(*rel)
        assert "select_neighbours(" in text and NAME in text, rel
    hdr = read("include", "splat_hip.h")
    assert hdr.index("int splat_selection_indices_device(") < hdr.index("int %s(" % NAME) < hdr.index("int splat_read_scene_device(")
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    assert NAME in note
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "select_neighbours" in read(doc), doc


def test_the_header_states_no_new_selection_bit():
    # an entry point of its own: the query and its tests are as they were
    assert C.sizeof(_lib.SelectQuery) == 92
    assert "SPLAT_SEL_NEIGHB" not in read("include", "splat_hip.h")


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
def test_256_threads_no_spills_no_scratch(kernels, name):
    md = kernels[name][1]
    print(name, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"], "lds", md[".group_segment_fixed_size"])
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md


# ---- Renderer.select_neighbours, as far as it judges its arguments itself ------------------------------------------------
class FakeTensor:
    """what _device_address looks at of a torch tensor"""

    class Device:
        type, index = "cuda", 0

    def __init__(self, numel, contiguous=True, itemsize=1):
        self._numel, self._contiguous, self._itemsize, self.device, self.dtype = numel, contiguous, itemsize, self.Device(), "torch.uint8"

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._contiguous

    def numel(self):
        return self._numel

    def element_size(self):
        return self._itemsize


@pytest.fixture
def R():
    """a Renderer without a context: whatever reaches the library comes back as SplatError(ERR_INVALID, "NULL context")"""
    r = splat_amd.Renderer.__new__(splat_amd.Renderer)
    r._L, r._h, r.n, r.config = _lib.lib(), None, 100, _lib.Config()
    return r


def test_the_signature():
    sig = inspect.signature(splat_amd.Renderer.select_neighbours)
    ps = list(sig.parameters.values())
    assert [p.name for p in ps] == ["self", "selection", "radius", "source", "at_least", "at_most", "op", "counts", "max_block_pairs",
                                    "stream"]
    assert all(p.kind == p.KEYWORD_ONLY for p in ps[3:]) and all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:3])
    assert [p.default for p in ps[3:]] == [None, 0, None, "set", None, None, None]
    doc = splat_amd.Renderer.select_neighbours.__doc__
    assert "select_neighbours(sel, r, at_most=k-1)" in doc and 'select_neighbours(sel, r, source=sel, at_least=1, op="add")' in doc


def test_renderer_select_neighbours_rejects_what_it_can_judge(R):
    with pytest.raises(ValueError, match="not contiguous"):
        R.select_neighbours(FakeTensor(100, contiguous=False), 1.0)
    with pytest.raises(TypeError, match="data_ptr"):
        R.select_neighbours(np.zeros(100, np.uint8), 1.0)        # a host array
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.select_neighbours(FakeTensor(99), 1.0)
    with pytest.raises(TypeError, match="one byte"):
        R.select_neighbours(FakeTensor(100, itemsize=4), 1.0)
    with pytest.raises(ValueError, match="op"):
        R.select_neighbours(FakeTensor(100), 1.0, op="xor")
    # ... the same for the source mask
    with pytest.raises(ValueError, match="source: not contiguous"):
        R.select_neighbours(FakeTensor(100), 1.0, source=FakeTensor(100, contiguous=False))
    with pytest.raises(ValueError, match="source: 100 bytes expected"):
        R.select_neighbours(FakeTensor(100), 1.0, source=FakeTensor(101))
    with pytest.raises(TypeError, match="source: one byte"):
        R.select_neighbours(FakeTensor(100), 1.0, source=FakeTensor(100, itemsize=2))
    # ... and what is this call's own
    with pytest.raises(ValueError, match="at_least"):
        R.select_neighbours(FakeTensor(100), 1.0, at_least=3, at_most=2)
    with pytest.raises(ValueError, match="radius"):
        R.select_neighbours(FakeTensor(100), -0.5)
    with pytest.raises(ValueError, match="radius"):
        R.select_neighbours(FakeTensor(100), float("nan"))
    with pytest.raises(TypeError, match="32-bit"):
        R.select_neighbours(FakeTensor(100), 1.0, counts=FakeTensor(100, itemsize=8))
    with pytest.raises(ValueError, match="100 elements expected"):
        R.select_neighbours(FakeTensor(100), 1.0, counts=FakeTensor(64, itemsize=4))
    with pytest.raises(ValueError, match="at least one"):
        R.select_neighbours(None, 1.0)
    # ... and a call it has nothing against reaches the library, which has no context here
    for kw in (dict(), dict(source=FakeTensor(100), at_least=1, op="add", stream=0), dict(at_most=7, counts=FakeTensor(100, itemsize=4)),
               dict(max_block_pairs=0)):
        with pytest.raises(splat_amd.SplatError) as e:
            R.select_neighbours(FakeTensor(100), 0.25, **kw)
        assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
        assert R.block_pairs is None
    with pytest.raises(splat_amd.SplatError) as e:
        R.select_neighbours(None, 0.25, counts=FakeTensor(100, itemsize=4))
    assert "NULL context" in str(e.value)
