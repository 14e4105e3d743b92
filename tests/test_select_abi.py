"""The selection entry points as far as they show without a GPU: the library exports both, a bad query is refused before the
context is looked at (so before any device work), every mirror of the ABI names them and their constants under version 7,
the gfx950 code object holds the new kernels with 256 threads and neither spills nor scratch, and Renderer.select refuses
what it can judge by itself."""
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

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_select_device", "splat_selection_indices_device")
KERNELS = ("splat::select_kernel<0, false>", "splat::select_kernel<1, false>", "splat::select_kernel<2, false>",
           "splat::select_kernel<2, true>", "splat::mask_count_kernel", "splat::mask_scan_kernel", "splat::mask_scatter_kernel")
CONSTANTS = (("VOLUME", 1), ("SCREEN", 2), ("DEPTH", 4), ("OPACITY", 8), ("OP_SET", 0), ("OP_ADD", 1), ("OP_SUBTRACT", 2),
             ("OP_INTERSECT", 3))


def test_the_library_exports_both_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def camera():
    cam = _lib.CameraC()
    cam.w, cam.h = 64.0, 48.0
    return cam


def select(ctx, q, cam=None, mask=None, op=0, sel=16):
    L = _lib.lib()
    p = C.c_void_p
    return L.splat_select_device(ctx, C.byref(q) if q is not None else None, C.byref(cam) if cam is not None else None,
                                 p(mask) if mask else None, op, p(sel) if sel else None, None, None)


def refused(why, *a, **kw):
    """(this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)"""
    assert select(None, *a, **kw) == _lib.ERR_INVALID
    got = _lib.lib().splat_last_error(None)
    assert why.encode() in got, got


def query(**kw):
    q = _lib.SelectQuery()
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_a_null_context_is_refused_before_any_device_work():
    refused("NULL context", query(), None)
    refused("NULL context", query(tests=15, x1=5, y1=5), camera())
    L = _lib.lib()
    n = C.c_uint64(7)
    assert L.splat_selection_indices_device(None, 4, C.c_void_p(16), C.c_void_p(16), 4, C.byref(n), None) == _lib.ERR_INVALID
    assert b"NULL context" in L.splat_last_error(None)
    assert L.splat_selection_indices_device(None, 0, None, None, 0, C.byref(n), None) == _lib.ERR_INVALID


def test_a_bad_query_is_refused_before_the_context_is_looked_at():
    # the query is judged first, so that it can be judged here: the reason a call without a context leaves behind is the
    # query's fault, not the missing context
    refused("NULL query", None)
    refused("unknown bits", query(tests=16))
    refused("unknown bits", query(tests=0x80000001))
    refused("unknown op", query(), op=4)
    refused("unknown volume_shape", query(tests=_lib.SEL_VOLUME, volume_shape=2))
    refused("unknown screen_rule", query(tests=_lib.SEL_SCREEN, screen_rule=2), camera())
    refused("without a camera", query(tests=_lib.SEL_SCREEN))
    refused("without a camera", query(tests=_lib.SEL_DEPTH))
    refused("without a camera", query(tests=_lib.SEL_VOLUME | _lib.SEL_DEPTH))
    refused("pixel mask", query(tests=_lib.SEL_SCREEN, screen_rule=1), camera(), mask=16)
    bad = camera()
    bad.w = 64.5
    refused("w/h", query(tests=_lib.SEL_SCREEN), bad)
    # ... and what is fine as far as the query goes ends at the missing context
    refused("NULL context", query(tests=_lib.SEL_SCREEN, screen_rule=0), camera(), mask=16)
    refused("NULL context", query(tests=_lib.SEL_SCREEN, screen_rule=1), camera())
    refused("NULL context", query(tests=_lib.SEL_VOLUME | _lib.SEL_OPACITY, volume_shape=1), None, op=3)


def test_the_constants_agree_between_header_binding_and_rust():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for name, value in CONSTANTS:
        assert getattr(_lib, "SEL_" + name) == value
        assert re.search(r"#define SPLAT_SEL_%s +%d " % (name, value), hdr), name
        assert "pub const SPLAT_SEL_%s: u32 = %d;" % (name, value) in ffi, name
    # the query's layout: 92 bytes, the header's fields in the header's order, in all three
    assert C.sizeof(_lib.SelectQuery) == 92
    body = re.search(r"typedef struct \{([^}]*)\} splat_select_query;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [re.sub(r"\[.*?\]", "", part.strip().split()[-1]) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == [f[0] for f in _lib.SelectQuery._fields_]
    rs = re.search(r"pub struct SplatSelectQuery \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub ([a-z0-9_]+):", re.sub(r"//.*", "", rs)) == c_fields


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()


def test_the_mirrors_name_both():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    # declared behind the indexed edit they feed, and named in the note on what version 7 gained
    assert hdr.index("int splat_update_gaussians_device(") < hdr.index("int splat_select_device(") < hdr.index("int splat_get_scene_layout(")
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    for name in NEW:
        assert name in note, name


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
    print(name, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"])
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md


# ---- Renderer.select, as far as it judges its arguments itself ---------------------------------------------------------
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


def test_renderer_select_rejects_what_it_can_judge(R):
    cam = camera()
    with pytest.raises(ValueError, match="not contiguous"):
        R.select(FakeTensor(100, contiguous=False))
    with pytest.raises(TypeError, match="data_ptr"):
        R.select(np.zeros(100, np.uint8))                       # a host array
    with pytest.raises(ValueError, match="touch"):
        R.select(FakeTensor(100), cam, rect=(0, 0, 5, 5), rule="touch", pixel_mask=FakeTensor(64 * 48))
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.select(FakeTensor(99))
    with pytest.raises(TypeError, match="one byte"):
        R.select(FakeTensor(100, itemsize=4))
    with pytest.raises(ValueError, match="bytes expected"):
        R.select(FakeTensor(100), cam, rect=(0, 0, 5, 5), pixel_mask=FakeTensor(64 * 48 - 1))
    with pytest.raises(ValueError, match="cam_c"):
        R.select(FakeTensor(100), rect=(0, 0, 5, 5))
    with pytest.raises(ValueError, match="3x4"):
        R.select(FakeTensor(100), box=np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError, match="op"):
        R.select(FakeTensor(100), op="xor")
    with pytest.raises(TypeError, match="data_ptr"):
        R.selection_indices(np.zeros(100, np.uint8), FakeTensor(100, itemsize=4))
    with pytest.raises(TypeError, match="32-bit"):
        R.selection_indices(FakeTensor(100), FakeTensor(100, itemsize=8))
    # ... and a call it has nothing against reaches the library, which has no context here
    with pytest.raises(splat_amd.SplatError) as e:
        R.select(FakeTensor(100), cam, rect=(0, 0, 5, 5), rule="touch", opacity=(0.1, 1.0), op="add", stream=0)
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
