"""The visibility query's two entry points as far as they show without a GPU: the library exports them, what they can judge of
their arguments is refused before the context is looked at (so before any device work) with the argument named, every mirror
of the ABI names them and the query struct under version 7, the gfx950 code object holds the new kernel with 256 threads,
neither spills nor scratch and the registers and LDS the compile reports, and Renderer.visibility / select_counts /
select_visible refuse what they can judge by themselves."""
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
VIS, COUNTS = "splat_visibility_device", "splat_select_counts_device"
NEW = (VIS, COUNTS)
KERNEL = "splat::visibility_kernel"
REUSED = ("splat::nb_apply_kernel",)
# what the compile reports.  LDS: 256 entries x (16 + 16 + 8 + 4 + 3 x 4) bytes = 14336, the four waves' flags 16, and the 256
# bytes the device library's workgroup reduction behind __syncthreads_or takes (a kernel that does nothing else has them)
VGPRS, LDS_BYTES = 30, 14336 + 16 + 256


def test_the_library_exports_the_two_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def camera(w=64.0, h=48.0):
    cam = _lib.CameraC()
    cam.w, cam.h, cam.sh_dim = w, h, 15
    return cam


def last():
    return _lib.lib().splat_last_error(None)


def vis_refused(why, q=True, cam=True, weight_min=1.0 / 255.0, op=0, w=64.0, h=48.0, pixels=4096, max_weight=8192, weight_sum=16384):
    query = _lib.VisibilityQuery(weight_min, 0, 0, 63, 47, op)
    p = C.c_void_p
    rc = _lib.lib().splat_visibility_device(None, C.byref(query) if q else None, C.byref(camera(w, h)) if cam else None, None, None,
                                            p(pixels) if pixels else None, p(max_weight) if max_weight else None,
                                            p(weight_sum) if weight_sum else None, None)
    assert rc == _lib.ERR_INVALID and why.encode() in last(), last()


def counts_refused(why, n=10, counts=4096, lo=1, hi=0xFFFFFFFF, op=0, sel=8192):
    count = C.c_uint64(0xABCD)
    rc = _lib.lib().splat_select_counts_device(None, n, C.c_void_p(counts) if counts else None, lo, hi, op, C.c_void_p(sel) if sel else None,
                                               C.byref(count), None)
    assert rc == _lib.ERR_INVALID and why.encode() in last(), last()
    assert count.value == 0xABCD, "a refused call writes nothing, not even *count_out"


def test_every_refusal_names_its_argument_before_the_context_is_looked_at():
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    vis_refused("NULL q", q=False)
    vis_refused("NULL cam", cam=False)
    for bad in (float("nan"), -0.5, 1.0, 2.0, float("inf")):
        vis_refused("weight_min", weight_min=bad)
    vis_refused("unknown op", op=2)
    for w, h in ((0.0, 48.0), (64.5, 48.0), (64.0, 65536.0), (float("nan"), 48.0)):
        vis_refused("w/h", w=w, h=h)
    vis_refused("d_pixels is misaligned", pixels=4098)
    vis_refused("d_max_weight is misaligned", max_weight=8193)
    vis_refused("d_weight_sum is misaligned", weight_sum=16388)          # 4-byte aligned is not enough
    vis_refused("all NULL", pixels=0, max_weight=0, weight_sum=0)
    vis_refused("NULL q", q=False, cam=False, pixels=0, max_weight=0, weight_sum=0)      # ... in that order
    vis_refused("weight_min", weight_min=-1.0, op=7, w=0.0)
    vis_refused("unknown op", op=7, w=0.0)
    vis_refused("NULL context")
    vis_refused("NULL context", weight_min=0.0, op=1, max_weight=0, weight_sum=0)        # one output is enough
    vis_refused("NULL context", weight_min=0.999, pixels=0, max_weight=0)
    counts_refused("count_min is above count_max", lo=5, hi=4)
    counts_refused("unknown op", op=4)
    counts_refused("too many", n=1 << 32)
    counts_refused("NULL d_counts", counts=0)
    counts_refused("d_counts is misaligned", counts=4097)
    counts_refused("NULL d_selection", sel=0)
    counts_refused("NULL context")
    counts_refused("NULL context", n=0, counts=0, sel=0)                 # nothing to judge: no buffer needed
    counts_refused("NULL context", lo=0, hi=0, op=3, sel=8193)           # a selection lies at any byte address


def test_the_mirrors_name_the_two_calls_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    for method in ("visibility", "select_counts", "select_visible"):
        assert callable(getattr(splat_amd.Renderer, method)), method
    # declared behind the pick, in this order, and named in the note on what version 7 gained
    at = [hdr.index("int " + name + "(") for name in ("splat_pick_device",) + NEW + ("splat_remove_gaussians_device",)]
    assert at == sorted(at)
    assert len(re.findall(r"^int splat_\w+\(", hdr[at[0]:at[-1]], re.M)) == 3, "nothing else is declared between them"
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    for name in NEW + ("splat_visibility_query", "SPLAT_VIS_"):
        assert name in note, name
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    for name, value in (("SET", 0), ("ACCUMULATE", 1)):
        assert re.search(r"#define SPLAT_VIS_%s\s+%du" % (name, value), hdr), name
        assert re.search(r"pub const SPLAT_VIS_%s: u32 = %d;" % (name, value), ffi), name
        assert getattr(_lib, "VIS_" + name) == value
    # the struct's layout: 24 bytes, the header's fields in the header's order, in all three
    assert C.sizeof(_lib.VisibilityQuery) == 24
    body = re.search(r"typedef struct \{([^}]*)\} splat_visibility_query;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [re.sub(r"\[.*?\]", "", part.strip().split()[-1]) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == [f[0] for f in _lib.VisibilityQuery._fields_] == ["weight_min", "x0", "y0", "x1", "y1", "op"]
    rs = re.search(r"pub struct SplatVisibilityQuery \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub ([a-z0-9_]+):", re.sub(r"//.*", "", rs)) == c_fields
    # the ctypes signatures are the header's
    for name, names in ((VIS, ["ctx", "q", "cam", "d_pixel_mask", "d_mask", "d_pixels", "d_max_weight", "d_weight_sum", "producer_stream"]),
                        (COUNTS, ["ctx", "n", "d_counts", "count_min", "count_max", "op", "d_selection", "count_out", "producer_stream"])):
        decl = re.search(r"int %s\(([^)]*)\)" % name, hdr).group(1)
        assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == names, name
        assert len([s for s in _lib.SYMBOLS if s[0] == name][0][2]) == len(names), name


def test_the_documents_say_what_a_caller_must_know():
    for rel in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "select_visible" in text and VIS in text, rel
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("R.select_visible(cam, sel, pixel_mask=lasso)", "R.select_visible(train_cams, sel); R.remove(sel, keep=True)"):
        assert word in readme, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("splat_visibility_query", "SPLAT_VIS_ACCUMULATE", "weight_sum", "splat_device_bytes"):
        assert word in integ[integ.index("(`" + VIS):], word
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    doc = hdr[hdr.index("/* VISIBILITY"):hdr.index("int " + VIS)]
    for word in ("retained", "splat_device_bytes", "16 bytes a Gaussian"):       # the state the query leaves behind, and the figure
        assert word in doc, word


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


def test_the_new_kernel_is_in_the_gfx950_code_object(kernels):
    for name in (KERNEL,) + REUSED:
        assert name in kernels, (name, sorted(kernels))


def test_256_threads_no_spills_no_scratch_and_the_figures_of_the_compile(kernels):
    md = kernels[KERNEL][1]
    print(KERNEL, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"], "lds", md.get(".group_segment_fixed_size", 0))
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md
    assert md[".vgpr_count"] == VGPRS, md[".vgpr_count"]
    assert md.get(".group_segment_fixed_size", 0) == LDS_BYTES, md


# ---- the Renderer's methods, as far as they judge their arguments themselves --------------------------------------------------
@pytest.fixture
def R():
    """a Renderer without a context: whatever reaches the library comes back as SplatError(ERR_INVALID, "NULL context")"""
    r = splat_amd.Renderer.__new__(splat_amd.Renderer)
    r._L, r._h, r.n, r.config = _lib.lib(), None, 100, _lib.Config()
    return r


def reaches_the_library(call):
    with pytest.raises(splat_amd.SplatError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)


def words(numel, itemsize=4):
    return FakeTensor(numel, itemsize=itemsize)


def test_renderer_visibility_rejects_what_it_can_judge(R):
    cam = camera()
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="weight_min"):
            R.visibility(cam, weight_min=bad, pixels=words(100))
    with pytest.raises(ValueError, match="at least one"):
        R.visibility(cam)
    with pytest.raises(ValueError, match="100 elements expected"):
        R.visibility(cam, pixels=words(99))
    with pytest.raises(TypeError, match="4-byte elements"):
        R.visibility(cam, pixels=words(100, 8))
    with pytest.raises(TypeError, match="4-byte elements"):
        R.visibility(cam, max_weight=words(100, 8))
    with pytest.raises(TypeError, match="8-byte elements"):
        R.visibility(cam, weight_sum=words(100, 4))
    with pytest.raises(ValueError, match="3072 bytes expected"):
        R.visibility(cam, pixels=words(100), pixel_mask=FakeTensor(3071))
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.visibility(cam, pixels=words(100), mask=FakeTensor(101))
    with pytest.raises(TypeError, match="data_ptr"):
        R.visibility(cam, pixels=np.zeros(100, np.uint32))
    with pytest.raises(ValueError):
        R.visibility(cam, pixels=words(100), rect=(0, 0, 5))
    reaches_the_library(lambda: R.visibility(cam, pixels=words(100)))
    reaches_the_library(lambda: R.visibility(cam, weight_min=0.0, rect=(3, 4, 20, 30), pixel_mask=FakeTensor(3072), mask=FakeTensor(100),
                                             pixels=words(100), max_weight=words(100), weight_sum=words(100, 8), accumulate=True, stream=0))
    reaches_the_library(lambda: R.visibility(cam, weight_sum=4096))


def test_renderer_select_counts_rejects_what_it_can_judge(R):
    sel = FakeTensor(100)
    with pytest.raises(ValueError, match="above at_most"):
        R.select_counts(words(100), sel, at_least=3, at_most=2)
    with pytest.raises(ValueError, match="32-bit counts"):
        R.select_counts(words(100), sel, at_least=-1)
    with pytest.raises(ValueError, match="op"):
        R.select_counts(words(100), sel, op="xor")
    with pytest.raises(TypeError, match="4-byte elements"):
        R.select_counts(words(100, 8), sel)
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.select_counts(words(100), FakeTensor(99))
    reaches_the_library(lambda: R.select_counts(words(100), sel))
    reaches_the_library(lambda: R.select_counts(4096, 8192, at_least=0, at_most=7, op="subtract", stream=0))


def test_renderer_select_visible_rejects_what_it_can_judge(R):
    cam, sel = camera(), FakeTensor(100)
    with pytest.raises(ValueError, match="at least one camera"):
        R.select_visible([], sel)
    with pytest.raises(ValueError, match="min_pixels"):
        R.select_visible(cam, sel, min_pixels=-1)
    with pytest.raises(ValueError, match="op"):
        R.select_visible(cam, sel, op="xor")
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.select_visible(cam, FakeTensor(99))
    with pytest.raises(ValueError, match="at least one camera"):
        R.select_visible(iter(()), sel)
    with pytest.raises(TypeError, match="a camera"):
        R.select_visible(7, sel)
    with pytest.raises(TypeError, match="every element"):
        R.select_visible((c for c in (cam, "cam")), sel)
    # a generator and an object array are sequences of cameras like a list: each gets as far as the library's allocation
    for cams in ((c for c in (cam, camera())), np.array([cam, camera()], dtype=object), [cam], cam):
        with pytest.raises(splat_amd.SplatError):
            R.select_visible(cams, sel)
