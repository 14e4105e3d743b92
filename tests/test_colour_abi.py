"""The four colour entry points as far as they show without a GPU: the library exports them, what they can judge of their
arguments is refused before the context is looked at (so before any device work) and in the documented order, every mirror of
the ABI names them and the query struct under version 7, the gfx950 code object holds the five new kernels with 256 threads,
neither spills nor scratch and no LDS beyond the selection's count, and Renderer.colours / select_colour / recolour refuse
what they can judge by themselves."""
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
EVAL, SELECT, RECOLOUR, RECOLOUR_K = ("splat_eval_colours_device", "splat_select_colour_device", "splat_recolour_scene_device",
                                      "splat_recolour_gaussians_device")
NEW = (EVAL, SELECT, RECOLOUR, RECOLOUR_K)
KERNELS = ("splat::eval_colour_kernel<false>", "splat::eval_colour_kernel<true>", "splat::select_colour_kernel",
           "splat::recolour_kernel<false>", "splat::recolour_kernel<true>")
REUSED = ("splat::inverse_order_kernel", "splat::index_check_kernel")
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
fp = C.POINTER(C.c_float)


def test_the_library_exports_the_four_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    assert [s[0] for s in _lib.SYMBOLS if s[0] in NEW] == list(NEW)


def camera():
    cam = _lib.CameraC()
    cam.w, cam.h, cam.sh_dim = 64.0, 48.0, 15
    return cam


def last():
    return _lib.lib().splat_last_error(None)


def eval_refused(why, cam=True, k=10, index=4096, out=8192):
    p = C.c_void_p
    rc = _lib.lib().splat_eval_colours_device(None, C.byref(camera()) if cam else None, k, p(index) if index else None,
                                              p(out) if out else None, None)
    assert rc == _lib.ERR_INVALID and why.encode() in last(), last()


def select_refused(why, q=True, cam=True, op=0, sel=4096, shape=1):
    query = _lib.ColourQuery()
    query.shape = shape
    count = C.c_uint64(0xABCD)
    rc = _lib.lib().splat_select_colour_device(None, C.byref(query) if q else None, C.byref(camera()) if cam else None, op,
                                               C.c_void_p(sel) if sel else None, C.byref(count), None)
    assert rc == _lib.ERR_INVALID and why.encode() in last(), last()
    assert count.value == 0xABCD, "a refused call writes nothing, not even *count_out"


def recolour_refused(why, m=IDENTITY, k=None, index=4096):
    L = _lib.lib()
    mp = np.ascontiguousarray(m, np.float32).ctypes.data_as(fp) if m is not None else None
    if k is None:
        rc = L.splat_recolour_scene_device(None, mp)
    else:
        rc = L.splat_recolour_gaussians_device(None, k, C.c_void_p(index) if index else None, mp, None)
    assert rc == _lib.ERR_INVALID and why.encode() in last(), last()


def with_entry(at, v):
    m = IDENTITY.copy()
    m[at] = v
    return m


def test_every_refusal_names_its_argument_before_the_context_is_looked_at():
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    eval_refused("cam", cam=False)
    eval_refused("d_rgb_out", out=0)
    eval_refused("d_rgb_out is misaligned", out=8194)
    eval_refused("cam", cam=False, out=0)                                # ... in that order
    eval_refused("NULL context")
    eval_refused("NULL context", index=0)                                # the whole-scene form: k is judged against n later
    eval_refused("NULL context", k=0, out=0)                             # no rows: no buffer needed
    eval_refused("NULL context", k=0, out=8194)
    select_refused("NULL q", q=False)
    select_refused("NULL cam", cam=False)
    select_refused("shape", shape=2)
    select_refused("unknown op", op=4)
    select_refused("d_selection", sel=0)
    select_refused("NULL q", q=False, cam=False, op=9, sel=0)
    select_refused("NULL cam", cam=False, shape=7, op=9, sel=0)
    select_refused("shape", shape=7, op=9, sel=0)
    select_refused("unknown op", op=9, sel=0)
    select_refused("NULL context")
    select_refused("NULL context", shape=0, op=3, sel=4097)              # a selection lies at any byte address
    for k in (None, 10):
        recolour_refused("NULL m", m=None, k=k)
        recolour_refused("non-finite", with_entry(0, np.nan), k=k)
        recolour_refused("non-finite", with_entry(7, np.inf), k=k)
        recolour_refused("non-finite", with_entry(11, -np.inf), k=k)
        recolour_refused("offset", with_entry(3, 3e38), k=k)             # every entry finite, (t + ...) / C0 not, in f32
        recolour_refused("NULL context", k=k)
        recolour_refused("NULL context", splat_amd.colour_matrix(saturation=0, contrast=1.2).ravel(), k=k)
    recolour_refused("d_index", k=10, index=0)
    recolour_refused("non-finite", with_entry(5, np.nan), k=10, index=0)  # the matrix first
    recolour_refused("NULL context", k=0, index=0)                       # no rows, no indices needed


def test_the_mirrors_name_the_four_calls_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    cpp = open(os.path.join(ROOT, "splat_amd", "csrc", "host", "splat_host.cpp")).read()
    for decl in ("void eval_colours_device(splat_ctx* ctx", "uint64_t select_colour_device(splat_ctx* ctx", "void recolour_scene_device(splat_ctx* ctx",
                 "void recolour_gaussians_device(splat_ctx* ctx"):
        assert decl in hpp and decl in cpp, decl
    for method in ("colours", "select_colour", "recolour"):
        assert callable(getattr(splat_amd.Renderer, method)), method
    assert callable(splat_amd.colour_matrix)
    # declared beside the sh rotation, in this order, and named in the note on what version 7 gained
    at = [hdr.index("int " + name + "(") for name in ("splat_rotate_sh_gaussians_device",) + NEW + ("splat_get_scene_layout",)]
    assert at == sorted(at)
    assert len(re.findall(r"^int splat_\w+\(", hdr[at[0]:at[-1]], re.M)) == 5, "nothing else is declared between them"
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    for name in NEW + ("splat_colour_query",):
        assert name in note, name
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    # the struct's layout: 56 bytes, the header's fields in the header's order, in all three
    assert C.sizeof(_lib.ColourQuery) == 56
    body = re.search(r"typedef struct \{([^}]*)\} splat_colour_query;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [re.sub(r"\[.*?\]", "", part.strip().split()[-1]) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert c_fields == [f[0] for f in _lib.ColourQuery._fields_] == ["colour_to_unit", "shape", "clamp"]
    rs = re.search(r"pub struct SplatColourQuery \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub ([a-z0-9_]+):", re.sub(r"//.*", "", rs)) == c_fields
    # the ctypes signatures are the header's
    for name, names in ((EVAL, ["ctx", "cam", "k", "d_index", "d_rgb_out", "producer_stream"]),
                        (SELECT, ["ctx", "q", "cam", "op", "d_selection", "count_out", "producer_stream"]),
                        (RECOLOUR, ["ctx", "m[12]"]), (RECOLOUR_K, ["ctx", "k", "d_index", "m[12]", "producer_stream"])):
        decl = re.search(r"int %s\(([^)]*)\)" % name, hdr).group(1)
        assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == names, name
        assert len([s for s in _lib.SYMBOLS if s[0] == name][0][2]) == len(names), name


def test_the_documents_say_what_a_caller_must_know():
    for rel in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        text = open(os.path.join(ROOT, rel)).read()
        assert "recolour" in text and "select_colour" in text, rel
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("R.colours(cam", "R.select_colour(cam, sel, rgb=rgb, tolerance=0.08)", "splat_amd.colour_matrix(saturation=0)"):
        assert word in readme, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("splat_colour_query", "splat_multi_ctx", "cam_pos", "sh_dim"):
        assert word in integ[integ.index(EVAL + "("):], word


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
def test_256_threads_no_spills_no_scratch_no_lds_beyond_the_count(kernels, name):
    md = kernels[name][1]
    print(name, "vgprs", md[".vgpr_count"], "sgprs", md[".sgpr_count"], "lds", md.get(".group_segment_fixed_size", 0))
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".max_flat_workgroup_size"] == 256, md
    assert md.get(".group_segment_fixed_size", 0) == (16 if "select" in name else 0), md     # four wave counts


@pytest.mark.parametrize("name", ("splat::recolour_kernel<false>", "splat::recolour_kernel<true>"))
def test_the_recolour_holds_a_gaussians_sh_in_registers(kernels, name):
    """48 coefficients and the thirteen planes they arrive in stay within 128 VGPRs: four waves a SIMD"""
    md = kernels[name][1]
    assert 48 <= md[".vgpr_count"] <= 128, md[".vgpr_count"]


# ---- the Renderer's methods, as far as they judge their arguments themselves --------------------------------------------------
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


def reaches_the_library(call):
    with pytest.raises(splat_amd.SplatError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)


def test_renderer_select_colour_rejects_what_it_can_judge(R):
    cam, sel = camera(), FakeTensor(100)
    with pytest.raises(ValueError, match="shape"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.1, shape="sphere")
    with pytest.raises(ValueError, match="tolerance"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="tolerance"):
        R.select_colour(cam, sel, tolerance=0.1)
    with pytest.raises(ValueError, match="tolerance"):
        R.select_colour(cam, sel)
    with pytest.raises(ValueError, match="positive"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=(0.1, 0.0, 0.1))
    with pytest.raises(ValueError, match="scalar or 3"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=(0.1, 0.2))
    with pytest.raises(ValueError, match="3 numbers"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5), tolerance=0.1)
    with pytest.raises(ValueError, match="3x4"):
        R.select_colour(cam, sel, matrix=np.eye(3))
    with pytest.raises(ValueError, match="one of the two"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.1, matrix=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="op"):
        R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.1, op="xor")
    with pytest.raises(ValueError, match="100 bytes expected"):
        R.select_colour(cam, FakeTensor(99), rgb=(0.5, 0.5, 0.5), tolerance=0.1)
    with pytest.raises(TypeError, match="data_ptr"):
        R.select_colour(cam, np.zeros(100, np.uint8), rgb=(0.5, 0.5, 0.5), tolerance=0.1)
    reaches_the_library(lambda: R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=0.08))
    reaches_the_library(lambda: R.select_colour(cam, sel, rgb=(0.5, 0.5, 0.5), tolerance=(0.1, 0.2, 0.3), shape="box", clamp=False, op="add",
                                                stream=0))
    reaches_the_library(lambda: R.select_colour(cam, 4096, matrix=np.zeros(12), op="intersect"))


def test_renderer_recolour_rejects_what_it_can_judge(R):
    with pytest.raises(ValueError, match="3x4"):
        R.recolour(np.eye(3))
    with pytest.raises(ValueError, match="3x4"):
        R.recolour(np.eye(4))
    with pytest.raises(TypeError, match="k= is required"):
        R.recolour(IDENTITY, 4096)
    with pytest.raises(TypeError, match="32-bit"):
        R.recolour(IDENTITY, FakeTensor(10, itemsize=8))
    with pytest.raises(ValueError, match="not contiguous"):
        R.recolour(IDENTITY, FakeTensor(10, itemsize=4, contiguous=False))
    with pytest.raises(TypeError, match="integer"):
        R.recolour(IDENTITY, [0.5, 1.5])
    with pytest.raises(ValueError, match="not negative"):
        R.recolour(IDENTITY, [3, -1])
    reaches_the_library(lambda: R.recolour(IDENTITY))
    reaches_the_library(lambda: R.recolour(splat_amd.colour_matrix(saturation=0), FakeTensor(10, itemsize=4)))
    reaches_the_library(lambda: R.recolour(IDENTITY.reshape(3, 4), 4096, k=3, stream=0))
    with pytest.raises(splat_amd.SplatError, match="non-finite"):
        R.recolour(np.full((3, 4), np.nan))


def test_renderer_colours_rejects_what_it_can_judge(R):
    cam = camera()
    with pytest.raises(ValueError, match="300 floats expected"):
        R.colours(cam, out=floats(299))
    with pytest.raises(ValueError, match="30 floats expected"):
        R.colours(cam, FakeTensor(10, itemsize=4), out=floats(300))
    with pytest.raises(TypeError, match="float32 expected"):
        R.colours(cam, out=FakeTensor(300, itemsize=4))
    with pytest.raises(TypeError, match="32-bit"):
        R.colours(cam, FakeTensor(10, itemsize=8), out=floats(30))
    with pytest.raises(TypeError, match="k= is required"):
        R.colours(cam, 4096, out=8192)
    with pytest.raises(TypeError, match="integer"):
        R.colours(cam, [0.5])
    out = floats(0)
    assert R.colours(cam, FakeTensor(0, itemsize=4), out=out) is out     # no rows: nothing is asked of the library
    assert R.colours(cam, []).shape == (0, 3)
    reaches_the_library(lambda: R.colours(cam, out=floats(300)))
    reaches_the_library(lambda: R.colours(cam, FakeTensor(10, itemsize=4), out=floats(30), stream=0))
    reaches_the_library(lambda: R.colours(cam, 4096, out=8192, k=5))
