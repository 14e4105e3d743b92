"""The pick as far as it shows without a GPU: the library exports the entry point, the three structs have the header's sizes
and field order in ctypes and Rust, every mirror and the version-7 note name the call, the ABI is still 7, a bad argument is
refused before the context is looked at with a reason that names it, the gfx950 code object holds the kernels with 256
threads and neither spills nor scratch, and Renderer.pick refuses what it can judge by itself."""
import ctypes as C
import inspect
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
NAME = "splat_pick_device"
KERNELS = ("splat::pick_hits_kernel<false>", "splat::pick_hits_kernel<true>", "splat::pick_resolve_kernel", "splat::pick_front_kernel<false>",
           "splat::pick_front_kernel<true>")
FIELDS = {"splat_pick_query": ("PickQuery", "SplatPickQuery", 16, ["alpha_min", "coverage_min", "max_hits", "max_layers"]),
          "splat_pick_result": ("PickResult", "SplatPickResult", 32, ["n_hits", "flags", "front_index", "front_depth", "front_alpha",
                                                                      "surface_index", "surface_depth", "surface_coverage"]),
          "splat_pick_layer": ("PickLayer", "SplatPickLayer", 16, ["index", "depth", "alpha", "coverage"])}


def read(*rel):
    return open(os.path.join(ROOT, *rel)).read()


def test_the_library_exports_the_entry_point():
    assert hasattr(C.CDLL(LIB), NAME)
    names = [s[0] for s in _lib.SYMBOLS]
    assert names[names.index("splat_select_neighbours_device") + 1] == NAME


@pytest.mark.parametrize("cname", sorted(FIELDS))
def test_struct_layouts_agree(cname):
    pyname, rsname, size, fields = FIELDS[cname]
    ct = getattr(_lib, pyname)
    assert C.sizeof(ct) == size and [f[0] for f in ct._fields_] == fields
    assert all(C.sizeof(f[1]) == 4 for f in ct._fields_)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, read("include", "splat_hip.h")).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    in_header = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", re.sub(r"^\s*(uint32_t|float)\s+", "", decl.strip()))]
    assert in_header == fields
    body = re.search(r"pub struct %s \{([^}]*)\}" % rsname, read("rust", "src", "ffi.rs")).group(1)
    assert re.findall(r"pub (\w+): (?:u32|f32)", body) == fields


def test_numpy_layouts_are_the_structs():
    for dt, ct in ((splat_amd.Renderer.PICK_RESULT_DTYPE, _lib.PickResult), (splat_amd.Renderer.PICK_LAYER_DTYPE, _lib.PickLayer)):
        assert dt.itemsize == C.sizeof(ct) and list(dt.names) == [f[0] for f in ct._fields_]
        assert [dt.fields[n][1] for n in dt.names] == [getattr(ct, n).offset for n in dt.names]


def test_the_constants():
    hdr = read("include", "splat_hip.h")
    for name, value, text in (("SPLAT_PICK_MAX_PIXELS", 256, "256"), ("SPLAT_PICK_MAX_HITS", 4096, "4096"),
                              ("SPLAT_PICK_NONE", 0xFFFFFFFF, "0xFFFFFFFFu"), ("SPLAT_PICK_TRUNCATED", 1, "1u")):
        assert re.search(r"#define %s\s+%s\n" % (name, text), hdr), name
        assert getattr(_lib, name[len("SPLAT_"):]) == value
        assert "pub const %s: u32" % name in read("rust", "src", "ffi.rs")


def test_abi_version_is_still_seven():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    assert "#define SPLAT_ABI_VERSION 7\n" in read("include", "splat_hip.h")
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in read("rust", "src", "ffi.rs")


def test_the_mirrors_name_the_call():
    for rel in (("include", "splat_hip.h"), ("rust", "src", "ffi.rs"), ("INTEGRATION.md",)):
        assert NAME + "(" in read(*rel), rel
    for rel in (("include", "splat_host.hpp"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = read(*rel)
        assert "pick(" in text and NAME in text, rel
    hdr = read("include", "splat_hip.h")
    assert hdr.index("int splat_select_neighbours_device(") < hdr.index("int %s(" % NAME) < hdr.index("int splat_read_scene_device(") \
        < hdr.index("int splat_get_scene_layout(")
    note = hdr.split("#define SPLAT_ABI_VERSION 7")[1].split("*/")[0]
    assert NAME in note
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "pick" in read(doc), doc
    assert 'r = R.pick(cam, [(x, y)])' in read("README.md") and 'sel[r["surface_index"][0]] = 1' in read("README.md")
    assert "SPLAT_MODE_LIBM_EXP" in hdr.split("The PICK")[1].split("#define SPLAT_PICK_MAX_PIXELS")[0]


# ---- refusals that need no device -------------------------------------------------------------------------------------
def camera(w=64.0, h=48.0):
    cam = _lib.CameraC()
    cam.w, cam.h = w, h
    return cam


def call(ctx=None, alpha_min=0.0, coverage_min=0.5, max_hits=1024, max_layers=0, cam=True, pixels=((3, 4),), n_pixels=None, results=16,
         layers=None, w=64.0, h=48.0, query=True):
    q = _lib.PickQuery(alpha_min, coverage_min, max_hits, max_layers)
    px = np.ascontiguousarray(pixels if pixels is not None else [], np.int32).reshape(-1)
    n = len(px) // 2 if n_pixels is None else n_pixels
    p = C.c_void_p
    return _lib.lib().splat_pick_device(ctx, C.byref(q) if query else None, C.byref(camera(w, h)) if cam else None, n,
                                        px.ctypes.data_as(C.POINTER(C.c_int32)) if len(px) else None, None,
                                        p(results) if results else None, p(layers) if layers else None, None)


def refused(why, **kw):
    """(this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)"""
    assert call(None, **kw) == _lib.ERR_INVALID
    got = _lib.lib().splat_last_error(None)
    assert why.encode() in got, got
    if why != "NULL context":
        assert b"context" not in got, got


def test_a_bad_argument_is_refused_before_the_context_is_looked_at():
    refused("n_pixels", pixels=[(1, 1)] * 257)
    refused("n_pixels", n_pixels=0xFFFFFFFF)
    refused("pixels_xy", pixels=[(64, 0)])                     # x = W
    refused("pixels_xy", pixels=[(0, 48)])                     # y = H
    refused("pixels_xy", pixels=[(-1, 0)])
    refused("pixels_xy", pixels=[(3, 4), (0, -1)])
    refused("pixels_xy", pixels=[(3, 4)] * 255 + [(64, 47)])
    refused("pixels_xy", pixels=None, n_pixels=1)
    refused("max_hits", max_hits=0)
    refused("max_hits", max_hits=4097)
    refused("max_hits", max_hits=0xFFFFFFFF)
    refused("max_layers", max_hits=4, max_layers=5)
    refused("coverage_min", coverage_min=0.0)
    refused("coverage_min", coverage_min=-0.5)
    refused("coverage_min", coverage_min=1.0000001)
    refused("coverage_min", coverage_min=float("nan"))
    refused("coverage_min", coverage_min=float("inf"))
    refused("alpha_min", alpha_min=float("nan"))
    refused("d_layers", max_layers=1, layers=None)
    refused("d_layers", max_layers=1, layers=18)               # misaligned
    refused("d_results", results=None)
    refused("d_results", results=17)
    refused("cam", cam=False)
    refused("cam", w=64.5)
    refused("cam", h=0.0)
    refused("NULL q", query=False)


def test_a_faultless_call_ends_at_the_null_context():
    refused("NULL context")
    refused("NULL context", pixels=[(0, 0), (63, 47), (63, 47)], max_hits=1, coverage_min=1.0, alpha_min=-1.0)
    refused("NULL context", pixels=[(1, 1)] * 256, max_hits=4096, max_layers=4096, layers=32, alpha_min=float("inf"))
    refused("NULL context", pixels=[], n_pixels=0, results=None)          # (n_pixels == 0 is fine, with a context)
    refused("NULL context", coverage_min=1e-45)


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
    assert md[".group_segment_fixed_size"] < 64 * 1024, md


# ---- Renderer.pick, as far as it judges its arguments itself -----------------------------------------------------------------
@pytest.fixture
def R():
    r = splat_amd.Renderer.__new__(splat_amd.Renderer)
    r._L, r._h, r.n, r.config = _lib.lib(), None, 100, _lib.Config()
    return r


def test_the_signature():
    ps = list(inspect.signature(splat_amd.Renderer.pick).parameters.values())
    assert [p.name for p in ps] == ["self", "cam_c", "pixels", "alpha_min", "coverage", "mask", "max_hits", "layers", "results", "layers_out",
                                    "stream"]
    assert all(p.kind == p.KEYWORD_ONLY for p in ps[3:]) and all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:3])
    assert [p.default for p in ps[3:]] == [0.0, 0.5, None, 1024, 0, None, None, None]
    assert "256" in splat_amd.Renderer.pick.__doc__ and "ValueError" in splat_amd.Renderer.pick.__doc__


def test_renderer_pick_rejects_what_it_can_judge(R):
    cam = camera()
    with pytest.raises(ValueError, match="at most 256"):
        R.pick(cam, [(1, 1)] * 257)
    with pytest.raises(ValueError, match="max_hits"):
        R.pick(cam, [(1, 1)], max_hits=0)
    with pytest.raises(ValueError, match="max_hits"):
        R.pick(cam, [(1, 1)], max_hits=4097)
    with pytest.raises(ValueError, match="layers"):
        R.pick(cam, [(1, 1)], max_hits=8, layers=9)
    with pytest.raises(TypeError, match="data_ptr"):
        R.pick(cam, [(1, 1)], mask=np.zeros(100, np.uint8))   # a host array
    # ... and with the caller's buffers a call it has nothing against reaches the library, which has no context here
    with pytest.raises(splat_amd.SplatError) as e:
        R.pick(cam, [(1, 1), (2, 2)], results=4096, layers=2, layers_out=8192)
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    with pytest.raises(splat_amd.SplatError) as e:
        R.pick(cam, [(64, 1)], results=4096)
    assert "pixels_xy" in str(e.value)
