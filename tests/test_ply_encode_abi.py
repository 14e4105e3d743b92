"""The PLY encoder as far as it shows without a GPU: the two entry points exist and refuse bad arguments -- with the argument
named -- before they look at the context or touch HIP, every mirror of the ABI names them under version 7, the Python
surface refuses what it can judge itself, and the gfx950 code object holds both flavours of ply_encode_kernel with 256
threads, neither spills nor scratch, and at most 64 KiB of LDS."""
import ctypes as C
import inspect
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

import splat_amd  # noqa: E402
from splat_amd import _lib  # noqa: E402
from splat_amd.gaussians import PLY_PROPS, inria_layout  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")
NEW = ("splat_encode_ply_scene_device", "splat_encode_ply_gaussians_device")
KERNELS = ("splat::ply_encode_kernel<false>", "splat::ply_encode_kernel<true>")
LDS_MAX = 64 * 1024


def test_the_library_exports_the_two_entry_points():
    L = C.CDLL(LIB)
    for name in NEW:
        assert hasattr(L, name), name
    names = [s[0] for s in _lib.SYMBOLS]
    assert [s for s in names if s in NEW] == list(NEW)
    assert names.index("splat_upload_ply_device") + 1 == names.index(NEW[0])       # behind the pair they invert


def call_both(ctx, lay, rows=4096, k=None, index=64):
    """(whole scene, indexed) with k = layout.n unless given"""
    L = _lib.lib()
    p = C.c_void_p
    lp = C.byref(lay) if lay is not None else None
    k = (lay.n if lay is not None else 4) if k is None else k
    return (L.splat_encode_ply_scene_device(ctx, lp, p(rows)),
            L.splat_encode_ply_gaussians_device(ctx, k, p(index), lp, p(rows), None))


def test_a_faultless_call_ends_at_the_null_context():
    # (this machine may have no GPU at all: a call that reached HIP would not come back with ERR_INVALID)
    L = _lib.lib()
    for lay in (inria_layout(4), inria_layout(0)):
        for rc in call_both(None, lay):
            assert rc == _lib.ERR_INVALID
            assert b"NULL context" in L.splat_last_error(None)


def spoil(**kw):
    lay = inria_layout(4)
    for k, v in kw.items():
        if k == "offset":
            lay.offset[v[0]] = v[1]
        else:
            setattr(lay, k, v)
    return lay


OPACITY = _lib.PLY_SLOT_OPACITY
BAD = [("stride 0", dict(stride=0), "stride"), ("stride 250", dict(stride=250), "stride"),
       ("stride above the stage", dict(stride=65532), "stride"), ("offset 218", dict(offset=(OPACITY, 218)), "offset"),
       ("offset -2", dict(offset=(OPACITY, -2)), "offset"), ("offset == stride", dict(offset=(OPACITY, 248)), "offset"),
       ("offset past the stride", dict(offset=(OPACITY, 1024)), "offset"),
       ("opacity on top of x", dict(offset=(OPACITY, 0)), "overlap"), ("2^32 - 1 rows", dict(n=0xFFFFFFFF), "layout->n")]


@pytest.mark.parametrize("what,kw,reason", BAD, ids=[b[0] for b in BAD])
def test_each_invalid_layout_is_refused_with_its_argument_named_before_the_context_is_looked_at(what, kw, reason):
    L = _lib.lib()
    bad = spoil(**kw)
    for which in (0, 1):
        call_both(None, inria_layout(4))                                   # (the reason is "NULL context" again)
        assert b"NULL context" in L.splat_last_error(None)
        assert call_both(None, bad)[which] == _lib.ERR_INVALID
        if which == 1:
            assert reason.encode() in L.splat_last_error(None), L.splat_last_error(None)
        else:
            L.splat_encode_ply_scene_device(None, C.byref(bad), C.c_void_p(4096))
            assert reason.encode() in L.splat_last_error(None), L.splat_last_error(None)


def test_the_largest_stride_and_the_last_offset_of_a_row_pass():
    L = _lib.lib()
    assert call_both(None, spoil(stride=65528)) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL context" in L.splat_last_error(None)
    assert call_both(None, spoil(stride=252, offset=(OPACITY, 248))) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL context" in L.splat_last_error(None)
    only_x = spoil()
    for k in range(1, _lib.PLY_SLOTS):
        only_x.offset[k] = -1
    only_x.stride = 4
    assert call_both(None, only_x) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL context" in L.splat_last_error(None)


def test_null_layout_misaligned_or_null_rows_null_index_and_k_mismatch():
    L = _lib.lib()
    assert call_both(None, None) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL layout" in L.splat_last_error(None)
    for rows in (4098, 4097):
        assert call_both(None, inria_layout(4), rows=rows) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
        assert b"d_rows_out" in L.splat_last_error(None) and b"misaligned" in L.splat_last_error(None)
    assert call_both(None, inria_layout(4), rows=0) == (_lib.ERR_INVALID, _lib.ERR_INVALID)
    assert b"NULL d_rows_out" in L.splat_last_error(None)
    assert call_both(None, inria_layout(4), index=0)[1] == _lib.ERR_INVALID
    assert b"NULL d_index" in L.splat_last_error(None)
    for k in (3, 5, 0):
        assert call_both(None, inria_layout(4), k=k)[1] == _lib.ERR_INVALID
        assert b"layout->n is not k" in L.splat_last_error(None)


def test_abi_version_is_still_seven_and_the_layout_is_untouched():
    assert _lib.lib().splat_abi_version() == _lib.ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    assert "#define SPLAT_ABI_VERSION 7\n" in hdr
    assert "pub const SPLAT_ABI_VERSION: u32 = 7;" in open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert "#define SPLAT_PLY_SLOTS 59\n" in hdr and _lib.PLY_SLOTS == 59
    assert C.sizeof(_lib.PlyLayout) == 8 + 4 + 4 * 59


def test_the_mirrors_name_both():
    for rel in (("rust", "src", "ffi.rs"), ("INTEGRATION.md",), ("include", "splat_hip.h"), ("splat_amd", "csrc", "host", "splat_host.cpp")):
        text = open(os.path.join(ROOT, *rel)).read()
        for name in NEW:
            assert name + "(" in text, (rel, name)
    hpp = open(os.path.join(ROOT, "include", "splat_host.hpp")).read()
    for name in NEW:
        assert name in hpp, name
    assert "void encode_ply(" in hpp and "save_ply_from_gpu(" in hpp and "inria_layout(" in hpp
    assert "splat_host_save_ply_from_gpu(" in open(os.path.join(ROOT, "splat_amd", "csrc", "host", "splat_host.cpp")).read()
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    added = hdr.split("Added under version 7")[1].split("*/")[0]
    for name in NEW:
        assert name in added, name
    # declared behind the pair they invert, with what a save keeps said plainly
    doc = hdr.split("int splat_upload_ply_device(")[1].split("int splat_encode_ply_gaussians_device(")[0]
    assert "int splat_encode_ply_scene_device(" in doc
    assert "keep their bits" in doc and "NOT bit for bit" in doc and "mean" in doc and "no unstaged path" in doc
    for rel in (("README.md",), ("DESIGN.md",)):
        text = open(os.path.join(ROOT, *rel)).read()
        assert "save_ply" in text and "bit for bit" in text, rel


def test_the_canonical_layout_is_the_file_write_ply_writes():
    lay = inria_layout(7)
    assert isinstance(lay, _lib.PlyLayout) and lay.n == 7 and lay.stride == 248 == 4 * len(PLY_PROPS)
    for k, name in enumerate(_lib.PLY_SLOT_NAMES):
        assert lay.offset[k] == 4 * PLY_PROPS.index(name), name
    named = {lay.offset[k] for k in range(_lib.PLY_SLOTS)}
    assert sorted(set(range(0, 248, 4)) - named) == [12, 16, 20]                # nx ny nz: no slot
    assert splat_amd.inria_layout is inria_layout
    with pytest.raises(ValueError):
        inria_layout(-1)
    # the C++ mirror's is the same structure
    H = C.CDLL(os.path.join(ROOT, "splat_amd", "libsplat_host.so"))
    H.splat_host_inria_layout.argtypes, H.splat_host_inria_layout.restype = [C.c_ulonglong, C.POINTER(_lib.PlyLayout)], None
    other = _lib.PlyLayout()
    H.splat_host_inria_layout(7, C.byref(other))
    assert bytes(other)[:12] == bytes(lay)[:12] and list(other.offset) == list(lay.offset)


def test_the_python_surface_exists():
    assert list(inspect.signature(splat_amd.Renderer.encode_ply_rows).parameters) == ["self", "rows", "layout", "index", "stream", "k"]
    assert list(inspect.signature(splat_amd.Renderer.save_ply).parameters) == ["self", "path", "index", "stream", "k"]
    for par in (inspect.signature(splat_amd.Renderer.encode_ply_rows).parameters, inspect.signature(splat_amd.Renderer.save_ply).parameters):
        assert par["index"].default is None and par["stream"].default is None and par["k"].default is None


class FakeTensor:
    """what _device_address looks at of a torch tensor"""

    class Device:
        type, index = "cuda", 0

    def __init__(self, numel, contiguous=True, itemsize=1, ptr=4096):
        self._numel, self._contiguous, self._itemsize, self._ptr = numel, contiguous, itemsize, ptr
        self.device, self.dtype = self.Device(), "torch.uint8"

    def data_ptr(self):
        return self._ptr

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


def test_encode_ply_rows_refuses_what_it_can_judge_itself(R):
    lay = inria_layout(100)
    rows = FakeTensor(100 * 248)
    with pytest.raises(splat_amd.SplatError) as e:
        R.encode_ply_rows(rows, lay)                                            # faultless: ends at the library's NULL context
    assert e.value.code == _lib.ERR_INVALID and "NULL context" in str(e.value)
    with pytest.raises(splat_amd.SplatError):
        R.encode_ply_rows(rows, inria_layout(3), index=FakeTensor(3, itemsize=4))
    with pytest.raises(TypeError):
        R.encode_ply_rows(rows, "layout")
    with pytest.raises(ValueError, match="100 Gaussians"):
        R.encode_ply_rows(rows, inria_layout(99))
    with pytest.raises(ValueError, match="bytes"):
        R.encode_ply_rows(FakeTensor(100 * 248 - 1), lay)
    with pytest.raises(ValueError, match="multiple of 4"):
        R.encode_ply_rows(FakeTensor(100 * 248, ptr=4098), lay)
    with pytest.raises(ValueError, match="not contiguous"):
        R.encode_ply_rows(FakeTensor(100 * 248, contiguous=False), lay)
    with pytest.raises(ValueError, match="stride"):
        R.encode_ply_rows(rows, spoil(n=100, stride=250))
    with pytest.raises(ValueError, match="stride"):
        R.encode_ply_rows(rows, spoil(n=100, stride=65532))
    with pytest.raises(ValueError, match="offset"):
        R.encode_ply_rows(rows, spoil(n=100, offset=(OPACITY, 218)))
    with pytest.raises(ValueError, match="offset"):
        R.encode_ply_rows(rows, spoil(n=100, offset=(OPACITY, 248)))
    with pytest.raises(ValueError, match="overlaps"):
        R.encode_ply_rows(rows, spoil(n=100, offset=(OPACITY, 0)))
    with pytest.raises(ValueError, match="3 rows for 5 indices"):
        R.encode_ply_rows(rows, inria_layout(3), index=FakeTensor(5, itemsize=4))
    with pytest.raises(TypeError, match="32-bit"):
        R.encode_ply_rows(rows, inria_layout(3), index=FakeTensor(3, itemsize=8))
    with pytest.raises(TypeError, match="k="):
        R.encode_ply_rows(rows, inria_layout(3), index=8192)


def test_save_ply_refuses_what_it_can_judge_itself(R, tmp_path):
    path = str(tmp_path / "out.ply")
    with pytest.raises(TypeError, match="32-bit"):
        R.save_ply(path, index=FakeTensor(3, itemsize=8))
    with pytest.raises(TypeError, match="k="):
        R.save_ply(path, index=8192)
    with pytest.raises(ValueError, match="stream"):
        R.save_ply(path, index=8192, k=3, stream=12345)
    with pytest.raises(ValueError, match="no context"):
        R.save_ply(path)                                                        # faultless: ends at the missing context
    assert not os.path.exists(path)


@pytest.fixture(scope="module")
def kernels():
    ks = {}
    for sym, md in codeobj.kernels(LIB).items():
        ks[codeobj.demangle(sym).split("(")[0].replace("void ", "")] = (sym, md)
    return ks


@pytest.mark.parametrize("name", KERNELS)
def test_256_threads_no_spills_no_scratch_and_lds_within_64_kib(kernels, name):
    assert name in kernels, (name, sorted(kernels))
    md = kernels[name][1]
    print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS" % (name, md[".vgpr_count"], md[".sgpr_count"], md[".group_segment_fixed_size"]))
    assert md.get(".vgpr_spill_count", 0) == 0 and md.get(".sgpr_spill_count", 0) == 0, md
    assert md[".private_segment_fixed_size"] == 0, md
    assert md[".group_segment_fixed_size"] <= LDS_MAX, md
    assert md[".max_flat_workgroup_size"] == 256, md
