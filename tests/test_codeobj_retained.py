"""The compositor flavours of frames composited from retained lists (composite_retained_kernel: the walks keep their staging
verdicts) are held to the budgets tests/test_codeobj.py holds composite_exact_kernel to -- seven workgroups per CU.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

LIB = os.path.join(ROOT, "splat_amd", "libsplat_hip.so")


@pytest.fixture(scope="module")
def kernels():
    return {codeobj.demangle(sym).split("(")[0].replace("void ", ""): md for sym, md in codeobj.kernels(LIB).items()}


def test_retained_compositor_register_and_lds_budgets(kernels):
    for flav in ("<false, false, 0>", "<false, false, 2>", "<false, true, 0>", "<false, true, 2>"):
        md = kernels["splat::composite_retained_kernel" + flav]
        assert md[".vgpr_count"] <= 72, (flav, md[".vgpr_count"])
        assert md[".sgpr_count"] <= 96, (flav, md[".sgpr_count"])
        assert md[".group_segment_fixed_size"] <= 22 * 1024 + 256, flav
    md0 = kernels["splat::composite_retained_kernel<false, false, 0>"]
    assert md0.get(".vgpr_spill_count", 0) == 0 and md0.get(".sgpr_spill_count", 0) == 0 and md0[".private_segment_fixed_size"] == 0
    md2 = kernels["splat::composite_retained_kernel<false, false, 2>"]
    assert md2.get(".vgpr_spill_count", 0) <= 1 and md2[".private_segment_fixed_size"] <= 256


def test_the_paired_flavours_exist(kernels):
    for flav in ("<true, false, 0>", "<true, false, 2>"):
        assert "splat::composite_retained_kernel" + flav in kernels
