"""The front end's kernels after the split of the per-frame body into its two halves and with the warp search beside them, read from
the gfx950 code object without a GPU (tools/isa_info.py): mfcc_warps_kernel, vtln_reduce_kernel and the changed mfcc_kernel and
stream_frontend_kernel have no scratch and spill nothing, and the two changed kernels still fit the eight waves per SIMD (at most 64
vector registers) they had.  (The warp search's LDS rule is checked in tests/test_vtln_cpu.py, through the host-only driver.)"""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")

KERNELS = ["mfcc_warps_kernel", "vtln_reduce_kernel", "mfcc_kernel", "stream_frontend_kernel"]


@pytest.fixture(scope="module")
def frontend_object():
    from speechrecognition_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        yield isa_info.kernel_metadata(isa_info.code_object("frontend", tmp))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(frontend_object, kernel):
    assert kernel in frontend_object, sorted(frontend_object)
    k = frontend_object[kernel]
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
    assert not k.get("uses_dynamic_stack", 0) or k["uses_dynamic_stack"] in (0, "false"), k


@pytest.mark.parametrize("kernel", ["mfcc_kernel", "stream_frontend_kernel", "mfcc_warps_kernel"])
def test_registers_leave_eight_waves_per_simd(frontend_object, kernel):
    k = frontend_object[kernel]
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 64, k
