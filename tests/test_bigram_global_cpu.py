"""The bigram search's global-states layout without a GPU: the entry point and the flag are in the library and the header, and the
new kernel's instantiations are in the gfx950 build without scratch (tools/isa_info.py, as tests/test_isa_cpu.py)."""
import ctypes
import os
import re
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

# bigram_gs_kernel<KW, GSM>: KW words per thread in the recombination; GSM 2 = the entries in device memory too (W > 4 720)
GS_KERNELS = ("bigram_gs_kernel<1, 1>", "bigram_gs_kernel<2, 1>", "bigram_gs_kernel<4, 1>", "bigram_gs_kernel<8, 1>", "bigram_gs_kernel<8, 2>")


def test_library_exports_describe_and_header_defines_the_flag():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert hasattr(lib, "sr_bigram_describe")
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+SR_BIGRAM_GLOBAL_STATES\s+2\b", hdr)
    assert re.search(r"SR_API int sr_bigram_describe\(const sr_bigram\* b, char\* out, size_t cap\);", hdr)
    assert capi.BIGRAM_GLOBAL_STATES == 2 and "sr_bigram_describe" in capi.SYMBOLS
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # an entry point more, no struct changed


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")
def test_global_states_kernels_have_no_scratch():
    from speechrecognition_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram", tmp))
    for kernel in GS_KERNELS:
        assert kernel in md, (kernel, sorted(md))
        k = md[kernel]
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, (kernel, k)   # 1024 threads = 4 waves per SIMD
        if kernel == "bigram_gs_kernel<8, 2>":
            # the one exception: eight words per thread AND the entries in device memory leave two VGPRs short of the
            # 128 a 1024-thread workgroup allows -- pinned here so that it cannot grow unnoticed
            assert k["private_segment_fixed_size"] <= 16 and k.get("vgpr_spill_count", 0) <= 2, (kernel, k)
        else:
            assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, (kernel, k)
