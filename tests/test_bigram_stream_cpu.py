"""Streaming bigram-LM recognition without a GPU: the sr_bigram_stream_* entry points are in the library, the header and the binding,
the ABI version is unchanged, the stream kernel's instantiations are in the gfx950 build within their resource limits
(tools/isa_info.py), a null model or search net is refused before any device is touched, and the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

SYMBOLS = ("sr_bigram_stream_open", "sr_bigram_stream_begin", "sr_bigram_stream_push", "sr_bigram_stream_partial", "sr_bigram_stream_end",
           "sr_bigram_stream_destroy")
# bigram_stream_kernel<KW, GSM>: the dispatch of bigram_gs_kernel
KERNELS = ("bigram_stream_kernel<1, 1>", "bigram_stream_kernel<2, 1>", "bigram_stream_kernel<4, 1>", "bigram_stream_kernel<8, 1>",
           "bigram_stream_kernel<8, 2>")


def _header():
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        return f.read()


def test_library_header_and_binding_carry_the_bigram_stream_entry_points():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    hdr = _header()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert re.search(r"SR_API int " + sym + r"\(", hdr), sym
        assert sym in capi.SYMBOLS, sym
    assert re.search(r"typedef struct sr_bigram_stream sr_bigram_stream;", hdr)
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # entry points and an opaque type more, no struct changed
    assert capi.SR_ABI_VERSION == 4 and lib.sr_abi_version() == 4
    assert hasattr(capi, "BigramStream") and hasattr(capi.Model, "bigram_stream")


def test_open_without_a_model_or_search_net_is_einval():
    from speechrecognition_amd import build, capi

    build.build()
    L = capi.lib()
    p = capi.BigramParams(capi.FLT_MAX, capi.FLT_MAX, capi.GMM_DEFAULT, 0, 0)
    out = ctypes.c_void_p()
    assert L.sr_bigram_stream_open(None, None, ctypes.byref(p), 4, 100, ctypes.byref(out)) == -1
    assert out.value is None
    assert L.sr_bigram_stream_destroy(None) == 0
    id_ = ctypes.c_uint32()
    assert L.sr_bigram_stream_begin(None, ctypes.byref(id_)) == -1
    assert L.sr_bigram_stream_push(None, 0, None, None, None) == -1


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")
def test_stream_kernel_instantiations_within_resource_limits():
    from speechrecognition_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram", tmp))
    for kernel in KERNELS:
        assert kernel in md, (kernel, sorted(md))
        k = md[kernel]
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, (kernel, k)   # 1024 threads = 4 waves per SIMD
        assert k.get("group_segment_fixed_size", 0) == 0, (kernel, k)        # LDS: dynamic only, bigram_gs_lds(W, ENG)
        if kernel == "bigram_stream_kernel<8, 2>":   # may match bigram_gs_kernel<8, 2>'s pinned ceiling
            assert k["private_segment_fixed_size"] <= 16 and k.get("vgpr_spill_count", 0) <= 2, (kernel, k)
        else:
            assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, (kernel, k)


def test_streaming_linear_search_mirror_compiles():
    """include/sr_sietill.hpp's sr::StreamingLinearSearch against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "bigram_stream_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
