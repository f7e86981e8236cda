"""Streaming recognition without a GPU: the sr_stream_* entry points are in the library, the header and the binding, the ABI
version is unchanged, the search kernel behind them is in the gfx950 build without scratch (tools/isa_info.py), and a null
model is refused before any device is touched."""
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

STREAM_SYMBOLS = ("sr_stream_open", "sr_stream_begin", "sr_stream_push", "sr_stream_partial", "sr_stream_end", "sr_stream_destroy")


def _header():
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        return f.read()


def test_library_header_and_binding_carry_the_stream_entry_points():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    hdr = _header()
    for sym in STREAM_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert re.search(r"SR_API int " + sym + r"\(", hdr), sym
        assert sym in capi.SYMBOLS, sym
    assert re.search(r"typedef struct sr_stream sr_stream;", hdr)
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # entry points and an opaque type more, no struct changed
    assert capi.SR_ABI_VERSION == 4 and lib.sr_abi_version() == 4


def test_open_without_a_model_is_einval():
    from speechrecognition_amd import build, capi

    build.build()
    L = capi.lib()
    sp = capi.SearchParams(100.0, 0.0, capi.GMM_DEFAULT, 0)
    out = ctypes.c_void_p()
    assert L.sr_stream_open(None, None, ctypes.byref(sp), 4, 100, ctypes.byref(out)) == -1
    assert out.value is None
    assert L.sr_stream_destroy(None) == 0


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")
def test_stream_kernel_has_no_scratch():
    from speechrecognition_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_decode", tmp))
    for kernel in ("decode_stream_kernel<1024>", "decode_big_kernel<1024>"):   # the latter shares the per-frame body (big_frame)
        assert kernel in md, (kernel, sorted(md))
        k = md[kernel]
        assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0, (kernel, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, (kernel, k)   # 1024 threads = 4 waves per SIMD


def test_streaming_recognizer_mirror_compiles():
    """include/sr_sietill.hpp's sr::StreamingRecognizer against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "stream_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
