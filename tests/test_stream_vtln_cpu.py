"""A VTLN warp per utterance of a stream set, without a GPU: sr_stream_set_warp and sr_bigram_stream_set_warp are in the library, the
header and the binding, the ABI version is unchanged, SR_STREAM_NO_WARP is the same number on both sides, a null stream set is
refused before any device is touched, and the C++ mirror's set_warp compiles and links into tests/cpp/stream_vtln_driver.cpp (its
GPU run is in tests/test_gpu_stream_vtln.py).  The kernel's registers are tests/test_isa_vtln_cpu.py's."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sr_stream_set_warp", "sr_bigram_stream_set_warp")
SR_EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        return f.read()


def compile_driver(exe):
    """tests/cpp/stream_vtln_driver.cpp against the built library, as tests/test_gpu_stream_audio.py compiles its driver"""
    lib_dir = os.path.join(ROOT, "speechrecognition_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stream_vtln_driver.cpp"), "-o", exe,
                           "-L" + lib_dir, "-lsrgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])


def test_library_header_and_binding_carry_the_entry_points():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    hdr = _header()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert re.search(r"SR_API int " + sym + r"\((?:struct )?\w+\* s, uint32_t id, uint32_t warp\);", hdr), sym
        assert sym in capi.SYMBOLS, sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)   # entry points more, no struct changed
    assert capi.SR_ABI_VERSION == 4 == lib.sr_abi_version()
    m = re.search(r"#define\s+SR_STREAM_NO_WARP\s+(0x[0-9A-Fa-f]+)u\b", hdr)
    assert m and int(m.group(1), 16) == capi.STREAM_NO_WARP == 0xFFFFFFFF
    for cls in (capi.Stream, capi.BigramStream):
        assert hasattr(cls, "set_warp")


def test_a_null_stream_set_is_einval():
    from speechrecognition_amd import build, capi

    build.build()
    L = capi.lib()
    for sym in SYMBOLS:
        assert getattr(L, sym)(None, 0, 0) == SR_EINVAL
        assert getattr(L, sym)(None, 0, capi.STREAM_NO_WARP) == SR_EINVAL
        assert b"null stream set" in L.sr_last_error()


def test_the_mirror_s_set_warp_compiles_and_links(tmp_path):
    from speechrecognition_amd import build

    build.build()
    mirror = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    for sym in SYMBOLS:
        assert sym + "(s_, id, warp)" in mirror
    exe = str(tmp_path / "stream_vtln_driver")
    compile_driver(exe)
    r = subprocess.run([exe], capture_output=True, text=True)   # no arguments: the usage line, before anything touches a device
    assert r.returncode == 2 and "usage" in r.stderr
