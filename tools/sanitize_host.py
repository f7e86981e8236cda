"""ASan + UBSan run of the HOST side of libsrgpu.so (sanitizers on the CPU build only: the GPU pool has no xnack+).

The host translation units (srgpu_api.cpp: handles, packing, shard/gather glue, the traceback walk; mixset.cpp: the
MIXSET parser / writer / host finalize; feeder.cpp: feeder, sr_shard_utterances, the multi-device driver; fmllr.cpp: the fMLLR
estimate; frontend.cpp: the front end's checks and tables) are compiled with
-fsanitize=address,undefined (device code untouched: -fno-gpu-sanitize) and linked with the regular kernel objects into
csrc/build/asan/libsrgpu_asan.so; tests/cpp/host_mirror_driver.cpp (include/sr_sietill.hpp: lexicon, edit distance, feature
post-processing, alignment dump) is built the same way.  Then the CPU tests of the boundary run against that library in a
Python that has the ASan runtime preloaded, and the driver's CPU modes run natively.  Any report fails the run
(-fno-sanitize-recover, abort_on_error).

Why it exists: the survey's own ASan run of the reference found two real memory bugs this code must stay compatible with
without sharing them -- the 2-float over-read of density_score_sse (Mixtures.cpp:653) and the T-sized cost arrays indexed by
position in align_sequence_full (Alignment.cpp:62-63).

usage: python tools/sanitize_host.py [pytest args]     exit code 0 = clean
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speechrecognition_amd import build as B  # noqa: E402

OUT = os.path.join(B.CSRC, "build", "asan")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-shared-libsan"]
HOST_UNITS = ["srgpu_api.cpp", "mixset.cpp", "feeder.cpp", "fmllr.cpp", "frontend.cpp"]
# (test_fmllr_cpu.py's driver test links tests/cpp/fmllr_driver.cpp against the regular libsrgpu.so: in this run it is the only
# fMLLR test that does not go through the sanitized estimate)
TESTS = ["tests/test_capi_cpu.py", "tests/test_traceback_cpu.py", "tests/test_sanitized_host_paths.py", "tests/test_fmllr_cpu.py"]


def runtime():
    p = subprocess.check_output(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    if not os.path.exists(p):
        raise RuntimeError("clang's shared ASan runtime not found: " + p)
    return p


def build():
    B.build()  # the regular library: its kernel objects are linked below
    os.makedirs(OUT, exist_ok=True)
    procs = []
    for src in HOST_UNITS:
        cmd = ["hipcc", "-x", "hip", "-c", os.path.join(B.CSRC, src), "-o", os.path.join(OUT, src + ".o"), "-O1", "-g", "-std=c++17",
               "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-fno-gpu-sanitize"] + SAN
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode:
            raise RuntimeError(f"sanitizer build of {src} failed:\n{out}")
    kernels = [os.path.join(B.CSRC, "build", s + ".o") for s in B.SOURCES if s.endswith(".hip")]
    lib = os.path.join(OUT, "libsrgpu_asan.so")
    subprocess.check_call(["hipcc", "-shared", "-o", lib] + [os.path.join(OUT, s + ".o") for s in HOST_UNITS] + kernels +
                          ["--offload-arch=gfx950", "-lpthread"] + SAN)
    drv = os.path.join(OUT, "host_mirror_driver_asan")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_mirror_driver.cpp"), "-o", drv, lib,
                           "-Wl,-rpath," + OUT, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(runtime())] + SAN)
    return lib, drv


def env(lib):
    e = dict(os.environ)
    e["SRGPU_LIB"] = lib
    e["LD_PRELOAD"] = runtime()
    # leaks: CPython never frees everything
    e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1:detect_stack_use_after_return=1"
    e["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    return e


def gpu_present():
    """/dev/kfd is the ROCm kernel driver's node: where it exists, a HIP call in the sanitized process would bring up a GPU under ASan."""
    return os.path.exists("/dev/kfd")


def main(argv):
    if gpu_present():
        print("sanitize_host.py: refusing to run on a host with a GPU (ASan runs on the CPU build only)", file=sys.stderr)
        return 2
    lib, drv = build()
    e = env(lib)
    e["SR_ASAN_DRIVER"] = drv
    # ASan's throwing operator new reports an allocation it cannot serve as an error by itself (it cannot return null to a
    # throwing new), so the one test that asks for 2 TB on purpose is left to the ordinary CPU suite
    skip = ["--deselect", "tests/test_capi_cpu.py::test_exception_barrier_turns_bad_alloc_into_a_status"]
    return subprocess.call([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + skip + TESTS + argv, cwd=ROOT, env=e)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
