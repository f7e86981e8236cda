"""The stable prefix of a streaming result without a GPU: sr_stream_stable, sr_bigram_stream_stable and sr_commit_points are in the
library, the header and the binding with the ABI version unchanged; null handles are refused before any device is touched; the
pairwise fold of tests/commit_reference.py finds what the intersection of the ancestor chains finds; the kernels behind the calls
are in the gfx950 build without scratch; and the stable() members of include/sr_sietill.hpp compile."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import commit_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

STABLE_SYMBOLS = ("sr_stream_stable", "sr_bigram_stream_stable", "sr_commit_points")


def test_library_header_and_binding_carry_the_stable_entry_points():
    from speechrecognition_amd import build, capi

    build.build()
    lib = ctypes.CDLL(build.LIB)
    with open(os.path.join(ROOT, "include", "srgpu.h")) as f:
        hdr = f.read()
    for sym in STABLE_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert re.search(r"SR_API int " + sym + r"\(", hdr), sym
        assert sym in capi.SYMBOLS, sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)  # functions only, no struct changed
    assert capi.SR_ABI_VERSION == 4 and lib.sr_abi_version() == 4
    assert callable(capi.Stream.stable) and callable(capi.BigramStream.stable) and callable(capi.commit_points)


def test_null_handles_are_einval():
    from speechrecognition_amd import build, capi

    build.build()
    L = capi.lib()
    ids = np.zeros(1, np.uint32)
    off = np.full(2, 77, np.uint64)
    commit = np.full(1, 77, np.uint32)
    assert L.sr_stream_stable(None, 1, ids.ctypes.data, None, 0, off.ctypes.data, commit.ctypes.data, None) == -1
    assert L.sr_bigram_stream_stable(None, 1, ids.ctypes.data, None, None, None, 0, off.ctypes.data, commit.ctypes.data) == -1
    par, nodes, fl, out = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.full(1, 77, np.uint32)
    noff = np.array([0, 1], np.uint64)
    assert L.sr_commit_points(None, 1, noff.ctypes.data, par.ctypes.data, noff.ctypes.data, nodes.ctypes.data, fl.ctypes.data, out.ctypes.data) == -1
    assert off[0] == 77 and commit[0] == 77 and out[0] == 77  # nothing written


def test_fold_agrees_with_ancestor_intersection_on_random_forests():
    rng = np.random.default_rng(905)
    moved = 0
    for i in range(200):
        n = int(rng.integers(1, 120))
        parent = commit_reference.random_forest(rng, n, depth_bias=float(rng.choice([0.0, 0.5, 0.9, 0.99])))
        assert parent[0] == 0 and all(parent[j] < j for j in range(1, n))
        nodes = rng.integers(0, n, size=int(rng.integers(1, 40)))
        want = commit_reference.brute_force(parent, nodes)
        got = commit_reference.commit_point(parent, nodes)
        assert got == want, (i, parent, nodes)
        assert commit_reference.commit_point(parent, rng.permutation(nodes)) == want  # the order does not matter
        assert commit_reference.commit_point(parent, nodes, floor=want) == want
        assert all(want in commit_reference.chain(parent, x) for x in nodes)
        moved += want != 0
    assert moved > 20  # not every set meets at the root
    assert commit_reference.commit_point(np.zeros(4, np.uint32), [], floor=2) == 2  # an empty set leaves the commit point


@pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")
def test_commit_kernels_are_built_without_scratch():
    from speechrecognition_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_decode", tmp))
        md.update(isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram", tmp)))
    for kernel in ("stream_commit_kernel<256>", "commit_points_kernel<256>", "bigram_stream_commit_kernel"):
        assert kernel in md, (kernel, sorted(md))
        k = md[kernel]
        assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (kernel, k)


def test_stable_members_of_the_mirror_compile():
    """include/sr_sietill.hpp's StreamingRecognizer::stable and StreamingLinearSearch::stable against srgpu.h (syntax and types)."""
    src = os.path.join(ROOT, "tests", "cpp", "stream_stable_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
