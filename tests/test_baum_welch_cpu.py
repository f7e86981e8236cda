"""Baum-Welch training pass without a GPU: the numpy forward-backward restatement (tests/fb_reference.py) is pinned to the
oracle's aligner, the two entry points exist in the library, the header and the binding, and the new kernels have no scratch."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import fb_reference as R
from tests.util import Case, golden_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sr_state_posteriors_corpus", "sr_baum_welch_corpus")
FB_KERNELS = ("fb_forward_kernel", "fb_backward_kernel")
ITEM_KERNELS = ("items_kernel<false, unsigned short>", "items_kernel<true, unsigned short>", "items_kernel<false, unsigned int>",
                "items_kernel<true, unsigned int>", "items_by_frame_kernel<false>", "items_by_frame_kernel<true>", "items_advance_kernel",
                "items_top_kernel")
EM_KERNELS = ("em_item_pairs_kernel", "em_assign_weighted_kernel", "em_iota_kernel")


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


@pytest.mark.parametrize("name", [n for n in golden_names() if "align_ref" in np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")).files])
def test_min_restatement_is_the_oracle_aligner(name, tmp_path, oracle_lib):
    """With min in place of log-add the restatement is align_full: same costs and state paths -- its topology and TDP keying
    are the aligner's.  The log-add version then sits inside V - log(#paths) <= F <= V and its posteriors sum to 1."""
    c = Case(name, tmp_path)
    o = c.oracle(oracle_lib)
    e = o.score_matrix(c.feats)
    ref = c.z["align_ref"]
    sil = c.lex.flatten()[2]
    st, cost = R.viterbi(e, ref, c.tdp, sil)
    ost, ocost = o.align_full(c.feats, ref)
    o.close()
    assert np.array_equal(st, ost) and np.array_equal(st, c.z["align_full_states"])
    assert cost == ocost == float(c.z["align_full_cost"])
    F, g = R.posteriors(e, ref, c.tdp, sil)
    T, N = len(c.feats), len(ref)
    assert cost - np.log(float(R.n_paths(T, N))) <= F <= cost
    assert np.abs(g.sum(axis=1) - 1.0).max() < 1e-9


def test_restatement_edge_cases():
    """T = 1 (F = e(0, ref[0])), N > T, a forbidden jump (+inf penalty) and the single-path case."""
    rng = np.random.default_rng(3)
    e = rng.uniform(1.0, 5.0, size=(6, 4))
    F, g = R.posteriors(e[:1], [2], (3.0, 0.0, 30.0), 0)
    assert F == e[0, 2] and g[0, 0] == 1.0
    ref = [1, 2, 3, 1, 2, 3, 1, 2, 3]  # N = 9 = 2 T - 1 with T = 5: the only path skips every frame
    F, g = R.posteriors(e[:5], ref, (3.0, 0.0, 30.0), 0)
    assert R.n_paths(5, 9) == 1 and np.isclose(F, sum(e[t, ref[2 * t]] for t in range(5)) + 4 * 30.0)
    assert np.allclose(g.sum(axis=1), 1.0)
    F, g = R.posteriors(e, [1, 2, 3, 1, 2, 3], (np.inf, 0.0, np.inf), 0)  # N = T, loop and skip forbidden: the diagonal
    assert np.isclose(F, sum(e[t, [1, 2, 3, 1, 2, 3][t]] for t in range(6)))
    assert np.allclose(g, np.eye(6)) and not np.isnan(g).any()


def test_entry_points_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for sym in ENTRY_POINTS:
        assert hasattr(L, sym), sym


def test_header_prototypes_and_binding():
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"SR_API\s+int\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)
    from speechrecognition_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.SYMBOLS)
    for attr in ("state_posteriors", "baum_welch", "baum_welch_on_device"):
        assert callable(getattr(capi.Corpus, attr, None)), attr
    hpp = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    assert "sr_baum_welch_corpus" in hpp and re.search(r"\bbaum_welch\s*\(", hpp)


def test_trainer_mirror_compiles():
    """include/sr_sietill.hpp's sr::Trainer::baum_welch against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "baum_welch_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_have_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        for obj, names in (("viterbi_fb", FB_KERNELS), ("posterior_items", ITEM_KERNELS), ("em_accumulate", EM_KERNELS)):
            md = isa_info.kernel_metadata(isa_info.code_object(obj, tmp))
            for k in names:
                assert k in md, (obj, k, sorted(md))
                assert md[k]["private_segment_fixed_size"] == 0 and md[k].get("vgpr_spill_count", 0) == 0, (k, md[k])
