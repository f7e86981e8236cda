"""Word posteriors over the recognition network without a GPU: the numpy restatement (tests/net_fb_reference.py) is pinned to the
oracle's decoder with the min semiring, to path enumeration with the log semiring, and checked for normalised posteriors and the
order of F in the scale; the two entry points exist in the library, the header and the bindings, and the new kernels have no
scratch."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from speechrecognition_amd import synth
from tests import net_fb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sr_word_posteriors_corpus", "sr_recognize_confidence_corpus")
KERNELS = ("netfb_forward_kernel", "netfb_backward_kernel", "netfb_words_kernel", "netfb_top_kernel", "netfb_conf_kernel")
TDP = (3.0, 0.0, 30.0)


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


def _lex(word_lens, sil_idx, start=0):
    """explicit lexicon: word w has word_lens[w] positions of fresh states (silence: one state)"""
    off, aut, s = [0], [], start
    for n in word_lens:
        aut += list(range(s, s + n))
        s += n
        off.append(len(aut))
    return synth.ExplicitLexicon(np.asarray(off, np.uint32), np.asarray(aut, np.uint16), sil_idx)


# (word lengths, silence word): one- and multi-position word 0, silence not at index 0, words of 1 .. 6 positions
LEXICA = [
    ([1, 3, 3, 2], 0),
    ([3, 1, 2, 4], 1),
    ([2, 4, 1, 6, 3], 2),
    ([5, 1, 6, 2, 3, 1, 4], 5),
    ([1, 2], 0),
]


def _net(lex):
    word_off, aut, sil_state = lex.flatten()
    return R.Net(word_off, aut, lex.silence_idx, sil_state)


@pytest.mark.parametrize("li", range(len(LEXICA)))
@pytest.mark.parametrize("tdp", [TDP, (3.0, 0.0, np.inf), (0.7, 1.3, 2.9)])
def test_min_restatement_is_the_oracle_decoder(li, tdp, tmp_path, oracle_lib):
    """With min in place of log-add, the restatement's per-frame best word end is the decoder's tb_score[1..T] at an infinite
    beam, bit for bit."""
    lex = _lex(*LEXICA[li])
    S = lex.n_states
    spec = synth.make_mixset(S, 2, 4, seed=5)
    mp = str(tmp_path / "m.mix")
    synth.write_mixset(mp, spec)
    rng = np.random.default_rng(11 + li)
    net = _net(lex)
    for T, wp in ((1, 10.0), (7, 10.0), (40, 2.5), (90, 0.0)):
        e = rng.uniform(0.0, 8.0, size=(T, S))
        e[:, rng.integers(0, S)] *= 0.1  # one state clearly best: long runs through a word
        o = oracle_lib.Oracle(mp, 4, lex, tdp=tdp, am_threshold=np.inf, word_penalty=wp)
        _, (tbs, _, _) = o.decode(np.zeros((T, 4), np.float32), dense=e, traceback=True)
        o.close()
        ours = R.best_ends(e, net, tdp, wp)
        assert np.array_equal(ours, tbs[1:]), (T, wp, ours, tbs[1:])


@pytest.mark.parametrize("li", [0, 1, 4])
def test_log_restatement_is_path_enumeration(li):
    lex = _lex(*LEXICA[li])
    net = _net(lex)
    rng = np.random.default_rng(20 + li)
    for T in range(1, 6):
        e = rng.uniform(0.0, 4.0, size=(T, lex.n_states))
        for scale in (0.1, 1.0, 3.0):
            F, _ = R.posteriors(e, net, (1.0, 0.5, 2.0), 1.5, scale)
            Fb = R.brute_force(e, net, (1.0, 0.5, 2.0), 1.5, scale)
            assert abs(F - Fb) <= 1e-12 * max(1.0, abs(Fb)), (T, scale, F, Fb)


@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_posteriors_sum_to_one_and_scale_order(li):
    lex = _lex(*LEXICA[li])
    net = _net(lex)
    rng = np.random.default_rng(40 + li)
    e = rng.uniform(0.0, 6.0, size=(60, lex.n_states))
    for scale in (0.05, 1.0):
        _, p = R.posteriors(e, net, TDP, 4.0, scale)
        assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-12
        assert (p >= 0).all()
    F = [R.posteriors(e, net, TDP, 4.0, k)[0] for k in (0.1, 1.0, 10.0)]
    V = R.best_ends(e, net, TDP, 4.0)[-1]
    assert F[0] <= F[1] <= F[2] <= V


def test_entry_points_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for sym in ENTRY_POINTS:
        assert hasattr(L, sym), sym


def test_header_prototypes_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"SR_API\s+int\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)
    from speechrecognition_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.SYMBOLS)
    for attr in ("word_posteriors", "recognize_confidence"):
        assert callable(getattr(capi.Corpus, attr, None)), attr
    hpp = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    assert "sr_recognize_confidence_corpus" in hpp and re.search(r"\brecognize_with_confidence\s*\(", hpp)


def test_confidence_driver_compiles():
    """include/sr_sietill.hpp's sr::Recognizer::recognize_with_confidence against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "confidence_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_have_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_netfb", tmp))
        for k in KERNELS:
            assert k in md, (k, sorted(md))
            assert md[k]["private_segment_fixed_size"] == 0 and md[k].get("vgpr_spill_count", 0) == 0, (k, md[k])
