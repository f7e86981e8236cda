"""Word posteriors over the bigram search network without a GPU: the numpy restatement (tests/bigram_fb_reference.py) is pinned to
path enumeration with the log semiring and to the oracle's bigram decoder with the min semiring, and checked for normalised
posteriors and the order of F in the scale; the two entry points exist in the library, the header and the bindings, and the new
kernels have no scratch."""
import ctypes
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from tests import bigram_fb_reference as R
from tests.test_bigram import FLT_MAX, SIL_TDP, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sr_bigram_word_posteriors_corpus", "sr_recognize_bigram_confidence_corpus")
KERNELS = ("bgfb_table_kernel", "bgfb_forward_kernel", "bgfb_backward_kernel", "bgfb_product_kernel", "bgfb_words_kernel",
           "bgfb_conf_kernel")
TDP = np.array([[3.0, 0.0, 30.0, 5.0], [1.0, 0.5, 4.0, 2.0]], np.float32)

# (word lengths, silence word): a two-state silence so that the copies have an interior; one- to three-state words
TINY = [
    ([2, 1, 3], 0),
    ([1, 2, 2], 0),
    ([2, 3, 1, 2], 1),
    ([1, 1], 0),
    ([3, 2], 1),
]


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


def _tiny(i, T):
    lens, sil = TINY[i]
    rng = np.random.default_rng(100 + i)
    word_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    mixtures = np.arange(word_off[-1], dtype=np.uint16)
    W = len(lens)
    lm = rng.uniform(0.2, 4.0, size=(W, W)).astype(np.float32)
    if W >= 3:
        others = [w for w in range(W) if w != sil]
        lm[others[0], others[1]] = np.inf  # a forbidden transition
        lm[others[1], others[0]] = np.nan  # and a NaN one: forbidden as well
    e = rng.uniform(-1.0, 6.0, size=(T, int(word_off[-1])))
    return R.Net(word_off, mixtures, sil), lm, e


@pytest.mark.parametrize("i", range(len(TINY)))
@pytest.mark.parametrize("T", [1, 2, 4, 6])
@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_log_restatement_is_path_enumeration(i, T, scale):
    if T == 6 and len(TINY[i][0]) > 3:
        T = 5  # (the enumeration grows as (2 W) ^ T)
    net, lm, e = _tiny(i, T)
    F, p = R.posteriors(e, net, lm, TDP, scale)
    Fb, pb = R.brute_force(e, net, lm, TDP, scale)
    assert abs(F - Fb) <= 1e-12 * max(1.0, abs(Fb)), (F, Fb)
    assert np.abs(p - pb).max() <= 1e-12


def test_no_frames():
    net, lm, e = _tiny(0, 0)
    F, p = R.posteriors(e, net, lm, TDP, 0.7)
    assert F == 0.0 and p.shape == (0, net.W)


@pytest.mark.parametrize("i", range(len(TINY)))
def test_posteriors_sum_to_one_and_scale_order(i):
    net, lm, e = _tiny(i, 40)
    Fs = []
    for k in (0.1, 1.0, 10.0, 200.0):
        F, p = R.posteriors(e, net, lm, TDP, k)
        assert np.abs(p.sum(axis=1) - 1.0).max() < 1e-10
        Fs.append(F)
    V, _ = R.best_cost(e, net, lm, TDP)
    assert Fs[0] <= Fs[1] <= Fs[2] <= Fs[3] <= V + 1e-9
    # F >= V - log(number of paths) / kappa, and there are at most (positions + 1) ^ T paths over T = 40 frames
    assert V - Fs[3] <= 40 * np.log(net.P + 1.0) / 200.0 + 1e-9


# test_bigram.py's _setup shapes: (seed, W, states per word, silence states, tdp)
SHAPES = [(1, 5, 3, 1, None), (2, 7, 2, 1, None), (3, 4, 4, 2, None), (4, 6, 1, 1, None),
          (31, 6, 3, 2, SIL_TDP), (32, 6, 3, 3, SIL_TDP), (33, 6, 3, 4, SIL_TDP)]
# the shapes on which the reference finds no frame at which the decoder's merge loses anything (test_min_restatement...: checked there)
QUIRK_FREE = {1, 2, 4}


def merge_loses(net, WE, tdp):
    """Does orc_bigram_decode's merge (mergeSilenceToBigramNodes, sr_oracle.c:769-781) lose a hypothesis the summed network keeps,
    at any frame?  Decided from the reference's own min-semiring word-end lists WE [T + 1, 2W], for a search without beams and a
    finite LM.  The decoder's word-end list is in the order its word hypotheses were activated: the words (ascending, silence last:
    frame 1 enters it from the extra start), then the copies in the order their words first ended.  The merge keeps one hypothesis per
    history at the index of the history's first entry and cuts the list to as many entries as there are histories, so
      (a) a history whose first entry lies at or behind that cut is dropped -- the quirk;
      (b) where both word h and its copy end, only the better survives, and when that is the copy, the next frame does not enter
          the copy from word h's end (the decoder enters a copy only from a surviving end of the word itself), which the summed
          network does.  With a one-state silence whose loop costs no more than its exit that entry is dominated by the copy's own
          loop (entry >= the copy's state + exit >= the copy's state + loop, same emission) and nothing is lost.
    Either makes the decoder's search space smaller than the network's: its best path may then cost more."""
    W, sil = net.W, net.sil
    td = np.asarray(tdp, np.float64).reshape(2, 4)
    dominated = net.slot_off[sil + 1] - net.slot_off[sil] == 1 and td[1, 0] <= td[1, 3]
    active = [w for w in range(W) if w != sil] + [sil]
    for t in range(1, WE.shape[0]):
        ends = [x for x in active if np.isfinite(WE[t, x])]
        first, n_hist = {}, 0
        for i, x in enumerate(ends):
            h = int(net.hist[x])
            if h not in first:
                first[h] = i
                n_hist += 1
        if any(i >= n_hist for i in first.values()):
            return True  # (a)
        for h in range(W):
            if not dominated and h != sil and np.isfinite(WE[t, h]) and np.isfinite(WE[t, h + W]) and WE[t, h + W] <= WE[t, h]:
                return True  # (b)
        for x in ends:  # the next frame activates the copies of the words that ended, in list order
            if x < W and x != sil and x + W not in active:
                active.append(x + W)
    return False


@pytest.mark.parametrize("shape", SHAPES)
def test_min_restatement_against_the_oracle_decoder(shape, tmp_path, oracle_lib):
    """min semiring, both beams off: the network's best cost is never above the decoder's last item score (the decoder's result is
    one path of the network), up to the decoder's float additions: slack = (4 T + 8) 2^-24 max(1, largest |partial score|) -- at most
    four per frame along a path (LM, transition, emission, exit).  Where the merge loses nothing the two are equal within it."""
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    o = oracle_lib.Oracle(mp, 12, lex)
    dense = o.score_matrix(feats)
    o.close()
    w, s, t = oracle_lib.bigram_decode(dense, word_off, mixtures, lex.silence_idx, lm, tdp, float(FLT_MAX), float(FLT_MAX))
    assert len(s) > 0
    s_last = float(s[-1])
    net = R.Net(word_off, mixtures, lex.silence_idx)
    best, WE = R.best_cost(dense, net, lm, tdp)
    T = dense.shape[0]
    partial = max(np.abs(WE[np.isfinite(WE)]).max(), np.abs(np.asarray(s, np.float64)).max())
    slack = (4 * T + 8) * 2.0 ** -24 * max(1.0, partial)
    print(f"seed {seed}: network {best:.6f} decoder {s_last:.6f} slack {slack:.3g} merge loses {merge_loses(net, WE, tdp)}")
    assert best <= s_last + slack
    assert (not merge_loses(net, WE, tdp)) == (seed in QUIRK_FREE)
    if seed in QUIRK_FREE:
        assert abs(best - s_last) <= slack


def test_at_least_two_quirk_free_shapes():
    assert len(QUIRK_FREE) >= 2 and QUIRK_FREE <= {s[0] for s in SHAPES}


def test_entry_points_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for sym in ENTRY_POINTS:
        assert hasattr(L, sym), sym


def test_header_prototypes_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"SR_API\s+int\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)
    assert "WITHOUT the positional cut" in hdr
    from speechrecognition_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.SYMBOLS)
    for attr in ("bigram_word_posteriors", "recognize_bigram_confidence"):
        assert callable(getattr(capi.Corpus, attr, None)), attr
    hpp = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    assert "sr_recognize_bigram_confidence_corpus" in hpp


def test_confidence_driver_compiles():
    """include/sr_sietill.hpp's sr::LinearSearch::recognize_with_confidence against srgpu.h (syntax and types; the GPU test runs it)."""
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "bigram_confidence_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_have_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram_fb", tmp))
        for k in KERNELS:
            assert k in md, (k, sorted(md))
            assert md[k]["private_segment_fixed_size"] == 0 and md[k].get("vgpr_spill_count", 0) == 0, (k, md[k])
