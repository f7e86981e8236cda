"""Word lattices over the bigram search network without a GPU: the tracked restatement (tests/bigram_lattice_reference.py) is pinned
to tests/bigram_fb_reference.py bit for bit and to path enumeration, its tie rules on costs from a grid; sr_bigram_lattice_nbest (host
code of the built library) against exhaustive enumeration and against the oracle's bigram decoder; the entry points exist in the
library, the header and the bindings, and the new kernels have no scratch."""
import ctypes
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import bigram_fb_reference as R
from tests import bigram_lattice_reference as BL
from tests.test_bigram import FLT_MAX, _setup
from tests.test_bigram_posteriors_cpu import QUIRK_FREE, SHAPES, TDP, TINY, _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sr_bigram_word_lattice_corpus", "sr_bigram_lattice_nbest")
KERNELS = ("bglat_transpose_kernel", "bglat_init_kernel", "bglat_entry_kernel<0>", "bglat_entry_kernel<1>", "bglat_entry_kernel<2>",
           "bglat_forward_kernel", "bglat_backward_kernel", "bglat_count_kernel", "bglat_write_kernel", "bglat_advance_kernel")
EINVAL = -1
INF = np.inf


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


@pytest.fixture(scope="module")
def capi(built_lib):
    from speechrecognition_amd import capi
    return capi


def _T(i, T):
    return 5 if T >= 6 and len(TINY[i][0]) > 3 else T  # (the enumeration grows as (2 W) ^ T)


@pytest.mark.parametrize("i", range(len(TINY)))
@pytest.mark.parametrize("T", [0, 1, 2, 4, 7, 40])
def test_tracked_forward_is_the_restatement(i, T):
    net, lm, e = _tiny(i, T)
    WE = BL.tracked_forward(e, net, lm, TDP)[0]
    assert WE.tobytes() == R.forward(e, net, lm, TDP, "min", 1.0)[1].tobytes()
    best, A = BL.arcs(e, net, lm, TDP)
    assert best == (R.best_cost(e, net, lm, TDP)[0] if T else 0.0)
    if T:  # bwd of the reference's own backward: alpha + beta at the word ends
        B = R.backward(e, net, lm, TDP, semiring="min")
        td = R._tdp(TDP, 1.0)
        for x, t, bw in zip(A["slot"], A["last"], A["bwd"]):
            want = B[t, net.last[x]] if t + 1 < T else td[net.slot_sil[x], 3]
            if t + 1 < T and np.isfinite(want):  # beta at the last state = min(in-word moves, exit + bwd) <= exit + bwd
                assert want <= td[net.slot_sil[x], 3] + bw
            assert bw >= 0.0 or np.isfinite(bw)


@pytest.mark.parametrize("i", range(len(TINY)))
@pytest.mark.parametrize("T", [1, 2, 4, 6])
def test_lattice_against_path_enumeration(i, T):
    T = _T(i, T)
    net, lm, e = _tiny(i, T)
    best, A = BL.arcs(e, net, lm, TDP)
    klm = R._klm(net, lm, 1.0)
    paths = BL.network_paths(e, net, lm, TDP)
    assert abs(min(c for c, _ in paths) - best) <= 1e-9
    # every arc: fwd + bwd = the cheapest network path through that word end; every word end on a path is an arc
    through = {}
    for c, ends in paths:
        for k in ends:
            through[k] = min(through.get(k, INF), c)
    have = {(int(x), int(t)): float(f + b) for x, t, f, b in zip(A["slot"], A["last"], A["fwd"], A["bwd"])}
    assert set(have) == set(through)
    for k, v in through.items():
        assert abs(have[k] - v) <= 1e-9, (k, have[k], v)
    # the cheapest lattice path is best; no lattice string is cheaper than the string's cheapest network path
    lp = BL.lattice_paths(A, T, net.sil, klm)
    assert abs(min(g for g, _ in lp) - best) <= 1e-9
    true = {}
    for c, ends in paths:
        s = tuple(int(net.word[net.first[x]]) for x, _ in ends if net.word[net.first[x]] != net.sil)
        true[s] = min(true.get(s, INF), c)
    for s, g in BL.strings_of(A, lp, net.sil).items():
        assert s in true and g >= true[s] - 1e-9, (s, g, true.get(s))
    # a beam keeps the arcs within it, in order
    bb, Ab = BL.arcs(e, net, lm, TDP, 3.0)
    keep = A["fwd"] + A["bwd"] <= best + 3.0
    assert bb == best and all(np.array_equal(Ab[k], A[k][keep]) for k in A)
    order = A["last"].astype(np.int64) * 2 * net.W + A["slot"]
    assert (np.diff(order) > 0).all()


def _grid_case(seed, lens, sil, T):
    rng = np.random.default_rng(seed)
    word_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    W = len(lens)
    net = R.Net(word_off, np.arange(word_off[-1], dtype=np.uint16), sil)
    lm = (rng.integers(0, 4, size=(W, W)) / 8.0).astype(np.float32)
    e = rng.integers(0, 3, size=(T, int(word_off[-1]))) / 8.0
    tdp = (rng.integers(0, 3, size=(2, 4)) / 8.0).astype(np.float32)
    return net, lm, e, tdp


def test_tie_rules_pinned():
    """costs on a grid of 1/8: every sum is exact, equal candidates abound"""
    # all costs 0, one-state words; word 2 cannot follow the silence history
    net = R.Net(np.array([0, 1, 2, 3]), np.arange(3), 0)
    lm = np.zeros((3, 3), np.float32)
    lm[2, 0] = np.inf
    best, A = BL.arcs(np.zeros((2, 3)), net, lm, np.zeros((2, 4), np.float32))
    arc = {(int(x), int(t)): (int(f), int(p)) for x, t, f, p in zip(A["slot"], A["last"], A["first"], A["pred"])}
    assert best == 0.0
    assert arc[(1, 1)] == (0, 0)  # the in-word move (entered at frame 0 from silence) before the equal entry at frame 1
    assert arc[(2, 1)] == (1, 1)  # entered at frame 1: histories 1 and 2 cost the same... only 1 has ended; silence is forbidden
    assert (2, 0) not in arc
    assert arc[(0, 1)] == (0, 0) and arc[(4, 1)] == (1, 1)  # the silence word loops; the copy after word 1 from word 1's end
    lm[2, 0] = 0.0
    best, A = BL.arcs(np.zeros((3, 3)), net, lm, np.zeros((2, 4), np.float32))
    arc = {(int(x), int(t)): (int(f), int(p)) for x, t, f, p in zip(A["slot"], A["last"], A["first"], A["pred"])}
    assert arc[(2, 2)] == (0, 0) and arc[(2, 0)] == (0, 0)
    lm[2, 0] = 0.125  # now word 2 is cheaper entered at frame 1: from histories 1 and 2?  2 has not ended at 0 cost; the smallest h
    best, A = BL.arcs(np.zeros((3, 3)), net, lm, np.zeros((2, 4), np.float32))
    arc = {(int(x), int(t)): (int(f), int(p)) for x, t, f, p in zip(A["slot"], A["last"], A["first"], A["pred"])}
    assert arc[(2, 1)] == (1, 1) and arc[(2, 2)] == (1, 1)  # in-word from (2, 1) before the equal entries at frame 2 (h = 1, 2)
    # random grids: exact sums, so the lattice reproduces best EXACTLY and fwd + bwd the enumeration's minima EXACTLY
    for seed, (lens, sil) in enumerate(TINY):
        T = 5 if len(lens) < 4 else 4
        net, lm, e, tdp = _grid_case(700 + seed, lens, sil, T)
        best, A = BL.arcs(e, net, lm, tdp)
        klm = R._klm(net, lm, 1.0)
        paths = BL.network_paths(e, net, lm, tdp)
        assert min(c for c, _ in paths) == best
        lp = BL.lattice_paths(A, T, net.sil, klm)
        assert min(g for g, _ in lp) == best
        through = {}
        for c, ends in paths:
            for k in ends:
                through[k] = min(through.get(k, INF), c)
        for x, t, f, b in zip(A["slot"], A["last"], A["fwd"], A["bwd"]):
            assert f + b == through[(int(x), int(t))]
        # first / pred of every arc describe a real cheapest entry: pred is the SMALLEST history attaining the entry's minimum
        WE, ST, PR, _ = BL.tracked_forward(e, net, lm, tdp)
        for x, t, f, p in zip(A["slot"], A["last"], A["first"], A["pred"]):
            if x < net.W and x != net.sil:
                terms = R.histories(net, WE[f], "min") + klm[x]
                assert int(np.argmin(terms)) == p and terms[p] == terms.min()


def _check_nbest(capi, A, T, W, sil, lm, n_best, lm_scale=1.0):
    klm = R._klm(R.Net(np.arange(W + 1), np.arange(W), sil), lm, 1.0)
    want = BL.nbest(A, T, sil, klm, n_best, lm_scale)
    got = capi.bigram_lattice_nbest(T, A["word"], A["hist"], A["first"], A["last"], A["am"], sil, lm, n_best, lm_scale)
    again = capi.bigram_lattice_nbest(T, A["word"], A["hist"], A["first"], A["last"], A["am"], sil, lm, n_best, lm_scale)
    assert [(tuple(w.tolist()), c) for w, c in got] == [(tuple(w.tolist()), c) for w, c in again]  # the same order on every call
    assert len(got) == len(want), (got, want)
    allc = BL.strings_of(A, BL.lattice_paths(A, T, sil, klm, lm_scale), sil)
    for (gw, gc), (ww, wc) in zip(got, want):
        assert abs(gc - wc) <= 1e-9, (got, want)
        assert abs(allc[tuple(gw.tolist())] - gc) <= 1e-9  # the string's own cheapest path
    assert len({tuple(w.tolist()) for w, _ in got}) == len(got)
    return got


def _random_lattice(seed, W, sil, T):
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("word", "hist", "first", "last", "am")}
    for t in range(T):
        for x in range(2 * W):
            if x == sil + W or rng.random() < 0.35:
                continue
            out["word"].append(x if x < W else sil)
            out["hist"].append(x if x < W else x - W)
            out["first"].append(int(rng.integers(0, t + 1)))
            out["last"].append(t)
            out["am"].append(float(rng.uniform(-1.0, 5.0)))
    return {k: np.asarray(v, np.float64 if k == "am" else np.uint32) for k, v in out.items()}


@pytest.mark.parametrize("seed", range(8))
def test_nbest_against_enumeration_random_lattices(seed, capi):
    W, sil, T = 3 + seed % 2, seed % 3, 5
    A = _random_lattice(800 + seed, W, sil, T)
    rng = np.random.default_rng(900 + seed)
    lm = rng.uniform(-0.5, 3.0, size=(W, W)).astype(np.float32)
    lm[(sil + 1) % W, (sil + 2) % W] = np.inf
    lm[(sil + 2) % W, (sil + 1) % W] = np.nan
    for n_best in (1, 3, 1000):
        _check_nbest(capi, A, T, W, sil, lm, n_best)
    _check_nbest(capi, A, T, W, sil, lm, 5, lm_scale=0.0)
    _check_nbest(capi, A, T, W, sil, lm, 5, lm_scale=2.5)


@pytest.mark.parametrize("i", range(len(TINY)))
def test_nbest_on_network_lattices_and_rescoring(i, capi):
    T = 5 if len(TINY[i][0]) > 3 else 6
    net, lm, e = _tiny(i, T)
    best, A = BL.arcs(e, net, lm, TDP)
    got = _check_nbest(capi, A, T, net.W, net.sil, lm, 4)
    assert abs(got[0][1] - best) <= 1e-9
    full = _check_nbest(capi, A, T, net.W, net.sil, lm, 10 ** 6)
    # the k-th entry is an upper bound of the network's k-th best string
    paths = BL.network_paths(e, net, lm, TDP)
    true = {}
    for c, ends in paths:
        s = tuple(int(net.word[net.first[x]]) for x, _ in ends if net.word[net.first[x]] != net.sil)
        true[s] = min(true.get(s, INF), c)
    for k, c in enumerate(sorted(true.values())[:len(full)]):
        assert full[k][1] >= c - 1e-9
    # rescoring with a second table
    lm2 = np.random.default_rng(950 + i).uniform(0.1, 5.0, size=lm.shape).astype(np.float32)
    _check_nbest(capi, A, T, net.W, net.sil, lm2, 4)
    _check_nbest(capi, A, T, net.W, net.sil, lm2, 4, lm_scale=0.5)
    # a beam-0 lattice holds the best path (up to a rounding of fwd + bwd against best)
    _, A0 = BL.arcs(e, net, lm, TDP, 1e-9)
    assert abs(_check_nbest(capi, A0, T, net.W, net.sil, lm, 2)[0][1] - best) <= 1e-9


def test_nbest_errors(capi):
    net, lm, e = _tiny(0, 4)
    best, A = BL.arcs(e, net, lm, TDP)
    W, sil, T = net.W, net.sil, 4
    fn = capi.lib().sr_bigram_lattice_nbest
    P = capi._ptr
    n = len(A["word"])
    lm = np.ascontiguousarray(lm, np.float32)

    def call(T=T, n_arcs=n, word=A["word"], hist=A["hist"], first=A["first"], last=A["last"], am=A["am"], W=W, sil=sil, lm=lm, scale=1.0,
             n_best=3, cap=100, null_out=False):
        arrs = [np.ascontiguousarray(a) for a in (word, hist, first, last, am)]
        out, off, cost, cnt = np.zeros(max(cap, 1), np.uint32), np.zeros(n_best + 2, np.uint64), np.zeros(n_best + 1), C.c_uint32(7)
        rc = fn(T, n_arcs, *[P(a) for a in arrs], W, sil, P(lm) if lm is not None else None, scale, n_best, P(out), cap, P(off),
                None if null_out else P(cost), C.byref(cnt))
        return rc, cnt.value

    assert call() == (0, 3)
    assert call(T=0, n_arcs=0) == (0, 0)
    assert call(n_best=0)[0] == EINVAL
    assert call(lm=None)[0] == EINVAL
    assert call(null_out=True)[0] == EINVAL
    for s in (np.nan, -1.0, -np.inf):
        assert call(scale=s)[0] == EINVAL, s
    assert call(cap=0) == (EINVAL, 0)  # words_cap too small
    for field, idx, val in (("hist", 0, W), ("word", 0, W), ("last", n - 1, T), ("first", n - 1, T), ("am", 1, np.nan), ("am", 1, -np.inf)):
        a = {k: v.copy() for k, v in A.items()}
        a[field][idx] = val
        assert call(word=a["word"], hist=a["hist"], first=a["first"], last=a["last"], am=a["am"])[0] == EINVAL, field
    rev = {k: v[::-1].copy() for k, v in A.items()}  # not in (last, slot) order
    assert call(word=rev["word"], hist=rev["hist"], first=rev["first"], last=rev["last"], am=rev["am"])[0] == EINVAL
    bad = A["hist"].copy()
    k = int(np.flatnonzero(A["word"] != sil)[0])
    bad[k] = (bad[k] + 1) % W  # a word whose history is not itself
    assert call(hist=bad)[0] == EINVAL
    assert call(sil=W)[0] == EINVAL


def test_nbest_standalone_driver_under_the_sanitizers(tmp_path):
    """tests/cpp/nbest_host_driver.cpp and nbest.cpp alone, built with -fsanitize=address,undefined and run as a plain program, every
    output array exactly as long as the call may fill it: test_nbest_against_enumeration_random_lattices' lattices and tables (T = 5, W 3 .. 4,
    one +inf and one NaN entry) at n_best 1, 3, 1000 and lm_scale 0, 1, 2.5, and every malformed input of test_nbest_errors.  Strings,
    counts and costs (1e-9) are the enumeration's; no report."""
    from tests.test_word_lattice_cpu import nbest_driver_case, run_nbest_driver
    cases, want = [], []
    for seed in range(8):
        W, sil, T = 3 + seed % 2, seed % 3, 5
        A = _random_lattice(800 + seed, W, sil, T)
        rng = np.random.default_rng(900 + seed)
        lm = rng.uniform(-0.5, 3.0, size=(W, W)).astype(np.float32)
        lm[(sil + 1) % W, (sil + 2) % W] = np.inf
        lm[(sil + 2) % W, (sil + 1) % W] = np.nan
        klm = R._klm(R.Net(np.arange(W + 1), np.arange(W), sil), lm, 1.0)
        for n_best, scale in ((1, 1.0), (3, 1.0), (1000, 1.0), (5, 0.0), (5, 2.5)):
            allc = BL.strings_of(A, BL.lattice_paths(A, T, sil, klm, scale), sil)
            ref = BL.nbest(A, T, sil, klm, n_best, scale)
            # all the words of all strings: enough for any n_best, and exactly the need where every string is given out
            cases.append(nbest_driver_case(T, A, sil, n_best, sum(len(s) for s in allc), W=W, lm=lm, lm_scale=scale))
            want.append((ref, allc))
    # the malformed inputs of test_nbest_errors
    net, lm, e = _tiny(0, 4)
    _, A = BL.arcs(e, net, lm, TDP)
    A = {k: A[k] for k in ("word", "hist", "first", "last", "am")}
    W, sil, T, n = net.W, net.sil, 4, len(A["word"])

    def case(T=T, a=A, W=W, sil=sil, scale=1.0, n_best=3, cap=100, **kw):
        return nbest_driver_case(T, a, sil, n_best, cap, W=W, lm=lm, lm_scale=scale, **kw)

    def with_(field, idx, val):
        a = {k: np.array(v) for k, v in A.items()}
        a[field][idx] = val
        return a

    bad_hist = int(np.flatnonzero(A["word"] != sil)[0])
    errs = [(case(), 0, 3), (case(T=0, a={k: v[:0] for k, v in A.items()}), 0, 0), (case(n_best=0), EINVAL, None),
            (case(null_lm=True), EINVAL, None), (case(null_cost=True), EINVAL, None)]
    errs += [(case(scale=s), EINVAL, None) for s in (np.nan, -1.0, -np.inf)]
    errs += [(case(cap=0), EINVAL, 0)]
    errs += [(case(a=with_(f, i, v)), EINVAL, None) for f, i, v in (("hist", 0, W), ("word", 0, W), ("last", n - 1, T), ("first", n - 1, T),
                                                                     ("am", 1, np.nan), ("am", 1, -np.inf))]
    errs += [(case(a={k: v[::-1] for k, v in A.items()}), EINVAL, None),   # not in (last, slot) order
             (case(a=with_("hist", bad_hist, (A["hist"][bad_hist] + 1) % W)), EINVAL, None),   # a word whose history is not itself
             (case(sil=W), EINVAL, None)]
    got = run_nbest_driver(tmp_path, cases + [c for c, _, _ in errs])
    for (ref, allc), (rc, count, err, strings) in zip(want, got):
        assert rc == 0 and count == len(strings) == len(ref), (rc, count, err, ref)
        for (gw, gc), (_, wc) in zip(strings, ref):
            assert abs(gc - wc) <= 1e-9 and abs(allc[gw] - gc) <= 1e-9, (strings, ref)   # the k-th cost; the string's own cheapest path
        assert len({w for w, _ in strings}) == count
    for (_, want_rc, want_count), (rc, count, err, strings) in zip(errs, got[len(want):]):
        assert rc == want_rc and (want_count is None or count == want_count) and bool(err) == bool(rc), (rc, count, err)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] in QUIRK_FREE])
def test_first_entry_is_the_oracle_decoders_result(shape, tmp_path, oracle_lib, capi):
    """beams off, the shapes on which the decoder's merge loses nothing: entry 1 spells the decoder's words with silence removed; its
    cost is within test_bigram_posteriors_cpu.py's float slack of the decoder's last score"""
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    o = oracle_lib.Oracle(mp, 12, lex)
    dense = o.score_matrix(feats)
    o.close()
    w, s, t = oracle_lib.bigram_decode(dense, word_off, mixtures, lex.silence_idx, lm, tdp, float(FLT_MAX), float(FLT_MAX))
    net = R.Net(word_off, mixtures, lex.silence_idx)
    best, A = BL.arcs(dense, net, lm, tdp)
    T = dense.shape[0]
    got = capi.bigram_lattice_nbest(T, A["word"], A["hist"], A["first"], A["last"], A["am"], net.sil, lm, 3)
    w = np.asarray(w)
    assert np.array_equal(got[0][0], w[w != net.sil]), (got[0][0], w)
    partial = max(np.abs(A["fwd"]).max(), np.abs(np.asarray(s, np.float64)).max())
    slack = (4 * T + 8) * 2.0 ** -24 * max(1.0, partial)
    assert abs(got[0][1] - float(s[-1])) <= slack and abs(got[0][1] - best) <= 1e-9 * max(1.0, abs(best))
    assert len(got) == 3 and got[0][1] <= got[1][1] <= got[2][1]


def test_entry_points_are_exported(built_lib):
    L = ctypes.CDLL(built_lib)
    for sym in ENTRY_POINTS:
        assert hasattr(L, sym), sym


def test_header_prototypes_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"SR_API\s+int\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)
    assert "among equal entry terms the smallest h" in hdr and "44 W + 16 bytes per frame" in hdr
    from speechrecognition_amd import capi
    assert set(ENTRY_POINTS) <= set(capi.SYMBOLS)
    assert callable(getattr(capi.Corpus, "bigram_word_lattice", None)) and callable(getattr(capi, "bigram_lattice_nbest", None))
    hpp = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    assert "sr_bigram_word_lattice_corpus" in hpp and "sr_bigram_lattice_nbest" in hpp


def test_nbest_driver_compiles():
    """include/sr_sietill.hpp's sr::LinearSearch::recognize_nbest against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "bigram_nbest_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_have_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_bigram_lattice", tmp))
        for k in KERNELS:
            assert k in md, (k, sorted(md))
            assert md[k]["private_segment_fixed_size"] == 0 and md[k].get("vgpr_spill_count", 0) == 0, (k, md[k])
