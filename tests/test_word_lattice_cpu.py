"""Word lattices and N-best lists without a GPU: the numpy restatement (tests/lattice_reference.py) is pinned to the oracle's
decoder (costs, best word and word start per frame, bit for bit) and to full path enumeration on tiny networks; sr_lattice_nbest
(host code of the built library) is held against exhaustive enumeration of lattice paths; the two entry points exist in the
library, the header and the bindings, the C++ driver compiles, and the new kernels have no scratch."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import lattice_reference as LR
from tests import net_fb_reference as R
from tests.test_word_posteriors_cpu import LEXICA, TDP, _lex, _net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sr_word_lattice_corpus", "sr_lattice_nbest")
KERNELS = ("lattice_forward_kernel", "lattice_backward_kernel", "lattice_count_kernel", "lattice_write_kernel")
EINVAL = -1


@pytest.fixture(scope="module")
def built_lib():
    from speechrecognition_amd import build
    return build.build()


@pytest.mark.parametrize("li", range(len(LEXICA)))
@pytest.mark.parametrize("tdp", [TDP, (3.0, 0.0, np.inf), (0.7, 1.3, 2.9)])
def test_restatement_is_the_oracle_decoder(li, tdp, tmp_path, oracle_lib):
    """E equals net_fb_reference.best_ends (and A its min-semiring forward) bit for bit; the best word end of every frame and
    the frame its word started at are the decoder's tb_word / tb_bkp at an infinite beam (lexica and seeds of
    test_min_restatement_is_the_oracle_decoder)"""
    lex = _lex(*LEXICA[li])
    S = lex.n_states
    spec = synth.make_mixset(S, 2, 4, seed=5)
    mp = str(tmp_path / "m.mix")
    synth.write_mixset(mp, spec)
    rng = np.random.default_rng(11 + li)
    net = _net(lex)
    for T, wp in ((1, 10.0), (7, 10.0), (40, 2.5), (90, 0.0)):
        e = rng.uniform(0.0, 8.0, size=(T, S))
        e[:, rng.integers(0, S)] *= 0.1
        o = oracle_lib.Oracle(mp, 4, lex, tdp=tdp, am_threshold=np.inf, word_penalty=wp)
        _, (tbs, tbw, tbb) = o.decode(np.zeros((T, 4), np.float32), dense=e, traceback=True)
        o.close()
        A, b, E, arg = LR.forward_min_with_starts(e, net, tdp, wp)
        A0, E0 = R.forward(e, net, tdp, wp, "min")
        assert np.array_equal(E, R.best_ends(e, net, tdp, wp)) and np.array_equal(E, E0) and np.array_equal(A, A0)
        assert np.array_equal(E, tbs[1:])
        ok = np.isfinite(E)  # (a frame no word end can reach yet has no best word end)
        assert np.array_equal(ok, arg >= 0) and (ok[-1] or T == 1)
        assert np.array_equal(net.word[arg[ok]], tbw[1:][ok]), (T, wp)
        assert np.array_equal(b[np.arange(T)[ok], arg[ok]], tbb[1:][ok]), (T, wp)


def test_ties_follow_the_decoder(tmp_path, oracle_lib):
    """costs on a coarse grid, so that equal candidates are common: the word and the start of the best word end still are the
    decoder's (the order in which it meets the candidates decides)"""
    for li in range(len(LEXICA)):
        lex = _lex(*LEXICA[li])
        S = lex.n_states
        mp = str(tmp_path / f"t{li}.mix")
        synth.write_mixset(mp, synth.make_mixset(S, 2, 4, seed=5))
        net = _net(lex)
        rng = np.random.default_rng(70 + li)
        for tdp, wp in (((1.0, 0.0, 2.0), 1.0), ((0.0, 0.0, 0.0), 0.0), ((1.0, 1.0, 1.0), 2.0)):
            e = rng.integers(0, 3, size=(30, S)).astype(np.float64)
            o = oracle_lib.Oracle(mp, 4, lex, tdp=tdp, am_threshold=np.inf, word_penalty=wp)
            _, (tbs, tbw, tbb) = o.decode(np.zeros((30, 4), np.float32), dense=e, traceback=True)
            o.close()
            _, b, E, arg = LR.forward_min_with_starts(e, net, tdp, wp)
            assert np.array_equal(E, tbs[1:])
            ok = np.isfinite(E)
            assert ok[-1] and np.array_equal(ok, arg >= 0)
            assert np.array_equal(net.word[arg[ok]], tbw[1:][ok]), (li, tdp)
            assert np.array_equal(b[np.arange(30)[ok], arg[ok]], tbb[1:][ok]), (li, tdp)


def _string_costs(paths, silence):
    best = {}
    for c, segs in paths:
        ws = tuple(w for w, _, _ in segs if w != silence)
        if ws not in best or c < best[ws]:
            best[ws] = c
    return sorted(best.values())


@pytest.mark.parametrize("li", [0, 1, 4])
def test_lattice_against_path_enumeration(li):
    """tiny nets: fwd + bwd is the cheapest enumerated path through each (word, end frame) (rtol 4 T 2^-53: enumeration adds in
    another order), first starts that word on some cheapest such path, the cheapest lattice path is E_{T-1} to rounding, every (word, end
    frame) some path uses has its arc, and the true k-th best distinct string never costs more than the lattice's k-th"""
    lex = _lex(*LEXICA[li])
    net = _net(lex)
    sil = lex.silence_idx
    rng = np.random.default_rng(90 + li)
    tdp, wp = (1.0, 0.5, 2.0), 1.5
    for T in range(1, 6):
        e = rng.uniform(0.0, 4.0, size=(T, lex.n_states))
        rtol = 4 * T * 2.0 ** -53
        paths = LR.network_paths(e, net, tdp, wp)
        assert paths
        through, starts = {}, {}
        for c, segs in paths:
            for w, f, l in segs:
                if c < through.get((w, l), np.inf):
                    through[(w, l)] = c
        for c, segs in paths:
            for w, f, l in segs:
                if c <= through[(w, l)] * (1 + rtol):
                    starts.setdefault((w, l), set()).add(f)
        arcs, best = LR.lattice(e, net, tdp, wp, np.inf)
        assert set(zip(arcs["word"].tolist(), arcs["last"].tolist())) == set(through)
        for i in range(len(arcs["word"])):
            key = (int(arcs["word"][i]), int(arcs["last"][i]))
            tot = arcs["fwd"][i] + arcs["bwd"][i]
            assert abs(tot - through[key]) <= rtol * abs(through[key]), (T, key, tot, through[key])
            assert int(arcs["first"][i]) in starts[key], (T, key, arcs["first"][i], starts[key])
        lat_paths = LR.lattice_paths(arcs, T)
        # (an arc's cost = fwd - E is rounded, and so is the sum over a path: the cheapest lattice path is E_{T-1} to rounding)
        assert abs(min(c for c, _ in lat_paths) - best) <= rtol * abs(best)
        assert abs(best - min(c for c, _ in paths)) <= rtol * abs(best)
        true = _string_costs(paths, sil)
        lat = [c for _, c in LR.nbest(arcs, T, sil, len(true))]
        assert 1 <= len(lat) <= len(true)
        for k, c in enumerate(lat):
            assert true[k] <= c * (1 + rtol), (T, k, true[k], c)
        assert abs(lat[0] - true[0]) <= rtol * abs(true[0])
        # a beam keeps exactly the arcs within it
        for beam in (0.0, 1.0):
            kept, _ = LR.lattice(e, net, tdp, wp, beam)
            want = [i for i in range(len(arcs["word"])) if arcs["fwd"][i] + arcs["bwd"][i] <= best + beam]
            assert np.array_equal(kept["word"], arcs["word"][want]) and np.array_equal(kept["last"], arcs["last"][want])
            # (at beam 0 an arc of the best path itself may miss the beam by a rounding of fwd + bwd)
            assert beam == 0.0 or any(abs(c - best) <= rtol * abs(best) for c, _ in LR.lattice_paths(kept, T))


def _random_lattice(rng, T, W, p, grid=True):
    arcs = {k: [] for k in LR.ARC_KEYS}
    for last in range(T):
        for w in range(W):
            if rng.random() < p:
                arcs["word"].append(w)
                arcs["first"].append(int(rng.integers(0, last + 1)))
                arcs["last"].append(last)
                arcs["cost"].append(float(rng.integers(0, 80)) / 8 if grid else float(rng.uniform(0, 10)))
    out = {k: np.asarray(arcs[k], dtype=np.float64 if k == "cost" else np.int64) for k in ("word", "first", "last", "cost")}
    return out


def _c_nbest(arcs, T, sil, n, **kw):
    return capi.lattice_nbest(T, arcs["word"], arcs["first"], arcs["last"], arcs["cost"], sil, n, **kw)


def test_nbest_against_exhaustive_enumeration(built_lib):
    """random small lattices with costs on a grid of 1/8 (sums are exact, so the costs must agree to the bit): dangling arcs,
    lattices without any complete path, T = 1, n_best beyond the number of strings"""
    rng = np.random.default_rng(123)
    n_nonempty = n_dangling = 0
    for case in range(300):
        T = 1 if case % 10 == 0 else int(rng.integers(2, 8))
        W = int(rng.integers(2, 5))
        sil = int(rng.integers(0, W))
        arcs = _random_lattice(rng, T, W, rng.uniform(0.3, 0.9))
        ref_all = LR.nbest(arcs, T, sil, 10 ** 9)
        used = {i for _, path in LR.lattice_paths(arcs, T) for i in path}
        n_dangling += len(used) < len(arcs["word"])
        n_nonempty += bool(ref_all)
        for n in (1, 3, len(ref_all) + 5):
            got = _c_nbest(arcs, T, sil, n)
            assert got == [] or all(isinstance(c, float) for _, c in got)
            assert len(got) == min(n, len(ref_all)), (case, n, got, ref_all)
            assert [c for _, c in got] == [c for _, c in ref_all[:len(got)]], (case, n)
            table = dict(ref_all)
            seen = set()
            for ws, c in got:
                key = tuple(int(x) for x in ws)
                assert key not in seen and table[key] == c and sil not in key
                seen.add(key)
            again = _c_nbest(arcs, T, sil, n)
            assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, again)) and len(got) == len(again)
    assert n_nonempty > 100 and n_dangling > 100


def test_nbest_float_costs(built_lib):
    """costs off the grid: the same strings' costs to rounding (the order of two strings closer than that may differ)"""
    rng = np.random.default_rng(321)
    for case in range(100):
        T, W = int(rng.integers(2, 7)), 3
        arcs = _random_lattice(rng, T, W, 0.8, grid=False)
        ref = LR.nbest(arcs, T, 0, 4)
        got = _c_nbest(arcs, T, 0, 4)
        assert len(got) == len(ref)
        for (ws, c), (rw, rc) in zip(got, ref):
            assert abs(c - rc) <= 1e-12 * max(1.0, abs(rc))


def test_nbest_of_a_network_lattice(built_lib):
    """the lattice of the restatement: entry 1 costs E_{T-1} (to the rounding of the arcs' cost = fwd - E and of their sum) and
    spells the best path's words"""
    lex = _lex(*LEXICA[2])
    net = _net(lex)
    rng = np.random.default_rng(7)
    e = rng.uniform(0.0, 8.0, size=(25, lex.n_states))
    arcs, best = LR.lattice(e, net, TDP, 4.0, 30.0)
    got = _c_nbest(arcs, 25, lex.silence_idx, 5)
    assert len(got) == 5 and abs(got[0][1] - best) <= 2 * 26 * 2.0 ** -53 * np.abs(arcs["fwd"]).max()
    assert [c for _, c in got] == sorted(c for _, c in got)
    _, b, E, arg = LR.forward_min_with_starts(e, net, TDP, 4.0)
    words, t = [], 25
    while t > 0:
        s = arg[t - 1]
        if net.word[s] != lex.silence_idx:
            words.append(int(net.word[s]))
        t = int(b[t - 1, s])
    assert got[0][0].tolist() == words[::-1]


def test_nbest_errors(built_lib):
    L = capi.lib()
    P = capi._ptr
    word, first, last = np.array([0, 1, 1], np.uint32), np.array([0, 0, 1], np.uint32), np.array([0, 1, 1], np.uint32)
    cost = np.array([1.0, 2.5, 1.0])
    out, off, oc, n = np.zeros(16, np.uint32), np.zeros(5, np.uint64), np.zeros(4), C.c_uint32(9)

    def call(T=2, na=3, w=word, f=first, l=last, c=cost, nb=4, cap=16):
        return L.sr_lattice_nbest(T, na, P(w), P(f), P(l), P(c), 7, nb, P(out), cap, P(off), P(oc), C.byref(n))

    assert call() == 0 and n.value == 2 and oc[:2].tolist() == [2.0, 2.5]
    assert out[:int(off[2])].tolist() == [0, 1, 1] and off[:3].tolist() == [0, 2, 3]
    assert call(nb=0) == EINVAL
    assert call(l=np.array([0, 1, 2], np.uint32)) == EINVAL  # last >= n_frames
    assert call(f=np.array([0, 2, 1], np.uint32)) == EINVAL  # first > last
    assert call(w=np.array([0, 1, 0], np.uint32)) == EINVAL  # (last, word) order: word falls within a frame
    assert call(l=np.array([1, 0, 1], np.uint32), f=np.array([0, 0, 0], np.uint32)) == EINVAL  # last falls
    assert call(c=np.array([1.0, np.nan, 1.0])) == EINVAL
    assert call(cap=2) == EINVAL and n.value == 0  # the second string does not fit
    assert call(cap=3) == 0 and n.value == 2
    assert call(c=np.array([1.0, np.inf, 1.0])) == 0 and n.value == 1  # an arc of infinite cost is on no path
    assert call(T=0, na=0) == 0 and n.value == 0
    assert call(na=0) == 0 and n.value == 0
    with pytest.raises(capi.SrError):
        capi.lattice_nbest(2, word, first, last, cost, 7, 0)


def nbest_driver_case(T, arcs, sil, n_best, cap, W=None, lm=None, lm_scale=1.0, null_lm=False, null_cost=False):
    """one case of tests/cpp/nbest_host_driver.cpp's file: sr_lattice_nbest, or -- W given -- sr_bigram_lattice_nbest (arcs with hist, am)"""
    kind = W is not None
    u32 = lambda k: np.ascontiguousarray(arcs[k], np.uint32).tobytes()
    n = len(arcs["word"])
    head = struct.pack("<IIIIIIQId", int(kind), int(null_lm) + 2 * int(null_cost), T, n, sil, n_best, cap, W or 0, lm_scale)
    body = u32("word") + (u32("hist") if kind else b"") + u32("first") + u32("last")
    body += np.ascontiguousarray(arcs["am" if kind else "cost"], np.float64).tobytes()
    if kind:
        body += (np.zeros((W, W), np.float32) if lm is None else np.ascontiguousarray(lm, np.float32)).tobytes()
    return head + body


def run_nbest_driver(tmp_path, cases):
    """builds nbest_host_driver.cpp with nbest.cpp alone under the sanitizers, runs it as a plain program on `cases` ->
    [(rc, count, error text, [(words, cost)])]; the run must end with status 0 and say nothing on stderr"""
    drv = str(tmp_path / "nbest_host_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "nbest_host_driver.cpp"),
                           os.path.join(ROOT, "speechrecognition_amd", "csrc", "nbest.cpp"), "-o", drv])
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    p = subprocess.run([drv, str(path)], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-2000:])
    out = []
    for ln in p.stdout.splitlines():
        f = ln.split()
        if f[0] == "case":
            assert int(f[1]) == len(out)
            out.append([int(f[3]), int(f[5]), "", []])
        elif f[0] == "err":
            out[-1][2] = ln[4:]
        else:
            assert f[0] == "s", ln
            out[-1][3].append((tuple(int(x) for x in f[2:]), struct.unpack("<d", struct.pack("<Q", int(f[1], 16)))[0]))
    assert len(out) == len(cases)
    return [tuple(o) for o in out]


def test_nbest_standalone_driver_under_the_sanitizers(tmp_path):
    """tests/cpp/nbest_host_driver.cpp and nbest.cpp alone, built with -fsanitize=address,undefined and run as a plain program, every
    output array exactly as long as the call may fill it: test_nbest_against_exhaustive_enumeration's lattices (T = 1 and 2 .. 7, W 2 .. 4,
    costs on the grid of 1/8, dangling arcs, lattices without a complete path, an arc of +inf cost), n_best 1, 3 and beyond the number
    of strings, a words_cap one short of the need, and every malformed input of test_nbest_errors.  Strings, counts and costs are the
    enumeration's, the costs to the bit; no report."""
    rng = np.random.default_rng(1234)
    cases, want = [], []
    n_nonempty = n_dangling = n_empty = n_inf = n_short = 0
    for case in range(80):
        T = 1 if case % 10 == 0 else int(rng.integers(2, 8))
        W = int(rng.integers(2, 5))
        sil = int(rng.integers(0, W))
        arcs = _random_lattice(rng, T, W, rng.uniform(0.3, 0.9))
        if case % 7 == 3 and len(arcs["cost"]):
            arcs["cost"][int(rng.integers(0, len(arcs["cost"])))] = np.inf   # on no path: its strings are not given out
            n_inf += 1
        ref_all = [(ws, c) for ws, c in LR.nbest(arcs, T, sil, 10 ** 9) if c < np.inf]
        used = {i for _, path in LR.lattice_paths(arcs, T) for i in path}
        n_dangling += len(used) < len(arcs["word"])
        n_nonempty += bool(ref_all)
        n_empty += not ref_all
        need = sum(len(ws) for ws, _ in ref_all)
        for n in (1, 3, len(ref_all) + 5):
            cases.append(nbest_driver_case(T, arcs, sil, n, need))
            want.append((sil, n, ref_all))
        if need:
            cases.append(nbest_driver_case(T, arcs, sil, len(ref_all) + 5, need - 1))
            want.append((sil, None, need - 1))
            n_short += 1
    assert n_nonempty > 30 and n_dangling > 30 and n_empty >= 1 and n_inf >= 5 and n_short > 30
    # the malformed inputs of test_nbest_errors (and its good calls)
    good = {"word": [0, 1, 1], "first": [0, 0, 1], "last": [0, 1, 1], "cost": [1.0, 2.5, 1.0]}
    none = {k: [] for k in good}
    errs = [(2, good, 4, 16, 0, 2), (2, good, 0, 16, EINVAL, None),
            (2, dict(good, last=[0, 1, 2]), 4, 16, EINVAL, None), (2, dict(good, first=[0, 2, 1]), 4, 16, EINVAL, None),
            (2, dict(good, word=[0, 1, 0]), 4, 16, EINVAL, None), (2, dict(good, last=[1, 0, 1], first=[0, 0, 0]), 4, 16, EINVAL, None),
            (2, dict(good, cost=[1.0, np.nan, 1.0]), 4, 16, EINVAL, None), (2, good, 4, 2, EINVAL, 0), (2, good, 4, 3, 0, 2),
            (2, dict(good, cost=[1.0, np.inf, 1.0]), 4, 16, 0, 1), (0, none, 4, 16, 0, 0), (2, none, 4, 16, 0, 0)]
    for T, a, nb, cap, _, _ in errs:
        cases.append(nbest_driver_case(T, a, 7, nb, cap))
    got = run_nbest_driver(tmp_path, cases)
    for (sil, n, ref_all), (rc, count, err, strings) in zip(want, got):
        if n is None:   # one word short: refused, nothing given out
            assert rc == EINVAL and count == 0 and err == f"words_cap {ref_all} is too small", (rc, count, err)
            continue
        assert rc == 0 and count == len(strings) == min(n, len(ref_all)), (rc, count, n, len(ref_all), err)
        assert [c for _, c in strings] == [c for _, c in ref_all[:count]]
        table = dict(ref_all)
        assert len({ws for ws, _ in strings}) == count and all(table[ws] == c and sil not in ws for ws, c in strings)
    for (T, a, nb, cap, want_rc, want_count), (rc, count, err, strings) in zip(errs, got[len(want):]):
        assert rc == want_rc and (want_count is None or count == want_count) and bool(err) == bool(rc), (a, nb, cap, rc, count, err)
    assert got[len(want)][3] == [((0, 1), 2.0), ((1,), 2.5)]


def test_entry_points_are_exported(built_lib):
    L = C.CDLL(built_lib)
    for sym in ENTRY_POINTS:
        assert hasattr(L, sym), sym


def test_header_prototypes_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"SR_API\s+int\s+" + sym + r"\s*\(", hdr), sym
    assert re.search(r"#define\s+SR_ABI_VERSION\s+4\b", hdr)
    assert set(ENTRY_POINTS) <= set(capi.SYMBOLS)
    assert callable(getattr(capi.Corpus, "word_lattice", None)) and callable(getattr(capi, "lattice_nbest", None))
    hpp = open(os.path.join(ROOT, "include", "sr_sietill.hpp")).read()
    assert "sr_word_lattice_corpus" in hpp and "sr_lattice_nbest" in hpp and re.search(r"\brecognize_nbest\s*\(", hpp)


def test_nbest_driver_compiles():
    """include/sr_sietill.hpp's sr::Recognizer::recognize_nbest against srgpu.h (syntax and types; the GPU test runs it)."""
    src = os.path.join(ROOT, "tests", "cpp", "nbest_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_new_kernels_have_no_scratch(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    if not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as tmp:
        md = isa_info.kernel_metadata(isa_info.code_object("viterbi_lattice", tmp))
        for k in KERNELS:
            assert k in md, (k, sorted(md))
            assert md[k]["private_segment_fixed_size"] == 0 and md[k].get("vgpr_spill_count", 0) == 0, (k, md[k])
