"""MLLT on the device (sr_mllt_statistics_corpus, sr_mllt_statistics_bw_corpus) against the numpy restatement
(tests/mllt_reference.py), and end to end with sr_mllt_estimate, sr_corpus_transform and sr_model_transform_means.

The statistics bound is the derivation at the top of test_gpu_fmllr.py.  u = 2^-53.  A sum of n terms added in any order errs by at
most (n - 1) u times the sum of the terms' absolute values (to first order); the device and the reference each add the n live pairs'
terms in an order of their own, so they differ by at most 2 (n - 1) u = (n - 1) 2^-52 of that sum.  Forming a term: z = (double) x - mu
is one rounding and z_j z_k one more, the same operations on the same inputs on both sides (identical bits); gamma iv one rounding,
likewise identical; the product of the two is rounded once in the reference and at most once in the matrix instruction; in soft mode
the membership itself -- the device's exp within 2 ulp, the sum of at most 8 of them, one division, the product with the posterior --
about a dozen u.  C_TERM = 32 halves of 2^-52 cover both sides with room; the bound is (n + 32) 2^-52 sum |terms| per entry."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import fmllr_reference as RF
from tests import mllt_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
C_TERM = 32
SEG = 1024   # pairs per segment (include/srgpu.h)
TDP = (3.0, 0.0, 30.0)
CASES = [(2, False), (13, True), (25, False), (39, True), (39, False), (63, False)]


def make_case(D, seed, n_utts=60, S=10, M=4, lens=(30, 90)):
    """random model and corpus as in test_gpu_fmllr.py: S mixtures of at most M densities; the last utterance has one frame"""
    rng = np.random.default_rng(seed)
    model = RF.random_model(rng, S, M, D)
    T = rng.integers(lens[0], lens[1], size=n_utts)
    T[-1] = 1
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    feats, auts = [], []
    for u in range(n_utts):
        N = 1 if T[u] == 1 else int(rng.integers(2, min(8, T[u]) + 1))
        a = rng.integers(0, S, size=N).astype(np.uint16)
        auts.append(a)
        st = a[np.minimum(np.arange(T[u]) * N // T[u], N - 1)]
        d = np.array([rng.integers(model[0][k], model[0][k + 1]) for k in st])
        feats.append((model[1][d] + 1.3 * rng.normal(size=(T[u], D)) / np.sqrt(model[2][d])).astype(np.float32))
    return model, np.concatenate(feats), off, auts


def open_model(model, max_approx, tied):
    m = capi.Model.from_tables(*model, max_approx=max_approx)
    if tied:   # one variance row per mixture, one mean row per density
        dens_off = model[0]
        n = int(dens_off[-1])
        dm = np.arange(n, dtype=np.uint32)
        dv = np.repeat(np.arange(len(dens_off) - 1, dtype=np.uint32), np.diff(dens_off.astype(np.int64)))
        capi._check(capi.lib().sr_model_set_tying(m.h, n, len(dens_off) - 1, dm.ctypes.data, dv.ctypes.data))
    return m


def aligned_states(corpus, auts, off):
    states, cost = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
    states = states.copy()
    for u, a in enumerate(auts):   # a one-frame utterance has no aligner path: its frame takes the automaton's only state
        if int(off[u + 1] - off[u]) == 1:
            states[int(off[u])] = a[0]
    return states


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_stats(got, ref, label):
    beta, G = got
    rbeta, rG, Gabs, n = ref
    f = (n + C_TERM) * EPS
    err, lim = np.abs(G - rG), f * Gabs
    ratio = float((err / np.where(lim > 0, lim, 1.0)).max())
    print(f"{label}: worst |gpu - ref| / bound = {ratio:.3f}, live pairs {n}")
    assert (err <= lim).all(), (label, ratio)
    assert abs(beta - rbeta) <= f * abs(rbeta), (label, beta, rbeta)
    assert np.array_equal(bits(G), bits(np.swapaxes(G, 1, 2))), (label, "G not exactly symmetric")
    if n == 0:
        assert beta == 0 and not G.any()
    return ratio


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", CASES)
def test_alignment_statistics_against_the_reference(D, tied, max_approx):
    # D = 63: a smaller corpus (the reference holds the D^2 products of every pair at once), still more than one segment
    model, feats, off, auts = make_case(D, 100 + D, **(dict(n_utts=30, lens=(30, 60)) if D == 63 else {}))
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        got = corpus.mllt_statistics(states, max_approx)
        again = corpus.mllt_statistics(states, max_approx)
        corpus.close()
    pairs = RF.alignment_pairs(feats, model, states, max_approx)
    ref = R.statistics(feats, model, pairs)
    check_stats(got, ref, f"align D={D} tied={tied} max_approx={max_approx}")
    assert got[0] == again[0] and np.array_equal(bits(got[1]), bits(again[1])), "two identical calls differ"
    if max_approx:   # one pair of weight 1 per frame: beta is the frame count, exactly
        assert got[0] == float(len(feats))
    assert ref[3] > SEG   # more than one segment


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", CASES)
def test_posterior_statistics_against_the_reference(D, tied, max_approx):
    # small corpora: the reference walks every posterior item in Python and holds the D^2 products of every pair at once
    model, feats, off, auts = make_case(D, 200 + D, n_utts=20 if D == 63 else 24, lens=(20, 50))
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 64)
        bw_cost, got = corpus.mllt_statistics_bw(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, max_approx)
        bw_cost2, again = corpus.mllt_statistics_bw(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, max_approx)
        corpus.close()
    assert int(count.max()) < 64   # no item lost
    assert np.array_equal(bits(cost), bits(bw_cost))
    pairs = RF.posterior_pairs(feats, model, count, state, weight, max_approx)
    ref = R.statistics(feats, model, pairs)
    check_stats(got, ref, f"posterior D={D} tied={tied} max_approx={max_approx}")
    assert got[0] == again[0] and np.array_equal(bits(got[1]), bits(again[1])), "two identical calls differ"
    assert ref[3] > SEG   # more than one segment


def test_workspace_rounds_do_not_change_the_bits(monkeypatch):
    """D = 39: a segment's partial sums are 48 x 784 doubles = 0.3 MB, so a workspace of 1 MiB holds 3 segments and the soft pairs of
    this corpus take more than one round; the additions are the same ones in the same order"""
    D = 39
    model, feats, off, auts = make_case(D, 100 + D)
    with open_model(model, False, False) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        whole = corpus.mllt_statistics(states, False)
        corpus.close()
    n_pairs = int(np.diff(model[0].astype(np.int64))[states].sum())   # dropped pairs keep their place
    assert n_pairs > 3 * SEG   # more segments than one round holds
    monkeypatch.setenv("SRGPU_MLLT_MB", "1")
    with open_model(model, False, False) as m:
        corpus = m.upload(feats, off)
        rounds = corpus.mllt_statistics(states, False)
        corpus.close()
    assert whole[0] == rounds[0] and np.array_equal(bits(whole[1]), bits(rounds[1]))


def test_shards_add_up():
    D = 13
    model, feats, off, auts = make_case(D, 7)
    o = off.astype(np.int64)
    n_utts = len(auts)
    with open_model(model, True, False) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        whole = corpus.mllt_statistics(states, True)
        corpus.close()
        pairs = RF.alignment_pairs(feats, model, states, True)
        ref = R.statistics(feats, model, pairs)
        check_stats(whole, ref, "whole")
        rng = np.random.default_rng(3)
        for split in (np.arange(n_utts) % 2 == 0, rng.random(n_utts) < 0.3):
            beta, G = 0.0, np.zeros((D, D, D))
            for part in (split, ~split):
                us = np.flatnonzero(part)
                f = np.concatenate([feats[o[u]:o[u + 1]] for u in us])
                st = np.concatenate([states[o[u]:o[u + 1]] for u in us])
                po = np.concatenate([[0], np.cumsum([o[u + 1] - o[u] for u in us])]).astype(np.uint64)
                c = m.upload(f, po)
                b, g = c.mllt_statistics(st, True)
                beta, G = beta + b, G + g
                c.close()
            check_stats((beta, G), ref, "two shards")
            assert beta == whole[0]
        # a corpus without frames: zeros
        empty = m.upload(np.zeros((0, D), np.float32), np.array([0], np.uint64))
        b, g = empty.mllt_statistics(np.zeros(0, np.uint16), True)
        assert b == 0.0 and not g.any()
        empty.close()


def test_errors_are_refused_before_any_launch():
    D = 5
    model, feats, off, auts = make_case(D, 9, n_utts=6, lens=(10, 20))
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states = aligned_states(corpus, auts, off)
        beta, G = np.full(1, 7.0), np.full((D, D, D), 7.0)
        assert L.sr_mllt_statistics_corpus(m.h, corpus.h, P(states), 1, None, P(G)) == -1
        assert L.sr_mllt_statistics_corpus(m.h, corpus.h, P(states), 1, P(beta), None) == -1
        bad_states = states.copy()
        bad_states[0] = 60000
        assert L.sr_mllt_statistics_corpus(m.h, corpus.h, P(bad_states), 1, P(beta), P(G)) == -1
        t3 = (C.c_double * 3)(*TDP)
        flat, aoff = corpus._aut(auts)
        cost = np.full(len(auts), 7.0)
        bw = lambda floor, b, g: L.sr_mllt_statistics_bw_corpus(m.h, corpus.h, P(flat), P(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, floor,  # noqa: E731
                                                                 1, P(cost), b, g)
        assert bw(0.0, None, P(G)) == -1 and bw(0.0, P(beta), None) == -1
        assert bw(-1.0, P(beta), P(G)) == -1
        assert beta[0] == 7.0 and (G == 7.0).all() and (cost == 7.0).all()
        assert bw(0.0, P(beta), P(G)) == 0 and beta[0] != 7.0   # the same call with a valid floor goes through
        corpus.close()
    wide = RF.random_model(np.random.default_rng(1), 3, 2, 64)
    with capi.Model.from_tables(*wide, max_approx=True) as m:
        corpus = m.upload(np.zeros((4, 64), np.float32), np.array([0, 4], np.uint64))
        b, g = np.full(1, 7.0), np.full((64, 64, 64), 7.0)
        st = np.zeros(4, np.uint16)
        assert L.sr_mllt_statistics_corpus(m.h, corpus.h, P(st), 1, P(b), P(g)) == -4
        assert b[0] == 7.0 and (g == 7.0).all()
        corpus.close()


def test_the_transform_lowers_the_cost_of_the_alignment():
    """Synthetic corpus drawn from a max-approx model along known alignments, then features and means mixed by one matrix M while the
    model keeps its diagonal variances: it sees correlated data.  With the alignment and the arg-min densities fixed,
    cost(adapted pair) - beta logdet = cost(original) - (Q(A) - Q(I)); the device's path scores re-pick the arg-min, which can only
    lower the left side."""
    D = 13
    rng = np.random.default_rng(77)
    dens_off, means, inv_vars, norm, logw = RF.random_model(rng, 10, 3, D)
    M = np.eye(D) + 0.3 * rng.normal(size=(D, D)) / np.sqrt(D)
    model = (dens_off, means @ M.T, inv_vars, norm, logw)
    n_utts = 18
    T = rng.integers(40, 80, size=n_utts)
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    feats, auts = [], []
    for u in range(n_utts):
        N = int(rng.integers(3, 8))
        a = rng.integers(0, 10, size=N).astype(np.uint16)
        auts.append(a)
        st = a[np.minimum(np.arange(T[u]) * N // T[u], N - 1)]
        d = np.array([rng.integers(dens_off[k], dens_off[k + 1]) for k in st])
        y = means[d] + rng.normal(size=(T[u], D)) / np.sqrt(inv_vars[d])
        feats.append((y @ M.T).astype(np.float32))
    feats = np.concatenate(feats)
    one = np.zeros(n_utts, np.uint32)
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        states, cost0 = corpus.align(auts, TDP, 0, capi.GMM_DEFAULT)
        # the reference's own gain and the float32 rounding of the adapted features, before any device statistic is looked at
        pairs = RF.alignment_pairs(feats, model, states, True)
        rbeta, rG, _, _ = R.statistics(feats, model, pairs)
        Aref, _ = R.estimate(rbeta, rG, 10)
        gain = R.aux(rbeta, rG, Aref)[0] - R.aux(rbeta, rG, np.eye(D))[0]
        y = RF.transform(feats, off, one, capi.mllt_affine(Aref)).astype(np.float64)
        dens = np.array([d for _, d, _ in pairs])
        mu = model[1][dens] @ Aref.T
        rounding = float((np.abs(y - mu) * model[2][dens] * np.abs(y)).sum()) * 2.0 ** -24
        print(f"reference gain {gain:.3f}, float32 rounding of the adapted features at most {rounding:.3e}")
        assert gain > 100 * rounding and gain > 0
        beta, G = corpus.mllt_statistics(states, True)
        A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=10)
        assert status == 0
        W = capi.mllt_affine(A)
        adapted = corpus.transform(one, W)
        with m.transform_means(np.zeros(m.n_densities, np.uint32), W) as m2:
            # the adapted features (sr_corpus_transform's documented loop, bit for bit) uploaded to the adapted model
            yf = RF.transform(feats, off, one, W)
            host = m.upload(yf, off)
            assert np.array_equal(bits(adapted.score(capi.GMM_EXACT)), bits(host.score(capi.GMM_EXACT)))
            host.close()
            c2 = m2.upload(yf, off)
            before = corpus.path_scores(states).sum()
            after = c2.path_scores(states).sum()
            jac = beta * logdet
            print(f"cost {before:.3f} -> {after:.3f} - {jac:.3f} = {after - jac:.3f}; Q gain {aux[-1] - aux[0]:.3f}")
            assert after - jac < before
            # re-aligning the adapted pair: the new best path costs no more than the old path does on it
            states2, cost2 = c2.align(auts, TDP, 0, capi.GMM_DEFAULT)
            old_path = cost0.sum() - before + after
            assert cost2.sum() <= old_path + 1e-9 * abs(old_path)
            c2.close()
        adapted.close()
        corpus.close()


def _xor(words):
    x = 0
    for b in words.tolist():
        x ^= b
        x = ((x << 1) | (x >> 63)) & 0xFFFFFFFFFFFFFFFF
    return x


def test_cpp_helper_adapts_corpus_and_model(tmp_path):
    """sr::Mllt through tests/cpp/mllt_driver: the same matrix, bit for bit, as the calls made from here; the same adapted features and
    the same scores of the adapted pair"""
    D = 13
    lex = synth.make_lexicon(6, 3, 1)
    spec = synth.make_mixset(lex.n_states, 3, D, seed=31)
    mp = os.path.join(str(tmp_path), "a.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(6, 60, 90, D, seed=32)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(4)
    orths = [rng.integers(1, 6, size=3).astype(np.uint32) for _ in range(6)]
    orths = [np.where(o == lex.silence_idx, (lex.silence_idx + 1) % 6, o).astype(np.uint32) for o in orths]
    blob = struct.pack("<I", len(lex.word_states))
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<Idddd", lex.silence_idx, *TDP, 10.0) + struct.pack("<I", 6)
    o = off.astype(np.int64)
    for u in range(6):
        blob += struct.pack("<II", 0, len(orths[u])) + orths[u].tobytes()
        blob += struct.pack("<I", int(o[u + 1] - o[u])) + feats[o[u]:o[u + 1]].tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    drv = str(tmp_path / "mllt_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mllt_driver.cpp"), "-o", drv,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([drv, "adapt", mp, str(D), str(case)], text=True).splitlines()
    assert not out[0].startswith("error"), out[0]
    auts = []
    for u in range(6):
        a = [sil]
        for w in orths[u]:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, dtype=np.uint16))
    one = np.zeros(6, np.uint32)
    with capi.Model.from_mixset(mp, D) as m:
        corpus = m.upload(feats, off)
        states, _ = corpus.align(auts, TDP, sil, capi.GMM_DEFAULT)
        beta, G = corpus.mllt_statistics(states, True)
        corpus.close()
        A, aux, logdet, status = capi.mllt_estimate(beta, G, n_sweeps=10, min_count=10.0)
        head = out[0].split()
        assert head[:2] == ["status", str(status)] and status == 0
        assert int(head[3], 16) == int(bits(np.array([logdet]))[0]) and int(head[5], 16) == int(bits(aux[-1:])[0])
        got = np.array([int(x, 16) for x in out[1].split()[1:]], dtype=np.uint64)
        assert np.array_equal(got, bits(A).reshape(-1))
        W = capi.mllt_affine(A)
        want = RF.transform(feats, off, one, W)
        assert out[2].split() == ["checksum", format(_xor(want.reshape(-1).view(np.uint32)), "x")]
        assert out[3] == "resident equal"
        with m.transform_means(np.zeros(m.n_densities, np.uint32), W) as m2:
            c2 = m2.upload(want, off)
            sc = c2.score(capi.GMM_EXACT)
            c2.close()
        assert out[4].split() == ["scores", format(_xor(bits(sc).reshape(-1)), "x")]
