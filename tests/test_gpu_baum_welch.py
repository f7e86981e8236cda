"""Baum-Welch training pass on the device (sr_state_posteriors_corpus, sr_baum_welch_corpus) against the numpy forward-backward
restatement (tests/fb_reference.py) on the oracle's emission costs, against the aligner and the Viterbi accumulator where the
two must agree, and on the EM property itself.  Tolerances: forward costs and posteriors by the measured rule of
tests/test_gpu_fb_scores.py -- 8 times the float64 restatement's own distance from its np.longdouble run on the same costs, plus 4 ulp
of the value, against the longdouble run -- and never more than the 1e-10 relative / 1e-9 absolute held before; statistics 1e-9
relative to the sum of |w x| (1e-12 in the single-path case, where the weights are 1 up to rounding)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import fb_reference as R
from tests.util import Case, golden_names

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDP = (3.0, 0.0, 30.0)
ALIGN_GOLDEN = [n for n in golden_names() if "align_ref" in np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")).files]


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _check_utterances(o, feats, off, auts, tdp, sil, cost, count, state, weight, items_floor=0.0, max_items=None, measured=True):
    """forward costs and per-frame items against the restatement: 1e-10 relative, 1e-9 absolute and -- measured -- the rule (the
    trellis of 8192 x 4200 keeps the fixed pair: its longdouble run alone takes longer than the whole module)"""
    LD = np.longdouble if measured else np.float64
    for u, ref in enumerate(auts):
        f = feats[int(off[u]):int(off[u + 1])]
        e = o.score_matrix(f)
        F, g = R.posteriors(e, ref, tdp, sil)
        F80, g80 = R.posteriors(e, ref, tdp, sil, dtype=LD) if measured else (F, g)
        assert _rel(cost[u], F) <= 1e-10, (u, cost[u], F)
        d_F = abs(float(LD(F) - F80))
        assert not measured or abs(float(LD(cost[u]) - F80)) <= 8 * d_F + 4 * np.spacing(abs(F)), (u, cost[u], F, d_F)
        mix, gm = R.mixture_posteriors(g, ref)
        gm80 = R.mixture_posteriors(g80, ref)[1]
        d_g = float(np.max(np.abs(gm - gm80)))
        col = {int(k): j for j, k in enumerate(mix)}
        for t in range(len(f)):
            ft = int(off[u]) + t
            n = int(count[ft])
            got = dict(zip(state[ft, :n].tolist(), weight[ft, :n].tolist()))
            assert len(got) == n
            for k, w in got.items():
                assert abs(w - gm[t, col[k]]) <= 1e-9, (u, t, k, w, gm[t, col[k]])
                assert not measured or abs(float(LD(w) - gm80[t, col[k]])) <= 8 * d_g + 4 * np.spacing(float(gm80[t, col[k]])), (u, t, k, w, gm[t, col[k]], d_g)
                assert w >= items_floor and w > 0
            # every mixture left out is below the floor (or past the truncation), up to the tolerance
            want = [(int(mix[j]), gm[t, j]) for j in range(len(mix)) if gm[t, j] > 0 and gm[t, j] >= items_floor]
            if max_items is None or len(want) <= max_items:
                for k, w in want:
                    assert k in got or w < items_floor + 1e-9 or w < 1e-9, (u, t, k, w)


@pytest.mark.parametrize("name", ALIGN_GOLDEN)
def test_forward_costs_and_posteriors_golden(name, tmp_path, oracle_lib):
    c = Case(name, tmp_path)
    T = c.feats.shape[0]
    off = np.array([0, T], dtype=np.uint64)
    ref = c.z["align_ref"]
    sil = c.lex.flatten()[2]
    o = c.oracle(oracle_lib)
    with capi.Model.from_mixset(c.mixset_path, c.dim, c.pooling, c.max_approx) as m:
        corpus = m.upload(c.feats, off)
        cost, count, state, weight = corpus.state_posteriors([ref], c.tdp, sil, capi.GMM_DEFAULT, 0.0, 64)
        _, vcost = corpus.align([ref], c.tdp, sil, capi.GMM_DEFAULT)
        corpus.close()
    _check_utterances(o, c.feats, off, [ref], c.tdp, sil, cost, count, state, weight)
    assert np.abs(weight.sum(axis=1) - 1.0).max() <= 1e-9
    V = float(vcost[0])
    assert V - np.log(float(R.n_paths(T, len(ref)))) - 1e-9 * abs(V) <= cost[0] <= V + 1e-9 * abs(V)
    o.close()


@pytest.mark.parametrize("pname", ["mixture", "none"])
def test_forward_costs_and_posteriors_real_speech(pname, tmp_path, oracle_lib):
    z = np.load(os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz"))
    lex = synth.sietill_lexicon()
    word_off, automaton, sil = lex.flatten()
    mp = tmp_path / "real.mix"
    mp.write_bytes(z[f"model_{pname}"].tobytes())
    tdp = tuple(float(x) for x in z["tdp"])
    auts = []
    for i in range(len(z["ref_off"]) - 1):
        a = [sil]
        for w in z["ref_flat"][z["ref_off"][i]:z["ref_off"][i + 1]]:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, dtype=np.uint16))
    pool = {"mixture": 1, "none": 2}[pname]
    o = oracle_lib.Oracle(str(mp), int(z["dim"]), lex, tdp=tdp, pooling=pool)
    with capi.Model.from_mixset(str(mp), int(z["dim"]), pool, True) as m:
        corpus = m.upload(z["feats"], z["frame_off"])
        cost, count, state, weight = corpus.state_posteriors(auts, tdp, sil, capi.GMM_DEFAULT, 0.0, 64)
        _, vcost = corpus.align(auts, tdp, sil, capi.GMM_DEFAULT)
        corpus.close()
    off = z["frame_off"].astype(np.int64)
    _check_utterances(o, z["feats"], off, auts, tdp, sil, cost, count, state, weight)
    o.close()
    for u in range(len(auts)):
        T, N = int(off[u + 1] - off[u]), len(auts[u])
        V = float(vcost[u])
        assert V - np.log(float(R.n_paths(T, N))) - 1e-9 * abs(V) <= cost[u] <= V + 1e-9 * abs(V)


def _synthetic(tmp_path, seed, S=40, M=4, D=13, tie_vars=False):
    spec = synth.make_mixset(S, M, D, seed=seed, tie_vars=tie_vars)
    mp = str(tmp_path / f"s{seed}.mix")
    synth.write_mixset(mp, spec)
    lex = synth.make_lexicon((S - 1) // 3, 3, 1)
    return spec, mp, lex


def test_forward_costs_synthetic_automata(tmp_path, oracle_lib):
    """~200 utterances, automata of 5..200 random positions (silence among them), N > T included, and the aligner's bound."""
    spec, mp, lex = _synthetic(tmp_path, 71)
    rng = np.random.default_rng(72)
    auts, lens = [], []
    for u in range(200):
        N = int(rng.integers(5, 201))
        T = int(rng.integers((N + 2) // 2, 2 * N + 1)) if u % 3 else int(rng.integers((N + 2) // 2, N))  # every third: N > T
        auts.append(rng.integers(0, 40, size=N).astype(np.uint16))
        lens.append(T)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    feats = rng.standard_normal((int(off[-1]), 13)).astype(np.float32)
    o = oracle_lib.Oracle(mp, 13, lex)
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 256)
        fit = [u for u in range(200) if len(auts[u]) <= lens[u]]
        sub_off = np.concatenate([[0], np.cumsum([lens[u] for u in fit])]).astype(np.uint64)
        sub = np.concatenate([feats[int(off[u]):int(off[u + 1])] for u in fit])
        corpus.close()
        c2 = m.upload(sub, sub_off)
        _, vcost = c2.align([auts[u] for u in fit], TDP, 0, capi.GMM_DEFAULT)
        c2.close()
    assert any(len(a) > t for a, t in zip(auts, lens))
    _check_utterances(o, feats, off, auts, TDP, 0, cost, count, state, weight)
    o.close()
    assert np.abs(weight.sum(axis=1) - 1.0).max() <= 1e-9
    for i, u in enumerate(fit):
        V = float(vcost[i])
        assert V - np.log(float(R.n_paths(lens[u], len(auts[u])))) - 1e-9 * abs(V) <= cost[u] <= V + 1e-9 * abs(V)


def test_forward_cost_at_the_position_limit(tmp_path, oracle_lib):
    """N = 8192 (align_max_positions) with T = 4200 frames, beside a one-frame utterance (F = e(0, ref[0]))."""
    spec, mp, lex = _synthetic(tmp_path, 81)
    rng = np.random.default_rng(82)
    auts = [rng.integers(0, 40, size=8192).astype(np.uint16), np.asarray([5], np.uint16)]
    off = np.array([0, 4200, 4201], dtype=np.uint64)
    feats = rng.standard_normal((4201, 13)).astype(np.float32)
    o = oracle_lib.Oracle(mp, 13, lex)
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 64)
        corpus.close()
    _check_utterances(o, feats, off, auts, TDP, 0, cost, count, state, weight, measured=False)
    assert cost[1] == o.score_matrix(feats[4200:])[0, 5]
    assert count[4200] == 1 and state[4200, 0] == 5 and weight[4200, 0] == 1.0
    o.close()


def test_posterior_order_floor_and_truncation(tmp_path, oracle_lib):
    spec, mp, lex = _synthetic(tmp_path, 91)
    rng = np.random.default_rng(92)
    word_off, automaton, sil = lex.flatten()
    auts, utts = [], []
    for i in range(6):
        ws = rng.integers(1, lex.n_words, size=3)
        utts.append(synth.sample_utterance(spec, lex, ws, seed=93 + i, noise=2.0))
        a = [sil]
        for w in ws:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    feats = np.concatenate(utts)
    o = oracle_lib.Oracle(mp, 13, lex)
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, off)
        full = corpus.state_posteriors(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, 64)
        cut = corpus.state_posteriors(auts, TDP, sil, capi.GMM_DEFAULT, 0.01, 2)
        corpus.close()
    _check_utterances(o, feats, off, auts, TDP, sil, *full)
    _check_utterances(o, feats, off, auts, TDP, sil, *cut, items_floor=0.01, max_items=2)
    o.close()
    cost, count, state, weight = cut
    assert np.array_equal(cost.view(np.uint64), full[0].view(np.uint64))
    assert (count <= 2).all() and (count >= 1).all()
    for t in range(len(feats)):
        n = int(count[t])
        w, s = weight[t, :n], state[t, :n]
        assert (w >= 0.01).all() and all(w[i] > w[i + 1] or (w[i] == w[i + 1] and s[i] < s[i + 1]) for i in range(n - 1))
        assert (weight[t, n:] == 0).all() and (state[t, n:] == 0).all()
        # the kept items are the largest of the untruncated list
        fn = int(full[1][t])
        ranked = sorted(zip(full[3][t, :fn].tolist(), full[2][t, :fn].tolist()), key=lambda p: (-p[0], p[1]))
        want = [p for p in ranked if p[0] >= 0.01][:2]
        assert [int(x) for x in s] == [p[1] for p in want]


def _many_mixtures_case(seed):
    """(automata, frame offsets, features): a random order of 100 distinct mixtures over 60 frames, utterances of one and of three
    frames, and 20 positions drawn from 5 mixtures (several positions to a mixture) over 37 frames"""
    rng = np.random.default_rng(seed)
    auts = [rng.permutation(100).astype(np.uint16), np.asarray([7], np.uint16), np.asarray([3, 90], np.uint16),
            rng.choice(rng.permutation(100)[:5], size=20).astype(np.uint16)]
    off = np.concatenate([[0], np.cumsum([60, 1, 3, 37])]).astype(np.uint64)
    feats = rng.standard_normal((int(off[-1]), 13)).astype(np.float32)
    return auts, off, feats


def test_posteriors_of_many_mixtures_and_short_utterances(tmp_path, oracle_lib):
    """Baum-Welch's items (a thread per frame sums every mixture of its automaton) on an automaton of 100 distinct mixtures -- every
    other test here has at most 40 -- beside very short utterances: items at floor 0 and above a floor with truncation, and the same
    bytes from a second call."""
    spec, mp, lex = _synthetic(tmp_path, 101, S=100)
    auts, off, feats = _many_mixtures_case(102)
    o = oracle_lib.Oracle(mp, 13, lex)
    # not vacuous: the reference alone puts mixtures of sorted rank >= 64 (here: id >= 64) into the items of many frames
    _, g = R.posteriors(o.score_matrix(feats[:60]), auts[0], TDP, 0)
    mix, gm = R.mixture_posteriors(g, auts[0])
    high_rank = sum(any(k >= 64 for k, _ in it) for it in R.items(mix, gm, 0.0))
    print("frames with a mixture of rank >= 64:", high_rank)
    assert len(mix) == 100 and high_rank >= 10
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, off)
        full = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 128)
        cut = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 1e-4, 4)
        again = [corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 128), corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 1e-4, 4)]
        corpus.close()
    _check_utterances(o, feats, off, auts, TDP, 0, *full)
    _check_utterances(o, feats, off, auts, TDP, 0, *cut, items_floor=1e-4, max_items=4)
    o.close()
    for first, second in zip((full, cut), again):
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()


def _single_path_case(tmp_path, seed, tie_vars=False):
    spec, mp, lex = _synthetic(tmp_path, seed, tie_vars=tie_vars)
    rng = np.random.default_rng(seed + 1)
    lens = rng.integers(20, 41, size=5)
    auts = [rng.integers(1, 40, size=int(T)).astype(np.uint16) for T in lens]  # no silence (state 0), N = T
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    feats = rng.standard_normal((int(off[-1]), 13)).astype(np.float32)
    return mp, auts, off, feats


@pytest.mark.parametrize("mode", ["first_pass", "max_approx", "soft"])
def test_single_path_anchor(tmp_path, mode):
    """N = T, loop = skip = +inf, no silence: the diagonal is the only path.  F is the aligner's cost, the posteriors are one-hot on
    the aligner's states and the statistics are sr_accumulate_corpus' on them."""
    mp, auts, off, feats = _single_path_case(tmp_path, 111)
    tdp = (np.inf, 1.5, np.inf)
    fp, ma = mode == "first_pass", mode == "max_approx"
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, off)
        states, vcost = corpus.align(auts, tdp, 0, capi.GMM_DEFAULT)
        cost, count, state, weight = corpus.state_posteriors(auts, tdp, 0, capi.GMM_DEFAULT, 0.0, 4)
        bcost, got = corpus.baum_welch(auts, tdp, 0, capi.GMM_DEFAULT, 0.0, fp, ma)
        want = corpus.accumulate(states, fp, ma)
        corpus.close()
    for u in range(len(auts)):
        assert _rel(cost[u], vcost[u]) <= 1e-12 and np.isfinite(cost[u])
    assert np.array_equal(bcost.view(np.uint64), cost.view(np.uint64))
    assert (count == 1).all() and np.array_equal(state[:, 0], states) and np.abs(weight[:, 0] - 1.0).max() <= 1e-12
    for g, w in zip(got, want):
        assert np.all(np.abs(g - w) <= 1e-12 * np.maximum(np.abs(w), 1.0))


@pytest.mark.parametrize("tie_vars", [False, True])
@pytest.mark.parametrize("mode", ["first_pass", "max_approx", "soft"])
def test_statistics_match_weighted_restatement(tmp_path, oracle_lib, mode, tie_vars):
    S, D = 13, 13
    spec = synth.make_mixset(S, [1, 3, 6, 2, 4, 5, 1, 2, 3, 4, 6, 2, 3], D, seed=121, tie_vars=tie_vars)
    mp = str(tmp_path / "m.mix")
    synth.write_mixset(mp, spec)
    lex = synth.make_lexicon(4, 3, 1)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(122)
    auts, utts = [], []
    for i in range(5):
        ws = rng.integers(1, lex.n_words, size=2)
        utts.append(synth.sample_utterance(spec, lex, ws, seed=123 + i, noise=1.5))
        a = [sil]
        for w in ws:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    feats = np.concatenate(utts)
    fp, ma = mode == "first_pass", mode == "max_approx"
    floor = 1e-3
    o = oracle_lib.Oracle(mp, D, lex)
    tables = o.tables()
    frame_items = []
    for u, ref in enumerate(auts):
        f = feats[int(off[u]):int(off[u + 1])]
        _, g = R.posteriors(o.score_matrix(f), ref, TDP, sil)
        frame_items += R.items(*R.mixture_posteriors(g, ref), floor)
    o.close()
    with capi.Model.from_mixset(mp, D) as m:
        corpus = m.upload(feats, off)
        _, got = corpus.baum_welch(auts, TDP, sil, capi.GMM_DEFAULT, floor, fp, ma)
        corpus.close()
    nm, nv = len(got[1]), len(got[3])
    ma_, mw, va, vw, sm, sv = R.accumulate(feats, frame_items, tables, nm, nv, fp, ma)
    assert np.all(np.abs(got[0] - ma_) <= 1e-9 * np.maximum(sm, 1e-300))
    assert np.all(np.abs(got[2] - va) <= 1e-9 * np.maximum(sv, 1e-4))
    assert np.all(np.abs(got[1] - mw) <= 1e-9 * np.maximum(mw, 1e-300)) and np.all(np.abs(got[3] - vw) <= 1e-9 * np.maximum(vw, 1e-300))
    assert got[1].sum() > 0.9 * len(feats)


def test_device_resident_statistics_and_determinism(tmp_path):
    spec, mp, lex = _synthetic(tmp_path, 131, M=5)
    rng = np.random.default_rng(132)
    word_off, automaton, sil = lex.flatten()
    auts, utts = [], []
    for i in range(8):
        ws = rng.integers(1, lex.n_words, size=3)
        utts.append(synth.sample_utterance(spec, lex, ws, seed=133 + i))
        a = [sil]
        for w in ws:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    feats = np.concatenate(utts)
    with capi.Model.from_mixset(mp, 13) as m:
        dens_off, dens_mean, dens_var = m.topology()
        corpus = m.upload(feats, off)
        runs = [corpus.baum_welch(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, False, False) for _ in range(2)]
        posts = [corpus.state_posteriors(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, 8) for _ in range(2)]
        for a, b in zip([runs[0][0], *runs[0][1]], [runs[1][0], *runs[1][1]]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for a, b in zip(posts[0], posts[1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        cost = corpus.baum_welch_on_device(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, False, False)
        assert np.array_equal(cost.view(np.uint64), runs[0][0].view(np.uint64))
        with corpus.next_model(capi.POOL_NONE, True) as m2, \
                capi.Model.from_statistics(13, dens_off, dens_mean, dens_var, runs[0][1], capi.POOL_NONE, True) as m3:
            a, b = m2.score_frames(feats[:200], capi.GMM_EXACT), m3.score_frames(feats[:200], capi.GMM_EXACT)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        corpus.close()


def test_em_iterations_decrease_the_total_forward_cost(tmp_path):
    """Three Baum-Welch iterations (soft memberships, no pooling) on a perturbed sum-mode model, data drawn from the true one."""
    spec = synth.make_mixset(25, 3, 13, seed=141)
    lex = synth.make_lexicon(8, 3, 1)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(142)
    auts, utts = [], []
    for i in range(24):
        ws = rng.integers(1, lex.n_words, size=3)
        utts.append(synth.sample_utterance(spec, lex, ws, seed=143 + i))
        a = [sil]
        for w in ws:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    feats = np.concatenate(utts)
    mu = spec.mean_acc / spec.mean_w[:, None]
    var = spec.var_acc / spec.var_w[:, None] - mu ** 2
    mu = mu + 0.5 * rng.standard_normal(mu.shape)
    spec.mean_acc, spec.var_acc = mu * spec.mean_w[:, None], (var + mu ** 2) * spec.var_w[:, None]
    mp = str(tmp_path / "perturbed.mix")
    synth.write_mixset(mp, spec)
    totals = []
    models = [capi.Model.from_mixset(mp, 13, capi.POOL_NONE, max_approx=False)]
    for it in range(4):
        corpus = models[-1].upload(feats, off)
        cost = corpus.baum_welch_on_device(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, False, False)
        totals.append(float(cost.sum()))
        if it < 3:
            models.append(corpus.next_model(capi.POOL_NONE, False))
        corpus.close()
    for m in reversed(models):
        m.close()
    assert all(np.isfinite(totals))
    assert totals[0] > totals[1] > totals[2] > totals[3], totals


def test_scale_configs2_shape(tmp_path, monkeypatch):
    """configs[2]'s shape (4000 states x 32, 1000 utterances of 200..400 frames, `sil w1 sil w2 sil w3 sil`): through
    sr_baum_welch_corpus within a 4 MiB trellis workspace -- several launch groups -- with the same bits as one group, and with
    floor 0 and first-pass memberships mean_w sums to the frame count."""
    lex = synth.make_lexicon(1333, 3, 1)
    spec = synth.make_mixset(lex.n_states, 32, 39, seed=23)
    mp = str(tmp_path / "m.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(1000, 200, 400, 39, seed=7)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(5)
    auts = []
    for u in range(1000):
        a = [sil]
        for w in rng.integers(1, lex.n_words, size=3):
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    out = []
    for mb in (None, "4"):
        if mb:
            monkeypatch.setenv("SRGPU_FB_MB", mb)
        with capi.Model.from_mixset(mp, 39) as m:
            corpus = m.upload(feats, off)
            out.append(corpus.baum_welch(auts, TDP, sil, capi.GMM_DEFAULT, 0.0, True, False))
            corpus.close()
    assert sum(len(a) * int(off[u + 1] - off[u]) for u, a in enumerate(auts)) * 8 > 4 * (4 << 20)
    for a, b in zip([out[0][0], *out[0][1]], [out[1][0], *out[1][1]]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    F = int(off[-1])
    assert abs(out[1][1][1].sum() - F) <= 1e-9 * F and np.isfinite(out[1][0]).all()


def _raw_posteriors(corpus, auts, **kw):
    flat, aoff = corpus._aut(auts)
    F = corpus.n_frames
    args = dict(tdp=TDP, sil=0, kernel=capi.GMM_DEFAULT, floor=0.0, max_items=4, cost=np.zeros(len(auts)), count=np.zeros(F, np.uint16),
                state=np.zeros(F * 4, np.uint16), weight=np.zeros(F * 4))
    args.update(kw)
    t3 = (C.c_double * 3)(*args["tdp"])
    p = capi._ptr
    return capi.lib().sr_state_posteriors_corpus(corpus.model.h, corpus.h, p(flat), p(aoff), C.byref(t3), args["sil"], args["kernel"],
                                                  args["floor"], args["max_items"], p(args["cost"]), p(args["count"]), p(args["state"]),
                                                  p(args["weight"]))


def _raw_baum_welch(corpus, auts, stats=True, drop=None, floor=0.0):
    flat, aoff = corpus._aut(auts)
    nm, nv, D = corpus.model.n_states * 4, corpus.model.n_states * 4, corpus.model.dim
    outs = [np.zeros(nm * D), np.zeros(nm), np.zeros(nv * D), np.zeros(nv)] if stats else [None] * 4
    if drop is not None:
        outs[drop] = None
    t3 = (C.c_double * 3)(*TDP)
    p = capi._ptr
    return capi.lib().sr_baum_welch_corpus(corpus.model.h, corpus.h, p(flat), p(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, floor, 0, 1,
                                            p(np.zeros(len(auts))), *[p(a) for a in outs])


def test_error_paths(tmp_path, monkeypatch):
    monkeypatch.setenv("SRGPU_FB_MB", "1")
    spec, mp, lex = _synthetic(tmp_path, 151)
    rng = np.random.default_rng(152)
    feats = rng.standard_normal((300, 13)).astype(np.float32)
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(feats, np.array([0, 100, 300], dtype=np.uint64))
        ok = [np.arange(1, 11, dtype=np.uint16), np.arange(1, 31, dtype=np.uint16)]
        assert _raw_posteriors(corpus, ok) == 0
        assert _raw_posteriors(corpus, ok, floor=-1.0) == -1
        assert _raw_posteriors(corpus, ok, floor=float("nan")) == -1
        assert _raw_posteriors(corpus, ok, max_items=0) == -1
        assert _raw_posteriors(corpus, ok, count=None) == -1                          # partial set of optional outputs
        assert _raw_posteriors(corpus, ok, count=None, state=None, weight=None) == 0  # cost only
        assert _raw_posteriors(corpus, ok, cost=None) == -1
        assert _raw_posteriors(corpus, [np.arange(1, 11, dtype=np.uint16), rng.integers(1, 40, 400).astype(np.uint16)]) == -1  # N > 2T-1
        assert _raw_posteriors(corpus, [ok[0], np.full(200, 99, np.uint16)]) == -1     # state >= n_states
        assert _raw_posteriors(corpus, [ok[0], np.zeros(0, np.uint16)]) == -1          # empty automaton
        assert _raw_baum_welch(corpus, ok, drop=2) == -1
        assert _raw_baum_welch(corpus, ok, floor=-0.5) == -1
        assert _raw_baum_welch(corpus, ok) == 0
        assert _raw_baum_welch(corpus, ok, stats=False) == 0
        assert _raw_baum_welch(corpus, ok, stats=False, floor=2.0) == -1  # nothing above the floor to keep on the device
        corpus.close()
        big = m.upload(rng.standard_normal((4200, 13)).astype(np.float32), np.array([0, 4200], dtype=np.uint64))
        assert _raw_posteriors(big, [rng.integers(1, 40, 8193).astype(np.uint16)]) == -4   # more positions than 8192
        assert _raw_posteriors(big, [rng.integers(1, 40, 100).astype(np.uint16)]) == -4    # trellis 100 x 4200 x 8 B > 1 MiB
        big.close()


def test_trainer_mirror(tmp_path, oracle_lib):
    """sr::Trainer::baum_welch (include/sr_sietill.hpp) through tests/cpp/baum_welch_driver.cpp: the binding's bits."""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "baum_welch_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "baum_welch_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    spec, mp, lex = _synthetic(tmp_path, 161)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(162)
    orths = [rng.integers(1, lex.n_words, size=3) for _ in range(4)]
    utts = [synth.sample_utterance(spec, lex, ws, seed=163 + i) for i, ws in enumerate(orths)]
    blob = struct.pack("<I", lex.n_words)
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<I4d", lex.silence_idx, *TDP, 1e-4) + struct.pack("<I", len(utts))
    for ws, f in zip(orths, utts):
        blob += struct.pack("<I", len(ws)) + np.asarray(ws, "<u4").tobytes()
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "bw", mp, "13", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    auts = []
    for ws in orths:
        a = [sil]
        for w in ws:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, np.uint16))
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    with capi.Model.from_mixset(mp, 13) as m:
        corpus = m.upload(np.concatenate(utts), off)
        cost, stats = corpus.baum_welch(auts, TDP, sil, capi.GMM_DEFAULT, 1e-4, False, True)
        corpus.close()
    for u in range(len(utts)):
        assert f"cost {u} {int(cost[u:u + 1].view(np.uint64)[0]):x}" in lines
    assert lines[len(utts)] == "stat mean_w " + " ".join(f"{int(x):x}" for x in stats[1].view(np.uint64))
    assert lines[len(utts) + 1] == "stat var_w " + " ".join(f"{int(x):x}" for x in stats[3].view(np.uint64))
    x = np.bitwise_xor.reduce(np.concatenate([stats[0].reshape(-1), stats[2].reshape(-1)]).view(np.uint64))
    assert lines[len(utts) + 2] == f"checksum {int(x):x}"
