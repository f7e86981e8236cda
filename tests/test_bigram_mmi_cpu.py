"""The bigram MMI restatement (tests/bigram_mmi_reference.py) pinned by itself: path enumeration keyed by word entries, finite
differences, and the criterion on a small sampled task.  The GPU tests (tests/test_gpu_bigram_mmi.py) hold the library against it."""
import numpy as np
import pytest

from speechrecognition_amd import synth
from tests import bigram_fb_reference as R
from tests import bigram_mmi_reference as BM
from tests import fb_reference as FB
from tests import mmi_reference as M
from tests.test_mmi_cpu import _scores

# (states per word, silence word, mixtures or None = one of its own per state): a one-state silence with one-state words, a
# multi-state silence that is not word 0 with ragged words, a two-state silence with a mixture shared between two words
TINY = [([1, 1, 1], 0, None), ([2, 3, 1], 1, None), ([2, 1, 2], 0, [0, 1, 2, 3, 2])]
TDP = np.array([[1.0, 0.5, 2.0, 0.7], [0.3, 0.2, 1.5, 0.4]])
DIM = 12
# test_one_ebw_step_raises_the_criterion: the smallest E of (1, 2, 4, 8) for which one EBW step raises sum(F_den - F_num) on
# criterion_task, found with the restatement alone; the GPU test takes its step at this E
CRITERION_E = 8.0
CRITERION_TDP = np.array([[3.0, 0.0, 30.0, 5.0], [1.0, 0.0, 40.0, 2.0]], np.float32)


def _tiny(li):
    lens, sil, mix = TINY[li]
    word_off = np.concatenate([[0], np.cumsum(lens)])
    mix = np.arange(word_off[-1]) if mix is None else np.asarray(mix)
    net = R.Net(word_off, mix, sil)
    rng = np.random.default_rng(300 + li)
    lm = rng.uniform(0.2, 3.0, size=(net.W, net.W))
    a, b = [w for w in range(net.W) if w != sil]
    lm[b, a] = np.nan    # b never follows a
    lm[a, b] = np.inf    # a never follows b
    return net, lm, int(mix.max()) + 1, (a, b)


def _close(x, y):
    return abs(x - y) <= 1e-12 * max(1.0, abs(y))


@pytest.mark.parametrize("li", range(len(TINY)))
def test_chain_is_path_enumeration(li):
    """every path of the free network under its sequence of word entries: the chain's F and occupancies are the key's mass and
    path-weighted emission counts, the masses sum to the free network's, the free occupancies are the summed counts, F_num >= F_den;
    the empty transcript, a repeated word and a transcript through a forbidden LM entry included"""
    net, lm, S, (a, b) = _tiny(li)
    rng = np.random.default_rng(310 + li)
    seen = set()
    for T in (1, 2, 4, 5):
        e = rng.uniform(0.0, 4.0, size=(T, S))
        for scale in (0.4, 1.0, 2.5):
            paths = BM.enumerate_paths(e, net, lm, TDP, scale)
            seen |= set(paths)
            total = sum(m for m, _ in paths.values())
            Fd, occ = BM.free_occupancies(e, net, lm, TDP, scale)
            assert _close(Fd, -np.log(total) / scale)
            assert _close(Fd, R.posteriors(e, net, lm, TDP, scale)[0])
            assert np.abs(occ - sum(c for _, c in paths.values()) / total).max() <= 1e-12
            assert np.abs(occ.sum(axis=1) - 1.0).max() <= 1e-12
            for key, (mass, cnt) in paths.items():
                Fn, on = BM.chain_occupancies(e, net, lm, TDP, key, scale)
                assert _close(Fn, -np.log(mass) / scale), (key, T)
                assert np.abs(on - cnt / mass).max() <= 1e-12, (key, T)
                assert Fn >= Fd - 1e-12 * abs(Fd)
            for bad in ([a, b], [b, a], [a, a, b], [a] * (T + 1)):  # forbidden LM entries (NaN, +inf); more words than frames
                assert tuple(bad) not in paths
                Fn, on = BM.chain_occupancies(e, net, lm, TDP, bad, scale)
                assert Fn == np.inf and not on.any()
    assert () in seen and (a,) in seen and (a, a) in seen and (b, b) in seen
    for n_words, want in ((0, 0.0), (1, np.inf)):  # no frames
        Fn, on = BM.chain_occupancies(np.zeros((0, S)), net, lm, TDP, [a] * n_words, 1.0)
        assert Fn == want and on.shape == (0, S)
    assert BM.free_occupancies(np.zeros((0, S)), net, lm, TDP, 1.0)[0] == 0.0


@pytest.mark.parametrize("li", range(len(TINY)))
def test_occupancy_is_the_gradient(li):
    """occ_t(k) = dF / d e(t, k) by central differences, on both networks (a mixture shared between words included)"""
    net, lm, S, (a, b) = _tiny(li)
    lm = np.where(np.isfinite(lm), lm, 1.3)  # (every transition allowed: the chain visits both words)
    rng = np.random.default_rng(320 + li)
    T, h = 7, 1e-5
    e = rng.uniform(0.0, 4.0, size=(T, S))
    nets = (lambda x, k: BM.free_occupancies(x, net, lm, TDP, k), lambda x, k: BM.chain_occupancies(x, net, lm, TDP, [a, a, b, b], k))
    for f in nets:
        for scale in (0.4, 1.0):
            F, occ = f(e, scale)
            assert np.isfinite(F)
            for t in range(T):
                for k in range(S):
                    d = np.zeros_like(e)
                    d[t, k] = h
                    g = (f(e + d, scale)[0] - f(e - d, scale)[0]) / (2 * h)
                    assert abs(g - occ[t, k]) <= 1e-8, (t, k, g, occ[t, k])


def criterion_task(tmp_path):
    """a small sampled task with confusable words and a bigram LM: -> (lex, mixset path, word_off, mixtures, lm, tdp, feats,
    frame_off, transcripts, kappa)"""
    lex = synth.make_lexicon(4, 3, 1)
    spec = synth.make_mixset(lex.n_states, 2, DIM, seed=910)
    mp = str(tmp_path / "bgcrit.mix")
    synth.write_mixset(mp, spec)
    word_off, mixtures, _ = lex.flatten()
    rng = np.random.default_rng(911)
    p = rng.dirichlet(np.ones(lex.n_words), size=lex.n_words)
    lm = (-np.log(p)).T.astype(np.float32).copy()
    trans = [[int(w) for w in rng.integers(1, lex.n_words, size=3)] for _ in range(6)]
    utts = [synth.sample_utterance(spec, lex, ws, seed=912 + i, frames_per_state=(1, 3), noise=2.5) for i, ws in enumerate(trans)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    return lex, mp, word_off, mixtures, lm, CRITERION_TDP, np.concatenate(utts), off, trans, 0.1


def _criterion_and_statistics(net, lm, tdp, feats, off, trans, scale, tb, means, inv_vars, norm):
    items, crit = [[], []], 0.0
    e_all = _scores(feats, means, inv_vars, norm, tb["logw"], tb["mix_off"])
    for u, tr in enumerate(trans):
        e = e_all[int(off[u]):int(off[u + 1])]
        Fn, on = BM.chain_occupancies(e, net, lm, tdp, tr, scale)
        Fd, od = BM.free_occupancies(e, net, lm, tdp, scale)
        crit += Fd - Fn
        items[0] += BM.frame_items(on)
        items[1] += BM.frame_items(od)
    tables = dict(tb, means=means, vars_inv=inv_vars, norm=norm)
    C_ = len(means)
    return crit, [FB.accumulate(feats, it, tables, C_, C_, False, True) for it in items]


def test_one_ebw_step_raises_the_criterion(tmp_path, oracle_lib):
    """criterion_task under the restatement alone: sum(F_den - F_num) = -173.90 before the step; after one EBW step (tau = 0,
    var_floor = 1e-3) -855.61 at E = 1, -565.65 at E = 2, -332.33 at E = 4, -145.38 at E = 8.  The smallest E that raises it, 8, is
    CRITERION_E: the GPU test takes its step there."""
    lex, mp, word_off, mixtures, lm, tdp, feats, off, trans, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    assert np.abs(_scores(feats, tb["means"], tb["vars_inv"], tb["norm"], tb["logw"], tb["mix_off"]) - o.score_matrix(feats)).max() <= 1e-9
    o.close()
    net = R.Net(word_off, mixtures, lex.silence_idx)
    crit0, (num, den) = _criterion_and_statistics(net, lm, tdp, feats, off, trans, scale, tb, tb["means"], tb["vars_inv"], tb["norm"])
    assert crit0 < 0
    raised = {}
    for E in (1.0, 2.0, 4.0, 8.0):
        means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), E, 0.0, 1e-3)
        norm = (DIM * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
        raised[E] = _criterion_and_statistics(net, lm, tdp, feats, off, trans, scale, tb, means, 1.0 / var, norm)[0]
        print("E", E, crit0, raised[E])
    assert min(E for E, c in raised.items() if c > crit0) == CRITERION_E
