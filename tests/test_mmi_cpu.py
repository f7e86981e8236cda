"""The MMI restatement (tests/mmi_reference.py) pinned by itself: path enumeration, finite differences, a hand-computed EBW case,
and the criterion on a small synthetic task.  The GPU tests (tests/test_gpu_mmi.py) hold the library against the restatement."""
import numpy as np
import pytest

from speechrecognition_amd import synth
from tests import fb_reference as FB
from tests import mmi_reference as M
from tests import net_fb_reference as R
from tests.test_word_posteriors_cpu import _lex

# silence is word 0: one position, several positions
TINY = [[1, 3, 2], [2, 1, 3], [1, 2, 2, 1], [3, 2, 1, 4]]
PEN = ((1.0, 0.5, 2.0), 1.5)
DIM = 13
# test_one_ebw_step_raises_the_criterion: the smallest E of (1, 2, 4, 8) for which one EBW step raises sum(F_den - F_num) on
# criterion_task, found with the restatement alone; the GPU test takes its step at this E
CRITERION_E = 4.0


def _net(lex):
    word_off, aut, sil_state = lex.flatten()
    return R.Net(word_off, aut, lex.silence_idx, sil_state)


@pytest.mark.parametrize("li", range(len(TINY)))
def test_restatement_is_path_enumeration(li):
    """every network path with its word string: F_num(string) = -log of the string's mass / kappa, the masses of all strings sum to
    exp(-kappa F_den), occupancies = path-weighted emission counts on both networks, F_num >= F_den"""
    net = _net(_lex(TINY[li], 0))
    rng = np.random.default_rng(60 + li)
    tdp, wp = PEN
    for T in (1, 2, 4, 6 if net.W < 4 else 5):
        e = rng.uniform(0.0, 4.0, size=(T, net.state.max() + 1))
        for scale in (0.3, 1.0, 2.5):
            paths = M.enumerate_paths(e, net, tdp, wp, scale)
            total = sum(m for m, _ in paths.values())
            Fd, occ = M.occupancies(e, M.free_graph(net), tdp, wp, scale)
            assert abs(Fd + np.log(total) / scale) <= 1e-12 * max(1.0, abs(Fd))
            assert abs(Fd - R.posteriors(e, net, tdp, wp, scale)[0]) <= 1e-12 * max(1.0, abs(Fd))
            assert np.abs(occ - sum(c for _, c in paths.values()) / total).max() <= 1e-12
            assert np.abs(occ.sum(axis=1) - 1.0).max() <= 1e-12
            for string, (mass, cnt) in paths.items():
                Fn, on = M.occupancies(e, M.chain_graph(net, string), tdp, wp, scale)
                assert abs(Fn + np.log(mass) / scale) <= 1e-12 * max(1.0, abs(Fn)), (string, T)
                assert np.abs(on - cnt / mass).max() <= 1e-12
                assert Fn >= Fd - 1e-12 * abs(Fd)
            # a string no path spells: more words than frames
            Fn, on = M.occupancies(e, M.chain_graph(net, [1] * (T + 1)), tdp, wp, scale)
            assert Fn == np.inf and not on.any()


@pytest.mark.parametrize("li", range(len(TINY)))
def test_occupancy_is_the_gradient(li):
    """occ_t(k) = dF / d e(t, k) by central differences, on both networks (repeated states inside a word included)"""
    lex = _lex(TINY[li], 0)
    word_off, aut, sil_state = lex.flatten()
    aut = aut.copy()
    aut[-1] = aut[-2]  # the last word repeats a state
    net = R.Net(word_off, aut, 0, sil_state)
    rng = np.random.default_rng(80 + li)
    T, S, h = 9, lex.n_states, 1e-5
    e = rng.uniform(0.0, 4.0, size=(T, S))
    for graph in (M.free_graph(net), M.chain_graph(net, [1, net.W - 1, 1])):
        for scale in (0.4, 1.0):
            _, occ = M.occupancies(e, graph, PEN[0], PEN[1], scale)
            for t in range(T):
                for k in range(S):
                    d = np.zeros_like(e)
                    d[t, k] = h
                    g = (M.occupancies(e + d, graph, *PEN, scale)[0] - M.occupancies(e - d, graph, *PEN, scale)[0]) / (2 * h)
                    assert abs(g - occ[t, k]) <= 1e-8, (t, k, g, occ[t, k])


def test_ebw_hand_computed():
    """two densities in one dimension.  Density 0: mu = 1, var = 2, gn = 4, xn = 6, sn = 13, gd = 2, xd = 4, sd = 10, E = 2:
    D = max(4, 1e-10) = 4, mu' = (6 - 4 + 4) / (4 - 2 + 4) = 1, var' = (13 - 10 + 4 (2 + 1)) / 6 - 1 = 1.5.
    Density 1: mu = 0, var = 1, gn = 1, xn = 1, sn = 1, gd = 3, xd = 0, sd = 6, E = 1: D = max(3, 2 * 2 + 1e-10) = 4 + 1e-10,
    mu' = 1 / (2 + 1e-10), var' = (1 - 6 + D) / (2 + 1e-10) - mu'^2 < 0: D doubles to 8 + 2e-10 -> mu' = 1 / 6, var' = 3 / 6 - 1 / 36
    (up to the 1e-10).  With tau = 4 density 0's numerator is scaled by 2: gn = 8, xn = 12, sn = 26, D = 4:
    mu' = (12 - 4 + 4) / 10 = 1.2, var' = (26 - 10 + 12) / 10 - 1.44 = 1.36."""
    means, iv = np.array([[1.0], [0.0]]), np.array([[0.5], [1.0]])
    seed = 1e-4
    num = (np.array([[6.0], [1.0]]), np.array([4.0, 1.0]), np.array([[13.0 + seed], [1.0 + seed]]))
    den = (np.array([[4.0], [0.0]]), np.array([2.0, 3.0]), np.array([[10.0 + seed], [6.0 + seed]]))
    m, v = M.ebw_update(means, iv, num, den, 2.0, 0.0, 1e-3)
    assert abs(m[0, 0] - 1.0) <= 1e-12 and abs(v[0, 0] - 1.5) <= 1e-12
    m, v = M.ebw_update(means, iv, num, den, 1.0, 0.0, 1e-3)
    assert abs(m[1, 0] - 1 / 6) <= 1e-9 and abs(v[1, 0] - (0.5 - 1 / 36)) <= 1e-9
    m, v = M.ebw_update(means, iv, num, den, 2.0, 4.0, 1e-3)
    assert abs(m[0, 0] - 1.2) <= 1e-12 and abs(v[0, 0] - 1.36) <= 1e-12
    # a floor no doubling reaches is clamped to; an unseen density stays
    m, v = M.ebw_update(means, iv, num, den, 2.0, 0.0, 5.0)
    assert v[0, 0] == 5.0
    zero = (np.zeros((2, 1)), np.zeros(2), np.full((2, 1), seed))
    m, v = M.ebw_update(means, iv, zero, zero, 2.0, 0.0, 1e-3)
    assert np.array_equal(m, means) and np.array_equal(v, 1.0 / iv)


def criterion_task(tmp_path):
    """a small synthetic task with confusable words: -> (lex, spec, mixset path, feats, frame_off, transcripts, word penalty, kappa)"""
    lex = synth.make_lexicon(4, 3, 1)
    spec = synth.make_mixset(lex.n_states, 2, DIM, seed=900)
    mp = str(tmp_path / "crit.mix")
    synth.write_mixset(mp, spec)
    rng = np.random.default_rng(901)
    trans = [[int(w) for w in rng.integers(1, lex.n_words, size=3)] for _ in range(6)]
    utts = [synth.sample_utterance(spec, lex, ws, seed=902 + i, frames_per_state=(1, 3), noise=2.5) for i, ws in enumerate(trans)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    return lex, spec, mp, np.concatenate(utts), off, trans, 2.0, 0.1


def _scores(feats, means, inv_vars, norm, logw, mix_off):
    """emission costs [T, S] by the arg-min density (norm + dist / 2 - log weight)"""
    x = feats.astype(np.float64)
    d = ((x[:, None, :] - means[None]) ** 2 * inv_vars[None]).sum(axis=2) / 2 + norm[None] - logw[None]
    return np.stack([d[:, mix_off[s]:mix_off[s + 1]].min(axis=1) for s in range(len(mix_off) - 1)], axis=1)


def _criterion_and_statistics(net, feats, off, trans, wp, scale, tb, means, inv_vars, norm):
    items, crit = [[], []], 0.0
    e_all = _scores(feats, means, inv_vars, norm, tb["logw"], tb["mix_off"])
    for u, tr in enumerate(trans):
        e = e_all[int(off[u]):int(off[u + 1])]
        Fn, on = M.occupancies(e, M.chain_graph(net, tr), (3.0, 0.0, 30.0), wp, scale)
        Fd, od = M.occupancies(e, M.free_graph(net), (3.0, 0.0, 30.0), wp, scale)
        crit += Fd - Fn
        items[0] += M.frame_items(on)
        items[1] += M.frame_items(od)
    tables = dict(tb, means=means, vars_inv=inv_vars, norm=norm)
    C_ = len(means)
    return crit, [FB.accumulate(feats, it, tables, C_, C_, False, True) for it in items]


def test_one_ebw_step_raises_the_criterion(tmp_path, oracle_lib):
    """criterion_task under the restatement alone: sum(F_den - F_num) = -335.33 before the step; after one EBW step (tau = 0,
    var_floor = 1e-3) -546.67 at E = 1, -409.68 at E = 2, -203.50 at E = 4, -50.36 at E = 8.  The smallest E that raises it, 4, is
    CRITERION_E: the GPU test takes its step there."""
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    assert np.abs(_scores(feats, tb["means"], tb["vars_inv"], tb["norm"], tb["logw"], tb["mix_off"]) - o.score_matrix(feats)).max() <= 1e-9
    o.close()
    net = _net(lex)
    crit0, (num, den) = _criterion_and_statistics(net, feats, off, trans, wp, scale, tb, tb["means"], tb["vars_inv"], tb["norm"])
    assert crit0 < 0
    raised = {}
    for E in (1.0, 2.0, 4.0, 8.0):
        means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), E, 0.0, 1e-3)
        norm = (DIM * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
        raised[E] = _criterion_and_statistics(net, feats, off, trans, wp, scale, tb, means, 1.0 / var, norm)[0]
        print("E", E, crit0, raised[E])
    assert min(E for E, c in raised.items() if c > crit0) == CRITERION_E
