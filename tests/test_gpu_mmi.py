"""MMI training on the device: sr_net_occupancies_corpus, sr_mmi_statistics_corpus and sr_model_create_from_mmi_statistics against
the numpy restatement (tests/mmi_reference.py, pinned by tests/test_mmi_cpu.py), the word posteriors, the decoder and themselves.
Tolerances are those of test_gpu_word_posteriors.py / test_gpu_baum_welch.py: costs 1e-10 relative, occupancies 1e-9 absolute,
statistics 1e-9 relative to sum |w x|; costs and occupancies also, wherever that is tighter, by the measured rule against the
restatement's np.longdouble run (test_gpu_word_posteriors.Ref; the `RULE` lines say which of the two holds)."""
import contextlib
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import fb_reference as FB
from tests import mmi_reference as M
from tests import net_fb_reference as R
from tests import netfb_cases as nc
from tests.test_gpu_word_posteriors import Ref, _check_items
from tests.test_mmi_cpu import CRITERION_E, criterion_task
from tests.test_word_posteriors_cpu import _lex
from tests.util import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDP = (3.0, 0.0, 30.0)
DIM = 13
EINVAL, ELIMIT = -1, -4  # include/srgpu.h
# silence is word 0: one position, several positions, ragged word lengths up to 6
LEXICA = [[1, 3, 3, 2], [3, 1, 2, 4], [2, 4, 1, 6, 3], [1, 2]]


def _rel(a, b):
    if a == b:  # (both +inf: no path)
        return 0.0
    return abs(a - b) / max(1.0, abs(b))


def _geq(a, b):
    """a >= b up to the costs' tolerance (+inf on both sides: no path through either network)"""
    return a == b or a >= b - 1e-10 * abs(b)


def _model(tmp_path, S, seed, Mx=2, dim=DIM):
    spec = synth.make_mixset(S, Mx, dim, seed=seed)
    mp = str(tmp_path / f"m{seed}.mix")
    synth.write_mixset(mp, spec)
    return spec, mp


def _net(lex):
    word_off, aut, sil_state = lex.flatten()
    return R.Net(word_off, aut, lex.silence_idx, sil_state)


def _capi_lex(m, lex, tdp=TDP):
    word_off, aut, sil_state = lex.flatten()
    return contextlib.closing(capi.Lexicon(m, word_off, aut, lex.silence_idx, tdp, sil_state))


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _refs(o, net, feats, off, trans, tdp, wp, scale):
    """per utterance ((F_num, occ_num), (F_den, occ_den)) of the restatement"""
    out = []
    for u in range(len(off) - 1):
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        out.append(tuple(_ref(e, g, tdp, wp, scale, f"{side} scale {scale} utterance {u} (T {len(e)})")
                         for side, g in (("chain", M.chain_graph(net, trans[u])), ("free", M.free_graph(net)))))
    return out


def _ref(e, graph, tdp, wp, scale, tag=None):
    with np.errstate(all="ignore"):
        return Ref(M.occupancies(e, graph, tdp, wp, scale), M.occupancies(e, graph, tdp, wp, scale, dtype=nc.LD), tag)


def _check_stats(got, feats, items, tables, max_approx):
    nm, nv = len(got[1]), len(got[3])
    ma, mw, va, vw, sm, sv = FB.accumulate(feats, items, tables, nm, nv, False, max_approx)
    assert np.all(np.abs(got[0] - ma) <= 1e-9 * np.maximum(sm, 1e-300))
    assert np.all(np.abs(got[2] - va) <= 1e-9 * np.maximum(sv, 1e-4))
    assert np.all(np.abs(got[1] - mw) <= 1e-9 * np.maximum(mw, 1e-300)) and np.all(np.abs(got[3] - vw) <= 1e-9 * np.maximum(vw, 1e-300))


def _against_restatement(o, m, lex, feats, off, trans, tdp, wp, scale, floors=(0.0, 1e-6), stats=True):
    """F_num, F_den, the occupancy items of both networks and both statistics sets"""
    net = _net(lex)
    S = lex.n_states
    refs = _refs(o, net, feats, off, trans, tdp, wp, scale)
    tables = o.tables()
    with _capi_lex(m, lex, tdp) as L:
        corpus = m.upload(feats, off)
        for side, tr in ((0, trans), (1, None)):
            for floor in floors:
                for K in (1, 3, S):
                    cost, count, state, weight = corpus.net_occupancies(L, wp, scale, tr, capi.GMM_PREFILTER, floor, K)
                    for u, ref in enumerate(refs):
                        r = ref[side]
                        F, occ = r
                        print("cost", side, u, cost[u], F)
                        assert _rel(cost[u], F) <= 1e-10, (side, u, cost[u], F)
                        assert r.holds_F(cost[u]), (side, u, cost[u], r.F80, r.tolF)
                        for t in range(occ.shape[0]):
                            ft = int(off[u]) + t
                            _check_items(occ[t], count[ft], state[ft], weight[ft], floor, K, r.p80[t], r.tol[t])
                            if K == S and floor == 0.0 and np.isfinite(F):
                                assert abs(weight[ft].sum() - 1.0) <= 1e-8
        if stats:
            for max_approx, floor in ((True, 0.0), (False, 1e-6)):
                fn, fd, num, den = corpus.mmi_statistics(L, wp, trans, scale, capi.GMM_PREFILTER, floor, max_approx)
                items = [[], []]
                for u, ref in enumerate(refs):
                    assert _rel(fn[u], ref[0][0]) <= 1e-10 and _rel(fd[u], ref[1][0]) <= 1e-10
                    assert ref[0].holds_F(fn[u]) and ref[1].holds_F(fd[u])
                    assert _geq(fn[u], fd[u])
                    for side in (0, 1):  # an utterance without a numerator path contributes to neither side
                        occ = ref[side][1] if np.isfinite(ref[0][0]) else np.zeros_like(ref[side][1])
                        items[side] += M.frame_items(occ, floor)
                _check_stats(num, feats, items[0], tables, max_approx)
                _check_stats(den, feats, items[1], tables, max_approx)
        corpus.close()
    return refs


def _long_chain_case():
    """(lexicon, transcripts, frame counts): 24 words of three fresh states each; the first transcript names them all"""
    return _lex([1] + [3] * 24, 0), [list(range(1, 25)), [2, 1]], [90, 12]


def test_chain_of_more_than_64_mixtures(tmp_path, oracle_lib):
    """a transcript whose chain carries 73 distinct mixtures: in chain mode the item kernel's lanes take them in two rounds of 64.  The
    reference alone says that mixtures of sorted rank >= 64 within the chain hold occupancy in at least 10 frames."""
    lex, trans, lens = _long_chain_case()
    spec, mp = _model(tmp_path, lex.n_states, 760)
    feats = synth.make_features(sum(lens), DIM, seed=761)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    with capi.Model.from_mixset(mp, DIM) as m:
        refs = _against_restatement(o, m, lex, feats, _off(lens), trans, TDP, 10.0, 0.3, floors=(0.0, 1e-6), stats=False)
    o.close()
    F, occ = refs[0][0]
    chain_mix = np.unique(M.chain_graph(_net(lex), trans[0]).state)
    assert np.isfinite(F) and len(chain_mix) == 73
    late = sum(bool((occ[t, chain_mix[64:]] > 0).any()) for t in range(lens[0]))
    print("frames with occupancy on a mixture of rank >= 64:", late)
    assert late >= 10


@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_against_restatement(li, tmp_path, oracle_lib):
    """ragged lexica with a one- and a multi-position silence; a T = 1 utterance, an empty transcript, a transcript too long for
    its utterance (F_num = +inf, no contribution to either side), repeated words; two penalty sets and scales"""
    lex = _lex(LEXICA[li], 0)
    W = lex.n_words
    spec, mp = _model(tmp_path, lex.n_states, 700 + li)
    lens = [1, 2, 17, 40, 9]
    rng = np.random.default_rng(710 + li)
    trans = [[], [1], list(rng.integers(1, W, size=4)), list(rng.integers(1, W, size=7)), [1] * 12]
    feats = synth.make_features(sum(lens), DIM, seed=702 + li)
    off = _off(lens)
    for tdp, wp, scale in ((TDP, 10.0, 1.0), ((3.0, 0.0, np.inf), 4.0, 0.3)):
        o = oracle_lib.Oracle(mp, DIM, lex, tdp=tdp)
        with capi.Model.from_mixset(mp, DIM) as m:
            refs = _against_restatement(o, m, lex, feats, off, trans, tdp, wp, scale)
        assert refs[4][0][0] == np.inf and np.isfinite(refs[4][1][0])
        o.close()


@pytest.mark.parametrize("name", ["sietill_lexicon_d25", "ragged_words"])
def test_golden_lexica(name, tmp_path, oracle_lib):
    """the goldens' lexica (repeated states inside a word: slots of one word share a mixture), the recognised words as transcript"""
    case = Case(name, tmp_path)
    o = case.oracle(oracle_lib)
    T = len(case.feats)
    cut = T // 3
    off = np.array([0, cut, T], np.uint64)
    words = [int(w) for w in case.z["words"]]
    trans = [words[:1], words]
    with capi.Model.from_mixset(case.mixset_path, case.dim, case.pooling, case.max_approx) as m:
        for scale in (1.0, 0.1):
            _against_restatement(o, m, case.lex, case.feats, off, trans, case.tdp, case.wp, scale, floors=(0.0,),
                                 stats=(case.pooling == capi.POOL_NONE and scale == 1.0))
    o.close()


def test_free_occupancies_sum_to_word_posteriors(tmp_path):
    """no mixture shared between words: the free network's occupancies summed over a word's mixtures are its posterior"""
    lex = _lex([2, 4, 1, 6, 3], 0)
    word_off, aut, _ = lex.flatten()
    spec, mp = _model(tmp_path, lex.n_states, 720)
    lens = [30, 75, 3]
    feats = synth.make_features(sum(lens), DIM, seed=721)
    off = _off(lens)
    S, W = lex.n_states, lex.n_words
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        for scale in (1.0, 0.2):
            cw, nw, word, pw = corpus.word_posteriors(L, 6.0, scale, capi.GMM_PREFILTER, 0.0, W)
            co, no, state, occ = corpus.net_occupancies(L, 6.0, scale, None, capi.GMM_PREFILTER, 0.0, S)
            assert np.array_equal(cw.view(np.uint64), co.view(np.uint64))
            for t in range(len(feats)):
                p, q = np.zeros(W), np.zeros(S)
                p[word[t, :nw[t]]] = pw[t, :nw[t]]
                q[state[t, :no[t]]] = occ[t, :no[t]]
                for w in range(W):
                    assert abs(q[aut[word_off[w]:word_off[w + 1]]].sum() - p[w]) <= 1e-9
                assert abs(q.sum() - 1.0) <= 1e-8
        corpus.close()


# ---- several launch groups (SRGPU_FB_MB) -------------------------------------------------------------------------------------------
MULTI_LENS = [150, 200, 420, 130, 110, 300, 180]


def launch_groups(nbytes, budget=1 << 20):
    """the launch groups of one scoring chunk: a group takes its first utterance, then the next ones while the sum stays in the budget"""
    groups, u = [], 0
    while u < len(nbytes):
        v, total = u + 1, nbytes[u]
        while v < len(nbytes) and total + nbytes[v] <= budget:
            total += nbytes[v]
            v += 1
        groups.append((u, v))
        u = v
    return groups


def several_groups(nbytes):
    """the precondition of the multi-group tests: every utterance fits 1 MiB alone; at least three groups, one of a single utterance
    and one of several"""
    assert max(nbytes) < 1 << 20
    groups = launch_groups(nbytes)
    sizes = [b - a for a, b in groups]
    assert len(groups) >= 3 and 1 in sizes and max(sizes) > 1, groups
    return groups


def _multi_group_outputs(mp, lex, feats, off, trans, wp, scale):
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:  # (the budget is read when the model is made)
        corpus = m.upload(feats, off)
        free = corpus.net_occupancies(L, wp, scale, None, capi.GMM_PREFILTER, 1e-6, 3)
        chain = corpus.net_occupancies(L, wp, scale, trans, capi.GMM_PREFILTER, 1e-6, 3)
        fn, fd, num, den = corpus.mmi_statistics(L, wp, trans, scale, capi.GMM_PREFILTER, 1e-6, False)
        corpus.close()
    return dict(free=free, chain=chain, stats=[fn, fd, *num, *den])


def test_several_launch_groups(tmp_path, oracle_lib, monkeypatch):
    """7 utterances that one launch takes at the default budget and that SRGPU_FB_MB=1 cuts into groups of one and of several, the
    free network (8 P T bytes) and the chains (8 N_u T_u) differently: equal bytes either way -- an utterance is one workgroup's
    work and the items are in frame order -- and, for an utterance that is not the first of its group, the restatement's F and
    occupancies"""
    lex = _lex([1] + [6] * 50, 0)
    word_off, aut, _ = lex.flatten()
    P, W = len(aut), lex.n_words
    rng = np.random.default_rng(771)
    n_words = [20, 30, 40, 10, 14, 40, 30]
    trans = [list(rng.integers(1, W, size=n)) for n in n_words]
    free_groups = several_groups([8 * P * T for T in MULTI_LENS])
    chain_groups = several_groups([8 * (7 * n + 1) * T for n, T in zip(n_words, MULTI_LENS)])   # a word: 6 positions and a silence
    assert free_groups == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 7)] and chain_groups == [(0, 2), (2, 4), (4, 6), (6, 7)]
    spec, mp = _model(tmp_path, lex.n_states, 770)
    feats = synth.make_features(sum(MULTI_LENS), DIM, seed=772)
    off = _off(MULTI_LENS)
    wp, scale = 10.0, 0.5
    monkeypatch.delenv("SRGPU_FB_MB", raising=False)
    one = _multi_group_outputs(mp, lex, feats, off, trans, wp, scale)
    monkeypatch.setenv("SRGPU_FB_MB", "1")
    cut = _multi_group_outputs(mp, lex, feats, off, trans, wp, scale)
    for k in one:
        for a, b in zip(one[k], cut[k]):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), k
    assert np.isfinite(cut["stats"][0]).all() and np.isfinite(cut["stats"][1]).all()
    # utterance 4 is the second of the free network's group (3, 5), utterance 3 the second of the chains' (2, 4)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    net = _net(lex)
    for key, u, graph in (("free", 4, M.free_graph(net)), ("chain", 3, M.chain_graph(net, trans[3]))):
        a, b = int(off[u]), int(off[u + 1])
        r = _ref(o.score_matrix(feats[a:b]), graph, TDP, wp, scale, f"several groups {key} utterance {u}")
        F, occ = r
        cost, count, state, weight = cut[key]
        print("several groups", key, u, cost[u], F)
        assert _rel(cost[u], F) <= 1e-10 and r.holds_F(cost[u])
        for t in range(b - a):
            _check_items(occ[t], count[a + t], state[a + t], weight[a + t], 1e-6, 3, r.p80[t], r.tol[t])
    o.close()


def _recognition_case(tmp_path, seed, n_words=6, n_utts=6):
    lex = synth.make_lexicon(n_words, 3, 2)
    spec, mp = _model(tmp_path, lex.n_states, seed, Mx=3)
    rng = np.random.default_rng(seed + 1)
    trans = [list(rng.integers(1, lex.n_words, size=int(rng.integers(1, 5)))) for _ in range(n_utts)]
    utts = [synth.sample_utterance(spec, lex, ws, seed=seed + 2 + i, noise=1.2) for i, ws in enumerate(trans)]
    return lex, spec, mp, np.concatenate(utts), _off([len(f) for f in utts]), trans


def test_ordering_and_viterbi_bound(tmp_path):
    """F_num >= F_den; with V = the decoder's best cost at a beam too wide to prune and at most (2 W + 3)^T paths,
    V - T log(2 W + 3) / kappa <= F_den <= V, and the same for F_num with the recognised words as transcript"""
    lex, spec, mp, feats, off, trans = _recognition_case(tmp_path, 730)
    W = lex.n_words
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        words, woff, (tbs, _, _) = corpus.recognize(L, 1e30, 10.0, capi.GMM_PREFILTER, traceback=True)
        hyp = [list(words[int(woff[u]):int(woff[u + 1])]) for u in range(len(off) - 1)]
        for scale in (1.0, 50.0):
            fd = corpus.net_occupancies(L, 10.0, scale, None, capi.GMM_PREFILTER, 0.0, 4)[0]
            fh = corpus.net_occupancies(L, 10.0, scale, hyp, capi.GMM_PREFILTER, 0.0, 4)[0]
            fn = corpus.net_occupancies(L, 10.0, scale, trans, capi.GMM_PREFILTER, 0.0, 4)[0]
            for u in range(len(off) - 1):
                T = int(off[u + 1] - off[u])
                V = float(tbs[int(off[u + 1]) + u])
                slack = 1e-10 * abs(V)
                print("bound", scale, u, V, fd[u], fh[u], fn[u])
                assert V - T * np.log(2 * W + 3) / scale - slack <= fd[u] <= V + slack
                assert V - T * np.log(2 * W + 3) / scale - slack <= fh[u] <= V + slack
                assert _geq(fh[u], fd[u]) and _geq(fn[u], fd[u])
        corpus.close()


def test_determinism_and_shards(tmp_path):
    """two identical calls return identical bits; the statistics of two half-corpora add up to the whole (the 1e-4 seed once per
    call and side)"""
    lex, spec, mp, feats, off, trans = _recognition_case(tmp_path, 740, n_utts=8)
    trans[3] = [1] * 200  # no path: gated out of both sides
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        runs = [corpus.mmi_statistics(L, 10.0, trans, 0.5, capi.GMM_PREFILTER, 1e-8, False) for _ in range(2)]
        occs = [corpus.net_occupancies(L, 10.0, 0.5, tr, capi.GMM_PREFILTER, 0.0, 5) for tr in (trans, trans, None, None)]
        corpus.close()
        flat = lambda r: [r[0], r[1], *r[2], *r[3]]
        for a, b in zip(flat(runs[0]), flat(runs[1])):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for i in (0, 2):
            for a, b in zip(occs[i], occs[i + 1]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert runs[0][0][3] == np.inf
        halves = []
        for u0, u1 in ((0, 4), (4, 8)):
            f0, f1 = int(off[u0]), int(off[u1])
            part = m.upload(feats[f0:f1], off[u0:u1 + 1] - off[u0])
            halves.append(part.mmi_statistics(L, 10.0, trans[u0:u1], 0.5, capi.GMM_PREFILTER, 1e-8, False))
            part.close()
    for side in (2, 3):
        whole, a, b = runs[0][side], halves[0][side], halves[1][side]
        for i in (1, 3):  # gn / gd
            assert np.all(np.abs(a[i] + b[i] - whole[i]) <= 1e-12 * np.maximum(np.abs(whole[i]), 1e-300))
        assert np.all(np.abs(a[0] + b[0] - whole[0]) <= 1e-9 * np.maximum(np.abs(a[0]) + np.abs(b[0]), 1e-300))
        assert np.all(np.abs(a[2] + b[2] - 1e-4 - whole[2]) <= 1e-9 * np.maximum(np.abs(whole[2]), 1e-4))
    assert np.array_equal(np.concatenate([halves[0][0], halves[1][0]]).view(np.uint64), runs[0][0].view(np.uint64))


def test_ebw_tables_and_criterion(tmp_path, oracle_lib):
    """the device model after one EBW step scores like the restatement's update (every density's score of probe frames, which
    fixes its mean, variance and norm, within 1e-12 relative), and the step raises the criterion as on the CPU"""
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    o.close()
    C_, D = tb["means"].shape
    assert np.array_equal(tb["mix_mean"], np.arange(C_)) and np.array_equal(tb["mix_var"], np.arange(C_))
    probe = np.random.default_rng(751).standard_normal((64, D)).astype(np.float32) * 2.0
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        fn, fd, num, den = corpus.mmi_statistics(L, wp, trans, scale, capi.GMM_PREFILTER, 0.0, True)
        for E, tau, vf in ((CRITERION_E, 0.0, 1e-3), (0.5, 20.0, 0.3)):
            means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), E, tau, vf)
            norm = (D * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
            with m.from_mmi_statistics(num, den, E, tau, vf) as m2, \
                    capi.Model.from_tables(tb["mix_off"], means, 1.0 / var, norm, tb["logw"]) as mr:
                got = m2.score_frames(probe, capi.GMM_EXACT)
                want = mr.score_frames(probe, capi.GMM_EXACT)
                assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
                assert [np.array_equal(a, b) for a, b in zip(m2.topology(), m.topology())] == [True] * 3
                if tau == 0.0:
                    with _capi_lex(m2, lex) as L2:
                        c2 = m2.upload(feats, off)
                        fn2, fd2, _, _ = c2.mmi_statistics(L2, wp, trans, scale, capi.GMM_PREFILTER, 0.0, True)
                        c2.close()
                    print("criterion", (fd - fn).sum(), (fd2 - fn2).sum())
                    assert (fd2 - fn2).sum() > (fd - fn).sum()
        corpus.close()


def test_errors(tmp_path):
    """every SR_EINVAL / SR_ELIMIT of the three entry points; all checks precede any launch"""
    lex = _lex([1, 3, 3, 2], 0)
    spec, mp = _model(tmp_path, lex.n_states, 760)
    feats = synth.make_features(20, DIM, seed=761)
    off = _off([12, 8])
    L_ = capi.lib()
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
        cost = np.zeros(2)
        cnt, st, wt = np.zeros(20, np.uint16), np.zeros((20, 2), np.uint16), np.zeros((20, 2))
        tr, toff = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint64)
        P = capi._ptr

        def occ(trans=tr, trans_off=toff, scale=1.0, floor=0.0, K=2, lexh=L.h, out=(cost, cnt, st, wt), spp=sp):
            return L_.sr_net_occupancies_corpus(m.h, corpus.h, lexh, C.byref(spp), scale, floor, K, P(trans), P(trans_off), *[P(a) for a in out])

        assert occ() == 0
        assert occ(trans=None) == EINVAL                                         # a partial transcript pair
        assert occ(trans_off=None) == EINVAL                                     # a partial transcript pair
        assert occ(trans=np.array([1, 4, 3], np.uint32)) == EINVAL               # word id >= n_words
        assert occ(trans=np.array([1, 0, 3], np.uint32)) == EINVAL               # the silence word
        assert occ(trans_off=np.array([1, 2, 3], np.uint64)) == EINVAL           # trans_off[0] != 0
        assert occ(trans_off=np.array([0, 3, 2], np.uint64)) == EINVAL           # decreasing
        assert occ(scale=0.0) == EINVAL and occ(scale=np.inf) == EINVAL and occ(floor=-1.0) == EINVAL
        assert occ(K=0) == EINVAL and occ(out=(cost, cnt, None, wt)) == EINVAL and occ(out=(None, cnt, st, wt)) == EINVAL
        assert occ(spp=capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 1)) == EINVAL
        assert occ(out=(cost, None, None, None)) == 0                            # costs alone
        # a chain beyond the position limit: 2800 words of 3 positions
        long_tr = np.ones(2800, np.uint32)
        assert occ(trans=long_tr, trans_off=np.array([0, 2800, 2800], np.uint64)) == ELIMIT and b"chain" in L_.sr_last_error()
        # word 0 is not the silence word
        lex2 = _lex([3, 1, 2, 3], 1)
        with _capi_lex(m, lex2) as L2:
            assert occ(lexh=L2.h) == EINVAL
            assert occ(lexh=L2.h, trans=None, trans_off=None) == 0               # the free network does not mind
        stats = [np.zeros((m.n_densities, DIM)), np.zeros(m.n_densities), np.zeros((m.n_densities, DIM)), np.zeros(m.n_densities)]
        fn, fd = np.zeros(2), np.zeros(2)

        def mmi(trans=tr, trans_off=toff, outs=None):
            outs = outs if outs is not None else [fn, fd] + stats + [a.copy() for a in stats]
            return L_.sr_mmi_statistics_corpus(m.h, corpus.h, L.h, C.byref(sp), 1.0, 0.0, 1, P(trans), P(trans_off), *[P(a) for a in outs])

        assert mmi() == 0
        assert mmi(trans=None, trans_off=None) == EINVAL                         # needs the transcripts
        assert mmi(outs=[fn, None] + stats + stats) == EINVAL and mmi(outs=[fn, fd] + stats + stats[:3] + [None]) == EINVAL
        num = den = tuple(stats)

        def ebw(E=2.0, tau=0.0, vf=1e-3, model=m, n=num):
            h = C.c_void_p()
            rc = L_.sr_model_create_from_mmi_statistics(model.h, *[P(a) for a in n + den], E, tau, vf, C.byref(h))
            if rc == 0:
                L_.sr_model_destroy(h)
            return rc

        assert ebw() == 0
        for kw in (dict(E=0.0), dict(E=-1.0), dict(E=np.inf), dict(E=np.nan), dict(tau=-1.0), dict(tau=np.inf), dict(tau=np.nan),
                   dict(vf=0.0), dict(vf=-1.0), dict(vf=np.inf), dict(vf=np.nan), dict(n=(None,) + num[1:])):
            assert ebw(**kw) == EINVAL, kw
        corpus.close()
    # a tied model: pooled variances
    with capi.Model.from_mixset(mp, DIM, capi.POOL_MIXTURE) as mt:
        nmr, nvr = C.c_uint32(), C.c_uint32()
        L_.sr_model_tying_info(mt.h, C.byref(nmr), C.byref(nvr))
        tied = (np.zeros((nmr.value, DIM)), np.zeros(nmr.value), np.zeros((nvr.value, DIM)), np.zeros(nvr.value))
        h = C.c_void_p()
        if nvr.value != mt.n_densities:
            assert L_.sr_model_create_from_mmi_statistics(mt.h, *[P(a) for a in tied + tied], 2.0, 0.0, 1e-3, C.byref(h)) == EINVAL


def test_cpp_driver(tmp_path):
    """sr::Trainer::mmi_iteration from C++ (tests/cpp/mmi_driver.cpp): its objective before and after one iteration is the Python
    binding's, and the iteration lowers it"""
    exe = str(tmp_path / "mmi_driver")
    lib_dir = os.path.join(ROOT, "speechrecognition_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mmi_driver.cpp"),
                    "-o", exe, "-L", lib_dir, "-lsrgpu", "-Wl,-rpath," + lib_dir], check=True)
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    inp = str(tmp_path / "case.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", lex.n_words))
        for n, r in zip(lex.word_states, lex.word_reps):
            f.write(struct.pack("<HH", int(n), int(r)))
        f.write(struct.pack("<I3d4d", lex.silence_idx, *TDP, wp, scale, CRITERION_E, 0.0))
        f.write(struct.pack("<I", len(trans)))
        for u, tr in enumerate(trans):
            x = np.ascontiguousarray(feats[int(off[u]):int(off[u + 1])], np.float32)
            f.write(struct.pack(f"<I{len(tr)}II", len(tr), *tr, len(x)))
            f.write(x.tobytes())
    r = subprocess.run([exe, "mmi", mp, str(DIM), inp], check=True, capture_output=True, text=True)
    obj = [struct.unpack("<d", struct.pack("<Q", int(line.split()[2], 16)))[0] for line in r.stdout.splitlines() if line.startswith("objective")]
    assert len(obj) == 2, r.stdout
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        fn, fd, num, den = corpus.mmi_statistics(L, wp, trans, scale, capi.GMM_DEFAULT, 0.0, True)
        corpus.close()
        assert abs(obj[0] - (fn - fd).sum()) <= 1e-10 * abs(obj[0])
        with m.from_mmi_statistics(num, den, CRITERION_E, 0.0, 1e-3) as m2, _capi_lex(m2, lex) as L2:
            c2 = m2.upload(feats, off)
            fn2, fd2, _, _ = c2.mmi_statistics(L2, wp, trans, scale, capi.GMM_DEFAULT, 0.0, True)
            c2.close()
        assert abs(obj[1] - (fn2 - fd2).sum()) <= 1e-10 * abs(obj[1])
    assert 0 <= obj[1] < obj[0]
