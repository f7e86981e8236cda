"""sMBR training on the device: sr_net_accuracies_corpus and sr_smbr_statistics_corpus against the numpy restatement
(tests/smbr_reference.py, pinned by tests/test_smbr_cpu.py), sr_net_occupancies_corpus and themselves.  Tolerances: costs 1e-10
relative; Abar and every gamma 1e-9 (1 + T_u) absolute -- the project's 1e-9 occupancy tolerance times the range of c - Abar --;
statistics 1e-9 relative to sum |w x| (test_gpu_mmi._check_stats).  F, Abar, every gamma and a frame's sum also, wherever that is
tighter, by the measured rule of tests/test_gpu_smbr_scores.py against the restatement's np.longdouble run (Rule below; the `RULE` lines
say which of the two holds)."""
import ctypes as C

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import mmi_reference as M
from tests import netfb_cases as nc
from tests import smbr_reference as SM
from tests.test_gpu_mmi import DIM, EINVAL, ELIMIT, LEXICA, MULTI_LENS, TDP, _capi_lex, _check_stats, _model, _net, _off, _rel, several_groups
from tests.test_mmi_cpu import criterion_task
from tests.test_smbr_cpu import SMBR_E, criterion_refs
from tests.test_word_posteriors_cpu import _lex

pytestmark = pytest.mark.gpu

LENS = [1, 2, 17, 40, 9]
PENALTIES = ((TDP, 10.0, 1.0), ((3.0, 0.0, np.inf), 4.0, 0.3))


def _refs(lex, lens, seed):
    """an alignment-like random sequence drawn from the lexicon's mixtures, one out-of-range frame, one all-out-of-range utterance"""
    rng = np.random.default_rng(seed)
    S = lex.n_states
    ref = rng.integers(0, S, size=sum(lens)).astype(np.uint16)
    off = _off(lens)
    ref[int(off[3]) + 5] = S + 7
    ref[int(off[4]):int(off[5])] = 65535
    return ref


def _smbr(e, graph, tdp, wp, ref, scale, tag=None):
    """(F, Abar, gamma) of the restatement in float64, with the longdouble run and its bounds beside it"""
    with np.errstate(all="ignore"):
        return Rule(SM.smbr(e, graph, tdp, wp, ref, scale), SM.smbr(e, graph, tdp, wp, ref, scale, dtype=nc.LD), tag)


class Rule(tuple):
    """(F, Abar, gamma) in float64 -- what the fixed tolerances are held against -- carrying the np.longdouble run (F80, A80, g80) and,
    against it, the measured bound where it is tighter than the fixed one (nc.tighter): tolF, tolA, tolg [T, S], tols (a frame's sum).  Abar
    and a frame's sum are held to the larger of their own float64 distance and gamma's, as in tests/test_gpu_smbr_scores.py."""

    def __new__(cls, r64, r80, tag=None):
        self = super().__new__(cls, r64)
        (F, A, g), (self.F80, self.A80, self.g80) = r64, r80
        fixed = 1e-9 * (1 + g.shape[0])
        if np.isfinite(self.F80):
            self.tolF = nc.tighter(1e-10 * max(1.0, abs(float(F))), F, self.F80, tag and tag + " F")
            self.tolg = nc.tighter(fixed, g, self.g80, tag and tag + " gamma")
            dw = nc.dist(g, self.g80)
            self.tolA = float(nc.bound(max(nc.dist(A, self.A80), dw), max(float(self.A80), 1.0)))
            self.tols = float(nc.bound(max(nc.dist(g.sum(axis=1), self.g80.sum(axis=1)), dw), 1.0))
            self.tolA, self.tols = (x if x <= fixed else np.inf for x in (self.tolA, self.tols))  # (as nc.tighter)
        else:
            self.tolF = self.tolA = self.tols = 0.0
            self.tolg = np.zeros(g.shape)
        return self

    def holds(self, cost, acc):
        if not np.isfinite(self.F80):
            return cost == self.F80 and acc == 0.0
        return abs(nc.LD(cost) - self.F80) <= self.tolF and abs(nc.LD(acc) - self.A80) <= self.tolA


def _check_signed_items(g, count, state, weight, floor, K, tol, g80=None, tolv=None):
    """one frame: the items are the mixtures with g != 0 and |g| >= floor, largest |g| first (ties: smaller id), at most K; a
    mixture whose |g| lies within tol of the floor (or of 0) may be on either side; the order is checked on |weight|.  g80, tolv: the
    longdouble run's gamma and the bound that holds against it (Rule)"""
    n = int(count)
    assert n <= K and not weight[n:].any() and not state[n:].any()
    ks, ws = state[:n].astype(int), weight[:n]
    assert len(set(ks.tolist())) == n
    for k, w in zip(ks, ws):
        assert w != 0.0 and abs(w) >= floor and abs(w - g[k]) <= tol, (k, w, g[k])
        if g80 is not None:
            assert abs(nc.LD(w) - g80[k]) <= tolv[k], (k, w, g80[k], tolv[k])
    for i in range(n - 1):
        a, b = abs(ws[i]), abs(ws[i + 1])
        assert a > b or (a == b and ks[i] < ks[i + 1])
    cut = max(floor, 0.0) + tol if n < K else abs(ws[-1]) + tol  # whoever exceeds it must have been kept
    missing = [k for k in range(len(g)) if k not in set(ks.tolist()) and abs(g[k]) > cut]
    assert not missing, (missing, g, ks, ws)


@pytest.fixture(scope="module")
def restated(tmp_path_factory, oracle_lib):
    """per (lexicon, penalty set): the restatement's (F, Abar, gamma) of every utterance, computed once"""
    out = {}
    for li, lens_ in enumerate(LEXICA):
        lex = _lex(lens_, 0)
        tmp = tmp_path_factory.mktemp(f"smbr{li}")
        spec, mp = _model(tmp, lex.n_states, 800 + li)
        feats = synth.make_features(sum(LENS), DIM, seed=802 + li)
        ref = _refs(lex, LENS, 803 + li)
        off = _off(LENS)
        net = _net(lex)
        for pi, (tdp, wp, scale) in enumerate(PENALTIES):
            o = oracle_lib.Oracle(mp, DIM, lex, tdp=tdp)
            res = []
            for u in range(len(LENS)):
                a, b = int(off[u]), int(off[u + 1])
                res.append(_smbr(o.score_matrix(feats[a:b]), M.free_graph(net), tdp, wp, ref[a:b].astype(np.int64), scale,
                                 f"lexicon {li} penalties {pi} utterance {u}"))
            out[li, pi] = dict(lex=lex, mp=mp, feats=feats, ref=ref, off=off, res=res, tables=o.tables())
            o.close()
    return out


@pytest.mark.parametrize("pi", range(len(PENALTIES)))
@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_against_restatement(li, pi, restated):
    """F, Abar and the items for floors 0 and 1e-6 and K in (1, 3, S); then both statistics sides with max_approx on and off"""
    r = restated[li, pi]
    lex, feats, off, ref = r["lex"], r["feats"], r["off"], r["ref"]
    tdp, wp, scale = PENALTIES[pi]
    S = lex.n_states
    with capi.Model.from_mixset(r["mp"], DIM) as m, _capi_lex(m, lex, tdp) as L:
        corpus = m.upload(feats, off)
        for floor in (0.0, 1e-6):
            for K in (1, 3, S):
                cost, acc, count, state, weight = corpus.net_accuracies(L, wp, ref, scale, capi.GMM_PREFILTER, floor, K)
                for u, rule in enumerate(r["res"]):
                    F, A, g = rule
                    T = g.shape[0]
                    tol = 1e-9 * (1 + T)
                    print("utt", u, cost[u], F, acc[u], A)
                    assert _rel(cost[u], F) <= 1e-10 and abs(acc[u] - A) <= tol and 0.0 <= acc[u] <= T + tol
                    assert rule.holds(cost[u], acc[u]), (u, cost[u], rule.F80, rule.tolF, acc[u], rule.A80, rule.tolA)
                    for t in range(T):
                        ft = int(off[u]) + t
                        _check_signed_items(g[t], count[ft], state[ft], weight[ft], floor, K, tol, rule.g80[t], rule.tolg[t])
                        if K == S and floor == 0.0:
                            assert abs(weight[ft].sum()) <= tol
                            assert abs(weight[ft].astype(nc.LD).sum() - rule.g80[t].sum()) <= rule.tols
        assert acc[4] == 0.0 and not count[int(off[4]):].any()  # every reference out of range
        for max_approx, floor in ((True, 0.0), (False, 1e-6)):
            cost, acc, num, den = corpus.smbr_statistics(L, wp, ref, scale, capi.GMM_PREFILTER, floor, max_approx)
            items = [[], []]
            for u, rule in enumerate(r["res"]):
                F, A, g = rule
                assert _rel(cost[u], F) <= 1e-10 and abs(acc[u] - A) <= 1e-9 * (1 + g.shape[0])
                assert rule.holds(cost[u], acc[u]), (u, cost[u], rule.F80, acc[u], rule.A80)
                items[0] += SM.signed_items(g, +1, floor)
                items[1] += SM.signed_items(g, -1, floor)
            _check_stats(num, feats, items[0], r["tables"], max_approx)
            _check_stats(den, feats, items[1], r["tables"], max_approx)
            if floor == 0.0:
                total = sum(np.abs(g).sum() for _, _, g in r["res"])
                print("balance", num[1].sum(), den[1].sum(), total)
                assert abs(num[1].sum() - den[1].sum()) <= 1e-9 * total
        corpus.close()


def _occ_acc(corpus, L, wp, scale, ref, off, S):
    """sum_t occ_t(ref_t) per utterance from sr_net_occupancies_corpus (floor 0, max_items S)"""
    _, count, state, weight = corpus.net_occupancies(L, wp, scale, None, capi.GMM_PREFILTER, 0.0, S)
    out = np.zeros(len(off) - 1)
    for u in range(len(off) - 1):
        for t in range(int(off[u]), int(off[u + 1])):
            hit = state[t, :count[t]] == ref[t]
            out[u] += weight[t, :count[t]][hit].sum()
    return out


@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_cross_check_with_the_occupancies(li, restated):
    """out_acc[u] = sum_t occ_t(ref_t) of the existing entry point; over constant references k = 0 .. S - 1 the accuracies sum to T_u
    -- to 0 for an utterance without a complete path (F_u = +inf: Abar_u = 0 by definition; the T = 1 utterance under the +inf skip
    when silence has three positions)"""
    r = restated[li, 1]
    lex, feats, off, ref = r["lex"], r["feats"], r["off"], r["ref"]
    tdp, wp, scale = PENALTIES[1]
    S = lex.n_states
    T = np.diff(off.astype(np.int64))
    with capi.Model.from_mixset(r["mp"], DIM) as m, _capi_lex(m, lex, tdp) as L:
        corpus = m.upload(feats, off)
        cost, acc = corpus.net_accuracies(L, wp, ref, scale, capi.GMM_PREFILTER, 0.0, 1)[:2]
        want = _occ_acc(corpus, L, wp, scale, ref, off, S)
        print("acc", acc, want)
        assert np.all(np.abs(acc - want) <= 1e-9 * (1 + T))
        total = sum(corpus.net_accuracies(L, wp, np.full(len(feats), k, np.uint16), scale, capi.GMM_PREFILTER, 0.0, 1)[1] for k in range(S))
        assert np.all(np.abs(total - np.where(np.isfinite(cost), T, 0)) <= 1e-9 * (1 + T))
        assert np.isfinite(cost[1:]).all() and np.isfinite(cost[0]) == np.isfinite(r["res"][0][0])
        corpus.close()


def _recognition_case(tmp_path, seed, n_utts=8):
    lex = synth.make_lexicon(6, 3, 2)
    spec, mp = _model(tmp_path, lex.n_states, seed, Mx=3)
    rng = np.random.default_rng(seed + 1)
    trans = [list(rng.integers(1, lex.n_words, size=int(rng.integers(1, 5)))) for _ in range(n_utts)]
    utts = [synth.sample_utterance(spec, lex, ws, seed=seed + 2 + i, noise=1.2) for i, ws in enumerate(trans)]
    feats, off = np.concatenate(utts), _off([len(f) for f in utts])
    ref = rng.integers(0, lex.n_states, size=len(feats)).astype(np.uint16)
    return lex, mp, feats, off, ref


def test_determinism_and_shards(tmp_path):
    """two identical calls return identical bits; the statistics of two half-corpora add up to the whole (the 1e-4 seed once per
    call and side), with test_gpu_mmi.test_determinism_and_shards' bounds"""
    lex, mp, feats, off, ref = _recognition_case(tmp_path, 840)
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        runs = [corpus.smbr_statistics(L, 10.0, ref, 0.5, capi.GMM_PREFILTER, 1e-8, False) for _ in range(2)]
        accs = [corpus.net_accuracies(L, 10.0, ref, 0.5, capi.GMM_PREFILTER, 0.0, 5) for _ in range(2)]
        corpus.close()
        flat = lambda r: [r[0], r[1], *r[2], *r[3]]
        for a, b in zip(flat(runs[0]), flat(runs[1])):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for a, b in zip(accs[0], accs[1]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.array_equal(accs[0][1].view(np.uint64), runs[0][1].view(np.uint64))
        halves = []
        for u0, u1 in ((0, 4), (4, 8)):
            f0, f1 = int(off[u0]), int(off[u1])
            part = m.upload(feats[f0:f1], off[u0:u1 + 1] - off[u0])
            halves.append(part.smbr_statistics(L, 10.0, ref[f0:f1], 0.5, capi.GMM_PREFILTER, 1e-8, False))
            part.close()
    for side in (2, 3):
        whole, a, b = runs[0][side], halves[0][side], halves[1][side]
        for i in (1, 3):
            assert np.all(np.abs(a[i] + b[i] - whole[i]) <= 1e-12 * np.maximum(np.abs(whole[i]), 1e-300))
        assert np.all(np.abs(a[0] + b[0] - whole[0]) <= 1e-9 * np.maximum(np.abs(a[0]) + np.abs(b[0]), 1e-300))
        assert np.all(np.abs(a[2] + b[2] - 1e-4 - whole[2]) <= 1e-9 * np.maximum(np.abs(whole[2]), 1e-4))
    for i in (0, 1):
        assert np.array_equal(np.concatenate([halves[0][i], halves[1][i]]).view(np.uint64), runs[0][i].view(np.uint64))


def _multi_group_outputs(mp, lex, feats, off, ref, wp, scale):
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:  # (the budget is read when the model is made)
        corpus = m.upload(feats, off)
        accs = corpus.net_accuracies(L, wp, ref, scale, capi.GMM_PREFILTER, 1e-6, 3)
        cost, acc, num, den = corpus.smbr_statistics(L, wp, ref, scale, capi.GMM_PREFILTER, 1e-6, False)
        corpus.close()
    return dict(accs=accs, stats=[cost, acc, *num, *den])


def test_several_launch_groups(tmp_path, oracle_lib, monkeypatch):
    """test_gpu_mmi.test_several_launch_groups for the accuracy pass (16 P T bytes): 7 utterances in one launch at the default budget,
    in groups of one and of several with SRGPU_FB_MB=1 -- equal bytes either way; and the restatement's F, Abar and gamma for an
    utterance that is not the first of its group"""
    lex = _lex([1] + [6] * 25, 0)
    P = len(lex.flatten()[1])
    assert several_groups([16 * P * T for T in MULTI_LENS]) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 7)]
    spec, mp = _model(tmp_path, lex.n_states, 870)
    feats = synth.make_features(sum(MULTI_LENS), DIM, seed=871)
    off = _off(MULTI_LENS)
    ref = np.random.default_rng(872).integers(0, lex.n_states, size=len(feats)).astype(np.uint16)
    wp, scale = 10.0, 0.5
    monkeypatch.delenv("SRGPU_FB_MB", raising=False)
    one = _multi_group_outputs(mp, lex, feats, off, ref, wp, scale)
    monkeypatch.setenv("SRGPU_FB_MB", "1")
    cut = _multi_group_outputs(mp, lex, feats, off, ref, wp, scale)
    for k in one:
        for a, b in zip(one[k], cut[k]):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), k
    # utterance 4 is the second of the group (3, 5)
    u, a, b = 4, int(off[4]), int(off[5])
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    rule = _smbr(o.score_matrix(feats[a:b]), M.free_graph(_net(lex)), TDP, wp, ref[a:b].astype(np.int64), scale, "several groups utterance 4")
    F, A, g = rule
    o.close()
    cost, acc, count, state, weight = cut["accs"]
    tol = 1e-9 * (1 + b - a)
    print("several groups", cost[u], F, acc[u], A)
    assert _rel(cost[u], F) <= 1e-10 and abs(acc[u] - A) <= tol
    assert _rel(cut["stats"][0][u], F) <= 1e-10 and abs(cut["stats"][1][u] - A) <= tol
    assert rule.holds(cost[u], acc[u]) and rule.holds(cut["stats"][0][u], cut["stats"][1][u])
    for t in range(b - a):
        _check_signed_items(g[t], count[a + t], state[a + t], weight[a + t], 1e-6, 3, tol, rule.g80[t], rule.tolg[t])


def _big_lexicon(n_positions, n_states, seed):
    """word 0 = a one-position silence (state 0); the other words 3 .. 6 positions of the model's other states, n_positions in all"""
    rng = np.random.default_rng(seed)
    off, aut = [0, 1], [0]
    while len(aut) < n_positions:
        n = min(int(rng.integers(3, 7)), n_positions - len(aut))
        aut.extend(int(x) for x in rng.integers(1, n_states, size=n))
        off.append(len(aut))
    return synth.ExplicitLexicon(np.asarray(off, np.uint32), np.asarray(aut, np.uint16), 0)


def test_position_limit(tmp_path):
    """a lexicon just above the exported limit: SR_ELIMIT; one of 4000 positions x 3 frames -- full LDS rows, every stride of the 512
    threads -- runs and agrees with the occupancies"""
    S = 40
    spec, mp = _model(tmp_path, S, 850)
    feats = synth.make_features(3, DIM, seed=851)
    off = _off([3])
    ref = np.array([0, 5, 65535], np.uint16)
    L_ = capi.lib()
    limit = capi.smbr_max_positions()
    assert 4000 <= limit < 8192
    with capi.Model.from_mixset(mp, DIM) as m:
        corpus = m.upload(feats, off)
        with _capi_lex(m, _big_lexicon(limit + 1, S, 852)) as L:
            sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
            cost, acc = np.zeros(1), np.zeros(1)
            P = capi._ptr
            rc = L_.sr_net_accuracies_corpus(m.h, corpus.h, L.h, C.byref(sp), 0.1, 0.0, 1, P(ref), P(cost), P(acc), None, None, None)
            assert rc == ELIMIT and b"positions" in L_.sr_last_error()
        for n in (4000, limit):
            with _capi_lex(m, _big_lexicon(n, S, 853)) as L:
                cost, acc, count, state, weight = corpus.net_accuracies(L, 10.0, ref, 0.1, capi.GMM_PREFILTER, 0.0, S)
                want = _occ_acc(corpus, L, 10.0, 0.1, ref, off, S)
                print("big", n, cost, acc, want)
                assert np.isfinite(cost[0]) and abs(acc[0] - want[0]) <= 1e-9 * 4
                assert np.all(np.abs(weight.sum(axis=1)) <= 1e-9 * 4)
        corpus.close()


def test_errors(tmp_path):
    """every SR_EINVAL of the two entry points, outputs untouched; all checks precede any launch"""
    lex = _lex([1, 3, 3, 2], 0)
    spec, mp = _model(tmp_path, lex.n_states, 860)
    feats = synth.make_features(20, DIM, seed=861)
    off = _off([12, 8])
    L_ = capi.lib()
    P = capi._ptr
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L, capi.Model.from_mixset(mp, DIM) as other:
        corpus = m.upload(feats, off)
        sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
        ref = np.zeros(20, np.uint16)
        mark = 7.0
        cost, acc = np.full(2, mark), np.full(2, mark)
        cnt, st, wt = np.full(20, 7, np.uint16), np.full((20, 2), 7, np.uint16), np.full((20, 2), mark)

        def call(scale=1.0, floor=0.0, K=2, lexh=L.h, refs=ref, out=(cost, acc, cnt, st, wt), spp=sp, ch=corpus.h):
            return L_.sr_net_accuracies_corpus(m.h, ch, lexh, C.byref(spp), scale, floor, K, P(refs), *[P(a) for a in out])

        with _capi_lex(other, lex) as L2:
            bad = [dict(scale=0.0), dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan), dict(floor=-1.0), dict(floor=np.nan),
                   dict(K=0), dict(K=65536), dict(refs=None), dict(out=(None, acc, cnt, st, wt)), dict(out=(cost, None, cnt, st, wt)),
                   dict(out=(cost, acc, None, st, wt)), dict(out=(cost, acc, cnt, None, wt)), dict(out=(cost, acc, cnt, st, None)),
                   dict(spp=capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 1)), dict(lexh=L2.h)]
            for kw in bad:
                assert call(**kw) == EINVAL, kw
        assert (cost == mark).all() and (acc == mark).all() and (cnt == 7).all() and (st == 7).all() and (wt == mark).all()
        assert call(out=(cost, acc, None, None, None)) == 0  # cost and accuracy alone
        assert call() == 0
        nd = m.n_densities
        stats = [np.full((nd, DIM), mark), np.full(nd, mark), np.full((nd, DIM), mark), np.full(nd, mark)]
        outs = [np.full(2, mark), np.full(2, mark)] + stats + [a.copy() for a in stats]

        def smbr(scale=1.0, floor=0.0, refs=ref, o=outs, spp=sp):
            return L_.sr_smbr_statistics_corpus(m.h, corpus.h, L.h, C.byref(spp), scale, floor, 1, P(refs), *[P(a) for a in o])

        for kw in [dict(scale=0.0), dict(scale=np.inf), dict(floor=-1.0), dict(refs=None),
                   dict(spp=capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 1))] + [dict(o=outs[:i] + [None] + outs[i + 1:]) for i in range(10)]:
            assert smbr(**kw) == EINVAL, kw
        assert all((a == mark).all() for a in outs)
        assert smbr() == 0
        corpus.close()


def test_end_to_end(tmp_path, oracle_lib):
    """statistics on the device, sr_model_create_from_mmi_statistics at the CPU criterion test's E, Abar again: it rises as under
    the restatement; the new tables are mmi_reference.ebw_update of the device's statistics (every density's score of probe frames
    within 1e-12 relative)"""
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    tb = o.tables()
    ref = criterion_refs(o, lex, feats, off, trans)
    o.close()
    D = tb["means"].shape[1]
    probe = np.random.default_rng(871).standard_normal((64, D)).astype(np.float32) * 2.0
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        cost, acc, num, den = corpus.smbr_statistics(L, wp, ref, scale, capi.GMM_PREFILTER, 0.0, True)
        means, var = M.ebw_update(tb["means"], tb["vars_inv"], (num[0], num[1], num[2]), (den[0], den[1], den[2]), SMBR_E, 0.0, 1e-3)
        norm = (D * np.log(2 * np.pi) + np.log(var).sum(axis=1)) / 2
        with m.from_mmi_statistics(num, den, SMBR_E, 0.0, 1e-3) as m2, \
                capi.Model.from_tables(tb["mix_off"], means, 1.0 / var, norm, tb["logw"]) as mr:
            got = m2.score_frames(probe, capi.GMM_EXACT)
            want = mr.score_frames(probe, capi.GMM_EXACT)
            assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
            with _capi_lex(m2, lex) as L2:
                c2 = m2.upload(feats, off)
                acc2 = c2.net_accuracies(L2, wp, ref, scale, capi.GMM_PREFILTER, 0.0, 1)[1]
                c2.close()
        print("expected accuracy", acc.sum(), acc2.sum(), len(feats))
        assert acc2.sum() > acc.sum()
        corpus.close()


def test_cpp_driver(tmp_path, oracle_lib):
    """sr::Trainer::smbr_iteration from C++ (tests/cpp/smbr_driver.cpp): its sum Abar before and after one iteration is the Python
    binding's to 1e-10 relative, and the iteration raises it"""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "smbr_driver")
    lib_dir = os.path.join(root, "speechrecognition_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "smbr_driver.cpp"),
                    "-o", exe, "-L", lib_dir, "-lsrgpu", "-Wl,-rpath," + lib_dir], check=True)
    lex, spec, mp, feats, off, trans, wp, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, DIM, lex)
    ref = criterion_refs(o, lex, feats, off, trans)
    o.close()
    inp = str(tmp_path / "case.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<I", lex.n_words))
        for n, r in zip(lex.word_states, lex.word_reps):
            f.write(struct.pack("<HH", int(n), int(r)))
        f.write(struct.pack("<I3d4d", lex.silence_idx, *TDP, wp, scale, SMBR_E, 0.0))
        f.write(struct.pack("<I", len(trans)))
        for u in range(len(trans)):
            a, b = int(off[u]), int(off[u + 1])
            f.write(struct.pack("<I", b - a))
            f.write(np.ascontiguousarray(feats[a:b], np.float32).tobytes())
            f.write(np.ascontiguousarray(ref[a:b], np.uint16).tobytes())
    r = subprocess.run([exe, "smbr", mp, str(DIM), inp], check=True, capture_output=True, text=True)
    lines = [line.split() for line in r.stdout.splitlines() if line.startswith("accuracy")]
    assert len(lines) == 2 and int(lines[0][3]) == len(feats), r.stdout
    got = [struct.unpack("<d", struct.pack("<Q", int(x[2], 16)))[0] for x in lines]
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        _, acc, num, den = corpus.smbr_statistics(L, wp, ref, scale, capi.GMM_DEFAULT, 0.0, True)
        corpus.close()
        assert abs(got[0] - acc.sum()) <= 1e-10 * abs(got[0])
        with m.from_mmi_statistics(num, den, SMBR_E, 0.0, 1e-3) as m2, _capi_lex(m2, lex) as L2:
            c2 = m2.upload(feats, off)
            acc2 = c2.smbr_statistics(L2, wp, ref, scale, capi.GMM_DEFAULT, 0.0, True)[1]
            c2.close()
        assert abs(got[1] - acc2.sum()) <= 1e-10 * abs(got[1])
    assert got[1] > got[0]
