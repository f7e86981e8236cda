"""MMI training against the bigram search network on the device: sr_bigram_occupancies_corpus and sr_bigram_mmi_statistics_corpus
against the numpy restatement (tests/bigram_mmi_reference.py, pinned by tests/test_bigram_mmi_cpu.py), the bigram word posteriors,
the decoder and themselves.  Tolerances are the project's (test_gpu_mmi.py / test_gpu_bigram_posteriors.py): costs 1e-10 relative,
occupancies 1e-9 absolute, statistics 1e-9 relative to sum |w x|.  Beside them, wherever it is tighter, the measured rule of tests/test_gpu_bgfb_scores.py against the restatement's
np.longdouble run (bigram_fb_cases.measured: 8 times the distance of the farther of the log-space and the linear-domain float64
restatement plus 4 ulp of the value; the `RULE` lines say which of the two holds); test_scale_shape keeps the fixed pair (a
longdouble run of its 2 667-word entry sums takes minutes)."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import bigram_fb_cases as bc
from tests import bigram_fb_reference as R
from tests import bigram_mmi_reference as BM
from tests.test_bigram import FLT_MAX, SIL_TDP, _setup
from tests.test_bigram_mmi_cpu import CRITERION_E, criterion_task
from tests.test_gpu_bigram_posteriors import BIG_TDP, _scale_case, linear_entry_sum
from tests.test_gpu_mmi import _check_stats, _geq
from tests.test_gpu_word_posteriors import _check_items, _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ELIMIT = -1, -4  # include/srgpu.h
# test_bigram.py's _setup shapes the bigram posterior tests use (seed, W, states per word, silence states, tdp): a multi-state silence
# (3, 33) and one-state words (4) among them
SHAPES = [(1, 5, 3, 1, None), (3, 4, 4, 2, None), (4, 6, 1, 1, None), (33, 6, 3, 4, SIL_TDP)]
# measured by occ_spread_on_cpu (see test_scale_shape's docstring)
OCC_SPREAD = 6.94e-17  # relative spread on F: 0 (the same bits)


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _corpus(feats, seed, W):
    """utterances and transcripts: the sampled utterance with three words, T = 1, T = 0 between two others, noise with an empty
    transcript, half of the first with repeated words, a transcript too long for its utterance, transcripts through the +inf and
    the NaN LM entry (_forbid)"""
    rng = np.random.default_rng(seed + 7)
    half = feats[: len(feats) // 2]
    utts = [feats, feats[:1], feats[:0], rng.standard_normal((37, 12)).astype(np.float32), half, feats[:3], feats, half]
    trans = [[2, 1, 3], [W - 1], [], [], [1, 1, 3], [1] * 5, [3, 1, 2], [2, 3]]
    return utts, np.concatenate(utts), _off([len(x) for x in utts]), trans


def _forbid(lm):
    lm = lm.copy()
    lm[2, 1] = np.inf  # word 2 never follows word 1
    lm[3, 2] = np.nan  # word 3 never follows word 2
    return np.ascontiguousarray(lm)


def _refs(o, utts, net, lm, tdp, trans, scale, S):
    """per utterance ((F_num, occ_num), (F_den, occ_den)) of the restatement"""
    out = []
    for x, tr in zip(utts, trans):
        e = o.score_matrix(x) if len(x) else np.zeros((0, S))
        out.append((BM.chain_occupancies(e, net, lm, tdp, tr, scale), BM.free_occupancies(e, net, lm, tdp, scale)))
    return out


def _rules(o, utts, net, lm, tdp, trans, scale, S, refs):
    """per utterance and side the longdouble run and the measured bounds on F and on every occupancy, where they are tighter than 1e-10
    relative and 1e-9 (bigram_fb_cases.measured; the `RULE` lines say which holds)"""
    out = []
    for u, (x, tr) in enumerate(zip(utts, trans)):
        e = o.score_matrix(x) if len(x) else np.zeros((0, S))
        num = lambda e=e, tr=tr, **kw: BM.chain_occupancies(e, net, lm, tdp, tr, scale, **kw)  # noqa: E731
        den = lambda e=e, **kw: BM.free_occupancies(e, net, lm, tdp, scale, **kw)  # noqa: E731
        fixed = lambda F: (1e-10 * max(1.0, abs(float(F))) if np.isfinite(F) else 0.0, 1e-9)  # noqa: E731
        out.append((bc.measured(num, refs[u][0], None, fixed(refs[u][0][0]), f"utterance {u} kappa {scale} chain"),
                    bc.measured(den, refs[u][1], bc.lin_entry(net.sil), fixed(refs[u][1][0]), f"utterance {u} kappa {scale} free")))
    return out


def _against_restatement(o, m, bg, allf, off, trans, refs, scale, S, floors=(0.0, 1e-6), modes=((True, 0.0), (False, 1e-6)), rules=None):
    """F_num, F_den, the occupancy items of both networks and both statistics sets"""
    tables = o.tables()
    corpus = m.upload(allf, off)
    for side, tr in ((0, trans), (1, None)):
        for floor in floors:
            for K in (1, 3, S):
                cost, count, state, weight = corpus.bigram_occupancies(bg, scale, tr, capi.GMM_PREFILTER, floor, K)
                for u, ref in enumerate(refs):
                    F, occ = ref[side]
                    print("cost", side, u, cost[u], F)
                    assert _rel(cost[u], F) <= 1e-10, (side, u, cost[u], F)
                    (F80, o80), (tolF, tolo) = rules[u][side] if rules else ((F, occ), (np.inf, np.full(occ.shape, np.inf)))
                    assert cost[u] == F80 or abs(bc.LD(cost[u]) - F80) <= tolF, (side, u, cost[u], F80, tolF)
                    for t in range(occ.shape[0]):
                        ft = int(off[u]) + t
                        _check_items(occ[t], count[ft], state[ft], weight[ft], floor, K, o80[t], tolo[t])
                        if K == S and floor == 0.0 and np.isfinite(F):
                            assert abs(weight[ft].sum() - 1.0) <= 1e-8
    for max_approx, floor in modes:
        fn, fd, num, den = corpus.bigram_mmi_statistics(bg, trans, scale, capi.GMM_PREFILTER, floor, max_approx)
        items = [[], []]
        for u, ref in enumerate(refs):
            assert _rel(fn[u], ref[0][0]) <= 1e-10 and _rel(fd[u], ref[1][0]) <= 1e-10
            assert _geq(fn[u], fd[u])
            for side in (0, 1):  # an utterance without a numerator path contributes to neither side
                occ = ref[side][1] if np.isfinite(ref[0][0]) else np.zeros_like(ref[side][1])
                items[side] += BM.frame_items(occ, floor)
        _check_stats(num, allf, items[0], tables, max_approx)
        _check_stats(den, allf, items[1], tables, max_approx)
    corpus.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_against_restatement(shape, tmp_path, oracle_lib):
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    lm = _forbid(lm)
    utts, allf, off, trans = _corpus(feats, seed, lex.n_words)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        for scale in (1.0, 0.3):
            refs = _refs(o, utts, net, lm, tdp, trans, scale, lex.n_states)
            assert refs[2][0][0] == 0.0 and refs[2][1][0] == 0.0          # T = 0, empty transcript
            assert refs[5][0][0] == np.inf and np.isfinite(refs[5][1][0])  # too long for its utterance
            assert refs[6][0][0] == np.inf and refs[7][0][0] == np.inf     # forbidden LM entries
            assert np.isfinite(refs[0][0][0]) and np.isfinite(refs[3][0][0])
            _against_restatement(o, m, bg, allf, off, trans, refs, scale, lex.n_states,
                                 rules=_rules(o, utts, net, lm, tdp, trans, scale, lex.n_states, refs))
        bg.close()
    o.close()


def test_one_state_words_negative_costs(tmp_path, oracle_lib):
    """tight variances: emission costs below 0; negative LM scores, forbidden entries; one-state words.  Statistics with the
    arg-min density only: on the noise utterance every density's exp(-score) underflows under these variances, so the soft
    memberships are 0 / 0 in the reference's accumulation itself."""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 41, 9, 1)
    synth.scale_variances(spec, 0.004)
    synth.write_mixset(mp, spec)
    feats = synth.sample_utterance(spec, lex, [1, 5, 2, 8], seed=43)
    lm = _forbid((lm - 2.0).astype(np.float32))
    utts, allf, off, trans = _corpus(feats, 41, lex.n_words)
    trans[0] = [1, 5, 2, 8]
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    assert o.score_matrix(allf).min() < 0
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        refs = _refs(o, utts, net, lm, tdp, trans, 0.5, lex.n_states)
        assert np.isfinite(refs[0][0][0])
        _against_restatement(o, m, bg, allf, off, trans, refs, 0.5, lex.n_states, floors=(0.0,), modes=((True, 0.0),),
                             rules=_rules(o, utts, net, lm, tdp, trans, 0.5, lex.n_states, refs))
        bg.close()
    o.close()


def test_consistency_with_word_posteriors(tmp_path):
    """F_den is sr_bigram_word_posteriors_corpus' cost bit for bit; no mixture shared between words: a word's occupancies sum to its
    posterior (silence's mixtures: the silence word and every copy); occupancies sum to 1"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 33, 6, 3, sil_states=4, tdp=SIL_TDP)
    owner = {}
    for w in range(lex.n_words):
        for k in mixtures[word_off[w]:word_off[w + 1]]:
            assert owner.setdefault(int(k), w) == w
    utts, allf, off, trans = _corpus(feats, 33, lex.n_words)
    S, W = lex.n_states, lex.n_words
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        for scale in (1.0, 0.2):
            cw, nw, word, pw = corpus.bigram_word_posteriors(bg, scale, capi.GMM_PREFILTER, 0.0, W)
            co, no, state, occ = corpus.bigram_occupancies(bg, scale, None, capi.GMM_PREFILTER, 0.0, S)
            assert np.array_equal(cw.view(np.uint64), co.view(np.uint64))
            fd = corpus.bigram_mmi_statistics(bg, trans, scale)[1]
            assert np.array_equal(cw.view(np.uint64), fd.view(np.uint64))
            assert np.isfinite(co[0]) and np.isfinite(co[3])
            utt = np.searchsorted(off, np.arange(len(allf)), side="right") - 1
            for t in range(len(allf)):
                p, q = np.zeros(W), np.zeros(S)
                p[word[t, :nw[t]]] = pw[t, :nw[t]]
                q[state[t, :no[t]]] = occ[t, :no[t]]
                for w in range(W):
                    assert abs(q[mixtures[word_off[w]:word_off[w + 1]]].sum() - p[w]) <= 1e-9
                if np.isfinite(co[utt[t]]):  # (the T = 1 utterance is shorter than any word here: no path, every occupancy 0)
                    assert abs(q.sum() - 1.0) <= 1e-8
        corpus.close()
        bg.close()


def test_ordering(tmp_path):
    """F_num >= F_den; F_den <= the score of the decoder's last item (beams off) up to its float rounding"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 12, 9, 2)
    utts, allf, off, trans = _corpus(feats, 12, lex.n_words)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        w, s, t, woff = corpus.recognize_bigram(bg, FLT_MAX, FLT_MAX)
        hyp = [[int(x) for x in w[int(woff[u]):int(woff[u + 1])] if x != lex.silence_idx] for u in range(len(utts))]
        fd = corpus.bigram_occupancies(bg, 1.0, None, max_items=1)[0]
        fh = corpus.bigram_occupancies(bg, 1.0, hyp, max_items=1)[0]
        fn = corpus.bigram_occupancies(bg, 1.0, trans, max_items=1)[0]
        for u in range(len(utts)):
            print("order", u, fd[u], fh[u], fn[u])
            assert _geq(fn[u], fd[u]) and _geq(fh[u], fd[u])
            if woff[u + 1] > woff[u]:
                s_last = float(s[int(woff[u + 1]) - 1])
                slack = (4 * len(utts[u]) + 8) * 2.0 ** -24 * max(1.0, float(np.abs(s[int(woff[u]):int(woff[u + 1])]).max()))
                assert fd[u] <= s_last + slack
                assert fh[u] <= s_last + slack  # the recognised words' network holds the best path
        corpus.close()
        bg.close()


def test_determinism_and_shards(tmp_path):
    """two identical calls return identical bytes, a call at another kappa in between (the table cache); the statistics of two
    half-corpora add up to the whole (the 1e-4 seed once per call and side); the halves' costs concatenated are the whole's bits"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 15, 40, 3)
    utts, allf, off, trans = _corpus(feats, 15, lex.n_words)
    flat = lambda r: [r[0], r[1], *r[2], *r[3]]  # noqa: E731
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        a = corpus.bigram_mmi_statistics(bg, trans, 0.4, capi.GMM_PREFILTER, 1e-8, False)
        oa = [corpus.bigram_occupancies(bg, 0.4, tr, max_items=5) for tr in (trans, None)]
        other = corpus.bigram_mmi_statistics(bg, trans, 0.9, capi.GMM_PREFILTER, 1e-8, False)
        assert not np.array_equal(other[1], a[1])
        b = corpus.bigram_mmi_statistics(bg, trans, 0.4, capi.GMM_PREFILTER, 1e-8, False)
        ob = [corpus.bigram_occupancies(bg, 0.4, tr, max_items=5) for tr in (trans, None)]
        corpus.close()
        for x, y in zip(flat(a), flat(b)):
            assert x.tobytes() == y.tobytes()
        for ra, rb in zip(oa, ob):
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes()
        assert a[0][5] == np.inf
        halves = []
        for u0, u1 in ((0, 4), (4, 8)):
            f0, f1 = int(off[u0]), int(off[u1])
            part = m.upload(allf[f0:f1], off[u0:u1 + 1] - off[u0])
            halves.append(part.bigram_mmi_statistics(bg, trans[u0:u1], 0.4, capi.GMM_PREFILTER, 1e-8, False))
            part.close()
        bg.close()
    for side in (2, 3):
        whole, x, y = a[side], halves[0][side], halves[1][side]
        for i in (1, 3):
            assert np.all(np.abs(x[i] + y[i] - whole[i]) <= 1e-12 * np.maximum(np.abs(whole[i]), 1e-300))
        assert np.all(np.abs(x[0] + y[0] - whole[0]) <= 1e-9 * np.maximum(np.abs(x[0]) + np.abs(y[0]), 1e-300))
        assert np.all(np.abs(x[2] + y[2] - 1e-4 - whole[2]) <= 1e-9 * np.maximum(np.abs(whole[2]), 1e-4))
    for i in (0, 1):
        assert np.concatenate([halves[0][i], halves[1][i]]).tobytes() == a[i].tobytes()


def test_one_ebw_step_raises_the_criterion(tmp_path):
    """one EBW step through sr_model_create_from_mmi_statistics and a fresh sr_bigram on the new model raises sum(F_den - F_num) on
    the task tests/test_bigram_mmi_cpu.py vetted, at its E"""
    lex, mp, word_off, mixtures, lm, tdp, feats, off, trans, scale = criterion_task(tmp_path)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        fn, fd, num, den = corpus.bigram_mmi_statistics(bg, trans, scale, capi.GMM_PREFILTER, 0.0, True)
        corpus.close()
        bg.close()
        with m.from_mmi_statistics(num, den, CRITERION_E, 0.0, 1e-3) as m2:
            bg2 = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
            c2 = m2.upload(feats, off)
            fn2, fd2, _, _ = c2.bigram_mmi_statistics(bg2, trans, scale, capi.GMM_PREFILTER, 0.0, True)
            c2.close()
            bg2.close()
    print("criterion", (fd - fn).sum(), (fd2 - fn2).sum())
    assert np.isfinite(fn).all() and (fd2 - fn2).sum() > (fd - fn).sum()


def test_errors(tmp_path):
    """every SR_EINVAL / SR_ELIMIT of the two entry points; all checks precede any launch (a refused call leaves the handles usable)"""
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 21, 8, 3)
    feats = synth.make_features(20, 12, seed=22)
    off = _off([12, 8])
    L_ = capi.lib()
    P = capi._ptr
    with capi.Model.from_mixset(mp, 12) as m, capi.Model.from_mixset(mp, 12) as m2:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        other = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        cost = np.zeros(2)
        cnt, st, wt = np.zeros(20, np.uint16), np.zeros((20, 2), np.uint16), np.zeros((20, 2))
        tr, toff = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint64)

        def occ(trans=tr, trans_off=toff, scale=1.0, floor=0.0, K=2, net=bg, out=(cost, cnt, st, wt)):
            return L_.sr_bigram_occupancies_corpus(m.h, corpus.h, net.h, capi.GMM_PREFILTER, scale, floor, K, P(trans), P(trans_off), *[P(a) for a in out])

        assert occ() == 0
        assert occ(trans=None) == EINVAL and occ(trans_off=None) == EINVAL          # a partial transcript pair
        assert occ(trans=None, trans_off=None) == 0                                  # the free network
        assert occ(trans=np.array([1, lex.n_words, 3], np.uint32)) == EINVAL         # word id >= n_words
        assert occ(trans=np.array([1, lex.silence_idx, 3], np.uint32)) == EINVAL     # the silence word
        assert occ(trans_off=np.array([1, 2, 3], np.uint64)) == EINVAL               # trans_off[0] != 0
        assert occ(trans_off=np.array([0, 3, 2], np.uint64)) == EINVAL               # decreasing
        for bad in (0.0, -1.0, np.inf, np.nan):
            assert occ(scale=bad) == EINVAL
        assert occ(floor=-0.1) == EINVAL and occ(floor=np.nan) == EINVAL
        assert occ(K=0) == EINVAL and occ(K=65536) == EINVAL
        assert occ(out=(cost, cnt, None, wt)) == EINVAL and occ(out=(None, cnt, st, wt)) == EINVAL
        assert occ(out=(cost, None, None, None), K=0) == 0                           # costs alone: max_items is not looked at
        assert occ(net=other) == EINVAL                                              # a net of another model
        # a chain past 8192 positions: 2100 words of 3 states and as many silence copies
        long_tr = np.ones(2100, np.uint32)
        assert occ(trans=long_tr, trans_off=np.array([0, 2100, 2100], np.uint64)) == ELIMIT and b"chain" in L_.sr_last_error()
        stats = [np.zeros((m.n_densities, 12)), np.zeros(m.n_densities), np.zeros((m.n_densities, 12)), np.zeros(m.n_densities)]
        fn, fd = np.zeros(2), np.zeros(2)

        def mmi(trans=tr, trans_off=toff, outs=None, net=bg, scale=1.0):
            outs = outs if outs is not None else [fn, fd] + stats + [a.copy() for a in stats]
            return L_.sr_bigram_mmi_statistics_corpus(m.h, corpus.h, net.h, capi.GMM_PREFILTER, scale, 0.0, 1, P(trans), P(trans_off), *[P(a) for a in outs])

        assert mmi() == 0
        assert mmi(trans=None, trans_off=None) == EINVAL                             # needs the transcripts
        assert mmi(outs=[fn, None] + stats + stats) == EINVAL and mmi(outs=[fn, fd] + stats + stats[:3] + [None]) == EINVAL
        assert mmi(net=other) == EINVAL and mmi(scale=0.0) == EINVAL
        assert mmi(trans=long_tr, trans_off=np.array([0, 2100, 2100], np.uint64)) == ELIMIT
        for bad_lm, code in ((-np.inf, EINVAL), (-800.0, ELIMIT)):                   # the LM limits of the linear-domain entry
            lm2 = lm.copy()
            lm2[2, 1] = bad_lm
            b2 = m.bigram(word_off, mixtures, lex.silence_idx, lm2, tdp)
            assert occ(net=b2) == code and mmi(net=b2) == code
            if code == ELIMIT:
                assert occ(net=b2, scale=0.5) == 0                                   # -kappa lm = 400: representable
            b2.close()
        assert occ() == 0 and np.isfinite(cost).all()                                # the handles survive the errors
        corpus.close()
        other.close()
        bg.close()


def test_workspace_limit_in_a_child_process(tmp_path):
    """SRGPU_FB_MB = 1: an utterance whose trellis alone exceeds the workspace is SR_ELIMIT from both calls, for the free network
    and for a chain; short utterances still run, one per launch group"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 23, 300, 3)
    data = str(tmp_path / "d.npz")
    np.savez(data, word_off=word_off, mixtures=mixtures, lm=lm, tdp=tdp, long=np.tile(feats, (12, 1))[:600], short=feats[:20])
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from speechrecognition_amd import capi\n"
            "z = np.load(sys.argv[3])\n"
            "with capi.Model.from_mixset(sys.argv[2], 12) as m:\n"
            "    bg = m.bigram(z['word_off'], z['mixtures'], 0, z['lm'], z['tdp'])\n"
            "    c = m.upload(z['long'], np.array([0, len(z['long'])], np.uint64))\n"
            "    for f in (lambda: c.bigram_occupancies(bg, 0.5), lambda: c.bigram_occupancies(bg, 0.5, [[1, 2]]),\n"
            "              lambda: c.bigram_mmi_statistics(bg, [[1, 2]], 0.5)):\n"
            "        try: f(); print('no error')\n"
            "        except capi.SrError as e: print('ELIMIT' if e.code == -4 and 'SRGPU_FB_MB' in str(e) else str(e))\n"
            "    c.close()\n"
            "    s = np.concatenate([z['short'], z['short'][:7], z['short']]); c = m.upload(s, np.array([0, 20, 27, 47], np.uint64))\n"
            "    fn, fd, num, den = c.bigram_mmi_statistics(bg, [[1], [2], [1]], 0.5)\n"
            "    print('finite' if np.isfinite(fd).all() and fd[0] == fd[2] and fn[0] == fn[2] and np.isfinite(fn).all() else (fn, fd))\n"
            "    c.close(); bg.close()\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT, mp, data], env=dict(os.environ, SRGPU_FB_MB="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ELIMIT", "ELIMIT", "ELIMIT", "finite"], r.stdout + r.stderr


# ---- scale shape ------------------------------------------------------------------------------------------------------------------
SAMPLE = (0, 150, 299)


def occ_spread_on_cpu(tmp_path, oracle_lib, sample=SAMPLE):
    """max |log-space reference - linear-domain second evaluation| over the sampled utterances, every 7th frame: (relative on F,
    absolute on the occupancies).  CPU only; neither side is the code under test."""
    lex, mp, word_off, mixtures, lm, feats, off = _scale_case(tmp_path)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    dF = dp = 0.0
    for u in sample:
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        F, p = BM.free_occupancies(e, net, lm, BIG_TDP, 0.1)
        F2, p2 = BM.free_occupancies(e, net, lm, BIG_TDP, 0.1, entry_sum=linear_entry_sum)
        dF, dp = max(dF, _rel(F2, F)), max(dp, float(np.abs(p2[::7] - p[::7]).max()))
    o.close()
    return dF, dp


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from speechrecognition_amd import capi
a = json.load(open(sys.argv[2]))
z = np.load(a["data"])
with capi.Model.from_mixset(a["mp"], 12) as m:
    bg = m.bigram(z["word_off"], z["mixtures"], a["sil"], z["lm"], z["tdp"])
    c = m.upload(z["feats"], z["off"])
    cost, count, state, weight = c.bigram_occupancies(bg, a["scale"], None, capi.GMM_PREFILTER, 1e-4, 8)
    c.close(); bg.close()
np.savez(a["out"], cost=cost, count=count, state=state, weight=weight)
'''


def test_scale_shape(tmp_path, oracle_lib):
    """bench.py's bigram lexicon shape (2667 words, 10 670 positions: 32-bit position lists, silence mixtures of 2667 positions summed
    across a wave), 300 utterances, SRGPU_FB_MB = 64 (about forty launch groups): the free occupancies (8 items, floor 1e-4) and F of
    three utterances (the first, the middle, the last), every 7th frame, against the reference; two identical calls give identical
    bytes.  The tolerance is max(1e-9, 10 x spread): the spread is the largest deviation, measured on the CPU (occ_spread_on_cpu
    above, the same utterances and frames), between the log-space reference and a second numpy evaluation that sums the entry in the
    linear domain in extended precision -- OCC_SPREAD, printed; ten times because the device sums in tile order, not sorted."""
    lex, mp, word_off, mixtures, lm, feats, off = _scale_case(tmp_path)
    assert lex.n_words == 2667
    tol = max(1e-9, 10 * OCC_SPREAD)
    scale, n_utts = 0.1, len(off) - 1
    data = str(tmp_path / "data.npz")
    np.savez(data, word_off=word_off, mixtures=mixtures, lm=lm, tdp=BIG_TDP, feats=feats, off=off)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    outs = []
    for tag in ("one", "again"):
        a = dict(mp=mp, sil=lex.silence_idx, scale=scale, data=data, out=str(tmp_path / f"{tag}.npz"))
        aj = tmp_path / f"{tag}.json"
        aj.write_text(json.dumps(a))
        r = subprocess.run([sys.executable, str(script), ROOT, str(aj)], env=dict(os.environ, SRGPU_FB_MB="64"), capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(np.load(a["out"]))
    one, again = outs
    for k in one.files:
        assert one[k].tobytes() == again[k].tobytes(), k
    cost, count, state, weight = one["cost"], one["count"], one["state"], one["weight"]
    assert np.isfinite(cost).all()
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    worst_F = worst_p = 0.0
    for u in (0, n_utts // 2, n_utts - 1):
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        F, occ = BM.free_occupancies(e, net, lm, BIG_TDP, scale)
        worst_F = max(worst_F, _rel(cost[u], F))
        for tt in range(0, occ.shape[0], 7):
            ft = int(off[u]) + tt
            n = int(count[ft])
            assert n > 0
            worst_p = max([worst_p] + [abs(weight[ft, i] - occ[tt, state[ft, i]]) for i in range(n)])
            want = sorted((x for x in occ[tt] if x >= 1e-4 + tol), reverse=True)[:8]  # nothing clearly above the floor is missing
            assert n >= len(want) and all(abs(weight[ft, i] - want[i]) <= tol for i in range(len(want)))
    print(f"scale shape: spread {OCC_SPREAD:.3g}; device against the reference, worst relative F {worst_F:.3g}, worst absolute "
          f"occupancy {worst_p:.3g} (bound {tol:.3g})")
    o.close()
    assert worst_F <= 1e-10 and worst_p <= tol


def test_cpp_driver(tmp_path):
    """sr::LinearSearch::mmi_statistics (include/sr_sietill.hpp) through tests/cpp/bigram_mmi_driver.cpp: the binding's bits"""
    exe = str(tmp_path / "bigram_mmi_driver")
    lib_dir = os.path.join(ROOT, "speechrecognition_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bigram_mmi_driver.cpp"),
                    "-o", exe, "-L", lib_dir, "-lsrgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 99, 20, 3)
    utts, allf, off, trans = _corpus(feats, 99, lex.n_words)
    W, scale, floor = len(word_off) - 1, 0.25, 1e-6
    blob = struct.pack("<I", W) + np.asarray(word_off, "<u4").tobytes() + np.asarray(mixtures, "<u2").tobytes()
    blob += struct.pack("<I", lex.silence_idx) + np.asarray(lm, "<f4").tobytes() + np.asarray(tdp, "<f4").tobytes()
    blob += struct.pack("<Idd", capi.GMM_DEFAULT, scale, floor) + struct.pack("<I", len(utts))
    for f, tr in zip(utts, trans):
        blob += struct.pack(f"<I{len(tr)}II", len(tr), *tr, len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "mmi", mp, "12", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        fn, fd, num, den = corpus.bigram_mmi_statistics(bg, trans, scale, capi.GMM_DEFAULT, floor, True)
        corpus.close()
        bg.close()
    hx = lambda x: f"{int(np.float64(x).view(np.uint64)):x}"  # noqa: E731
    want = [f"cost {u} {hx(fn[u])} {hx(fd[u])}" for u in range(len(utts))]
    for s, side in enumerate((num, den)):
        for a, arr in enumerate(side):
            want += [f"stat {s} {a} {i} {hx(x)}" for i, x in enumerate(arr.reshape(-1))]
    assert num[1].sum() > 0 and den[1].sum() > 0 and out.stdout.splitlines() == want
