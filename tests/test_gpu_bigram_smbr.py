"""sMBR training against the bigram search network on the device: sr_bigram_accuracies_corpus and sr_bigram_smbr_statistics_corpus
against the numpy restatement (tests/bigram_smbr_reference.py, pinned by tests/test_bigram_smbr_cpu.py), the bigram word posteriors
and occupancies, and themselves.  Tolerances are the project's (test_gpu_smbr.py / test_gpu_bigram_mmi.py): F 1e-10 relative; Abar
and every gamma 1e-9 (1 + T_u) absolute; statistics 1e-9 relative to sum |w x| (test_gpu_mmi._check_stats).  Beside them, wherever it is tighter, the measured rule of tests/test_gpu_bgfb_scores.py against the restatement's
np.longdouble run (bigram_fb_cases.measured: 8 times the distance of the farther of the log-space and the linear-domain float64
restatement plus 4 ulp of the value; the `RULE` lines say which of the two holds); the statistics keep their fixed bound.

Where the statistics are compared.  A weight gamma = occ (c - Abar) carries the absolute rounding error of c - Abar, a few ulp of
Abar, in the device and in the restatement alike.  Where one mixture holds ALL of a frame's posterior in FP64 (every other path's
exp underflows) its weight is 0 in exact arithmetic and pure rounding noise in either evaluation, and a density that collects only such
weights has statistics made of noise: at kappa = 1 on _setup's sampled utterances the restatement disagrees with ITSELF (evaluated
with every frame scoring one more, which changes neither Abar nor gamma in exact arithmetic) by 3.8e-7 to 2.5 times sum |w x|, at
kappa = 0.3 by up to 5.6e-9, at kappa = 0.1 and 0.05 by at most 3e-12 (every shape, floor and membership mode; the tight-variance
task of test_one_state_words_negative_costs: 1e0 and more at any kappa).  So F, Abar and every gamma are compared at kappa = 1 and
0.3 too, the statistics at STAT_SCALES, and _against_restatement asserts from the restatement alone, before it looks at the device,
that this self-disagreement is below a tenth of the tolerance."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import bigram_fb_cases as bc
from tests import bigram_fb_reference as R
from tests import bigram_smbr_reference as BS
from tests import fb_reference as FB
from tests import smbr_reference as SM
from tests.test_bigram import _setup
from tests.test_bigram_mmi_cpu import criterion_task
from tests.test_bigram_smbr_cpu import BIGRAM_SMBR_E
from tests.test_gpu_bigram_mmi import SHAPES, _forbid, _off
from tests.test_gpu_mmi import _check_stats, launch_groups
from tests.test_gpu_smbr import _check_signed_items
from tests.test_gpu_word_posteriors import _rel
from tests.test_smbr_cpu import criterion_refs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ELIMIT = -1, -4  # include/srgpu.h
STAT_SCALES = (0.1, 0.05)  # see the module's docstring


def _corpus(feats, seed, S):
    """utterances and references: the sampled utterance, T = 1, T = 0 between two others, noise, half of the first, three frames
    (every reference out of range).  The references are random mixtures with single out-of-range frames among them."""
    rng = np.random.default_rng(seed + 7)
    half = feats[: len(feats) // 2]
    utts = [feats, feats[:1], feats[:0], rng.standard_normal((37, feats.shape[1])).astype(np.float32), half, feats[:3]]
    off = _off([len(x) for x in utts])
    ref = rng.integers(0, S, size=int(off[-1])).astype(np.uint16)
    ref[5] = S + 7
    ref[int(off[3]) + 11] = 65535
    ref[int(off[5]):] = S
    return utts, np.concatenate(utts), off, ref


def _refs(o, utts, off, ref, net, lm, tdp, scale, S, shift=0.0):
    """per utterance the restatement's (F, Abar, gamma)"""
    out = []
    for u, x in enumerate(utts):
        e = o.score_matrix(x) if len(x) else np.zeros((0, S))
        out.append(BS.smbr(e, net, lm, tdp, ref[int(off[u]):int(off[u + 1])].astype(np.int64), scale, shift))
    return out


def _rules(o, utts, off, ref, net, lm, tdp, scale, S, res):
    """per utterance the longdouble run and the measured bounds on F, Abar and every gamma, where they are tighter than 1e-10 relative
    and 1e-9 (1 + T) (bigram_fb_cases.measured; the `RULE` lines say which holds)"""
    out = []
    for u, x in enumerate(utts):
        e = o.score_matrix(x) if len(x) else np.zeros((0, S))
        r = ref[int(off[u]):int(off[u + 1])].astype(np.int64)
        run = lambda e=e, r=r, **kw: BS.smbr(e, net, lm, tdp, r, scale, **kw)  # noqa: E731
        tol = 1e-9 * (1 + len(x))
        out.append(bc.measured(run, res[u], bc.lin_entry_mean(net.sil), (1e-10 * max(1.0, abs(float(res[u][0]))), tol, tol),
                               f"utterance {u} kappa {scale}"))
    return out


def _side_items(res, floor):
    items = [[], []]
    for _, _, g in res:
        items[0] += SM.signed_items(g, +1, floor)
        items[1] += SM.signed_items(g, -1, floor)
    return items


def _well_conditioned(res, shifted, feats, tables, nm, nv, max_approx, floor):
    """the precondition of a statistics comparison, from the restatement alone: its sums under the two evaluations agree to a tenth
    of the tolerance (1e-10 of sum |w x|)"""
    worst = 0.0
    for a, b in zip(_side_items(res, floor), _side_items(shifted, floor)):
        x, y = (FB.accumulate(feats, it, tables, nm, nv, False, max_approx) for it in (a, b))
        worst = max(worst, float((np.abs(x[0] - y[0]) / np.maximum(x[4], 1e-300)).max()), float((np.abs(x[2] - y[2]) / np.maximum(x[5], 1e-4)).max()))
    print("restatement against itself", max_approx, floor, worst)
    assert worst <= 1e-10, worst


def _stats(got, feats, items, tables, max_approx, tag):
    """test_gpu_mmi._check_stats, the worst |device - restatement| / sum |w x| of the mean and variance sums printed first"""
    nm, nv = len(got[1]), len(got[3])
    ma, mw, va, vw, sm, sv = FB.accumulate(feats, items, tables, nm, nv, False, max_approx)
    print("statistics", tag, "worst mean_acc", float((np.abs(got[0] - ma) / np.maximum(sm, 1e-300)).max()),
          "worst var_acc", float((np.abs(got[2] - va) / np.maximum(sv, 1e-4)).max()))
    _check_stats(got, feats, items, tables, max_approx)


def _against_restatement(o, m, bg, allf, off, ref, res, scale, S, floors=(0.0, 1e-6), modes=((True, 0.0), (False, 1e-6)), shifted=None,
                         rules=None):
    """F, Abar and the signed items for every floor and K in (1, 3, S); then, with `shifted` (the restatement's second evaluation),
    both statistics sides for every membership mode; without it the statistics call's F and Abar alone"""
    tables = o.tables()
    corpus = m.upload(allf, off)
    for floor in floors:
        for K in (1, 3, S):
            cost, acc, count, state, weight = corpus.bigram_accuracies(bg, ref, scale, capi.GMM_PREFILTER, floor, K)
            for u, (F, A, g) in enumerate(res):
                T = g.shape[0]
                tol = 1e-9 * (1 + T)
                print("utt", u, cost[u], F, acc[u], A)
                assert _rel(cost[u], F) <= 1e-10 and abs(acc[u] - A) <= tol and 0.0 <= acc[u] <= T + tol
                (F80, A80, g80), (tolF, tolA, tolg) = rules[u] if rules else ((F, A, g), (np.inf, np.inf, np.full(g.shape, np.inf)))
                assert cost[u] == F80 or abs(bc.LD(cost[u]) - F80) <= tolF, (u, cost[u], F80, tolF)
                # (Abar, a sum of occupancies, is held to the larger of its own bound and the weights': test_gpu_bgsmbr_scores.py)
                assert abs(bc.LD(acc[u]) - A80) <= max(float(tolA), float(np.max(tolg)) if tolg.size else 0.0), (u, acc[u], A80, tolA)
                for t in range(T):
                    ft = int(off[u]) + t
                    _check_signed_items(g[t], count[ft], state[ft], weight[ft], floor, K, tol, g80[t], tolg[t])
                    if K == S and floor == 0.0:
                        assert abs(weight[ft].sum()) <= tol
    for max_approx, floor in modes:
        cost, acc, num, den = corpus.bigram_smbr_statistics(bg, ref, scale, capi.GMM_PREFILTER, floor, max_approx)
        for u, (F, A, g) in enumerate(res):
            assert _rel(cost[u], F) <= 1e-10 and abs(acc[u] - A) <= 1e-9 * (1 + g.shape[0])
        if shifted is None:
            continue
        _well_conditioned(res, shifted, allf, tables, len(num[1]), len(num[3]), max_approx, floor)
        items = _side_items(res, floor)
        _stats(num, allf, items[0], tables, max_approx, ("num", scale, max_approx, floor))
        _stats(den, allf, items[1], tables, max_approx, ("den", scale, max_approx, floor))
        if floor == 0.0:
            total = sum(np.abs(g).sum() for _, _, g in res)
            print("balance", num[1].sum(), den[1].sum(), total)
            assert abs(num[1].sum() - den[1].sum()) <= 1e-9 * total
    corpus.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_against_restatement(shape, tmp_path, oracle_lib):
    """test_gpu_bigram_mmi's shapes (a multi-state silence, one-state words among them), forbidden LM entries (+inf, NaN), T = 1 and
    T = 0 between two others, references with out-of-range frames and an utterance without any reference in range; F, Abar and the
    items at four scales, the statistics of both membership modes at STAT_SCALES"""
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    lm = _forbid(lm)
    S = lex.n_states
    utts, allf, off, ref = _corpus(feats, seed, S)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        for scale in (1.0, 0.3) + STAT_SCALES:
            res = _refs(o, utts, off, ref, net, lm, tdp, scale, S)
            assert res[2][0] == 0.0 and res[2][1] == 0.0           # T = 0
            assert np.isfinite(res[0][0]) and np.isfinite(res[3][0]) and res[0][1] > 0.0
            assert res[5][1] == 0.0 and not res[5][2].any()         # every reference out of range
            shifted = _refs(o, utts, off, ref, net, lm, tdp, scale, S, 1.0) if scale in STAT_SCALES else None
            _against_restatement(o, m, bg, allf, off, ref, res, scale, S, shifted=shifted,
                                 rules=_rules(o, utts, off, ref, net, lm, tdp, scale, S, res))
        bg.close()
    o.close()


def test_one_state_words_negative_costs(tmp_path, oracle_lib):
    """tight variances: emission costs below 0; negative LM scores, forbidden entries; one-state words.  F, Abar and every gamma, from
    both entry points; the statistics themselves are not compared here (the module's docstring: under these variances every frame's
    posterior sits on one mixture and the restatement's own sums are rounding noise)."""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 41, 9, 1)
    synth.scale_variances(spec, 0.004)
    synth.write_mixset(mp, spec)
    feats = synth.sample_utterance(spec, lex, [1, 5, 2, 8], seed=43)
    lm = _forbid((lm - 2.0).astype(np.float32))
    S = lex.n_states
    utts, allf, off, ref = _corpus(feats, 41, S)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    assert o.score_matrix(allf).min() < 0
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        res = _refs(o, utts, off, ref, net, lm, tdp, 0.5, S)
        assert np.isfinite(res[0][0])
        _against_restatement(o, m, bg, allf, off, ref, res, 0.5, S, floors=(0.0,), modes=((True, 0.0),),
                             rules=_rules(o, utts, off, ref, net, lm, tdp, 0.5, S, res))
        bg.close()
    o.close()


def _occ_acc(corpus, bg, scale, ref, off, S):
    """sum_t occ_t(ref_t) per utterance from sr_bigram_occupancies_corpus (free network, floor 0, max_items S)"""
    _, count, state, weight = corpus.bigram_occupancies(bg, scale, None, capi.GMM_PREFILTER, 0.0, S)
    out = np.zeros(len(off) - 1)
    for u in range(len(off) - 1):
        for t in range(int(off[u]), int(off[u + 1])):
            hit = state[t, :count[t]] == ref[t]
            out[u] += weight[t, :count[t]][hit].sum()
    return out


def test_consistency_with_posteriors_and_occupancies(tmp_path):
    """out_cost is sr_bigram_word_posteriors_corpus' F bit for bit (both entry points); Abar_u = sum_t occ_t(ref_t) of
    sr_bigram_occupancies_corpus; the signed items of a frame sum to 0 at floor 0; constant references k = 0 .. S - 1 give accuracies
    that sum to T_u (0 without a complete path)"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 33, 6, 3, sil_states=4, tdp=np.array(
        [[3.0, 0.0, 30.0, 5.0], [1.0, 7.0, 3.0, 2.0]], np.float32))
    S = lex.n_states
    utts, allf, off, ref = _corpus(feats, 33, S)
    T = np.diff(off.astype(np.int64))
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        for scale in (1.0, 0.2):
            cw = corpus.bigram_word_posteriors(bg, scale, capi.GMM_PREFILTER, 0.0, 1)[0]
            cost, acc, count, state, weight = corpus.bigram_accuracies(bg, ref, scale, capi.GMM_PREFILTER, 0.0, S)
            cs, accs = corpus.bigram_smbr_statistics(bg, ref, scale)[:2]
            assert np.array_equal(cw.view(np.uint64), cost.view(np.uint64)) and np.array_equal(cw.view(np.uint64), cs.view(np.uint64))
            assert np.array_equal(acc.view(np.uint64), accs.view(np.uint64))
            assert np.isfinite(cost[0]) and np.isfinite(cost[3])
            want = _occ_acc(corpus, bg, scale, ref, off, S)
            print("acc", acc, want)
            assert np.all(np.abs(acc - want) <= 1e-9 * (1 + T)) and np.all(acc >= 0.0) and np.all(acc <= T + 1e-9 * (1 + T))
            utt = np.searchsorted(off, np.arange(len(allf)), side="right") - 1
            assert np.all(np.abs(weight.sum(axis=1)) <= 1e-9 * (1 + T[utt]))
            total = sum(corpus.bigram_accuracies(bg, np.full(len(allf), k, np.uint16), scale, capi.GMM_PREFILTER, 0.0, 1)[1] for k in range(S))
            assert np.all(np.abs(total - np.where(np.isfinite(cost), T, 0)) <= 1e-9 * (1 + T))
        corpus.close()
        bg.close()


@pytest.mark.parametrize("W,spw", [(20, 2), (70, 1)])
def test_wide_silence_mixture(W, spw, tmp_path, oracle_lib):
    """the silence mixture is carried by the silence word and every slot's copy: W + 2 positions for W words beside silence -- more
    than the 16 a lane sums alone (W = 20) and more than a wave's 64 lanes (W = 70), so bgocc_items' whole-wave path runs in its
    signed mode, with one and with two strides"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 50 + W, W, spw)
    S = lex.n_states
    net = R.Net(word_off, mixtures, lex.silence_idx)
    carried = int((net.state == mixtures[word_off[lex.silence_idx]]).sum())
    assert carried == lex.n_words + 1 and carried > (16 if W == 20 else 64)
    rng = np.random.default_rng(W)
    utts = [feats[:23], feats[:9]]
    allf, off = np.concatenate(utts), _off([23, 9])
    ref = rng.integers(0, S, size=32).astype(np.uint16)
    ref[::3] = mixtures[word_off[lex.silence_idx]]  # the wide mixture carries hits
    o = oracle_lib.Oracle(mp, 12, lex)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        res = _refs(o, utts, off, ref, net, lm, tdp, 0.4, S)
        assert np.isfinite(res[0][0]) and np.abs(res[0][2][:, mixtures[word_off[lex.silence_idx]]]).max() > 1e-6
        shifted = _refs(o, utts, off, ref, net, lm, tdp, 0.4, S, 1.0)
        _against_restatement(o, m, bg, allf, off, ref, res, 0.4, S, floors=(0.0,), modes=((True, 0.0),), shifted=shifted)
        bg.close()
    o.close()


GROUPS_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from speechrecognition_amd import capi
z = np.load(sys.argv[3])
with capi.Model.from_mixset(sys.argv[2], 12) as m:
    bg = m.bigram(z["word_off"], z["mixtures"], 0, z["lm"], z["tdp"])
    c = m.upload(z["long"], np.array([0, len(z["long"])], np.uint64))
    for f in (lambda: c.bigram_accuracies(bg, z["long_ref"], 0.5), lambda: c.bigram_smbr_statistics(bg, z["long_ref"], 0.5)):
        try:
            f()
            print("no error")
        except capi.SrError as e:
            print("ELIMIT" if e.code == -4 and "SRGPU_FB_MB" in str(e) else str(e))
    c.close()
    c = m.upload(z["feats"], z["off"])
    a = c.bigram_accuracies(bg, z["ref"], 0.5, capi.GMM_PREFILTER, 1e-6, 3)
    s = c.bigram_smbr_statistics(bg, z["ref"], 0.5, capi.GMM_PREFILTER, 1e-6, False)
    c.close(); bg.close()
np.savez(sys.argv[4], *a, s[0], s[1], *s[2], *s[3])
'''


def _group_outputs(mp, z):
    with capi.Model.from_mixset(mp, 12) as m:  # (the budget is read when the model is made)
        bg = m.bigram(z["word_off"], z["mixtures"], 0, z["lm"], z["tdp"])
        c = m.upload(z["feats"], z["off"])
        a = c.bigram_accuracies(bg, z["ref"], 0.5, capi.GMM_PREFILTER, 1e-6, 3)
        s = c.bigram_smbr_statistics(bg, z["ref"], 0.5, capi.GMM_PREFILTER, 1e-6, False)
        c.close()
        bg.close()
    return [*a, s[0], s[1], *s[2], *s[3]]


def test_several_launch_groups_in_a_child_process(tmp_path):
    """SRGPU_FB_MB = 1 in a child process: the corpus falls into several launch groups (the pass' bytes: 16 P T plus 48 Kp + 32 P + 16
    per utterance), one of several utterances and one of a single one, and every output equals the one-group run's bytes; an
    utterance that alone needs more than the workspace is SR_ELIMIT from both calls"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 23, 60, 3)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    Kp = (lex.n_words + 63) // 64 * 64
    rng = np.random.default_rng(24)
    lens = [100, 140, 41, 250, 12, 60, 1]  # (groups (0, 2), (2, 3), (3, 4), (4, 7): the longest is not the first in two of them)
    pool = np.tile(feats, (6, 1))
    utts = [pool[i:i + n] for i, n in enumerate(lens)]
    allf, off = np.concatenate(utts), _off(lens)
    cost = [16 * net.P * n + 48 * Kp + 32 * net.P + 16 for n in lens]
    assert max(cost) < 1 << 20 and sum(cost) < 64 << 20
    groups = launch_groups(cost)
    sizes = [b - a for a, b in groups]
    assert len(groups) >= 3 and 1 in sizes and max(sizes) > 1, groups
    long = np.tile(feats, (12, 1))[:600]
    assert 16 * net.P * len(long) > 1 << 20
    z = dict(word_off=word_off, mixtures=mixtures, lm=lm, tdp=tdp, feats=allf, off=off,
             ref=rng.integers(0, lex.n_states, size=len(allf)).astype(np.uint16), long=long,
             long_ref=rng.integers(0, lex.n_states, size=len(long)).astype(np.uint16))
    data, out = str(tmp_path / "d.npz"), str(tmp_path / "out.npz")
    np.savez(data, **z)
    script = tmp_path / "child.py"
    script.write_text(GROUPS_CHILD)
    env = dict(os.environ, SRGPU_FB_MB="1")
    r = subprocess.run([sys.executable, str(script), ROOT, mp, data, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ELIMIT", "ELIMIT"], r.stdout + r.stderr
    assert "SRGPU_FB_MB" not in os.environ
    one = _group_outputs(mp, z)
    cut = np.load(out)
    assert len(cut.files) == len(one) == 15
    for i, a in enumerate(one):
        assert np.asarray(a).tobytes() == cut[f"arr_{i}"].tobytes(), i
    assert np.isfinite(one[0]).all() and one[1].sum() > 0 and one[2].any()


def test_determinism_and_shards(tmp_path):
    """two identical calls return identical bytes, a call at another kappa in between (the table cache); the statistics of two
    half-corpora add up to the whole (the 1e-4 seed once per call and side); the halves' costs and accuracies concatenated are the
    whole's bits"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 15, 40, 3)
    utts, allf, off, ref = _corpus(feats, 15, lex.n_states)
    flat = lambda r: [r[0], r[1], *r[2], *r[3]]  # noqa: E731
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        a = corpus.bigram_smbr_statistics(bg, ref, 0.4, capi.GMM_PREFILTER, 1e-8, False)
        oa = corpus.bigram_accuracies(bg, ref, 0.4, max_items=5)
        other = corpus.bigram_smbr_statistics(bg, ref, 0.9, capi.GMM_PREFILTER, 1e-8, False)
        assert not np.array_equal(other[1], a[1])
        b = corpus.bigram_smbr_statistics(bg, ref, 0.4, capi.GMM_PREFILTER, 1e-8, False)
        ob = corpus.bigram_accuracies(bg, ref, 0.4, max_items=5)
        corpus.close()
        for x, y in zip(flat(a), flat(b)):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(oa, ob):
            assert x.tobytes() == y.tobytes()
        assert oa[1].tobytes() == a[1].tobytes() and a[2][1].sum() > 0 and a[3][1].sum() > 0
        halves = []
        for u0, u1 in ((0, 3), (3, 6)):
            f0, f1 = int(off[u0]), int(off[u1])
            part = m.upload(allf[f0:f1], off[u0:u1 + 1] - off[u0])
            halves.append(part.bigram_smbr_statistics(bg, ref[f0:f1], 0.4, capi.GMM_PREFILTER, 1e-8, False))
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


def test_one_ebw_step_raises_the_expected_accuracy(tmp_path, oracle_lib):
    """one EBW step through sr_model_create_from_mmi_statistics and a fresh sr_bigram on the new model raises sum_u Abar_u on the
    task tests/test_bigram_smbr_cpu.py vetted, at its E = 32: under the restatement 83.36 of 152 frames before the step, 84.22 after
    (64.33 at E = 8, 67.51 at E = 16, 95.31 at E = 64)"""
    lex, mp, word_off, mixtures, lm, tdp, feats, off, trans, scale = criterion_task(tmp_path)
    o = oracle_lib.Oracle(mp, 12, lex)
    ref = criterion_refs(o, lex, feats, off, trans)
    o.close()
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        cost, acc, num, den = corpus.bigram_smbr_statistics(bg, ref, scale, capi.GMM_PREFILTER, 0.0, True)
        corpus.close()
        bg.close()
        with m.from_mmi_statistics(num, den, BIGRAM_SMBR_E, 0.0, 1e-3) as m2:
            bg2 = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
            c2 = m2.upload(feats, off)
            acc2 = c2.bigram_accuracies(bg2, ref, scale, capi.GMM_PREFILTER, 0.0, 1)[1]
            c2.close()
            bg2.close()
    print("expected accuracy", acc.sum(), acc2.sum(), len(feats))
    assert np.isfinite(cost).all() and abs(acc.sum() - 83.36) < 0.01 and acc2.sum() > acc.sum()


def test_errors(tmp_path):
    """every SR_EINVAL / SR_ELIMIT of the two entry points, outputs untouched; all checks precede any launch (a refused call leaves the
    handles usable)"""
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 21, 8, 3)
    feats = synth.make_features(20, 12, seed=22)
    off = _off([12, 8])
    L_ = capi.lib()
    P = capi._ptr
    mark = 7.0
    with capi.Model.from_mixset(mp, 12) as m, capi.Model.from_mixset(mp, 12) as m2:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        other = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        foreign = m2.upload(feats, off)
        ref = np.zeros(20, np.uint16)
        cost, acc = np.full(2, mark), np.full(2, mark)
        cnt, st, wt = np.full(20, 7, np.uint16), np.full((20, 2), 7, np.uint16), np.full((20, 2), mark)

        def call(scale=1.0, floor=0.0, K=2, net=bg, refs=ref, out=(cost, acc, cnt, st, wt), ch=corpus.h):
            return L_.sr_bigram_accuracies_corpus(m.h, ch, net.h, capi.GMM_PREFILTER, scale, floor, K, P(refs), *[P(a) for a in out])

        bad = [dict(scale=0.0), dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan), dict(floor=-0.1), dict(floor=np.nan),
               dict(K=0), dict(K=65536), dict(refs=None), dict(out=(None, acc, cnt, st, wt)), dict(out=(cost, None, cnt, st, wt)),
               dict(out=(cost, acc, None, st, wt)), dict(out=(cost, acc, cnt, None, wt)), dict(out=(cost, acc, cnt, st, None)),
               dict(net=other), dict(ch=foreign.h)]
        for kw in bad:
            assert call(**kw) == EINVAL, kw
        nd = m.n_densities
        stats = [np.full((nd, 12), mark), np.full(nd, mark), np.full((nd, 12), mark), np.full(nd, mark)]
        outs = [np.full(2, mark), np.full(2, mark)] + stats + [a.copy() for a in stats]

        def smbr(scale=1.0, floor=0.0, refs=ref, o=outs, net=bg):
            return L_.sr_bigram_smbr_statistics_corpus(m.h, corpus.h, net.h, capi.GMM_PREFILTER, scale, floor, 1, P(refs), *[P(a) for a in o])

        for kw in [dict(scale=0.0), dict(scale=np.inf), dict(floor=-1.0), dict(refs=None), dict(net=other)] + \
                [dict(o=outs[:i] + [None] + outs[i + 1:]) for i in range(10)]:
            assert smbr(**kw) == EINVAL, kw
        for bad_lm, code in ((-np.inf, EINVAL), (-800.0, ELIMIT)):  # the LM limits of the linear-domain entry
            lm2 = lm.copy()
            lm2[2, 1] = bad_lm
            b2 = m.bigram(word_off, mixtures, lex.silence_idx, lm2, tdp)
            assert call(net=b2) == code and smbr(net=b2) == code
            if code == ELIMIT:
                assert call(net=b2, scale=0.5) == 0  # -kappa lm = 400: representable
                cost[:], acc[:], cnt[:], st[:], wt[:] = mark, mark, 7, 7, mark
            b2.close()
        assert (cost == mark).all() and (acc == mark).all() and (cnt == 7).all() and (st == 7).all() and (wt == mark).all()
        assert all((a == mark).all() for a in outs)
        assert call(out=(cost, acc, None, None, None), K=0) == 0  # cost and accuracy alone: max_items is not looked at
        assert call() == 0 and smbr() == 0 and np.isfinite(cost).all()  # the handles survive the errors
        foreign.close()
        corpus.close()
        other.close()
        bg.close()


def test_cpp_driver(tmp_path):
    """sr::LinearSearch::smbr_statistics and ::accuracies (include/sr_sietill.hpp) through tests/cpp/bigram_smbr_driver.cpp: the
    binding's bits"""
    exe = str(tmp_path / "bigram_smbr_driver")
    lib_dir = os.path.join(ROOT, "speechrecognition_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bigram_smbr_driver.cpp"),
                    "-o", exe, "-L", lib_dir, "-lsrgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 99, 20, 3)
    utts, allf, off, ref = _corpus(feats, 99, lex.n_states)
    W, scale, floor, K = len(word_off) - 1, 0.25, 1e-6, 3
    blob = struct.pack("<I", W) + np.asarray(word_off, "<u4").tobytes() + np.asarray(mixtures, "<u2").tobytes()
    blob += struct.pack("<I", lex.silence_idx) + np.asarray(lm, "<f4").tobytes() + np.asarray(tdp, "<f4").tobytes()
    blob += struct.pack("<IddI", capi.GMM_DEFAULT, scale, floor, K) + struct.pack("<I", len(utts))
    for u, f in enumerate(utts):
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes() + np.asarray(ref[int(off[u]):int(off[u + 1])], "<u2").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "smbr", mp, "12", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        cost, acc, num, den = corpus.bigram_smbr_statistics(bg, ref, scale, capi.GMM_DEFAULT, floor, True)
        _, _, count, state, weight = corpus.bigram_accuracies(bg, ref, scale, capi.GMM_DEFAULT, floor, K)
        corpus.close()
        bg.close()
    hx = lambda x: f"{int(np.float64(x).view(np.uint64)):x}"  # noqa: E731
    want = [f"cost {u} {hx(cost[u])} {hx(acc[u])}" for u in range(len(utts))]
    for s, side in enumerate((num, den)):
        for a, arr in enumerate(side):
            want += [f"stat {s} {a} {i} {hx(x)}" for i, x in enumerate(arr.reshape(-1))]
    for t in range(len(allf)):
        want.append(" ".join([f"item {t} {count[t]}"] + [f"{state[t, i]} {hx(weight[t, i])}" for i in range(count[t])]))
    assert num[1].sum() > 0 and den[1].sum() > 0 and count.any() and out.stdout.splitlines() == want
