"""Word posteriors and confidences of the bigram search on the device (sr_bigram_word_posteriors_corpus,
sr_recognize_bigram_confidence_corpus) against the numpy restatement of its network's forward-backward
(tests/bigram_fb_reference.py) on the oracle's emission costs.  Tolerances: F_u 1e-10 relative, posteriors and confidences 1e-9
absolute (the project's for the zerogram network; the product's summation error, about W T 2^-53 on an exponent, is far below them
at these sizes).  Beside them, wherever it is tighter, the measured rule of tests/test_gpu_bgfb_scores.py against the restatement's
np.longdouble run (bigram_fb_cases.measured: 8 times the distance of the farther of the log-space and the linear-domain float64
restatement plus 4 ulp of the value; the `RULE` lines say which of the two holds); test_scale_shape keeps the fixed pair (a
longdouble run of its 2 667-word entry sums takes minutes)."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import bigram_fb_cases as bc
from tests import bigram_fb_reference as R
from tests.test_bigram import FLT_MAX, SIL_TDP, _setup
from tests.test_gpu_word_posteriors import _check_items, _rel

pytestmark = pytest.mark.gpu

# test_bigram.py's _setup shapes (seed, W, states per word, silence states, tdp) and a few beyond them
SHAPES = [(1, 5, 3, 1, None), (2, 7, 2, 1, None), (3, 4, 4, 2, None), (4, 6, 1, 1, None), (31, 6, 3, 2, SIL_TDP), (33, 6, 3, 4, SIL_TDP),
          (15, 40, 3, 1, None), (16, 70, 2, 2, SIL_TDP)]


def _corpus(feats, seed):
    """the sampled utterance, noise, a T = 0 utterance between two others, half of the first, T = 1"""
    rng = np.random.default_rng(seed + 5)
    utts = [feats, rng.standard_normal((37, 12)).astype(np.float32), feats[:0], feats[: len(feats) // 2], feats[:1]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    return utts, np.concatenate(utts), off


def _refs(o, utts, net, lm, tdp, scale):
    return [R.posteriors(o.score_matrix(x) if len(x) else np.zeros((0, 1)), net, lm, tdp, scale) for x in utts]


def _rules(o, utts, net, lm, tdp, scale, refs):
    """per utterance the longdouble run and the measured bounds on F and on every posterior, where they are tighter than 1e-10 relative
    and 1e-9 (bigram_fb_cases.measured; the `RULE` lines say which holds)"""
    out = []
    for u, x in enumerate(utts):
        e = o.score_matrix(x) if len(x) else np.zeros((0, 1))
        run = lambda e=e, **kw: R.posteriors(e, net, lm, tdp, scale, **kw)  # noqa: E731
        out.append(bc.measured(run, refs[u], bc.lin_entry(net.sil), (1e-10 * max(1.0, abs(float(refs[u][0]))), 1e-9), f"utterance {u} kappa {scale}"))
    return out


def _against(corpus, bg, refs, off, W, scale, floors=(0.0, 1e-6), Ks=None, rules=None):
    for floor in floors:
        for K in (Ks or (1, 3, W)):
            cost, count, word, weight = corpus.bigram_word_posteriors(bg, scale, capi.GMM_PREFILTER, floor, K)
            for u, (F, p) in enumerate(refs):
                assert _rel(cost[u], F) <= 1e-10, (u, cost[u], F)
                (F80, p80), (tolF, tolp) = rules[u] if rules else ((F, p), (np.inf, np.full(p.shape, np.inf)))
                assert cost[u] == F80 or abs(bc.LD(cost[u]) - F80) <= tolF, (u, cost[u], F80, tolF)
                for t in range(p.shape[0]):
                    ft = int(off[u]) + t
                    _check_items(p[t], count[ft], word[ft], weight[ft], floor, K, p80[t], tolp[t])


@pytest.mark.parametrize("shape", SHAPES)
def test_posteriors_against_restatement(shape, tmp_path, oracle_lib):
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    utts, allf, off = _corpus(feats, seed)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        for scale in (1.0, 0.3):  # (the second call rebuilds the cached table for its kappa)
            refs = _refs(o, utts, net, lm, tdp, scale)
            assert refs[2][0] == 0.0
            _against(corpus, bg, refs, off, lex.n_words, scale, Ks=(1, lex.n_words) if W > 10 else None,
                     rules=_rules(o, utts, net, lm, tdp, scale, refs))
        corpus.close()
        bg.close()
    o.close()


def test_one_state_words_negative_costs_and_forbidden_transitions(tmp_path, oracle_lib):
    """tight variances: emission costs below 0; +inf and NaN LM entries, negative LM scores"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 41, 9, 1)
    synth.scale_variances(spec, 0.004)
    synth.write_mixset(mp, spec)
    feats = synth.sample_utterance(spec, lex, [1, 5, 2, 8], seed=43)  # (drawn from the tightened model: close to its means)
    rng = np.random.default_rng(42)
    lm = (lm - 2.0).astype(np.float32)
    lm[rng.random(lm.shape) < 0.15] = np.inf
    lm[:, 3] = np.nan
    lm[2, 0] = 1.0  # (some word can follow the start's silence history)
    lm = np.ascontiguousarray(lm)
    utts, allf, off = _corpus(feats, 41)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    assert o.score_matrix(allf).min() < 0
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        refs = _refs(o, utts, net, lm, tdp, 0.5)
        _against(corpus, bg, refs, off, lex.n_words, 0.5, floors=(0.0,), rules=_rules(o, utts, net, lm, tdp, 0.5, refs))
        corpus.close()
        bg.close()
    o.close()


def test_identical_calls_identical_bytes(tmp_path, oracle_lib):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 15, 40, 3)
    utts, allf, off = _corpus(feats, 15)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        a = corpus.bigram_word_posteriors(bg, 0.4, max_items=5)
        b = corpus.bigram_word_posteriors(bg, 0.4, max_items=5)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        other = corpus.bigram_word_posteriors(bg, 0.9, max_items=5)   # another kappa in between
        assert not np.array_equal(other[0], a[0])
        c = corpus.bigram_word_posteriors(bg, 0.4, max_items=5)
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes()
        corpus.close()
        bg.close()


@pytest.mark.parametrize("beams", [(FLT_MAX, FLT_MAX), (60.0, 30.0)])
def test_confidences(beams, tmp_path, oracle_lib):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 12, 9, 2)
    utts, allf, off = _corpus(feats, 12)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    scale = 0.3
    o = oracle_lib.Oracle(mp, 12, lex)
    refs = _refs(o, utts, net, lm, tdp, scale)
    o.close()
    acp, lmp = float(beams[0]), float(beams[1])
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        cost = corpus.bigram_word_posteriors(bg, 1.0, max_items=1)[0]
        for flags in ({}, {"dense_states": True}, {"global_states": True}):
            w, s, t, woff = corpus.recognize_bigram(bg, acp, lmp, **flags)
            cw, cs, ct, coff, conf = corpus.recognize_bigram_confidence(bg, scale, acp, lmp, **flags)
            assert cw.tobytes() == w.tobytes() and cs.tobytes() == s.tobytes() and ct.tobytes() == t.tobytes() and coff.tobytes() == woff.tobytes()
            assert len(conf) == len(w) and np.all(conf > 0) and np.all(conf <= 1)
            for u, (F, p) in enumerate(refs):
                t0 = 0
                for i in range(int(woff[u]), int(woff[u + 1])):
                    want = p[t0:int(t[i]), int(w[i])].max()
                    assert abs(conf[i] - want) <= 1e-9, (u, i, conf[i], want)
                    t0 = int(t[i])
                if woff[u + 1] > woff[u] and beams[0] == FLT_MAX:
                    T = len(utts[u])
                    s_last = float(s[int(woff[u + 1]) - 1])
                    slack = (4 * T + 8) * 2.0 ** -24 * max(1.0, float(np.abs(s[int(woff[u]):int(woff[u + 1])]).max()))
                    assert cost[u] <= s_last + slack
        corpus.close()
        bg.close()


def test_errors(tmp_path, oracle_lib):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 21, 8, 3)
    off = np.array([0, len(feats)], np.uint64)
    EINVAL, ELIMIT = -1, -4
    import ctypes as C
    with capi.Model.from_mixset(mp, 12) as m, capi.Model.from_mixset(mp, 12) as m2:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        other = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)

        def code(fn):
            with pytest.raises(capi.SrError) as ei:
                fn()
            return ei.value.code

        for bad in (0.0, -1.0, np.inf, np.nan):
            assert code(lambda: corpus.bigram_word_posteriors(bg, bad)) == EINVAL
            assert code(lambda: corpus.recognize_bigram_confidence(bg, bad)) == EINVAL
        assert code(lambda: corpus.bigram_word_posteriors(bg, 1.0, floor=-0.1)) == EINVAL
        assert code(lambda: corpus.bigram_word_posteriors(bg, 1.0, floor=np.nan)) == EINVAL
        assert code(lambda: corpus.bigram_word_posteriors(bg, 1.0, max_items=0)) == EINVAL
        assert code(lambda: corpus.bigram_word_posteriors(bg, 1.0, max_items=65536)) == EINVAL
        assert code(lambda: corpus.bigram_word_posteriors(other, 1.0)) == EINVAL
        cost = np.zeros(1)
        cnt = np.zeros(len(feats), np.uint16)
        rc = capi.lib().sr_bigram_word_posteriors_corpus(m.h, corpus.h, bg.h, capi.GMM_PREFILTER, 1.0, 0.0, 4, cost.ctypes.data_as(C.c_void_p),
                                                         cnt.ctypes.data_as(C.c_void_p), None, None)
        assert rc == EINVAL  # a partial item set
        rc = capi.lib().sr_bigram_word_posteriors_corpus(m.h, corpus.h, bg.h, capi.GMM_PREFILTER, 1.0, 0.0, 0, cost.ctypes.data_as(C.c_void_p),
                                                         None, None, None)
        assert rc == 0  # no items: max_items is not looked at
        lm2 = lm.copy()
        lm2[2, 1] = -np.inf
        b2 = m.bigram(word_off, mixtures, lex.silence_idx, lm2, tdp)
        assert code(lambda: corpus.bigram_word_posteriors(b2, 1.0)) == EINVAL
        b2.close()
        lm3 = lm.copy()
        lm3[2, 1] = -800.0
        b3 = m.bigram(word_off, mixtures, lex.silence_idx, lm3, tdp)
        assert code(lambda: corpus.bigram_word_posteriors(b3, 1.0)) == ELIMIT
        assert corpus.bigram_word_posteriors(b3, 0.5)[0].shape == (1,)  # -kappa lm = 400: representable
        b3.close()
        assert np.isfinite(corpus.bigram_word_posteriors(bg, 1.0)[0][0])  # the handles survive the errors
        corpus.close()
        other.close()
        bg.close()


# ---- scale shape, launch groups, score chunks, the workspace limit, the C++ wrapper --------------------------------------------
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_TDP = np.array([[3.0, 0.0, 30.0, 5.0], [1.0, 0.0, 40.0, 2.0]], np.float32)  # _setup's
SPREAD = 6.9e-17  # measured, see test_scale_shape's docstring


def linear_entry_sum(vec, klm, axis):
    """the W x W entry sum in the linear domain: exp(-klm) times exp(m - vec), accumulated in extended precision (64-bit mantissa,
    11 bits beyond the double: what math.fsum would give to well below a double's last bit at these lengths)"""
    m = vec[np.isfinite(vec)].min() if np.isfinite(vec).any() else np.inf
    if not np.isfinite(m):
        return np.full(klm.shape[1 - axis], np.inf)
    a = np.where(np.isfinite(vec), np.exp(m - np.where(np.isfinite(vec), vec, m)), 0.0).astype(np.longdouble)
    Lk = np.exp(-klm).astype(np.longdouble)
    X = (Lk * (a[None, :] if axis == 1 else a[:, None])).sum(axis=axis)
    with np.errstate(divide="ignore"):
        return np.where(X > 0, m - np.log(np.where(X > 0, X, 1.0)), np.inf).astype(np.float64)


def _scale_case(tmp_path, n_utts=300):
    """bench.py's configs[4] bigram lexicon (silence + 2666 words of three states, two more on the last) with a Dirichlet bigram as
    tests/test_bigram.py::_setup draws it, one density per state, synthetic utterances of 40 .. 120 frames"""
    lex = synth.make_lexicon(2666, 3, 1, extra_states_last=2)
    spec = synth.make_mixset(lex.n_states, 1, 12, seed=500)
    mp = str(tmp_path / "scale.mix")
    synth.write_mixset(mp, spec)
    word_off, mixtures, _ = lex.flatten()
    rng = np.random.default_rng(501)
    p = rng.dirichlet(np.ones(lex.n_words), size=lex.n_words)
    lm = (-np.log(p)).T.astype(np.float32).copy()
    feats, off = synth.make_batch(n_utts, 40, 120, 12, seed=502)
    return lex, mp, word_off, mixtures, lm, feats, np.asarray(off, np.uint64)


def spread_on_cpu(tmp_path, oracle_lib, sample=(0, 150, 299)):
    """max |log-space reference - linear-domain second evaluation| over the sampled utterances: (relative on F, absolute on p)"""
    lex, mp, word_off, mixtures, lm, feats, off = _scale_case(tmp_path)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    dF = dp = 0.0
    for u in sample:
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        F, p = R.posteriors(e, net, lm, BIG_TDP, 0.1)
        F2, p2 = R.posteriors(e, net, lm, BIG_TDP, 0.1, entry_sum=linear_entry_sum)
        dF, dp = max(dF, _rel(F2, F)), max(dp, float(np.abs(p2 - p).max()))
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
    cost, count, word, weight = c.bigram_word_posteriors(bg, a["scale"], capi.GMM_PREFILTER, 1e-4, 4)
    w, s, t, woff, conf = c.recognize_bigram_confidence(bg, a["scale"], 200.0, 30.0)
    c.close(); bg.close()
np.savez(a["out"], cost=cost, count=count, word=word, weight=weight, w=w, s=s, t=t, woff=woff, conf=conf)
'''


def test_scale_shape(tmp_path, oracle_lib):
    """bench.py's bigram lexicon shape (2667 words, 10 670 positions, Kp = 2688), 300 utterances, SRGPU_FB_MB = 64 so that about forty
    launch groups of seven or eight utterances form: three utterances (the first, the middle, the last), every 7th frame, against
    the reference; two identical calls give identical bytes; two score chunks (a child process with a small SRGPU_SCORE_CHUNK_MB)
    give the same results as one.  The tolerance is max(1e-9, 10 x spread), the spread being the largest deviation, measured on
    the CPU (spread_on_cpu above, on the same three utterances), between the log-space reference and a second numpy evaluation
    that sums the entry in the linear domain in extended precision: 0 on F (the same bits), 6.9e-17 absolute on the posteriors
    (SPREAD; on these noise features no posterior is large) -- so the bound is the project's 1e-9, and 1e-10 relative on F.  Ten
    times: the device sums in tile order, not sorted."""
    lex, mp, word_off, mixtures, lm, feats, off = _scale_case(tmp_path)
    assert lex.n_words == 2667 and 7990 <= int(word_off[-1]) <= 8192
    tol = max(1e-9, 10 * SPREAD)
    scale, n_utts = 0.1, len(off) - 1
    data = str(tmp_path / "data.npz")
    np.savez(data, word_off=word_off, mixtures=mixtures, lm=lm, tdp=BIG_TDP, feats=feats, off=off)
    args = dict(mp=mp, sil=lex.silence_idx, scale=scale, data=data, out=str(tmp_path / "one.npz"))
    script = tmp_path / "child.py"
    script.write_text(CHILD)

    def child(tag, **env):
        a = dict(args, out=str(tmp_path / f"{tag}.npz"))
        aj = tmp_path / f"{tag}.json"
        aj.write_text(json.dumps(a))
        r = subprocess.run([sys.executable, str(script), ROOT, str(aj)], env=dict(os.environ, SRGPU_FB_MB="64", **env), capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.load(a["out"])

    one = child("one")
    again = child("again")
    chunk_mb = max(1, int(feats.shape[0] * lex.n_states * 8 / 2**20 * 0.6))
    two = child("two", SRGPU_SCORE_CHUNK_MB=str(chunk_mb))
    for k in one.files:
        assert one[k].tobytes() == again[k].tobytes(), k
        assert np.array_equal(one[k], two[k]), k
    cost, count, word, weight = one["cost"], one["count"], one["word"], one["weight"]
    w, t, woff, conf = one["w"], one["t"], one["woff"], one["conf"]
    assert np.isfinite(cost).all() and (conf > 0).all() and (conf <= 1).all()
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    worst_F = worst_p = 0.0
    for u in (0, n_utts // 2, n_utts - 1):
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        F, p = R.posteriors(e, net, lm, BIG_TDP, scale)
        worst_F = max(worst_F, _rel(cost[u], F))
        for tt in range(0, p.shape[0], 7):
            ft = int(off[u]) + tt
            n = int(count[ft])
            worst_p = max([worst_p] + [abs(weight[ft, i] - p[tt, word[ft, i]]) for i in range(n)])
        t0 = 0
        for i in range(int(woff[u]), int(woff[u + 1])):
            worst_p = max(worst_p, abs(conf[i] - p[t0:int(t[i]), int(w[i])].max()))
            t0 = int(t[i])
    print(f"scale shape: device against the reference, worst relative F {worst_F:.3g}, worst absolute posterior {worst_p:.3g} (bound {tol:.3g})")
    o.close()
    assert worst_F <= 1e-10 and worst_p <= tol


def test_workspace_limit_in_a_child_process(tmp_path):
    """SRGPU_FB_MB = 1: an utterance whose trellis alone exceeds the workspace is SR_ELIMIT from both calls; a short one still runs
    (one utterance per launch group)"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 23, 300, 3)
    data = str(tmp_path / "d.npz")
    np.savez(data, word_off=word_off, mixtures=mixtures, lm=lm, tdp=tdp, long=np.tile(feats, (12, 1))[:600], short=feats[:20])
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from speechrecognition_amd import capi\n"
            "z = np.load(sys.argv[3])\n"
            "with capi.Model.from_mixset(sys.argv[2], 12) as m:\n"
            "    bg = m.bigram(z['word_off'], z['mixtures'], 0, z['lm'], z['tdp'])\n"
            "    c = m.upload(z['long'], np.array([0, len(z['long'])], np.uint64))\n"
            "    for f in (lambda: c.bigram_word_posteriors(bg, 0.5), lambda: c.recognize_bigram_confidence(bg, 0.5)):\n"
            "        try: f(); print('no error')\n"
            "        except capi.SrError as e: print('ELIMIT' if e.code == -4 and 'SRGPU_FB_MB' in str(e) else str(e))\n"
            "    c.close()\n"
            "    s = np.concatenate([z['short'], z['short'][:7], z['short']]); c = m.upload(s, np.array([0, 20, 27, 47], np.uint64))\n"
            "    cost = c.bigram_word_posteriors(bg, 0.5)[0]; print('finite' if np.isfinite(cost).all() and cost[0] == cost[2] else cost)\n"
            "    c.close(); bg.close()\n")
    assert len(np.load(data)["long"]) == 600  # 600 frames x 1204 positions x 8 bytes > 1 MiB; 20 frames fit
    r = subprocess.run([sys.executable, "-c", code, ROOT, mp, data], env=dict(os.environ, SRGPU_FB_MB="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ELIMIT", "ELIMIT", "finite"], r.stdout + r.stderr


def test_bad_flags_build_nothing(tmp_path):
    """sr_bigram_params.flags are checked before any table is built"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 24, 8, 3)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, np.array([0, len(feats)], np.uint64))
        with pytest.raises(capi.SrError) as ei:
            corpus.recognize_bigram_confidence(bg, 0.5, dense_states=True, global_states=True)
        assert ei.value.code == -1
        corpus.close()
        bg.close()


def test_cpp_driver(tmp_path):
    """sr::LinearSearch::recognize_with_confidence (include/sr_sietill.hpp) through tests/cpp/bigram_confidence_driver.cpp: the
    binding's words, score bits, times and confidence bits"""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "bigram_confidence_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bigram_confidence_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 99, 20, 3)
    rng = np.random.default_rng(100)
    utts = [feats, feats[: len(feats) // 2], rng.standard_normal((17, 12)).astype(np.float32)]
    acp, lmp, scale = 90.0, 10.0, 0.25
    W = len(word_off) - 1
    blob = struct.pack("<I", W) + np.asarray(word_off, "<u4").tobytes() + np.asarray(mixtures, "<u2").tobytes()
    blob += struct.pack("<I", lex.silence_idx) + np.asarray(lm, "<f4").tobytes() + np.asarray(tdp, "<f4").tobytes()
    blob += struct.pack("<ffId", acp, lmp, capi.GMM_DEFAULT, scale) + struct.pack("<I", len(utts))
    for f in utts:
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "conf", mp, "12", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(np.concatenate(utts), off)
        w, s, t, woff, conf = corpus.recognize_bigram_confidence(bg, scale, acp, lmp, capi.GMM_DEFAULT)
        corpus.close()
        bg.close()
    want = []
    for u in range(len(utts)):
        for i in range(int(woff[u]), int(woff[u + 1])):
            want.append(f"item {u} {w[i]} {int(s[i:i + 1].view(np.uint32)[0]):x} {t[i]} {int(conf[i:i + 1].view(np.uint64)[0]):x}")
    assert len(want) > 0 and out.stdout.splitlines() == want
