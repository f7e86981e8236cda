"""Word posteriors and confidences on the device (sr_word_posteriors_corpus, sr_recognize_confidence_corpus) against the numpy
restatement of the recognition network's forward-backward (tests/net_fb_reference.py) on the oracle's emission costs, and against
the decoder where the two must agree.  Tolerances: F_u 1e-10 relative, posteriors and confidences 1e-9 absolute against the float64
restatement, and -- wherever that is tighter -- the measured rule of tests/test_gpu_netfb_scores.py against the restatement's
np.longdouble run (netfb_cases.tighter: 8 times the float64 run's distance plus 4 ulp of the value; the `RULE` lines say which of the
two holds in each case).  Measured: the rule is the tighter one for every F and every weight of this file, the configs[2]- and
configs[4]-sized cases included (F 3e-13 .. 3e-12 against 1e-8, posteriors 5e-15 .. 2e-14 against 1e-9), except the posteriors of
test_long_utterance: after 10 000 frames (F ~ 1e5) the float64 run lies 1.1e-9 from the longdouble one and the rule gives 9e-9, so that
case keeps 1e-9 against the float64 run."""
import contextlib
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import net_fb_reference as R
from tests import netfb_cases as nc
from tests.test_word_posteriors_cpu import LEXICA, _lex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDP = (3.0, 0.0, 30.0)
DIM = 13


def _rel(a, b):
    if a == b:  # (both +inf: no complete path)
        return 0.0
    return abs(a - b) / max(1.0, abs(b))


def _model(tmp_path, S, seed, M=2, var_factor=None):
    spec = synth.make_mixset(S, M, DIM, seed=seed)
    if var_factor is not None:
        synth.scale_variances(spec, var_factor)
    mp = str(tmp_path / f"m{seed}.mix")
    synth.write_mixset(mp, spec)
    return spec, mp


def _net(lex):
    word_off, aut, sil_state = lex.flatten()
    return R.Net(word_off, aut, lex.silence_idx, sil_state)


def _capi_lex(m, lex, tdp=TDP):
    word_off, aut, sil_state = lex.flatten()
    return contextlib.closing(capi.Lexicon(m, word_off, aut, lex.silence_idx, tdp, sil_state))


class Ref:
    """the restatement of one utterance in float64 (F, p: what the fixed tolerances are held against) and in np.longdouble (F80, p80)
    with the measured bound, where it is tighter than the fixed one (nc.tighter), for F (tolF) and for every weight (tol [T, n])"""

    def __init__(self, f64, f80, tag=None, fixed=1e-9):
        (self.F, self.p), (self.F80, self.p80) = f64, f80
        if np.isfinite(self.F80):
            self.tolF = nc.tighter(1e-10 * max(1.0, abs(float(self.F))), self.F, self.F80, tag and tag + " F")
            self.tol = nc.tighter(fixed, self.p, self.p80, tag and tag + " weights")
        else:
            self.tolF, self.tol = 0.0, np.zeros(self.p.shape)

    def holds_F(self, cost):
        return cost == self.F80 if not np.isfinite(self.F80) else abs(nc.LD(cost) - self.F80) <= self.tolF

    def __iter__(self):  # (F, p) as before
        return iter((self.F, self.p))

    def __getitem__(self, i):
        return (self.F, self.p)[i]


def _ref(e, net, tdp, wp, scale, tag=None):
    with np.errstate(all="ignore"):
        return Ref(R.posteriors(e, net, tdp, wp, scale), R.posteriors(e, net, tdp, wp, scale, dtype=nc.LD), tag)


def _check_items(p, count, word, weight, floor, K, p80=None, tol=None):
    """the device's items of one frame against the restatement's word posteriors p[W]: the listed words carry their posterior,
    in order; no word missing that ranks clearly above the last listed one, and none above the floor left out of a short list.
    p80, tol: the longdouble run's posteriors and the bound that holds against them (Ref)"""
    n = int(count)
    assert n <= K
    got = list(zip(word[:n].tolist(), weight[:n].tolist()))
    for w, x in got:
        assert abs(x - p[w]) <= 1e-9, (w, x, p[w])
        if p80 is not None:
            assert abs(nc.LD(x) - p80[w]) <= tol[w], (w, x, p80[w], tol[w])
        assert x > 0 and x >= floor
    for i in range(1, n):  # largest first, ties: smaller id first
        assert got[i - 1][1] > got[i][1] or (got[i - 1][1] == got[i][1] and got[i - 1][0] < got[i][0])
    assert not word[n:].any() and not weight[n:].any()
    ids = {w for w, _ in got}
    low = min(x for _, x in got) if n == K else floor
    for w in range(len(p)):
        if w not in ids:
            assert p[w] <= max(low, floor) + 1e-9 or p[w] <= 1e-9, (w, p[w], got)


def _against_restatement(o, m, lex, feats, off, tdp, wp, scale, floors=(0.0, 1e-6), Ks=None, items=True):
    net = _net(lex)
    W = lex.n_words
    with _capi_lex(m, lex, tdp) as L:
        corpus = m.upload(feats, off)
        refs = []
        for u in range(len(off) - 1):
            e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
            refs.append(_ref(e, net, tdp, wp, scale, f"word posteriors W {W} scale {scale} utterance {u} (T {len(e)})"))
        for floor in floors:
            for K in (Ks or (1, 3, W)):
                cost, count, word, weight = corpus.word_posteriors(L, wp, scale, capi.GMM_PREFILTER, floor, K)
                for u, r in enumerate(refs):
                    F, p = r
                    assert _rel(cost[u], F) <= 1e-10, (u, cost[u], F)
                    assert r.holds_F(cost[u]), (u, cost[u], r.F80, r.tolF)
                    if not items:
                        continue
                    for t in range(p.shape[0]):
                        ft = int(off[u]) + t
                        _check_items(p[t], count[ft], word[ft], weight[ft], floor, K, r.p80[t], r.tol[t])
        corpus.close()
    return refs


@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_posteriors_against_restatement(li, tmp_path, oracle_lib):
    """the CPU tests' lexica (one- and multi-position word 0, silence not first, words of 1 .. 6 positions), a T = 1 utterance,
    the usual and a +inf skip penalty, two scales"""
    lex = _lex(*LEXICA[li])
    spec, mp = _model(tmp_path, lex.n_states, 300 + li)
    lens = [1, 2, 17, 60, 133]
    feats = synth.make_features(sum(lens), DIM, seed=302 + li)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    for tdp, wp, scale in ((TDP, 10.0, 1.0), ((3.0, 0.0, np.inf), 4.0, 0.3)):
        o = oracle_lib.Oracle(mp, DIM, lex, tdp=tdp)
        with capi.Model.from_mixset(mp, DIM) as m:
            _against_restatement(o, m, lex, feats, off, tdp, wp, scale)
        o.close()


def test_negative_emission_costs(tmp_path, oracle_lib):
    """tight variances: emission costs below 0 (F and posteriors)"""
    lex = synth.make_lexicon(3, 3, 1)
    spec, mp = _model(tmp_path, lex.n_states, 320, var_factor=0.004)
    utts = [synth.sample_utterance(spec, lex, ws, seed=321 + i) for i, ws in enumerate(([1, 2], [3, 1, 2, 3], [2, 3, 1, 1, 3, 2]))]
    utts[0] = utts[0][:5]
    feats = np.concatenate(utts)
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    assert o.score_matrix(feats).min() < 0
    with capi.Model.from_mixset(mp, DIM) as m:
        _against_restatement(o, m, lex, feats, off, TDP, 10.0, 0.5, floors=(0.0,), Ks=(lex.n_words,))
    o.close()


def test_long_utterance(tmp_path, oracle_lib):
    """one utterance of 10 000 frames"""
    lex = _lex([1, 3, 2, 5, 3], 0)
    spec, mp = _model(tmp_path, lex.n_states, 330)
    feats = synth.make_features(10000, DIM, seed=331)
    off = np.array([0, 10000], np.uint64)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    with capi.Model.from_mixset(mp, DIM) as m:
        refs = _against_restatement(o, m, lex, feats, off, TDP, 10.0, 0.2, floors=(0.0,), Ks=(lex.n_words,))
    assert np.abs(refs[0][1].sum(axis=1) - 1.0).max() < 1e-8  # (F ~ 1e5 after 10 000 frames: the log-space sums carry ~1e-9)
    o.close()


def _spans(tb_word, tb_bkp, T, sil):
    """(word, first, last) of each recognised word from a traceback dump [T + 1] (Recognizer.cpp:222-231)"""
    out, t = [], T
    while t > 0:
        w, b = int(tb_word[t]), int(tb_bkp[t])
        if w != sil:
            out.append((w, b, t - 1))
        t = b
    return out[::-1]


def _recognition_case(tmp_path, seed, states_per_word, reps, n_words=12, n_utts=12):
    lex = synth.make_lexicon(n_words, states_per_word, reps)
    spec, mp = _model(tmp_path, lex.n_states, seed, M=3)
    rng = np.random.default_rng(seed + 1)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=int(rng.integers(1, 5))), seed=seed + 2 + i)
            for i in range(n_utts)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    return lex, spec, mp, np.concatenate(utts), off


@pytest.mark.parametrize("shape", [(3, 1), (3, 2)])  # words of <= 4 positions (word-per-lane route) and of 6 (slot route)
@pytest.mark.parametrize("beam", [60.0, 200.0])
def test_confidence_against_decoder(shape, beam, tmp_path, oracle_lib):
    lex, spec, mp, feats, off = _recognition_case(tmp_path, 340 + shape[1], *shape)
    sil = lex.silence_idx
    net = _net(lex)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        words, woff, (tbs, tbw, tbb) = corpus.recognize(L, beam, 10.0, capi.GMM_PREFILTER, traceback=True)
        for scale in (1.0, 0.1):
            cw, cwoff, conf, first, last = corpus.recognize_confidence(L, beam, 10.0, scale, capi.GMM_PREFILTER)
            assert np.array_equal(cw, words) and np.array_equal(cwoff, woff)
            assert (conf > 0).all() and (conf <= 1.0).all()
            cost = corpus.word_posteriors(L, 10.0, scale, capi.GMM_PREFILTER, 0.0, 1)[0]
            for u in range(len(off) - 1):
                T = int(off[u + 1] - off[u])
                tb0 = int(off[u]) + u
                sp = _spans(tbw[tb0:tb0 + T + 1], tbb[tb0:tb0 + T + 1], T, sil)
                a, b = int(woff[u]), int(woff[u + 1])
                assert sp == list(zip(cw[a:b].tolist(), first[a:b].tolist(), last[a:b].tolist()))
                V = tbs[tb0 + T]
                assert cost[u] <= V + 1e-12 * abs(V)
                r = _ref(o.score_matrix(feats[int(off[u]):int(off[u + 1])]), net, TDP, 10.0, scale,
                         f"confidences shape {shape} beam {beam} scale {scale} utterance {u}")
                F, p = r
                assert _rel(cost[u], F) <= 1e-10 and r.holds_F(cost[u])
                for i in range(a, b):
                    assert abs(conf[i] - p[first[i]:last[i] + 1, cw[i]].max()) <= 1e-9
                    assert _conf_holds(r, conf[i], first[i], last[i], cw[i])
        corpus.close()
    o.close()


def _conf_holds(r, conf, first, last, w):
    """a confidence = the largest posterior of the word over its frames (at most 1), against the longdouble run"""
    span = slice(int(first), int(last) + 1)
    return abs(nc.LD(conf) - min(r.p80[span, w].max(), nc.LD(1.0))) <= r.tol[span, w].max()


def _big_case(tmp_path, n_words, extra, n_utts, seed):
    """a configs[2]- / configs[4]-shaped lexicon (silence + n_words three-state words) on synthetic features of 200 .. 400 frames"""
    lex = synth.make_lexicon(n_words, 3, 1, extra_states_last=extra)
    spec, mp = _model(tmp_path, lex.n_states, seed, M=1)
    feats, off = synth.make_batch(n_utts, 200, 400, DIM, seed=seed + 1)
    return lex, mp, feats, np.asarray(off, np.uint64)


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from speechrecognition_amd import capi
a = json.load(open(sys.argv[2]))
z = np.load(a["data"])
with capi.Model.from_mixset(a["mp"], a["dim"]) as m:
    L = capi.Lexicon(m, z["word_off"], z["aut"], a["sil"], a["tdp"], a["sil_state"])
    c = m.upload(z["feats"], z["off"])
    cost, count, word, weight = c.word_posteriors(L, a["wp"], a["scale"], capi.GMM_PREFILTER, 1e-4, 4)
    w, woff, conf, first, last = c.recognize_confidence(L, 200.0, a["wp"], a["scale"], capi.GMM_PREFILTER)
    c.close(); L.close()
np.savez(a["out"], cost=cost, count=count, word=word, weight=weight, w=w, woff=woff, conf=conf, first=first, last=last)
'''


def _run(m, L, feats, off, wp, scale):
    c = m.upload(feats, off)
    r = c.word_posteriors(L, wp, scale, capi.GMM_PREFILTER, 1e-4, 4) + c.recognize_confidence(L, 200.0, wp, scale, capi.GMM_PREFILTER)
    c.close()
    return r


@pytest.mark.parametrize("cfg", ["configs2", "configs4"])
def test_scale_shapes(cfg, tmp_path, oracle_lib):
    """configs[2]'s lexicon (4000 positions) and configs[4]'s (about 8000, several SRGPU_FB_MB groups): a sample of utterances
    against the restatement, two identical calls give identical bits, and two score chunks (a child process with a small
    SRGPU_SCORE_CHUNK_MB) give the same results as one"""
    n_words, extra, n_utts, fb_mb = (1333, 0, 300, 1024) if cfg == "configs2" else (2666, 2, 1000, 160)
    lex, mp, feats, off = _big_case(tmp_path, n_words, extra, n_utts, 350 if cfg == "configs2" else 360)
    word_off, aut, sil_state = lex.flatten()
    assert (cfg == "configs2" and len(aut) == 4000) or (cfg == "configs4" and 7990 <= len(aut) <= 8192)
    wp, scale = 10.0, 0.1
    env_keep = os.environ.get("SRGPU_FB_MB")
    os.environ["SRGPU_FB_MB"] = str(fb_mb)
    try:
        with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
            r1 = _run(m, L, feats, off, wp, scale)
            r2 = _run(m, L, feats, off, wp, scale)
    finally:
        if env_keep is None:
            os.environ.pop("SRGPU_FB_MB")
        else:
            os.environ["SRGPU_FB_MB"] = env_keep
    for x, y in zip(r1, r2):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    cost, count, word, weight, w, woff, conf, first, last = r1
    assert np.isfinite(cost).all() and (conf > 0).all() and (conf <= 1).all()
    net = _net(lex)
    o = oracle_lib.Oracle(mp, DIM, lex, tdp=TDP)
    for u in (0, n_utts // 2, n_utts - 1):
        e = o.score_matrix(feats[int(off[u]):int(off[u + 1])])
        r = _ref(e, net, TDP, wp, scale, f"{cfg} utterance {u} (T {len(e)})")
        F, p = r
        assert _rel(cost[u], F) <= 1e-10, (u, cost[u], F)
        assert r.holds_F(cost[u]), (u, cost[u], r.F80, r.tolF)
        for t in range(0, p.shape[0], 7):
            ft = int(off[u]) + t
            _check_items(p[t], count[ft], word[ft], weight[ft], 1e-4, 4, r.p80[t], r.tol[t])
        for i in range(int(woff[u]), int(woff[u + 1])):
            assert abs(conf[i] - p[first[i]:last[i] + 1, w[i]].max()) <= 1e-9
            assert _conf_holds(r, conf[i], first[i], last[i], w[i])
    o.close()
    # two score chunks
    data = str(tmp_path / "data.npz")
    np.savez(data, word_off=word_off, aut=aut, feats=feats, off=off)
    args = dict(mp=mp, dim=DIM, sil=lex.silence_idx, sil_state=int(sil_state), tdp=list(TDP), wp=wp, scale=scale, data=data,
                out=str(tmp_path / "child.npz"))
    aj = tmp_path / "args.json"
    aj.write_text(json.dumps(args))
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    chunk_mb = max(1, int(feats.shape[0] * lex.n_states * 8 / 2**20 * 0.6))
    env = dict(os.environ, SRGPU_SCORE_CHUNK_MB=str(chunk_mb), SRGPU_FB_MB=str(fb_mb))
    r = subprocess.run([sys.executable, str(script), ROOT, str(aj)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(args["out"])
    for k, x in zip(("cost", "count", "word", "weight", "w", "woff", "conf", "first", "last"), r1):
        assert np.array_equal(z[k], x), k


def _raw(m, corpus, L, sp, scale, floor, K, outs):
    return capi.lib().sr_word_posteriors_corpus(m.h, corpus.h, L.h, C.byref(sp), scale, floor, K, *outs)


def test_errors(tmp_path):
    lex = _lex([1, 3, 2], 0)
    spec, mp = _model(tmp_path, lex.n_states, 370)
    feats = synth.make_features(50, DIM, seed=371)
    off = np.array([0, 20, 50], np.uint64)
    EINVAL, ELIMIT = -1, -4
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L, capi.Model.from_mixset(mp, DIM) as m2, _capi_lex(m2, lex) as L2:
        corpus = m.upload(feats, off)
        cost = np.zeros(2)
        cnt, wd, wt = np.zeros(50, np.uint16), np.zeros(50 * 3, np.uint32), np.zeros(50 * 3)
        P = capi._ptr
        full = (P(cost), P(cnt), P(wd), P(wt))
        sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
        assert _raw(m, corpus, L, sp, 1.0, 0.0, 3, full) == 0
        for scale in (0.0, -1.0, np.inf, np.nan):
            assert _raw(m, corpus, L, sp, scale, 0.0, 3, full) == EINVAL, scale
        for floor in (-1e-9, np.nan):
            assert _raw(m, corpus, L, sp, 1.0, floor, 3, full) == EINVAL, floor
        for K in (0, 65536):
            assert _raw(m, corpus, L, sp, 1.0, 0.0, K, full) == EINVAL, K
        assert _raw(m, corpus, L, sp, 1.0, 0.0, 0, (P(cost), None, None, None)) == 0  # items not requested: max_items unused
        for partial in ((P(cost), P(cnt), None, None), (P(cost), None, P(wd), P(wt)), (P(cost), P(cnt), P(wd), None)):
            assert _raw(m, corpus, L, sp, 1.0, 0.0, 3, partial) == EINVAL
        assert _raw(m, corpus, L2, sp, 1.0, 0.0, 3, full) == EINVAL  # lexicon of another model
        bad = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 1)
        assert _raw(m, corpus, L, bad, 1.0, 0.0, 3, full) == EINVAL
        w, wo = np.zeros(50, np.uint32), np.zeros(3, np.uint64)
        cf, fi, la = np.zeros(50), np.zeros(50, np.uint32), np.zeros(50, np.uint32)
        rc = capi.lib().sr_recognize_confidence_corpus
        assert rc(m.h, corpus.h, L.h, C.byref(sp), 1.0, P(w), P(wo), P(cf), P(fi), P(la)) == 0
        for scale in (0.0, np.nan):
            assert rc(m.h, corpus.h, L.h, C.byref(sp), scale, P(w), P(wo), P(cf), P(fi), P(la)) == EINVAL
        assert rc(m.h, corpus.h, L2.h, C.byref(sp), 1.0, P(w), P(wo), P(cf), P(fi), P(la)) == EINVAL
        corpus.close()
        # a lexicon of more than 8192 positions
        big = synth.make_lexicon(2731, 3, 1)  # 8194 positions
        spec_b, mp_b = _model(tmp_path, big.n_states, 372, M=1)
    with capi.Model.from_mixset(mp_b, DIM) as mb, _capi_lex(mb, big) as Lb:
        cb = mb.upload(feats, off)
        with pytest.raises(RuntimeError, match="8192"):
            cb.word_posteriors(Lb, 10.0)
        with pytest.raises(RuntimeError, match="8192"):
            cb.recognize_confidence(Lb, 200.0, 10.0)
        cb.close()
    # one utterance that alone needs more than SRGPU_FB_MB (a child process: the budget is read when the model is made)
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from speechrecognition_amd import capi, synth\n"
            "lex = synth.make_lexicon(300, 3, 1); wo, au, ss = lex.flatten()\n"
            "with capi.Model.from_mixset(sys.argv[2], 13) as m:\n"
            "    L = capi.Lexicon(m, wo, au, 0, (3.0, 0.0, 30.0), ss); c = m.upload(synth.make_features(600, 13, seed=1), np.array([0, 600], np.uint64))\n"
            "    for f in (lambda: c.word_posteriors(L, 10.0), lambda: c.recognize_confidence(L, 200.0, 10.0)):\n"
            "        try: f(); print('no error')\n"
            "        except RuntimeError as e: print('ELIMIT' if 'SRGPU_FB_MB' in str(e) else str(e))\n")
    spec_c, mp_c = _model(tmp_path, 901, 373, M=1)
    r = subprocess.run([sys.executable, "-c", code, ROOT, mp_c], env=dict(os.environ, SRGPU_FB_MB="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ELIMIT", "ELIMIT"], r.stdout


def test_cpp_driver(tmp_path):
    """sr::Recognizer::recognize_with_confidence (include/sr_sietill.hpp) through tests/cpp/confidence_driver.cpp: the binding's
    words, spans and confidence bits"""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "confidence_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "confidence_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lex, spec, mp, feats, off = _recognition_case(tmp_path, 380, 3, 1, n_utts=5)
    am, wp, scale = 200.0, 10.0, 0.25
    blob = struct.pack("<I", lex.n_words)
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<I6d", lex.silence_idx, *TDP, am, wp, scale) + struct.pack("<I", len(off) - 1)
    for u in range(len(off) - 1):
        f = feats[int(off[u]):int(off[u + 1])]
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "conf", mp, str(DIM), str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        w, woff, conf, first, last = corpus.recognize_confidence(L, am, wp, scale, capi.GMM_DEFAULT)
        corpus.close()
    want = []
    for u in range(len(off) - 1):
        for i in range(int(woff[u]), int(woff[u + 1])):
            want.append(f"word {u} {w[i]} {first[i]} {last[i]} {int(conf[i:i + 1].view(np.uint64)[0]):x}")
    assert len(want) > 0 and out.stdout.splitlines() == want
