"""Word lattices on the device (sr_word_lattice_corpus) against the numpy restatement (tests/lattice_reference.py) on the device's
own emission costs -- EXACT equality of every arc field: min and + in a fixed order leave no room for a tolerance -- and against
the decoder, whose unpruned result the lattice must contain; sr_lattice_nbest on those lattices."""
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
from tests import lattice_reference as LR
from tests import net_fb_reference as R
from tests.test_word_posteriors_cpu import LEXICA, _lex
from tests.util import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDP = (3.0, 0.0, 30.0)
DIM = 13
EINVAL, ELIMIT = -1, -4
FIELDS = ("word", "first", "last", "fwd", "bwd", "cost")
POSITION_LIMIT = 8176


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _path_tol(a, T):
    """bound on |sum of a path's arc costs - the path's true cost|: every arc's cost = fwd - E is rounded once (half an ulp of
    at most max |fwd|) and so is each of the at most T additions of the sum"""
    return 2 * (T + 1) * 2.0 ** -53 * float(np.abs(a["fwd"]).max()) if len(a["fwd"]) else 0.0


def _utt(r, u):
    """utterance u's arcs of a Corpus.word_lattice result as a dict"""
    a, b = int(r[0][u]), int(r[0][u + 1])
    return {k: r[2 + i][a:b] for i, k in enumerate(FIELDS)}


def _against_restatement(m, lex, feats, off, tdp, wp, beams, kernel=capi.GMM_PREFILTER, utts=None):
    """-> the beam = +inf result; every utterance (or those of `utts`) against the restatement on corpus.score()'s rows"""
    net = _net(lex)
    with _capi_lex(m, lex, tdp) as L:
        corpus = m.upload(feats, off)
        scores = corpus.score(kernel)
        out = None
        for beam in beams:
            r = corpus.word_lattice(L, wp, beam, kernel)
            assert len(r[0]) == len(off) and r[0][0] == 0 and len(r[2]) == int(r[0][-1])
            for u in (range(len(off) - 1) if utts is None else utts):
                e = scores[int(off[u]):int(off[u + 1])]
                arcs, best = LR.lattice(e, net, tdp, wp, beam)
                got = _utt(r, u)
                assert (r[1][u] == best) or (np.isinf(best) and np.isinf(r[1][u])), (u, beam, r[1][u], best)
                for k in FIELDS:
                    assert np.array_equal(got[k], arcs[k].astype(got[k].dtype)), (u, beam, k, got[k][:8], arcs[k][:8])
                    if got[k].dtype == np.float64:
                        assert np.array_equal(_bits(got[k]), _bits(arcs[k])), (u, beam, k)
                        assert not np.isnan(got[k]).any()
            if np.isinf(beam):
                out = r
        corpus.close()
    return out


@pytest.mark.parametrize("li", range(len(LEXICA)))
def test_lattice_against_restatement(li, tmp_path):
    """the CPU tests' lexica (one- and multi-position word 0, silence not first, words of 1 .. 6 positions, a one-position
    silence), T = 0 and T = 1 utterances, the usual and a +inf skip penalty, beams 0, finite and +inf"""
    lex = _lex(*LEXICA[li])
    spec, mp = _model(tmp_path, lex.n_states, 500 + li)
    lens = [1, 0, 2, 17, 0, 60, 133]
    feats = synth.make_features(sum(lens), DIM, seed=502 + li)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    for tdp, wp in ((TDP, 10.0), ((3.0, 0.0, np.inf), 4.0), ((0.7, 1.3, 2.9), 0.0)):
        with capi.Model.from_mixset(mp, DIM) as m:
            r = _against_restatement(m, lex, feats, off, tdp, wp, (0.0, 25.0, np.inf))
        assert r[0][2] == r[0][1] and np.isinf(r[1][1])  # T = 0: no arcs, best = +inf
        assert int(r[0][-1]) > 0


def test_ragged_lexica(tmp_path):
    """random ragged lexica (words of many lengths, a one-position word 0 among them)"""
    rng = np.random.default_rng(510)
    for i in range(3):
        lex = synth.make_ragged_lexicon(40, rng, short=bool(i & 1))
        spec, mp = _model(tmp_path, lex.n_states, 511 + i)
        feats, off = synth.make_batch(6, 20, 90, DIM, seed=515 + i)
        with capi.Model.from_mixset(mp, DIM) as m:
            _against_restatement(m, lex, feats, np.asarray(off, np.uint64), TDP, 10.0, (8.0, np.inf))


def test_negative_emission_costs(tmp_path):
    """tight variances: emission costs below 0"""
    lex = synth.make_lexicon(3, 3, 1)
    spec, mp = _model(tmp_path, lex.n_states, 520, var_factor=0.004)
    utts = [synth.sample_utterance(spec, lex, ws, seed=521 + i) for i, ws in enumerate(([1, 2], [3, 1, 2, 3], [2, 3, 1, 1, 3, 2]))]
    utts[0] = utts[0][:5]
    feats = np.concatenate(utts)
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    with capi.Model.from_mixset(mp, DIM) as m:
        c = m.upload(feats, off)
        assert c.score(capi.GMM_PREFILTER).min() < 0
        c.close()
        _against_restatement(m, lex, feats, off, TDP, 10.0, (0.0, 40.0, np.inf))


@pytest.mark.parametrize("name", ["sietill_lexicon_d25", "ragged_words"])
def test_golden_lexica(name, tmp_path):
    c = Case(name, tmp_path)
    f = c.feats
    utts = [f, f[:50], f[17:], f[:1]]
    feats = np.concatenate(utts)
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    net = _net(c.lex)
    with capi.Model.from_mixset(c.mixset_path, c.dim, c.pooling, c.max_approx) as m:
        r = _against_restatement(m, c.lex, feats, off, c.tdp, c.wp, (0.0, 50.0, np.inf), kernel=capi.GMM_DEFAULT)
        with _capi_lex(m, c.lex, c.tdp) as L:
            corpus = m.upload(feats, off)
            words, woff = corpus.recognize(L, 1e30, c.wp, capi.GMM_DEFAULT)
            corpus.close()
    # the unpruned decoder's words lead the golden utterance's N-best list
    got = capi.lattice_nbest(len(f), *[_utt(r, 0)[k] for k in ("word", "first", "last", "cost")], c.lex.silence_idx, 3)
    assert abs(got[0][1] - r[1][0]) <= _path_tol(_utt(r, 0), len(f)) and len(got) == 3 and got[0][1] <= got[1][1] <= got[2][1]
    assert np.array_equal(got[0][0], words[int(woff[0]):int(woff[1])]), (got[0][0], words[:int(woff[1])])
    assert net.W == c.lex.n_words


def _recognition_case(tmp_path, seed, states_per_word, reps, n_words=12, n_utts=12):
    lex = synth.make_lexicon(n_words, states_per_word, reps)
    spec, mp = _model(tmp_path, lex.n_states, seed, M=3)
    rng = np.random.default_rng(seed + 1)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=int(rng.integers(1, 5))), seed=seed + 2 + i)
            for i in range(n_utts)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in utts])]).astype(np.uint64)
    return lex, spec, mp, np.concatenate(utts), off


def _spans(tb_word, tb_bkp, T):
    out, t = [], T
    while t > 0:
        w, b = int(tb_word[t]), int(tb_bkp[t])
        out.append((w, b, t - 1))
        t = b
    return out[::-1]


@pytest.mark.parametrize("shape", [(3, 1), (3, 2)])
def test_lattice_against_decoder(shape, tmp_path):
    """out_best is sr_recognize_corpus' tb_score[T] at am_threshold = 1e30, the 1-best spells its words and costs out_best up to
    the rounding of the arcs' cost = fwd - E and of their sum, every arc of its
    traceback (silence included) is in the lattice with the traceback's frames, and the beam-0 lattice holds nothing else (an
    arc of the best path itself may miss beam 0 by a rounding of fwd + bwd: then it is within 4 T ulp)"""
    lex, spec, mp, feats, off = _recognition_case(tmp_path, 540 + shape[1], *shape)
    sil = lex.silence_idx
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        words, woff, (tbs, tbw, tbb) = corpus.recognize(L, 1e30, 10.0, capi.GMM_PREFILTER, traceback=True)
        full = corpus.word_lattice(L, 10.0, np.inf)
        zero = corpus.word_lattice(L, 10.0, 0.0)
        again = corpus.word_lattice(L, 10.0, np.inf)
        corpus.close()
    for x, y in zip(full, again):  # two calls: identical bits
        assert np.array_equal(_bits(x), _bits(y))
    for u in range(len(off) - 1):
        T = int(off[u + 1] - off[u])
        tb0 = int(off[u]) + u
        assert full[1][u] == tbs[tb0 + T] == zero[1][u]
        a = _utt(full, u)
        nb = capi.lattice_nbest(T, a["word"], a["first"], a["last"], a["cost"], sil, 1)
        assert len(nb) == 1 and abs(nb[0][1] - full[1][u]) <= _path_tol(a, T), (u, nb[0][1], full[1][u])
        assert np.array_equal(nb[0][0], words[int(woff[u]):int(woff[u + 1])])
        sp = _spans(tbw[tb0:tb0 + T + 1], tbb[tb0:tb0 + T + 1], T)
        have = {(int(w), int(f), int(l)): float(x + y) for w, f, l, x, y in zip(a["word"], a["first"], a["last"], a["fwd"], a["bwd"])}
        z = _utt(zero, u)
        kept = set(zip(z["word"].tolist(), z["first"].tolist(), z["last"].tolist()))
        assert kept <= set(sp), (u, kept - set(sp))
        for s in sp:
            assert s in have, (u, s)
            assert s in kept or 0 < have[s] - full[1][u] <= 4 * T * 2.0 ** -53 * abs(full[1][u]), (u, s, have[s], full[1][u])
        # N-best: distinct strings, costs ascending, deterministic
        n5 = capi.lattice_nbest(T, a["word"], a["first"], a["last"], a["cost"], sil, 5)
        assert [c for _, c in n5] == sorted(c for _, c in n5) and len({tuple(w.tolist()) for w, _ in n5}) == len(n5)
        assert np.array_equal(n5[0][0], nb[0][0])


def _shape_case(tmp_path, n_words, extra, n_utts, seed, t_min, t_max):
    lex = synth.make_lexicon(n_words, 3, 1, extra_states_last=extra)
    spec, mp = _model(tmp_path, lex.n_states, seed, M=1)
    feats, off = synth.make_batch(n_utts, t_min, t_max, DIM, seed=seed + 1)
    return lex, mp, feats, np.asarray(off, np.uint64)


def test_position_limit(tmp_path):
    """a lexicon of exactly the stated limit (8176 positions: the whole 160 KiB LDS) against the restatement, configs[4]'s
    lexicon shape (8001) runs, and one position more is SR_ELIMIT"""
    lex, mp, feats, off = _shape_case(tmp_path, 2725, 0, 3, 550, 12, 30)
    assert len(lex.flatten()[1]) == POSITION_LIMIT
    with capi.Model.from_mixset(mp, DIM) as m:
        _against_restatement(m, lex, feats, off, TDP, 10.0, (30.0, np.inf), utts=(0, 2))
    lex4, mp4, feats4, off4 = _shape_case(tmp_path, 2666, 2, 4, 552, 12, 30)
    assert len(lex4.flatten()[1]) == 8001
    with capi.Model.from_mixset(mp4, DIM) as m:
        _against_restatement(m, lex4, feats4, off4, TDP, 10.0, (30.0,), utts=(1,))
    big, mpb, featsb, offb = _shape_case(tmp_path, 2725, 1, 2, 554, 12, 30)
    assert len(big.flatten()[1]) == POSITION_LIMIT + 1
    with capi.Model.from_mixset(mpb, DIM) as mb, _capi_lex(mb, big) as Lb:
        cb = mb.upload(featsb, offb)
        with pytest.raises(capi.SrError, match=str(POSITION_LIMIT)) as ei:
            cb.word_lattice(Lb, 10.0)
        assert ei.value.code == ELIMIT
        cb.close()


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
    r = c.word_lattice(L, a["wp"], a["beam"])
    c.close(); L.close()
np.savez(a["out"], **{"r%d" % i: x for i, x in enumerate(r)})
'''


def test_groups_and_chunks(tmp_path):
    """a corpus that needs several SRGPU_FB_MB groups and two score chunks (a child process with both set small) gives the bits
    of one group and one chunk; an utterance that alone exceeds SRGPU_FB_MB is SR_ELIMIT"""
    lex, mp, feats, off = _shape_case(tmp_path, 400, 0, 14, 560, 60, 110)
    word_off, aut, sil_state = lex.flatten()
    wp, beam = 10.0, 60.0
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        c = m.upload(feats, off)
        want = c.word_lattice(L, wp, beam)
        c.close()
    assert int(want[0][-1]) > 0
    per_frame = 10 * lex.n_words + 32
    assert per_frame * int(off[-1]) > 3 * 2**20 and per_frame * int(np.diff(off).max()) <= 2**20  # > 3 groups at 1 MiB
    data = str(tmp_path / "data.npz")
    np.savez(data, word_off=word_off, aut=aut, feats=feats, off=off)
    args = dict(mp=mp, dim=DIM, sil=lex.silence_idx, sil_state=int(sil_state), tdp=list(TDP), wp=wp, beam=beam, data=data,
                out=str(tmp_path / "child.npz"))
    aj = tmp_path / "args.json"
    aj.write_text(json.dumps(args))
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    chunk_mb = max(1, int(feats.shape[0] * lex.n_states * 8 / 2**20 * 0.6))
    env = dict(os.environ, SRGPU_SCORE_CHUNK_MB=str(chunk_mb), SRGPU_FB_MB="1")
    r = subprocess.run([sys.executable, str(script), ROOT, str(aj)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(args["out"])
    for i, x in enumerate(want):
        assert np.array_equal(_bits(z["r%d" % i]), _bits(x)), i
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); from speechrecognition_amd import capi, synth\n"
            "lex = synth.make_lexicon(2000, 3, 1); wo, au, ss = lex.flatten()\n"
            "with capi.Model.from_mixset(sys.argv[2], 13) as m:\n"
            "    L = capi.Lexicon(m, wo, au, 0, (3.0, 0.0, 30.0), ss); c = m.upload(synth.make_features(100, 13, seed=1), np.array([0, 100], np.uint64))\n"
            "    try: c.word_lattice(L, 10.0); print('no error')\n"
            "    except capi.SrError as e: print('ELIMIT' if e.code == -4 and 'SRGPU_FB_MB' in str(e) else str(e))\n")
    spec_c, mp_c = _model(tmp_path, 6001, 563, M=1)
    r = subprocess.run([sys.executable, "-c", code, ROOT, mp_c], env=dict(os.environ, SRGPU_FB_MB="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ELIMIT"], r.stdout


def test_sizing_protocol_and_errors(tmp_path):
    lex = _lex([1, 3, 2], 0)
    spec, mp = _model(tmp_path, lex.n_states, 570)
    feats = synth.make_features(50, DIM, seed=571)
    off = np.array([0, 20, 50], np.uint64)
    P = capi._ptr
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L, capi.Model.from_mixset(mp, DIM) as m2, _capi_lex(m2, lex) as L2:
        corpus = m.upload(feats, off)
        fn = capi.lib().sr_word_lattice_corpus
        sp = capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 0)
        aoff, best = np.zeros(3, np.uint64), np.zeros(2)

        def arrays(n):
            return [np.full(n, 77, np.uint32) for _ in range(3)] + [np.full(n, 77.0) for _ in range(3)]

        def call(beam=np.inf, cap=0, arr=(None,) * 6, lexicon=L, params=sp):
            return fn(m.h, corpus.h, lexicon.h, C.byref(params), beam, cap, P(aoff), P(best), *[P(a) for a in arr])

        assert call() == 0  # the sizing call
        n = int(aoff[2])
        assert 0 < int(aoff[1]) < n and np.isfinite(best).all()
        counts = aoff.copy()
        full = arrays(n)
        assert call(cap=n, arr=full) == 0 and np.array_equal(aoff, counts)
        assert (full[0] < 3).all() and (full[1] <= full[2]).all()
        order = full[2].astype(np.int64) * 3 + full[0]
        for u in range(2):
            a, b = int(aoff[u]), int(aoff[u + 1])
            assert (np.diff(order[a:b]) > 0).all() and full[2][a:b].max() == int(off[u + 1] - off[u]) - 1
        small = arrays(n)
        aoff[:] = 0
        assert call(cap=n - 1, arr=small) == EINVAL and np.array_equal(aoff, counts)  # too small: counts right, arrays untouched
        assert all((a == 77).all() for a in small)
        bigger = arrays(n + 10)
        assert call(cap=n + 10, arr=bigger) == 0
        assert all(np.array_equal(_bits(x[:n]), _bits(y)) and (x[n:] == 77).all() for x, y in zip(bigger, full))
        # a finite beam: fewer arcs, a subset
        assert call(beam=5.0) == 0 and 0 < int(aoff[2]) < n
        for beam in (-1e-9, -np.inf, np.nan):
            assert call(beam=beam) == EINVAL, beam
        for k in range(6):  # a partial set of arc arrays
            part = list(full)
            part[k] = None
            assert call(cap=n, arr=part) == EINVAL, k
        assert call(lexicon=L2) == EINVAL  # lexicon of another model
        assert call(params=capi.SearchParams(np.inf, 10.0, capi.GMM_PREFILTER, 1)) == EINVAL
        corpus.close()


def test_profile_accounts_the_lattice(tmp_path):
    lex = _lex([1, 3, 2], 0)
    spec, mp = _model(tmp_path, lex.n_states, 575)
    feats = synth.make_features(200, DIM, seed=576)
    off = np.array([0, 80, 200], np.uint64)
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        m.profile(True)
        corpus.word_lattice(L, 10.0, 20.0)
        p = m.profile_read()
        m.profile(False)
        corpus.close()
    assert p["search_ms"] > 0 and p["search_launches"] >= 2
    assert p["search_bytes"] == 2 * (30.0 * lex.n_words + 48.0) * 200 and p["frames"] == 400  # (the sizing and the filling call)


def test_cpp_driver(tmp_path):
    """sr::Recognizer::recognize_nbest (include/sr_sietill.hpp) through tests/cpp/nbest_driver.cpp: the binding's strings and
    cost bits"""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "nbest_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "nbest_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lex, spec, mp, feats, off = _recognition_case(tmp_path, 580, 3, 1, n_utts=5)
    wp, beam, n_best = 10.0, 80.0, 4
    blob = struct.pack("<I", lex.n_words)
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<I5d", lex.silence_idx, *TDP, wp, beam) + struct.pack("<II", n_best, len(off) - 1)
    for u in range(len(off) - 1):
        f = feats[int(off[u]):int(off[u + 1])]
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "nbest", mp, str(DIM), str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with capi.Model.from_mixset(mp, DIM) as m, _capi_lex(m, lex) as L:
        corpus = m.upload(feats, off)
        r = corpus.word_lattice(L, wp, beam, capi.GMM_DEFAULT)
        corpus.close()
    want = []
    for u in range(len(off) - 1):
        a = _utt(r, u)
        hyps = capi.lattice_nbest(int(off[u + 1] - off[u]), a["word"], a["first"], a["last"], a["cost"], lex.silence_idx, n_best)
        for k, (ws, c) in enumerate(hyps):
            want.append(" ".join([f"hyp {u} {k} {int(np.array([c]).view(np.uint64)[0]):x}"] + [str(int(w)) for w in ws]))
    assert len(want) > 5 and out.stdout.splitlines() == want
