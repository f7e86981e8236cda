"""Word lattices of the bigram search on the device (sr_bigram_word_lattice_corpus) against the numpy restatement
(tests/bigram_lattice_reference.py) on the oracle's dense scores (the device's scores are those bits: test_gpu_parity) -- EXACT
equality of every arc field: min and + in a specified order leave no room for a tolerance, and am = (fwd - c_in) - lmc is two
stated subtractions -- and against the bigram decoder on the shapes where its merge loses nothing; sr_bigram_lattice_nbest on those
lattices."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import bigram_fb_reference as R
from tests import bigram_lattice_reference as BL
from tests.test_bigram import FLT_MAX, SIL_TDP, _setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ELIMIT = -1, -4
FIELDS = ("word", "hist", "pred", "first", "last", "fwd", "bwd", "am")
# test_bigram.py's _setup shapes (seed, W, states per word, silence states, tdp): one-state words (4), multi-state silence (3, 31 ..)
SHAPES = [(1, 5, 3, 1, None), (2, 7, 2, 1, None), (3, 4, 4, 2, None), (4, 6, 1, 1, None),
          (31, 6, 3, 2, SIL_TDP), (32, 6, 3, 3, SIL_TDP), (33, 6, 3, 4, SIL_TDP)]
QUIRK_FREE = {1, 2, 4}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _corpus(feats, seed):
    """the sampled utterance, noise, a T = 0 utterance between two others, half of the first, T = 1"""
    rng = np.random.default_rng(seed + 5)
    utts = [feats, rng.standard_normal((37, 12)).astype(np.float32), feats[:0], feats[: len(feats) // 2], feats[:1]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    return utts, np.concatenate(utts), off


def _utt(r, u):
    a, b = int(r[0][u]), int(r[0][u + 1])
    return {k: r[2 + i][a:b] for i, k in enumerate(FIELDS)}


def _against_restatement(corpus, bg, dense, off, net, lm, tdp, beams):
    out = None
    for beam in beams:
        r = corpus.bigram_word_lattice(bg, beam)
        assert len(r[0]) == len(off) and r[0][0] == 0 and len(r[2]) == int(r[0][-1])
        for u in range(len(off) - 1):
            e = dense[int(off[u]):int(off[u + 1])]
            best, arcs = BL.arcs(e, net, lm, tdp, beam)
            got = _utt(r, u)
            assert (r[1][u] == best) or (np.isinf(best) and np.isinf(r[1][u])), (u, beam, r[1][u], best)
            for k in FIELDS:
                assert len(got[k]) == len(arcs[k]), (u, beam, k, len(got[k]), len(arcs[k]))
                assert np.array_equal(_bits(got[k]), _bits(arcs[k].astype(got[k].dtype))), (u, beam, k, got[k][:8], arcs[k][:8])
                assert not (got[k].dtype == np.float64 and np.isnan(got[k]).any())
        if np.isinf(beam):
            out = r
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_lattice_against_restatement(shape, tmp_path, oracle_lib):
    """the seven _setup shapes on the sampled utterance, noise, T = 0 between two others and T = 1; beams 0, finite and +inf"""
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    utts, allf, off = _corpus(feats, seed)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    dense = o.score_matrix(allf)
    o.close()
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        assert np.array_equal(_bits(corpus.score(capi.GMM_PREFILTER)), _bits(dense))
        r = _against_restatement(corpus, bg, dense, off, net, lm, tdp, (0.0, 15.0, np.inf))
        corpus.close()
        bg.close()
    assert r[0][3] == r[0][2] and r[1][2] == 0.0  # T = 0: no arcs, best = 0
    assert int(r[0][-1]) > 0


def test_one_state_words_negative_costs_and_forbidden_transitions(tmp_path, oracle_lib):
    """tight variances: emission costs below 0; +inf and NaN LM entries, negative LM scores"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 41, 9, 1)
    synth.scale_variances(spec, 0.004)
    synth.write_mixset(mp, spec)
    feats = synth.sample_utterance(spec, lex, [1, 5, 2, 8], seed=43)
    rng = np.random.default_rng(42)
    lm = (lm - 2.0).astype(np.float32)
    lm[rng.random(lm.shape) < 0.15] = np.inf
    lm[:, 3] = np.nan
    lm[2, 0] = 1.0  # (some word can follow the start's silence history)
    lm = np.ascontiguousarray(lm)
    assert (lm[np.isfinite(lm)] < 0).any()
    utts, allf, off = _corpus(feats, 41)
    net = R.Net(word_off, mixtures, lex.silence_idx)
    o = oracle_lib.Oracle(mp, 12, lex)
    dense = o.score_matrix(allf)
    o.close()
    assert dense.min() < 0
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        _against_restatement(corpus, bg, dense, off, net, lm, tdp, (0.0, 10.0, np.inf))
        corpus.close()
        bg.close()
        lm2 = lm.copy()
        lm2[1, 2] = -np.inf
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm2, tdp)
        corpus = m.upload(allf, off)
        with pytest.raises(capi.SrError, match="-inf") as ei:
            corpus.bigram_word_lattice(bg)
        assert ei.value.code == EINVAL
        corpus.close()
        bg.close()


def _best_path(a, best, W, sil):
    """the arcs of the cheapest path, traced back from the cheapest final word end through first / pred -> [(word, last)]"""
    by = {(int(BL.slot_of(int(w), int(h), W, sil)), int(l)): i for i, (w, h, l) in enumerate(zip(a["word"], a["hist"], a["last"]))}
    T = int(a["last"].max()) + 1
    ends = [i for i in range(len(a["last"])) if int(a["last"][i]) == T - 1 and a["fwd"][i] == best]
    i = ends[0]
    out = []
    while True:
        out.append((int(a["word"][i]), int(a["last"][i])))
        f = int(a["first"][i])
        if f == 0:
            return out[::-1]
        w, h, pr = int(a["word"][i]), int(a["hist"][i]), int(a["pred"][i])
        if w == sil:
            cands = [sil if h == sil else h]  # the silence word follows itself, the copy h + W word h
        else:
            cands = [pr] if pr == sil else [pr, pr + W]
        cands = [by[(x, f - 1)] for x in cands if (x, f - 1) in by]
        i = min(cands, key=lambda j: a["fwd"][j])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] in QUIRK_FREE])
def test_best_path_is_the_decoders(shape, tmp_path, oracle_lib):
    """where the decoder's merge loses nothing (test_bigram_posteriors_cpu.py), beams off: the best path's (word, last) pairs are
    the items (word, time) of sr_recognize_bigram_corpus (time = frames consumed = last + 1), and entry 1 of the N-best list
    spells its words without silence"""
    seed, W, spw, sil_states, tdp = shape
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, seed, W, spw, sil_states=sil_states, tdp=tdp)
    off = np.array([0, len(feats)], np.uint64)
    sil = lex.silence_idx
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, sil, lm, tdp)
        corpus = m.upload(feats, off)
        w, s, t, woff = corpus.recognize_bigram(bg, float(FLT_MAX), float(FLT_MAX))
        r = corpus.bigram_word_lattice(bg)
        corpus.close()
        bg.close()
    a = _utt(r, 0)
    path = _best_path(a, r[1][0], lex.n_words, sil)
    assert path == [(int(x), int(y) - 1) for x, y in zip(w, t)], (path, list(zip(w, t)))
    nb = capi.bigram_lattice_nbest(len(feats), a["word"], a["hist"], a["first"], a["last"], a["am"], sil, lm, 3)
    assert np.array_equal(nb[0][0], w[w != sil])
    # the sum of (lm + am) along the path against best: each am is two roundings of at most half an ulp of max |fwd|, each of the
    # path's at most 2 T additions one more
    tol = 4 * (len(feats) + 1) * 2.0 ** -53 * float(np.abs(a["fwd"]).max())
    assert abs(nb[0][1] - r[1][0]) <= tol, (nb[0][1], r[1][0], tol)
    assert [c for _, c in nb] == sorted(c for _, c in nb)


def test_identical_calls_identical_bytes(tmp_path):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 15, 40, 3)
    utts, allf, off = _corpus(feats, 15)
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(allf, off)
        a = corpus.bigram_word_lattice(bg, 30.0)
        corpus.bigram_word_posteriors(bg, 0.4, max_items=2)  # (another pass on the shared workspace in between)
        b = corpus.bigram_word_lattice(bg, 30.0)
        corpus.close()
        bg.close()
    assert int(a[0][-1]) > 0
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


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
    try:
        r = c.bigram_word_lattice(bg, a["beam"])
        np.savez(a["out"], **{"r%d" % i: x for i, x in enumerate(r)})
        print("ok")
    except capi.SrError as e:
        print("ELIMIT" if e.code == -4 and "SRGPU_FB_MB" in str(e) else str(e))
    c.close(); bg.close()
'''


def _child(tmp_path, name, env, **args):
    aj = tmp_path / (name + ".json")
    aj.write_text(json.dumps(args))
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(aj)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_groups_and_chunks(tmp_path):
    """a corpus that needs several SRGPU_FB_MB groups and two score chunks (a child process with both set small) gives the bits of
    one group and one chunk; an utterance that alone exceeds SRGPU_FB_MB is SR_ELIMIT"""
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 16, 70, 2, sil_states=2, tdp=SIL_TDP)
    rng = np.random.default_rng(77)
    utts = [feats] + [rng.standard_normal((int(n), 12)).astype(np.float32) for n in rng.integers(60, 140, size=30)]
    allf = np.concatenate(utts)
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    beam = 40.0
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        c = m.upload(allf, off)
        want = c.bigram_word_lattice(bg, beam)
        c.close()
        bg.close()
    assert int(want[0][-1]) > 0
    W = lex.n_words
    P = int(word_off[-1]) + W * int(word_off[lex.silence_idx + 1] - word_off[lex.silence_idx])
    per_frame, per_utt = 44 * W + 16, 28 * ((W + 63) // 64 * 64) + 28 * P
    assert per_frame * int(off[-1]) > 3 * 2**20 and per_frame * int(np.diff(off).max()) + per_utt <= 2**20  # > 3 groups at 1 MiB
    data = str(tmp_path / "data.npz")
    np.savez(data, word_off=word_off, mixtures=mixtures, lm=lm, tdp=tdp, feats=allf, off=off)
    chunk_mb = max(1, int(allf.shape[0] * lex.n_states * 8 / 2**20 * 0.6))
    assert allf.shape[0] * lex.n_states * 8 > chunk_mb * 2**20
    out = str(tmp_path / "child.npz")
    got = _child(tmp_path, "a", dict(SRGPU_SCORE_CHUNK_MB=str(chunk_mb), SRGPU_FB_MB="1"), mp=mp, sil=lex.silence_idx, beam=beam, data=data, out=out)
    assert got == ["ok"], got
    z = np.load(out)
    for i, x in enumerate(want):
        assert np.array_equal(_bits(z["r%d" % i]), _bits(x)), i
    # the other arg-min route: the same bits
    out2 = str(tmp_path / "child2.npz")
    assert _child(tmp_path, "b", dict(SRGPU_BGLAT_ARGMIN="rescan"), mp=mp, sil=lex.silence_idx, beam=beam, data=data, out=out2) == ["ok"]
    z = np.load(out2)
    for i, x in enumerate(want):
        assert np.array_equal(_bits(z["r%d" % i]), _bits(x)), i
    # one utterance of 400 frames: 400 (44 W + 16) bytes > 1 MiB
    long = rng.standard_normal((400, 12)).astype(np.float32)
    assert per_frame * 400 > 2**20
    data2 = str(tmp_path / "data2.npz")
    np.savez(data2, word_off=word_off, mixtures=mixtures, lm=lm, tdp=tdp, feats=long, off=np.array([0, 400], np.uint64))
    assert _child(tmp_path, "c", dict(SRGPU_FB_MB="1"), mp=mp, sil=lex.silence_idx, beam=beam, data=data2, out=out) == ["ELIMIT"]


def test_sizing_protocol_and_errors(tmp_path):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 1, 5, 3)
    W = lex.n_words
    feats = feats[:50] if len(feats) >= 50 else np.concatenate([feats] * 4)[:50]
    off = np.array([0, 20, 50], np.uint64)
    P = capi._ptr
    with capi.Model.from_mixset(mp, 12) as m, capi.Model.from_mixset(mp, 12) as m2:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        bg2 = m2.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        fn = capi.lib().sr_bigram_word_lattice_corpus
        aoff, best = np.zeros(3, np.uint64), np.zeros(2)

        def arrays(n):
            return [np.full(n, 77, np.uint32) for _ in range(5)] + [np.full(n, 77.0) for _ in range(3)]

        def call(beam=np.inf, cap=0, arr=(None,) * 8, net=bg):
            return fn(m.h, corpus.h, net.h, capi.GMM_PREFILTER, beam, cap, P(aoff), P(best), *[P(a) for a in arr])

        assert call() == 0  # the sizing call
        n = int(aoff[2])
        assert 0 < int(aoff[1]) < n and np.isfinite(best).all()
        counts = aoff.copy()
        full = arrays(n)
        assert call(cap=n, arr=full) == 0 and np.array_equal(aoff, counts)
        word, hist, pred, first, last = full[:5]
        assert (word < W).all() and (hist < W).all() and (pred < W).all() and (first <= last).all()
        slot = np.array([BL.slot_of(int(w), int(h), W, lex.silence_idx) for w, h in zip(word, hist)])
        order = last.astype(np.int64) * 2 * W + slot
        for u in range(2):
            a, b = int(aoff[u]), int(aoff[u + 1])
            assert (np.diff(order[a:b]) > 0).all() and last[a:b].max() == int(off[u + 1] - off[u]) - 1
        small = arrays(n)
        aoff[:] = 0
        assert call(cap=n - 1, arr=small) == EINVAL and np.array_equal(aoff, counts)  # too small: counts right, arrays untouched
        assert all((a == 77).all() for a in small)
        bigger = arrays(n + 10)
        assert call(cap=n + 10, arr=bigger) == 0
        assert all(np.array_equal(_bits(x[:n]), _bits(y)) and (x[n:] == 77).all() for x, y in zip(bigger, full))
        assert call(beam=5.0) == 0 and 0 < int(aoff[2]) < n  # a finite beam: fewer arcs
        for beam in (-1e-9, -np.inf, np.nan):
            assert call(beam=beam) == EINVAL, beam
        for k in range(8):  # a partial set of arc arrays
            part = list(full)
            part[k] = None
            assert call(cap=n, arr=part) == EINVAL, k
        assert call(net=bg2) == EINVAL  # a bigram net of another model
        corpus.close()
        # more than 65535 frames in one utterance: SR_ELIMIT -- the corpus upload already refuses it, so the lattice's own check of
        # the same limit cannot be reached through a corpus
        longf = np.zeros((65536, 12), np.float32)
        with pytest.raises(capi.SrError, match="65535") as ei:
            m.upload(longf, np.array([0, 65536], np.uint64))
        assert ei.value.code == ELIMIT
        bg.close()
        bg2.close()


def test_profile_accounts_the_lattice(tmp_path):
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 2, 7, 2)
    feats = np.concatenate([feats] * 8)[:200]
    assert len(feats) == 200
    off = np.array([0, 80, 200], np.uint64)
    W = lex.n_words
    Pn = int(word_off[-1]) + W * int(word_off[lex.silence_idx + 1] - word_off[lex.silence_idx])
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus = m.upload(feats, off)
        m.profile(True)
        corpus.bigram_word_lattice(bg, 20.0)
        p = m.profile_read()
        m.profile(False)
        corpus.close()
        bg.close()
    assert p["search_ms"] > 0 and p["search_launches"] >= 2
    assert p["search_bytes"] == 2 * (44.0 * Pn + 120.0 * W) * 200 and p["frames"] == 400  # (the sizing and the filling call)


def test_cpp_driver(tmp_path):
    """sr::LinearSearch::recognize_nbest (include/sr_sietill.hpp) through tests/cpp/bigram_nbest_driver.cpp: the binding's strings
    and cost bits"""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "bigram_nbest_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bigram_nbest_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lex, spec, mp, word_off, mixtures, lm, tdp, feats = _setup(tmp_path, 12, 9, 2)
    utts, allf, off = _corpus(feats, 12)
    W, sil, beam, n_best = lex.n_words, lex.silence_idx, 60.0, 4
    blob = struct.pack("<II", W, sil) + np.asarray(word_off, "<u4").tobytes() + np.asarray(mixtures, "<u2").tobytes()
    blob += np.ascontiguousarray(lm, "<f4").tobytes() + np.ascontiguousarray(tdp, "<f4").tobytes()
    blob += struct.pack("<dII", beam, n_best, len(off) - 1)
    for u in range(len(off) - 1):
        f = allf[int(off[u]):int(off[u + 1])]
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, mp, "12", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    with capi.Model.from_mixset(mp, 12) as m:
        bg = m.bigram(word_off, mixtures, sil, lm, tdp)
        corpus = m.upload(allf, off)
        r = corpus.bigram_word_lattice(bg, beam, capi.GMM_DEFAULT)
        corpus.close()
        bg.close()
    want = []
    for u in range(len(off) - 1):
        a = _utt(r, u)
        hyps = capi.bigram_lattice_nbest(int(off[u + 1] - off[u]), a["word"], a["hist"], a["first"], a["last"], a["am"], sil, lm, n_best)
        for k, (ws, c) in enumerate(hyps):
            want.append(" ".join([f"hyp {u} {k} {int(np.array([c]).view(np.uint64)[0]):x}"] + [str(int(w)) for w in ws]))
    assert len(want) > 5 and out.stdout.splitlines() == want
