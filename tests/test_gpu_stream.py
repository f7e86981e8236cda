"""Streaming recognition (sr_stream_*, decode_stream_kernel): utterances fed in pieces, several per push, beginning and ending
at different times.  The final words and traceback must equal sr_recognize_corpus' on the whole utterances (same gmm_kernel)
and, for max-approx models, the oracle's Recognizer::recognizeSequence_pruned; the partial result after t frames must equal the
oracle's decode of the first t frames.  Then slot reuse, the error paths and the profile counters."""
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests.util import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz")
PIECES = ("one", "seven", "irregular", "whole")


def _piece(mode, rng, left):
    k = {"one": 1, "seven": 7, "irregular": int(rng.integers(1, 24)), "whole": left}[mode]
    return min(k, left)


def _stream_all(st, utts, rng, max_open):
    """Every utterance through `st`: at most max_open open at once; each push carries a random subset of the open ones, each with
    a piece whose size follows the utterance's mode (PIECES[u % 4]); a finished utterance is ended a random number of pushes
    later.  -> {u: (words, (tb_score, tb_word, tb_bkp))}"""
    todo, open_, done, out = list(range(len(utts))), {}, {}, {}
    pushes = 0
    while todo or open_ or done:
        while todo and len(open_) + len(done) < max_open:
            u = todo.pop(0)
            open_[u] = (st.begin(), 0)
        batch = {}
        for u in list(open_):
            if rng.random() < 0.75:
                sid, t = open_[u]
                k = _piece(PIECES[u % 4], rng, len(utts[u]) - t)
                batch[sid] = utts[u][t:t + k]
                open_[u] = (sid, t + k)
        if batch:
            st.push(batch)
            pushes += 1
        for u in list(open_):
            if open_[u][1] == len(utts[u]):
                done[u] = open_.pop(u)[0]
        for u in list(done):
            if rng.random() < 0.5:
                out[u] = st.end(done.pop(u), traceback=True)
    return out, pushes


def _check_against_batch(got, words, woff, tb, off):
    tbs, tbw, tbb = tb
    for u, (w, (s, wd, b)) in got.items():
        assert np.array_equal(w, words[int(woff[u]):int(woff[u + 1])]), u
        T = int(off[u + 1] - off[u])
        base = int(off[u]) + u
        assert len(s) == T + 1
        assert np.array_equal(s.view(np.uint64), tbs[base:base + T + 1].view(np.uint64)), u
        assert np.array_equal(wd, tbw[base:base + T + 1]) and np.array_equal(b, tbb[base:base + T + 1]), u


def _check_against_oracle(got, utts, o, scores=None, off=None):
    for u, (w, (s, wd, b)) in got.items():
        dense = None if scores is None else scores[int(off[u]):int(off[u + 1])]
        ow, (os_, oww, ob) = o.decode(utts[u], dense=dense, traceback=True)
        assert np.array_equal(w, ow), u
        assert np.array_equal(s.view(np.uint64), os_.view(np.uint64)) and np.array_equal(wd, oww) and np.array_equal(b, ob), u


def _cuts(tb_score_u, T, rng):
    """1, a few random frames, the last, and the first frame with no surviving word end (if any)"""
    cuts = {1, T} | set(int(x) for x in rng.integers(1, T + 1, size=3))
    dead = np.nonzero(np.isinf(tb_score_u[1:]))[0]
    if len(dead):
        cuts.add(int(dead[0]) + 1)
    return sorted(cuts)


def _check_partials(m, lexh, beam, wp, kernel, feats, cuts, want_of):
    """One stream, fed up to each cut in turn (pieces of 3): partial() there equals want_of(t); reading it changes nothing, so the
    final result still follows."""
    with m.stream(lexh, beam, wp, kernel, max_streams=1, max_frames=len(feats)) as st:
        sid = st.begin()
        t = 0
        for c in cuts:
            while t < c:
                k = min(3, c - t)
                st.push({sid: feats[t:t + k]})
                t += k
            w, n = st.partial(sid, frames=True)
            assert n == c
            assert np.array_equal(w, want_of(c)), c
        return st.end(sid)


def _run_case(m, lexh, utts, beam, wp, kernel, seed, o=None, scores=None, max_open=5, partial_utts=(0,)):
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    feats = np.concatenate(utts)
    corpus = m.upload(feats, off)
    words, woff, tb = corpus.recognize(lexh, beam, wp, kernel, traceback=True)
    corpus.close()
    rng = np.random.default_rng(seed)
    with m.stream(lexh, beam, wp, kernel, max_streams=max_open, max_frames=max(len(x) for x in utts)) as st:
        got, pushes = _stream_all(st, utts, rng, max_open)
    assert sorted(got) == list(range(len(utts))) and pushes > len(utts) // max_open
    _check_against_batch(got, words, woff, tb, off)
    if o is not None:
        _check_against_oracle(got, utts, o, scores, off)
    for u in partial_utts:
        f = utts[u]
        b = int(off[u]) + u
        cuts = _cuts(tb[0][b:b + len(f) + 1], len(f), rng)
        if o is not None:
            want_of = lambda t: o.decode(f[:t], dense=None if scores is None else scores[int(off[u]):int(off[u]) + t])  # noqa: E731
        else:  # sum mode through SR_GMM_MFMA / DEFAULT: the batch path on the prefixes as complete utterances
            poff = np.concatenate([[0], np.cumsum(cuts)]).astype(np.uint64)
            pc = m.upload(np.concatenate([f[:t] for t in cuts]), poff)
            pw, pwoff = pc.recognize(lexh, beam, wp, kernel)
            pc.close()
            by = {t: pw[int(pwoff[i]):int(pwoff[i + 1])] for i, t in enumerate(cuts)}
            want_of = by.__getitem__
        final = _check_partials(m, lexh, beam, wp, kernel, f, cuts, want_of)
        assert np.array_equal(final, words[int(woff[u]):int(woff[u + 1])])
    return words, woff


@pytest.mark.parametrize("kernel", [capi.GMM_DEFAULT, capi.GMM_MFMA])
def test_cfg2_shape_matches_batch_and_oracle(tmp_path, oracle_lib, kernel):
    lex = synth.make_lexicon(1333, 3, 1)  # configs[2]: 4000 states x 32 densities, 1333 three-state words
    spec = synth.make_mixset(lex.n_states, 32, 39, seed=1701)
    mp = str(tmp_path / "cfg2.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(1702)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=2), seed=1710 + i, frames_per_state=(1, 3))
            for i in range(28)]
    utts += [synth.make_features(int(n), 39, seed=1750 + i) for i, n in enumerate((1, 2, 40, 90))]  # 32 utterances
    beam, wp = 200.0, 10.0
    with capi.Model.from_mixset(mp, 39) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
        o = oracle_lib.Oracle(mp, 39, lex, am_threshold=beam, word_penalty=wp) if kernel == capi.GMM_DEFAULT else None
        scores = o.score_matrix(np.concatenate(utts), n_threads=16) if o else None
        words, _ = _run_case(m, lexh, utts, beam, wp, kernel, 1703, o, scores, max_open=8, partial_utts=(0, 5))
        assert len(words) > 0
        if o:
            o.close()
        lexh.close()


@pytest.mark.parametrize("name", ["sietill_lexicon_d25", "sietill_lexicon_d25_tightbeam"])
def test_golden_sietill_lexicon(name, tmp_path, oracle_lib):
    c = Case(name, tmp_path)
    f = c.feats
    utts = [f, f[:50], f[17:], f[:1], f[40:121], f]  # the golden utterance and pieces of it as utterances of their own
    word_off, automaton, sil = c.lex.flatten()
    with capi.Model.from_mixset(c.mixset_path, c.dim, c.pooling, c.max_approx) as m:
        lexh = m.lexicon(word_off, automaton, c.lex.silence_idx, c.tdp, sil)
        o = c.oracle(oracle_lib)
        words, woff = _run_case(m, lexh, utts, c.beam, c.wp, capi.GMM_DEFAULT, 31, o, max_open=3, partial_utts=(0, 4))
        assert np.array_equal(words[int(woff[0]):int(woff[1])], c.z["words"])
        o.close()
        lexh.close()


def test_real_speech_negative_costs(tmp_path, oracle_lib):
    z = np.load(REAL)
    lex = synth.sietill_lexicon()
    word_off, automaton, sil = lex.flatten()
    mp = tmp_path / "real.mix"
    mp.write_bytes(z["model_none"].tobytes())
    off = z["frame_off"].astype(np.int64)
    utts = [z["feats"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    tdp = tuple(float(x) for x in z["tdp"])
    dim = int(z["dim"])
    with capi.Model.from_mixset(str(mp), dim, capi.POOL_NONE, True) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, tdp, sil)
        for tag in ("wide", "tight"):
            beam, wp = float(z[f"none_{tag}_beam"]), float(z[f"none_{tag}_wp"])
            o = oracle_lib.Oracle(str(mp), dim, lex, tdp=tdp, am_threshold=beam, word_penalty=wp, pooling=capi.POOL_NONE)
            if tag == "wide":
                assert (o.score_matrix(z["feats"], n_threads=8) < 0).any()  # the sequential boundary replay is live
            words, woff = _run_case(m, lexh, utts, beam, wp, capi.GMM_DEFAULT, 41, o, max_open=6, partial_utts=(0,))
            assert np.array_equal(words, z[f"none_{tag}_words"])
            o.close()
        lexh.close()


def test_big_lexicon_negative_costs(tmp_path, oracle_lib):
    dim = 12
    lex = synth.make_lexicon(1400, 3, 2)  # 8401 positions: beyond the LDS kernels
    word_off, automaton, sil = lex.flatten()
    assert int(word_off[-1]) > 8192
    spec = synth.make_mixset(lex.n_states, 2, dim, seed=2301, var_floor=0.002)
    mu = spec.mean_acc / spec.mean_w[:, None]
    var = 0.004 * (spec.var_acc / spec.var_w[:, None] - mu ** 2)
    spec.var_acc = (var + mu ** 2) * spec.var_w[:, None]
    mp = str(tmp_path / "big.mix")
    synth.write_mixset(mp, spec)
    rng = np.random.default_rng(2302)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=2), seed=2310 + i, frames_per_state=(1, 2), noise=0.8)
            for i in range(4)]
    utts.append(synth.make_features(9, dim, seed=2320))
    beam, wp = 120.0, 4.0
    with capi.Model.from_mixset(mp, dim) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)
        o = oracle_lib.Oracle(mp, dim, lex, am_threshold=beam, word_penalty=wp)
        assert (o.score_matrix(np.concatenate(utts)) < 0).any()
        _run_case(m, lexh, utts, beam, wp, capi.GMM_EXACT, 51, o, max_open=3, partial_utts=(0,))
        o.close()
        lexh.close()


@pytest.mark.parametrize("kernel", [capi.GMM_EXACT, capi.GMM_DEFAULT])
def test_sum_mode(kernel, tmp_path):
    c = Case("sum_mode", tmp_path)
    assert not c.max_approx
    f = c.feats
    utts = [f, f[:23], f[5:], f[:1], f]
    word_off, automaton, sil = c.lex.flatten()
    with capi.Model.from_mixset(c.mixset_path, c.dim, c.pooling, c.max_approx) as m:
        lexh = m.lexicon(word_off, automaton, c.lex.silence_idx, c.tdp, sil)
        words, woff = _run_case(m, lexh, utts, c.beam, c.wp, kernel, 61, None, max_open=2, partial_utts=(0,))
        assert np.array_equal(words[int(woff[0]):int(woff[1])], c.z["words"])
        lexh.close()


def _small(tmp_path, seed=71):
    lex = synth.make_lexicon(30, 3, 1)
    spec = synth.make_mixset(lex.n_states, 4, 39, seed=seed)
    mp = str(tmp_path / f"s{seed}.mix")
    synth.write_mixset(mp, spec)
    word_off, automaton, sil = lex.flatten()
    return lex, spec, mp, (word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil)


def test_slot_reuse_200_utterances(tmp_path):
    lex, spec, mp, lexargs = _small(tmp_path)
    rng = np.random.default_rng(72)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=int(rng.integers(1, 4))), seed=800 + i,
                                   frames_per_state=(1, 3)) for i in range(200)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    with capi.Model.from_mixset(mp, 39) as m:
        lexh = m.lexicon(*lexargs)
        corpus = m.upload(np.concatenate(utts), off)
        words, woff, tb = corpus.recognize(lexh, 150.0, 5.0, capi.GMM_DEFAULT, traceback=True)
        corpus.close()
        with m.stream(lexh, 150.0, 5.0, capi.GMM_DEFAULT, max_streams=8, max_frames=max(len(x) for x in utts)) as st:
            got, _ = _stream_all(st, utts, rng, 8)
        _check_against_batch(got, words, woff, tb, off)
        lexh.close()


def test_error_paths_leave_other_streams_unchanged(tmp_path):
    lex, spec, mp, lexargs = _small(tmp_path, 81)
    rng = np.random.default_rng(82)
    a_f, b_f = (synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=3), seed=83 + i, frames_per_state=(2, 3))
                for i in range(2))
    T = max(len(a_f), len(b_f))
    off = np.array([0, len(a_f), len(a_f) + len(b_f)], np.uint64)
    with capi.Model.from_mixset(mp, 39) as m:
        lexh = m.lexicon(*lexargs)
        corpus = m.upload(np.concatenate([a_f, b_f]), off)
        words, woff = corpus.recognize(lexh, 150.0, 5.0, capi.GMM_DEFAULT)
        corpus.close()
        L = capi.lib()
        with pytest.raises(capi.SrError) as e:
            m.stream(lexh, 150.0, 5.0, capi.GMM_DEFAULT, max_streams=0, max_frames=T)
        assert e.value.code == -1
        sp = capi.SearchParams(150.0, 5.0, capi.GMM_DEFAULT, capi.SEARCH_GENERAL_KERNEL)
        h = capi.C.c_void_p()
        assert L.sr_stream_open(m.h, lexh.h, capi.C.byref(sp), 2, T, capi.C.byref(h)) == -1
        with pytest.raises(capi.SrError) as e:
            m.stream(lexh, 150.0, 5.0, capi.GMM_DEFAULT, max_streams=2, max_frames=70000)
        assert e.value.code == -4
        with m.stream(lexh, 150.0, 5.0, capi.GMM_DEFAULT, max_streams=3, max_frames=T) as st:
            a, b, x = st.begin(), st.begin(), st.begin()
            with pytest.raises(capi.SrError) as e:
                st.begin()                                       # full set
            assert e.value.code == -4
            st.push({a: a_f[:10], b: b_f[:4], x: b_f[:3]})
            st.end(x)
            for bad, code in (({a: a_f[10:12], b: np.concatenate([b_f[4:], b_f[:T]])}, -4),   # b past max_frames
                              ({b: b_f[4:6], x: b_f[3:5]}, -1)):                             # x has ended
                with pytest.raises(capi.SrError) as e:
                    st.push(bad)
                assert e.value.code == code
            ids = np.array([a, a], np.uint32)                    # a twice in one push
            fo = np.array([0, 1, 2], np.uint64)
            assert L.sr_stream_push(st.h, 2, capi._ptr(ids), capi._ptr(np.ascontiguousarray(a_f[10:12])), capi._ptr(fo)) == -1
            assert "twice" in L.sr_last_error().decode()
            assert st.partial(a, frames=True)[1] == 10 and st.partial(b, frames=True)[1] == 4
            n = capi.C.c_uint32()
            out = np.zeros(1, np.uint32)
            rc = L.sr_stream_partial(st.h, a, capi._ptr(out), 0, capi.C.byref(n), None)   # cap too small (if a has words)
            if n.value > 0:
                assert rc == -1 and str(n.value) in L.sr_last_error().decode()
            st.push({a: a_f[10:], b: b_f[4:]})
            c = st.begin()                                       # x's slot again, under a new id
            assert c != x
            n_words = capi.C.c_uint32()
            rc = L.sr_stream_end(st.h, a, None, 0, capi.C.byref(n_words), None, None, None)
            if n_words.value > 0:                                # too small: a stays open
                assert rc == -1 and str(n_words.value) in L.sr_last_error().decode()
            assert np.array_equal(st.end(a), words[int(woff[0]):int(woff[1])])
            assert np.array_equal(st.end(b), words[int(woff[1]):int(woff[2])])
            w, (s, wd, bk) = st.end(c, traceback=True)           # ended after 0 frames: the empty utterance
            assert len(w) == 0 and s.tolist() == [0.0] and wd.tolist() == [0] and bk.tolist() == [0]
            with pytest.raises(capi.SrError) as e:
                st.partial(a)
            assert e.value.code == -1
        lexh.close()


def test_profile_counts_one_search_launch_per_push(tmp_path):
    lex, spec, mp, lexargs = _small(tmp_path, 91)
    feats = synth.make_features(40, 39, seed=92)
    with capi.Model.from_mixset(mp, 39) as m:
        lexh = m.lexicon(*lexargs)
        with m.stream(lexh, 150.0, 5.0, capi.GMM_DEFAULT, max_streams=4, max_frames=40) as st:
            ids = [st.begin() for _ in range(4)]
            st.push({i: feats[:5] for i in ids})                 # warm: packing, staging
            m.profile(True)
            st.push({i: feats[5 + 3 * j:12 + 3 * j] for j, i in enumerate(ids)})   # 4 streams x 7 frames
            p = m.profile_read()
            assert p["frames"] == 28 and p["search_launches"] == 1 and p["gmm_launches"] >= 1
            assert p["search_ms"] > 0 and p["gmm_ms"] > 0
            m.profile(False)
        lexh.close()


def test_streaming_recognizer_mirror(tmp_path, oracle_lib):
    """sr::StreamingRecognizer (include/sr_sietill.hpp) through tests/cpp/stream_driver.cpp"""
    from speechrecognition_amd import build

    build.build()
    exe = str(tmp_path / "stream_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stream_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    lex, spec, mp, _ = _small(tmp_path, 101)
    rng = np.random.default_rng(102)
    utts = [synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=3), seed=103 + i) for i in range(4)]
    beam, wp, tdp, piece = 120.0, 10.0, (3.0, 0.0, 30.0), 9
    blob = struct.pack("<I", lex.n_words)
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<I5dII", lex.silence_idx, *tdp, beam, wp, capi.GMM_DEFAULT, piece)
    blob += struct.pack("<I", len(utts))
    for f in utts:
        blob += struct.pack("<I", len(f)) + np.ascontiguousarray(f, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, "stream", mp, "39", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    o = oracle_lib.Oracle(mp, 39, lex, tdp=tdp, am_threshold=beam, word_penalty=wp)
    for u, f in enumerate(utts):
        part = [int(x) for x in [l for l in lines if l.startswith(f"partial {u}")][0].split()[2:]]
        final = [int(x) for x in [l for l in lines if l.startswith(f"final {u}")][0].split()[2:]]
        assert part == list(o.decode(f[:piece])) and final == list(o.decode(f))
    assert "ended_again refused" in lines
    o.close()
