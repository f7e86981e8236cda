"""The tail of a recognition call (gather_words.hip): the device packs every utterance's words into one block of pinned host memory
and the host copies it out; SRGPU_GATHER=host keeps the earlier route (everything copied, a loop on the host).  Both must return
the same bytes, which are the oracle's words.  Integers throughout: no tolerance anywhere.

Sizes: 1 utterance; 3; 70 (more than a wave of the scan); 1030 (more than one 1024-wide tile of the scan, and 129 groups of the copy
kernel, the last one of 6 utterances).  Utterances of 1 .. 40 frames, one of them forced to a single frame; two in three are noise,
which this lexicon and word penalty mostly decode to silence alone -- no words, an empty segment of the scan -- and every third
is drawn from the model along two words."""
import functools

import numpy as np
import pytest

from speechrecognition_amd import capi, synth

pytestmark = pytest.mark.gpu

D, M = 9, 4
AM_THRESHOLD, WORD_PENALTY = 200.0, 10.0
ROUTES = ("device", "host")


def _lexicon():
    return synth.make_lexicon(4, 3, 1)  # silence + 4 words of 3 states: 13 states


def _model_file(tmp_path):
    lex = _lexicon()
    spec = synth.make_mixset(lex.n_states, M, D, seed=5)
    mp = str(tmp_path / "tiny.mix")
    synth.write_mixset(mp, spec)
    return lex, spec, mp


@functools.lru_cache(maxsize=None)
def _batch(U):
    """(feats, frame_off) of U utterances; built once per size and never written to"""
    lex = _lexicon()
    spec = synth.make_mixset(lex.n_states, M, D, seed=5)
    rng = np.random.default_rng(1000 + U)
    lens = rng.integers(1, 41, size=U)
    lens[U // 2] = 1
    utts = []
    for u in range(U):
        n = int(lens[u])
        if u % 3 == 2:
            x = synth.sample_utterance(spec, lex, rng.integers(1, lex.n_words, size=2), seed=7 * U + u, frames_per_state=(2, 4))[:n]
            if len(x) < n:
                x = np.concatenate([x, synth.make_features(n - len(x), D, seed=u)])
        else:
            x = synth.make_features(n, D, seed=3 * U + u)
        utts.append(x.astype(np.float32))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    feats = np.concatenate(utts)
    feats.setflags(write=False)
    off.setflags(write=False)
    return feats, off


_ORACLE = {}


def _oracle_words(oracle_lib, tmp_path, U):
    """(words, word_off) of the batch by the oracle, utterance by utterance; once per size"""
    if U not in _ORACLE:
        lex, _, mp = _model_file(tmp_path)
        feats, off = _batch(U)
        orc = oracle_lib.Oracle(mp, D, lex, am_threshold=AM_THRESHOLD, word_penalty=WORD_PENALTY)
        per = [orc.decode(feats[int(off[u]):int(off[u + 1])]) for u in range(U)]
        orc.close()
        woff = np.concatenate([[0], np.cumsum([len(w) for w in per])]).astype(np.uint64)
        words = np.concatenate(per).astype(np.uint32) if U else np.zeros(0, np.uint32)
        _ORACLE[U] = (words, woff)
    return _ORACLE[U]


def _recognize(monkeypatch, mp, lex, U, route, chunk_mb=None):
    feats, off = _batch(U)
    monkeypatch.setenv("SRGPU_GATHER", route)
    if chunk_mb is None:
        monkeypatch.delenv("SRGPU_SCORE_CHUNK_MB", raising=False)
    else:
        monkeypatch.setenv("SRGPU_SCORE_CHUNK_MB", str(chunk_mb))
    word_off, automaton, sil_state = lex.flatten()
    with capi.Model.from_mixset(mp, D) as m:  # (both knobs are read when the model is created)
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, (3.0, 0.0, 30.0), sil_state)
        corpus = m.upload(feats, off)
        words, woff = corpus.recognize(lexh, AM_THRESHOLD, WORD_PENALTY)
        again, woff2 = corpus.recognize(lexh, AM_THRESHOLD, WORD_PENALTY)  # the corpus's result block, used a second time
        assert np.array_equal(words, again) and np.array_equal(woff, woff2)
        corpus.close()
        lexh.close()
    return words[:int(woff[-1])].copy(), woff


@pytest.mark.parametrize("U", [1, 3, 70, 1030])
def test_device_route_returns_the_host_routes_bytes_and_the_oracles_words(tmp_path, monkeypatch, oracle_lib, U):
    lex, _, mp = _model_file(tmp_path)
    want_words, want_off = _oracle_words(oracle_lib, tmp_path, U)
    counts = np.diff(want_off.astype(np.int64))
    if U >= 70:  # the batch is what the docstring says it is
        assert (counts == 0).sum() >= 5 and (counts > 0).sum() >= 5, counts
        assert (np.diff(_batch(U)[1].astype(np.int64)) == 1).any()
    got = {route: _recognize(monkeypatch, mp, lex, U, route) for route in ROUTES}
    dw, do = got["device"]
    hw, ho = got["host"]
    assert do.dtype == np.uint64 and dw.dtype == np.uint32
    assert do.tobytes() == ho.tobytes()
    assert dw.tobytes() == hw.tobytes()
    assert np.array_equal(do, want_off)
    assert np.array_equal(dw, want_words)


def test_several_score_chunks(tmp_path, monkeypatch, oracle_lib):
    """SRGPU_SCORE_CHUNK_MB=0: every utterance a chunk of its own, the compaction behind the last of 70 searches"""
    lex, _, mp = _model_file(tmp_path)
    want_words, want_off = _oracle_words(oracle_lib, tmp_path, 70)
    dw, do = _recognize(monkeypatch, mp, lex, 70, "device", chunk_mb=0)
    hw, ho = _recognize(monkeypatch, mp, lex, 70, "host", chunk_mb=0)
    assert do.tobytes() == ho.tobytes() and dw.tobytes() == hw.tobytes()
    assert np.array_equal(do, want_off) and np.array_equal(dw, want_words)


def test_bigram_search_all_four_arrays(tmp_path, monkeypatch, oracle_lib):
    """sr_recognize_bigram_corpus at U = 70: word, score, time and offsets of the device route equal the host route's bit for bit,
    and the oracle's LinearSearch restatement"""
    lex, _, mp = _model_file(tmp_path)
    feats, off = _batch(70)
    word_off, mixtures, _ = lex.flatten()
    W = lex.n_words
    p = np.random.default_rng(8).dirichlet(np.ones(W), size=W)
    lm = (-np.log(p)).T.astype(np.float32).copy()
    tdp = np.array([[3.0, 0.0, 3.0, 5.0], [0.0001, 3.0, np.inf, 2.0]], np.float32)  # cheap word exits: 1 .. 7 entries per utterance
    got = {}
    for route in ROUTES:
        monkeypatch.setenv("SRGPU_GATHER", route)
        with capi.Model.from_mixset(mp, D) as m:
            bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
            corpus = m.upload(feats, off)
            got[route] = corpus.recognize_bigram(bg, 200.0, capi.FLT_MAX)
            corpus.close()
            bg.close()
    for a, b in zip(got["device"], got["host"]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    gw, gs, gt, goff = got["device"]
    assert len(set(np.diff(goff.astype(np.int64)).tolist())) >= 4  # (segments of several lengths)
    orc = oracle_lib.Oracle(mp, D, lex)
    for u in range(70):
        dense = orc.score_matrix(feats[int(off[u]):int(off[u + 1])])
        w, s, t = oracle_lib.bigram_decode(dense, word_off, mixtures, lex.silence_idx, lm, tdp, 200.0, capi.FLT_MAX)
        a, b = int(goff[u]), int(goff[u + 1])
        assert np.array_equal(gw[a:b], w) and np.array_equal(gt[a:b], t), u
        assert np.array_equal(gs[a:b].view(np.uint32), s.view(np.uint32)), u
    orc.close()


# ---- the checks, through sr_gather_words: search outputs made up by the test -------------------------------------------------------

def _made_up(U, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, size=U)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    counts = np.minimum(rng.integers(0, 12, size=U), lens).astype(np.uint32)
    counts[rng.integers(0, U, size=max(1, U // 4))] = 0
    words = rng.integers(0, 1 << 32, size=int(off[-1]), dtype=np.uint64).astype(np.uint32)  # slots beyond a count hold junk
    return lens, off, counts, np.zeros(U, np.uint32), words


def _packed(off, counts, words):
    per = [words[int(off[u]):int(off[u]) + int(counts[u])] for u in range(len(counts))]
    return np.concatenate(per), np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)


@pytest.fixture(params=ROUTES)
def routed_model(request, tmp_path, monkeypatch):
    _, _, mp = _model_file(tmp_path)
    monkeypatch.setenv("SRGPU_GATHER", request.param)
    with capi.Model.from_mixset(mp, D) as m:
        yield m


@pytest.mark.parametrize("U", [1, 8, 9, 70, 1030, 2100])
def test_hook_packs_the_words(routed_model, U):
    lens, off, counts, flags, words = _made_up(U, 40 + U)
    flags[U // 3] = 1 | 2  # the slow-path and replay marks are not errors
    counts[U - 1] = lens[U - 1]  # a full last utterance: the last slot of the array is read
    want_words, want_off = _packed(off, counts, words)
    got_words, got_off = routed_model.gather_words(off, counts, flags, words)
    assert np.array_equal(got_off, want_off)
    assert got_words.tobytes() == want_words.tobytes()


def test_hook_no_utterances_and_no_words(routed_model):
    got_words, got_off = routed_model.gather_words(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert len(got_words) == 0 and got_off.tolist() == [0]
    lens, off, counts, flags, words = _made_up(1500, 3)
    got_words, got_off = routed_model.gather_words(off, np.zeros_like(counts), flags, words)
    assert len(got_words) == 0 and not got_off.any()


@pytest.mark.parametrize("U", [70, 1030])
def test_hook_lower_utterance_wins_count_before_flag(routed_model, U):
    """a corrupt flag on utterance 5 (U = 1030: beyond the first tile), a count above T on utterance 2: the count error of 2"""
    lens, off, counts, flags, words = _made_up(U, 50 + U)
    hi = 5 if U == 70 else 1027
    flags[hi] = 4
    counts[2] = lens[2] + 3
    counts[hi + 1] = lens[hi + 1] + 1  # (a later count error does not displace the first)
    with pytest.raises(capi.SrError) as e:
        routed_model.gather_words(off, counts, flags, words)
    assert e.value.code == capi.SR_ECORRUPT
    assert f"utterance 2: {int(lens[2]) + 3} words for {int(lens[2])} frames" in str(e.value)


def test_hook_lower_utterance_wins_flag_before_count(routed_model):
    lens, off, counts, flags, words = _made_up(1030, 61)
    flags[1025] = 4
    counts[1029] = lens[1029] + 1
    with pytest.raises(capi.SrError) as e:
        routed_model.gather_words(off, counts, flags, words)
    assert e.value.code == capi.SR_ECORRUPT
    assert "utterance 1025: the traceback does not walk back to frame 0" in str(e.value)


def test_hook_same_utterance_reports_corrupt(routed_model):
    lens, off, counts, flags, words = _made_up(70, 62)
    flags[33] = 4 | 1
    counts[33] = lens[33] + 7
    with pytest.raises(capi.SrError) as e:
        routed_model.gather_words(off, counts, flags, words)
    assert e.value.code == capi.SR_ECORRUPT
    assert "utterance 33: the traceback does not walk back to frame 0" in str(e.value)


def test_unknown_route_name_is_refused(tmp_path, monkeypatch):
    _, _, mp = _model_file(tmp_path)
    monkeypatch.setenv("SRGPU_GATHER", "sideways")
    with pytest.raises(capi.SrError):
        capi.Model.from_mixset(mp, D)
