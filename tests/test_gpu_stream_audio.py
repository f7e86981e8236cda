"""Streaming from audio (sr_stream_push_audio, sr_stream_finish_audio and the bigram twins; stream_frontend_kernel): utterances fed as
PCM samples in pieces of every kind -- whole, a shift at a time, one sample at a time, 37 at a time, random sizes, a second at a time --
several per push, at most five open at once.  No tolerance anywhere: with energy_max_norm == 0 the streamed rows must carry the bits
of sr_corpus_from_audio on the whole utterances, so the words and the traceback must be the batch's on that corpus; with the energy
maximum on, the rows must be the batch's no-maximum rows with the causal maximum of tests/stream_audio_reference.py applied."""
import os

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import frontend_reference as R
from tests import stream_audio_reference as SR
from tests.test_gpu_frontend import MFCC16, MFCC64, batch, post_of, u32
from tests.test_gpu_stream import _check_against_batch

pytestmark = pytest.mark.gpu

MFCC_GAP = dict(MFCC64, shift=80)                       # shift > window: samples between the frames are passed over
TDP = (3.0, 0.0, 30.0)
FRAMES = [0, 1, 2, 3, 4, 7, 17, 60, 250]
MODES = ["one", "one", "whole", "one", "one", "shift", "37", "random", "16000"]   # by utterance; "one" only where T <= 4
SR_EINVAL, SR_ELIMIT = -1, -4


def utterances(p):
    """the test signals end to end, cut to FRAMES frames each (a few samples more, so that a tail is left over)"""
    base = np.concatenate(R.signals(p["sample_rate"]))
    out = []
    for i, T in enumerate(FRAMES):
        n = p["window"] - 1 if T == 0 else p["window"] + (T - 1) * p["shift"] + (7 * i) % p["shift"]
        o = 1000 * i
        out.append(base[o:o + n].copy())
        assert R.n_frames(len(out[-1]), p) == T
    return out


def piece(mode, rng, left, p):
    k = {"whole": left, "shift": p["shift"], "one": 1, "37": 37, "random": int(rng.integers(1, 1001)), "16000": 16000}[mode]
    return min(k, left)


def stream_audio(st, utts, modes, p, seed, finish, max_open=5, after_push=None):
    """Every utterance through `st` as audio: at most max_open open at once, each push carries a random subset of the open ones with a
    piece by the utterance's mode; an utterance with no samples left is finished and ended a random number of pushes later, several
    finished in one call where it happens.  -> ({u: its rows, concatenated}, {u: finish(st, id)}, pushes)"""
    rng = np.random.default_rng(seed)
    todo, open_, done = list(range(len(utts))), {}, {}
    rows = {u: [] for u in todo}
    out, pushes = {}, 0
    while todo or open_ or done:
        while todo and len(open_) + len(done) < max_open:
            u = todo.pop(0)
            open_[u] = (st.begin(), 0)
        push = {}
        for u in list(open_):
            if rng.random() < 0.75:
                sid, at = open_[u]
                k = piece(modes[u], rng, len(utts[u]) - at, p)
                push[sid] = (u, utts[u][at:at + k])
                open_[u] = (sid, at + k)
        if push:
            got = st.push_audio({sid: x for sid, (u, x) in push.items()}, feats=True)
            pushes += 1
            for sid, (u, _) in push.items():
                rows[u].append(got[sid])
                if after_push:
                    after_push(u, sid, open_[u][1])
        ready = [u for u in open_ if open_[u][1] == len(utts[u]) and rng.random() < 0.6]
        if ready:
            got = st.finish_audio([open_[u][0] for u in ready], feats=True)
            for u in ready:
                sid = open_.pop(u)[0]
                rows[u].append(got[sid])
                done[u] = sid
        for u in list(done):
            if rng.random() < 0.5:
                out[u] = finish(st, done.pop(u))
    return {u: np.concatenate(r) for u, r in rows.items()}, out, pushes


def norm_of(dim, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=dim) * 3.0, rng.uniform(0.5, 3.0, size=dim)


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """the lexicon of the front-end tests' end-to-end case and a 3-density mixset per dimension -> make(dim) = (mixset path, lexicon parts)"""
    tmp = tmp_path_factory.mktemp("streamaudio")
    lex = synth.make_lexicon(6, 3, 1)
    word_off, automaton, sil = lex.flatten()

    def make(dim):
        mp = os.path.join(str(tmp), f"e{dim}.mix")
        if not os.path.exists(mp):
            synth.write_mixset(mp, synth.make_mixset(lex.n_states, 3, dim, seed=41))
        return mp, (word_off, automaton, lex.silence_idx, TDP, sil)
    return make


def batch_rows(fe, utts):
    samples, soff = batch(utts)
    corpus = fe.from_audio(samples, soff)
    rows, off = corpus.download(), corpus.frame_off.astype(np.int64)
    return corpus, rows, off


def assert_rows(got, rows, off, utts):
    for u in range(len(utts)):
        want = rows[off[u]:off[u + 1]]
        assert got[u].shape == want.shape, (u, got[u].shape, want.shape)
        assert np.array_equal(u32(got[u]), u32(want)), (u, int(np.argmax((u32(got[u]) != u32(want)).any(axis=1))))


# ---- 1. features -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("p", [MFCC16, MFCC64, MFCC_GAP], ids=["400-160", "64-32", "64-80"])
def test_streamed_rows_are_the_batch_front_end_s(net, p, normalise):
    dim = 2 * p["n_cepstra"] + 1
    mp, lexparts = net(dim)
    utts = utterances(p)
    post = post_of(p, energy_max_norm=0)
    if normalise:
        post["mean"], post["stddev"] = norm_of(dim, 5)
    with capi.Model.from_mixset(mp, dim) as m, m.frontend(p, post) as fe:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off = batch_rows(fe, utts)
        assert np.array_equal(np.diff(off), FRAMES)
        corpus.close()
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe)
            first, _, pushes = stream_audio(st, utts, MODES, p, 21, lambda st, sid: st.end(sid))
            assert pushes > 100
            assert_rows(first, rows, off, utts)
            again, _, _ = stream_audio(st, utts, MODES, p, 21, lambda st, sid: st.end(sid))
            for u in range(len(utts)):
                assert np.array_equal(u32(again[u]), u32(first[u])), u
            # another assignment of the cuts, and another interleaving: the same bits
            other, _, _ = stream_audio(st, utts, ["whole", "whole", "37", "shift", "random", "37", "shift", "16000", "random"], p, 22,
                                       lambda st, sid: st.end(sid), max_open=3)
            assert_rows(other, rows, off, utts)
        lexh.close()


# ---- 2. words, zerogram ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [capi.GMM_PREFILTER, capi.GMM_EXACT], ids=["prefilter", "exact"])
def test_streamed_words_and_traceback_are_the_batch_s(net, kernel):
    p = MFCC16
    mp, lexparts = net(25)
    utts = utterances(p)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as fe:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off = batch_rows(fe, utts)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, kernel, traceback=True)
        corpus.close()
        partials = []

        def after_push(u, sid, n_samples):
            if len(partials) < 8 and u >= 5 and n_samples % 3 == 0:
                w, n = st.partial(sid, frames=True)
                assert n == max(fe.frames(n_samples) - 3, 0)
                partials.append((u, n, w))

        with m.stream(lexh, 500.0, 10.0, kernel, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe)
            got_rows, got, _ = stream_audio(st, utts, MODES, p, 31, lambda st, sid: st.end(sid, traceback=True), after_push=after_push)
        assert_rows(got_rows, rows, off, utts)
        assert sorted(got) == list(range(len(utts)))
        _check_against_batch(got, words, woff, tb, corpus.frame_off)
        # a partial result is the batch's on the rows searched so far
        partials = [x for x in partials if x[1] > 0]
        assert partials
        poff = np.concatenate([[0], np.cumsum([n for _, n, _ in partials])]).astype(np.uint64)
        pc = m.upload(np.concatenate([rows[off[u]:off[u] + n] for u, n, _ in partials]), poff)
        pw, pwoff = pc.recognize(lexh, 500.0, 10.0, kernel)
        pc.close()
        for i, (u, n, w) in enumerate(partials):
            assert np.array_equal(w, pw[int(pwoff[i]):int(pwoff[i + 1])]), (u, n)
        lexh.close()


# ---- 3. bigram -------------------------------------------------------------------------------------------------------------------
def test_streamed_bigram_items_are_the_batch_s(tmp_path):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    p = MFCC16
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=25)
    utts = utterances(p)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as fe:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus, rows, off = batch_rows(fe, utts)
        gw, gs, gt, goff = corpus.recognize_bigram(bg, 60.0, 30.0, capi.GMM_PREFILTER)
        corpus.close()
        with m.bigram_stream(bg, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES) + 1) as st:
            st.set_frontend(fe)
            got_rows, got, _ = stream_audio(st, utts, MODES, p, 41, lambda st, sid: st.end(sid))
        assert_rows(got_rows, rows, off, utts)
        for u in range(len(utts)):
            a, b = int(goff[u]), int(goff[u + 1])
            assert _same(got[u], (gw[a:b], gs[a:b], gt[a:b])), u
        bg.close()


# ---- 4. the energy maximum -------------------------------------------------------------------------------------------------------
def loud_start(p):
    """quiet noise with a loud first 800 samples: the energy maximum lies in the first frames"""
    x = R.signals(p["sample_rate"], seed=8)[3][:6000].astype(np.int32)
    x[:800] += R.signals(p["sample_rate"], seed=9)[0][:800].astype(np.int32) * 20
    return np.clip(x, -32768, 32767).astype(np.int16)


def periodic(p, n=4000):
    """a period of 16 samples: every frame but the first has the same samples and the same sample before them, so the maximum is tied"""
    return np.tile(np.rint(9000.0 * np.sin(2.0 * np.pi * np.arange(16) / 16.0)).astype(np.int16), n // 16)


@pytest.mark.parametrize("case", ["plain", "normalised", "signed-zeros"])
def test_the_energy_maximum_is_the_causal_one(net, case):
    p = MFCC16
    mp, lexparts = net(25)
    utts = utterances(p) + [loud_start(p), periodic(p)]
    modes = MODES + ["random", "37"]
    loud, tied = len(utts) - 2, len(utts) - 1
    norm = {}
    if case != "plain":
        mean, stddev = norm_of(25, 6)
        if case == "signed-zeros":   # component 0 becomes +0 above the mean and -0 below it: a maximum of zero in both signs, tied everywhere
            mean[0], stddev[0] = 60.0, np.inf
        norm = dict(mean=mean, stddev=stddev)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0, **norm)) as fe0, \
            m.frontend(p, post_of(p, energy_max_norm=1, **norm)) as fe1:
        lexh = m.lexicon(*lexparts)
        c0, plain_rows, off = batch_rows(fe0, utts)
        c1, max_rows, _ = batch_rows(fe1, utts)
        c0.close()
        c1.close()
        want = np.concatenate([SR.causal_max(plain_rows[off[u]:off[u + 1]], 3) for u in range(len(utts))])
        # the constructed utterance: its maximum is in the first step + 1 frames, so the causal rows are the batch's
        lr = plain_rows[off[loud]:off[loud + 1]]
        assert int(np.argmax(lr[:, 0])) <= 3
        assert np.array_equal(u32(want[off[loud]:off[loud + 1]]), u32(max_rows[off[loud]:off[loud + 1]]))
        tr = plain_rows[off[tied]:off[tied + 1], 0]
        assert len(tr) > 20 and len(np.unique(u32(tr[1:]))) == 1
        if case == "signed-zeros":
            z = plain_rows[:, 0]
            assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
        else:   # elsewhere the causal maximum is not the batch's: the noise utterances' maxima come late
            assert not np.array_equal(u32(want), u32(max_rows))
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe1)
            got, _, _ = stream_audio(st, utts, modes, p, 51, lambda st, sid: st.end(sid))
        assert_rows(got, want, off, utts)
        assert np.array_equal(u32(got[loud]), u32(max_rows[off[loud]:off[loud + 1]]))
        lexh.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_as_it_was(net):
    p = MFCC16
    mp, lexparts = net(25)
    mp13, _ = net(13)
    utt = utterances(p)[6]                       # 17 frames
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    post = post_of(p, energy_max_norm=0)
    with capi.Model.from_mixset(mp, 25) as m, capi.Model.from_mixset(mp13, 13) as other, m.frontend(p, post) as fe, \
            m.frontend(None, post) as cep_only, other.frontend(MFCC64, post_of(MFCC64)) as foreign:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off = batch_rows(fe, [utt])
        corpus.close()
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=3, max_frames=17) as st:
            def raw_push(ids, samples, soff, out=None, cap=0, foff=None):
                ids = np.asarray(ids, np.uint32)
                return L.sr_stream_push_audio(st.h, len(ids), P(ids), P(samples), P(soff), P(out), cap, P(foff))

            def refused(code, call):
                with pytest.raises(capi.SrError) as e:
                    call()
                assert e.value.code == code, e.value
                return str(e.value)

            two = np.array([0, 500], np.uint64)
            sid = st.begin()
            assert raw_push([sid], utt[:500], two) == SR_EINVAL                                  # no front end
            assert L.sr_stream_set_frontend(st.h, fe.h) == SR_EINVAL                            # an id is open
            assert st.end(sid).size == 0
            assert L.sr_stream_set_frontend(st.h, foreign.h) == SR_EINVAL                       # another model's
            assert L.sr_stream_set_frontend(st.h, cep_only.h) == SR_EINVAL                      # cepstra only
            sid = st.begin()
            assert raw_push([sid], utt[:500], two) == SR_EINVAL                                 # ... and still none attached
            assert st.end(sid).size == 0
            st.set_frontend(fe)
            a, b = st.begin(), st.begin()
            parts = {a: [], b: []}
            parts[a].append(st.push_audio({a: utt[:1000]}, feats=True)[a])                      # 4 statics, 1 row
            assert len(parts[a][0]) == 1
            # every refusal below is followed by the same valid pushes; the rows must still be the batch's
            three = np.array([0, 300, 600], np.uint64)
            assert raw_push([a, a], utt[1000:1600], three) == SR_EINVAL                         # an id twice
            assert raw_push([a, 77], utt[1000:1600], three) == SR_EINVAL                        # an id that is not open
            assert raw_push([a], utt[1000:1500], np.array([1, 501], np.uint64)) == SR_EINVAL    # sample_off[0] != 0
            assert raw_push([a, b], utt[1000:1600], np.array([0, 400, 300], np.uint64)) == SR_EINVAL   # falling
            assert raw_push([a], None, two) == SR_EINVAL
            foff = np.full(2, 99, np.uint64)
            out = np.full((1, 25), 7.5, np.float32)
            assert raw_push([a], utt[1000:1500], two, out, 1, foff) == SR_EINVAL                # 3 rows, room for 1
            assert foff[1] == 3 and b"3 rows" in L.sr_last_error() and (out == 7.5).all()
            refused(SR_EINVAL, lambda: st.push({a: rows[:2]}))                                  # feature rows on an audio id
            refused(SR_EINVAL, lambda: st.end(a))                                               # not finished: the id stays open
            assert raw_push([a], utt, np.array([0, len(utt)], np.uint64)) == SR_ELIMIT          # past max_frames
            st.push({b: rows[:2]})
            assert raw_push([b], utt[:500], two) == SR_EINVAL                                   # audio on a feature id
            assert L.sr_stream_finish_audio(st.h, 1, P(np.array([b], np.uint32)), None, 0, None) == SR_EINVAL
            st.push({b: rows[2:]})
            parts[a].append(st.push_audio({a: utt[1000:1500]}, feats=True)[a])
            assert st.partial(a, frames=True)[1] == 4
            parts[a].append(st.push_audio({a: utt[1500:]}, feats=True)[a])
            parts[a].append(st.finish_audio([a], feats=True)[a])
            assert np.array_equal(u32(np.concatenate(parts[a])), u32(rows))
            refused(SR_EINVAL, lambda: st.push_audio({a: utt[:10]}))                            # audio after the finish
            refused(SR_EINVAL, lambda: st.finish_audio([a]))
            wa, wb = st.end(a, traceback=True), st.end(b, traceback=True)
            refused(SR_EINVAL, lambda: st.push_audio({a: utt[:10]}))                            # an ended id
            # the audio id and the feature id saw the same rows: the same result
            assert np.array_equal(wa[0], wb[0]) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(wa[1], wb[1]))
            # the slot is reused by an utterance of the other kind
            c = st.begin()
            st.push({c: rows})
            assert np.array_equal(st.end(c), wa[0])
            st.set_frontend(None)
            d = st.begin()
            refused(SR_EINVAL, lambda: st.push_audio({d: utt[:10]}))
            st.end(d)
        lexh.close()


# ---- 6. existing behaviour -------------------------------------------------------------------------------------------------------
def test_a_set_with_a_front_end_still_takes_rows(net):
    p = MFCC16
    mp, lexparts = net(25)
    utts = utterances(p)[5:8]
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as fe:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off = batch_rows(fe, utts)
        corpus.close()
        feats = [rows[off[u]:off[u + 1]] for u in range(3)]

        def run(st, audio_too):
            ids = [st.begin() for _ in range(3)]
            extra = st.begin() if audio_too else None
            for t in range(0, 60, 7):
                st.push({i: f[t:t + 7] for i, f in zip(ids, feats)})
                if audio_too:
                    st.push_audio({extra: utts[2][t * 160:(t + 7) * 160]})
            if audio_too:
                st.finish_audio([extra])
                st.end(extra)
            return [st.end(i, traceback=True) for i in ids]

        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=4, max_frames=60) as st:
            want = run(st, False)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=4, max_frames=60) as st:
            st.set_frontend(fe)
            got = run(st, True)
        for (w, tb), (gw, gtb) in zip(want, got):
            assert np.array_equal(w, gw) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(tb, gtb))
        lexh.close()


# ---- 7. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror_streams_audio_to_the_same_words_and_bits(tmp_path):
    """sr::StreamingRecognizer and sr::StreamingLinearSearch (include/sr_sietill.hpp) fed samples through tests/cpp/stream_audio_driver.cpp"""
    import struct
    import subprocess
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "stream_audio_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stream_audio_driver.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    p = MFCC16
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 61, 9, 2, D=25)
    _, automaton, sil_state = lex.flatten()
    utts = [utterances(p)[7], utterances(p)[6]]
    beam, wp, acp, lmp, piece = 500.0, 10.0, 60.0, 30.0, 1111
    blob = struct.pack("<5I3d2f", p["window"], p["shift"], p["n_fft"], p["n_mel"], p["n_cepstra"], p["sample_rate"], p["f_low"], p["f_high"],
                       p["preemphasis"], p["energy_floor"])
    blob += struct.pack("<I", len(word_off) - 1) + np.asarray(word_off, "<u4").tobytes() + np.asarray(mixtures, "<u2").tobytes()
    blob += struct.pack("<I5d", lex.silence_idx, *TDP, beam, wp) + np.asarray(lm, "<f4").tobytes() + np.asarray(tdp, "<f4").tobytes()
    blob += struct.pack("<ffIII", acp, lmp, capi.GMM_PREFILTER, piece, len(utts))
    for x in utts:
        blob += struct.pack("<I", len(x)) + np.ascontiguousarray(x, "<i2").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, mp, "25", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0)) as fe:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, TDP, sil_state)
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        for u, x in enumerate(utts):
            with m.stream(lexh, beam, wp, capi.GMM_PREFILTER, max_streams=1, max_frames=4096) as st:
                st.set_frontend(fe)
                sid = st.begin()
                st.push_audio({sid: x})
                st.finish_audio([sid])
                words = st.end(sid)
            assert [int(v) for v in [ln for ln in lines if ln.startswith(f"words {u}")][0].split()[2:]] == list(words), u
            with m.bigram_stream(bg, acp, lmp, capi.GMM_PREFILTER, max_streams=1, max_frames=4096) as st:
                st.set_frontend(fe)
                sid = st.begin()
                st.push_audio({sid: x})
                st.finish_audio([sid])
                items = st.end(sid)
            v = [int(t, 16) for t in [ln for ln in lines if ln.startswith(f"items {u}")][0].split()[2:]]
            assert _same((v[0::3], np.asarray(v[1::3], np.uint32).view(np.float32), v[2::3]), items), u
        bg.close()
        lexh.close()
