"""sr_stream_stable (stream_commit_kernel): the stable prefix of a zerogram stream's result, its commit point and the trailing
silence, after every push.

(a) Safety: what stable() returned after t frames is a prefix of partial() at t and at every later frame whose traceback entry is
    finite; the commit point never decreases; asking changes nothing (the final words and traceback equal sr_recognize_corpus').
(b) Exactness: tests/stream_commit_reference.py runs the same search in numpy with its hypotheses in the open.  It must first
    reproduce the library's own traceback; then commit point, stable words and trailing silence must equal what
    tests/commit_reference.py gives on the reference's alive set at every frame.  This is the check that catches a kernel reading
    the other (stale) buffer of the search's double-buffered hypotheses: that answer is safe, only late, so (a) passes it.
    The fixtures were chosen so that the commit point is strictly between 0 and t at a quarter of the frames at least and the
    trailing silence is non-zero at some: both are asserted.
(c) Several streams in one call at frames of both parities, slot reuse, and error paths that leave every output untouched."""
import math
import os

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import stream_commit_reference as scr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz")
SR_EINVAL = -1
TDP = (3.0, 0.0, 30.0)
WP = 10.0
DIM = 39
# every word has two positions or more (stream_commit_reference): silence is one state held for several positions
LEXICA = {
    "w6x3": synth.LexiconSpec(np.array([1, 3, 3, 3, 3, 3], np.uint16), np.array([3, 1, 1, 1, 1, 1], np.uint16), 0),   # 6 words x 3 positions
    "w5x9": synth.LexiconSpec(np.array([1, 3, 4, 5, 11], np.uint16), np.array([9, 3, 3, 2, 1], np.uint16), 0),        # 9, 9, 12, 10, 11 positions
}
# (seed, words, frames per state): utterances of 59 and 75 frames (w6x3), 100 and 71 frames (w5x9)
UTTS = {"w6x3": ((4110, 3, (2, 4)), (4111, 2, (3, 6))), "w5x9": ((4110, 3, (1, 2)), (4111, 2, (1, 2)))}


class Setup:
    def __init__(self, name, tmp):
        self.lex = LEXICA[name]
        self.spec = synth.make_mixset(self.lex.n_states, 2, DIM, seed=4101)
        self.mp = str(tmp / (name + ".mix"))
        synth.write_mixset(self.mp, self.spec)
        self.word_off, self.automaton, self.sil_state = self.lex.flatten()
        self.utts = []
        for seed, nw, fps in UTTS[name]:
            words = np.random.default_rng(seed).integers(1, self.lex.n_words, size=nw)
            self.utts.append(synth.sample_utterance(self.spec, self.lex, words, seed=seed, frames_per_state=fps))
        self.model = capi.Model.from_mixset(self.mp, DIM)
        self.lexh = self.model.lexicon(self.word_off, self.automaton, self.lex.silence_idx, TDP, self.sil_state)
        self.scores = [self.model.score_frames(u, capi.GMM_DEFAULT) for u in self.utts]
        self.net = scr.Net(self.word_off, self.automaton, self.lex.silence_idx, self.sil_state, TDP)
        self._ref = {}

    def reference(self, u, beam):
        """per frame t = 0 .. T of utterance u: (commit, silence), and the final traceback -- computed once per (u, beam)"""
        if (u, beam) not in self._ref:
            assert (self.scores[u] >= 0).all()  # the restatement's premise
            s = scr.Search(self.net, beam, WP)
            per = [(s.commit(), s.silence())]
            for row in self.scores[u]:
                s.push(row)
                per.append((s.commit(), s.silence()))
            self._ref[(u, beam)] = (per, np.array(s.tb_score), np.array(s.tb_word, np.uint16), np.array(s.tb_bkp, np.uint16))
        return self._ref[(u, beam)]

    def close(self):
        self.lexh.close()
        self.model.close()


@pytest.fixture(scope="module", params=sorted(LEXICA))
def setup(request, tmp_path_factory):
    s = Setup(request.param, tmp_path_factory.mktemp("stable"))
    yield s
    s.close()


def _is_prefix(a, b):
    return len(a) <= len(b) and np.array_equal(a, b[: len(a)])


def _stream(st, feats, piece):
    """one utterance through `st` in pieces; after every push: (t, partial, stable words, commit, silence); then the final result"""
    sid = st.begin()
    rec = []
    words0, commit0, sil0 = st.stable([sid])
    assert len(words0[0]) == 0 and commit0[0] == 0 and sil0[0] == 0  # nothing pushed: B = {0}
    for t in range(0, len(feats), piece):
        st.push({sid: feats[t:t + piece]})
        words, commit, sil = st.stable([sid])
        rec.append((min(t + piece, len(feats)), st.partial(sid), words[0], int(commit[0]), int(sil[0])))
    return rec, st.end(sid, traceback=True)


def _check_safety(rec, tb_score):
    for i, (t, _, stable, commit, _) in enumerate(rec):
        assert commit <= t
        if i:
            assert commit >= rec[i - 1][3], (t, commit, rec[i - 1][3])  # never moves back
            assert _is_prefix(rec[i - 1][2], stable), t                 # and neither do the words
        for t2, partial2, _, _, _ in rec[i:]:
            if math.isfinite(tb_score[t2]):
                assert _is_prefix(stable, partial2), (t, t2, stable, partial2)


def _batch(s, u, beam):
    c = s.model.upload(s.utts[u], np.array([0, len(s.utts[u])], np.uint64))
    words, _, tb = c.recognize(s.lexh, beam, WP, capi.GMM_DEFAULT, traceback=True)
    c.close()
    return words, tb


@pytest.mark.parametrize("beam", [60.0, math.inf])
def test_safety_and_exactness_at_every_push(setup, beam):
    s = setup
    for u, feats in enumerate(s.utts):
        T = len(feats)
        assert 40 <= T <= 120
        per, ref_score, ref_word, ref_bkp = s.reference(u, beam)
        # the fixtures exercise the commit point and the silence count (chosen on the CPU; held here)
        assert sum(0 < per[t][0] < t for t in range(1, T + 1)) * 4 >= T
        assert any(per[t][1] > 0 for t in range(1, T + 1))
        bwords, (btb_s, btb_w, btb_b) = _batch(s, u, beam)
        for piece in (1, 3, 7) if u == 0 else (1,):  # 3 and 7: a call's floor is several frames old, both buffer parities are read
            with s.model.stream(s.lexh, beam, WP, capi.GMM_DEFAULT, max_streams=1, max_frames=T) as st:
                rec, (fwords, (tb_s, tb_w, tb_b)) = _stream(st, feats, piece)
            # asking changed nothing: the batch decoder's result, bit for bit
            assert np.array_equal(fwords, bwords)
            assert np.array_equal(tb_s.view(np.uint64), btb_s[: T + 1].view(np.uint64))
            assert np.array_equal(tb_w, btb_w[: T + 1]) and np.array_equal(tb_b, btb_b[: T + 1])
            # the restatement reproduces the library's traceback, or its alive sets mean nothing
            assert np.array_equal(tb_w, ref_word) and np.array_equal(tb_b, ref_bkp), (u, piece)
            assert np.array_equal(tb_s.view(np.uint64), ref_score.view(np.uint64))
            _check_safety(rec, tb_s)
            for t, _, stable, commit, sil in rec:
                assert commit == per[t][0], (u, piece, t, commit, per[t][0])
                assert np.array_equal(stable, scr.walk(tb_w, tb_b, commit, s.lex.silence_idx)), (u, piece, t)
                assert sil == per[t][1], (u, piece, t, sil, per[t][1])


def test_two_streams_in_one_call_and_slot_reuse(setup):
    s = setup
    beam = 60.0
    f0, f1 = s.utts
    per0, *_ = s.reference(0, beam)
    per1, *_ = s.reference(1, beam)
    with s.model.stream(s.lexh, beam, WP, capi.GMM_DEFAULT, max_streams=2, max_frames=max(len(f0), len(f1))) as st:
        a, b = st.begin(), st.begin()
        st.push({a: f0[:40], b: f1[:33]})  # one at an even frame, one at an odd frame
        words, commit, sil = st.stable([b, a])
        assert [int(x) for x in commit] == [per1[33][0], per0[40][0]] and [int(x) for x in sil] == [per1[33][1], per0[40][1]]
        pa, pb = st.partial(a), st.partial(b)
        assert _is_prefix(words[1], pa) and _is_prefix(words[0], pb)
        st.push({a: f0[40:41]})
        words, commit, sil = st.stable([a, b])  # a moved on, b did not
        assert [int(x) for x in commit] == [per0[41][0], per1[33][0]] and [int(x) for x in sil] == [per0[41][1], per1[33][1]]
        st.push({a: f0[41:]})
        _, commit, _ = st.stable([a])
        assert int(commit[0]) == per0[len(f0)][0] > 10
        st.end(a)
        # the slot's next utterance starts from commit point 0, not from the last utterance's
        c = st.begin()
        assert c % 2 == a % 2 and c != a
        words, commit, sil = st.stable([c])
        assert len(words[0]) == 0 and int(commit[0]) == 0 and int(sil[0]) == 0
        for t in (5, 12, 33):
            st.push({c: f1[st.frames[c]:t]})
            words, commit, sil = st.stable([c, b])
            assert int(commit[0]) == per1[t][0] and int(sil[0]) == per1[t][1], t
            assert int(commit[0]) < per0[len(f0)][0]
        assert np.array_equal(words[0], words[1])  # the same utterance at the same frame in the other slot
        st.end(b), st.end(c)


def test_error_paths_leave_the_outputs_untouched(setup):
    s = setup
    L = capi.lib()
    f0 = s.utts[0]
    with s.model.stream(s.lexh, 60.0, WP, capi.GMM_DEFAULT, max_streams=3, max_frames=len(f0)) as st:
        a, b, gone = st.begin(), st.begin(), st.begin()
        st.push({a: f0, b: f0[:50]})
        st.end(gone)
        want_words, want_commit, _ = st.stable([a, b])
        assert len(want_words[0]) >= 2

        def call(ids, cap, silence=True):
            ids = np.asarray(ids, np.uint32)
            out = np.full(64, 0xABCD, np.uint32)
            off = np.full(len(ids) + 1, 0xABCD, np.uint64)
            commit, sil = np.full(len(ids), 0xABCD, np.uint32), np.full(len(ids), 0xABCD, np.uint32)
            rc = L.sr_stream_stable(st.h, len(ids), ids.ctypes.data, out.ctypes.data, cap, off.ctypes.data, commit.ctypes.data,
                                    sil.ctypes.data if silence else None)
            return rc, out, off, commit, sil

        for ids in ([a, 9999], [a, gone], [a, b, a]):  # unknown, ended, repeated
            rc, out, off, commit, sil = call(ids, 64)
            assert rc == SR_EINVAL
            assert (out == 0xABCD).all() and (off == 0xABCD).all() and (commit == 0xABCD).all() and (sil == 0xABCD).all()
        n0, n1 = len(want_words[0]), len(want_words[1])
        rc, out, off, commit, sil = call([a, b], n0 + n1 - 1)  # one slot short: the offsets needed, nothing else
        assert rc == SR_EINVAL and [int(x) for x in off] == [0, n0, n0 + n1]
        assert (out == 0xABCD).all() and (commit == 0xABCD).all() and (sil == 0xABCD).all()
        rc, out, off, commit, sil = call([a, b], n0 + n1, silence=False)  # exactly enough; out_silence may be NULL
        assert rc == 0 and [int(x) for x in off] == [0, n0, n0 + n1]
        assert np.array_equal(out[:n0], want_words[0]) and np.array_equal(out[n0:n0 + n1], want_words[1]) and (out[n0 + n1:] == 0xABCD).all()
        assert np.array_equal(commit, want_commit) and (sil == 0xABCD).all()


def test_real_speech_negative_costs_is_safe(tmp_path):
    """the sequential boundary replay is live here (negative emission costs): safety, monotonicity and the unchanged final result"""
    z = np.load(REAL)
    lex = synth.sietill_lexicon()
    word_off, automaton, sil = lex.flatten()
    mp = tmp_path / "real.mix"
    mp.write_bytes(z["model_none"].tobytes())
    off = z["frame_off"].astype(np.int64)
    tdp = tuple(float(x) for x in z["tdp"])
    dim = int(z["dim"])
    beam, wp = float(z["none_wide_beam"]), float(z["none_wide_wp"])
    with capi.Model.from_mixset(str(mp), dim, capi.POOL_NONE, True) as m:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, tdp, sil)
        moved = 0
        for u in range(2):
            feats = z["feats"][off[u]:off[u + 1]]
            c = m.upload(feats, np.array([0, len(feats)], np.uint64))
            bwords, _, (btb_s, btb_w, btb_b) = c.recognize(lexh, beam, wp, capi.GMM_DEFAULT, traceback=True)
            c.close()
            with m.stream(lexh, beam, wp, capi.GMM_DEFAULT, max_streams=1, max_frames=len(feats)) as st:
                rec, (fwords, (tb_s, tb_w, tb_b)) = _stream(st, feats, 3)
            assert np.array_equal(fwords, bwords) and np.array_equal(tb_w, btb_w[: len(feats) + 1]) and np.array_equal(tb_b, btb_b[: len(feats) + 1])
            assert np.array_equal(tb_s.view(np.uint64), btb_s[: len(feats) + 1].view(np.uint64))
            _check_safety(rec, tb_s)
            for t, _, stable, commit, _ in rec:
                assert np.array_equal(stable, scr.walk(tb_w, tb_b, commit, lex.silence_idx))
            moved += rec[-1][3] > 0
        assert moved  # the commit point does leave frame 0 on real speech
        lexh.close()
