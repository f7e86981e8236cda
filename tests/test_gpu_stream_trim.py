"""sr_stream_trim (stream_trim_kernel): dropping the committed frames of an open zerogram utterance, so that max_frames bounds the
uncommitted window and not the utterance.

Every figure is held against tests/stream_trim_reference.py, which restates the trim on the numpy search of
tests/stream_commit_reference.py (itself held against the library's traceback in tests/test_gpu_stream_stable.py) -- no tolerance
anywhere: words, commit frames and dropped-frame counts are integers, and the final words must be sr_recognize_corpus' on the
whole utterance.  The utterances are three to four sampled utterances back to back (248 and 306 frames); the window each needs is
computed from the reference alone and is far below half the utterance, so every stream here is opened with a max_frames the
utterance passes many times over: without the trim its pushes are SR_ELIMIT."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import frontend_reference as FR
from tests import stream_trim_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden_real", "sietill_real.npz")
DRIVER = os.path.join(ROOT, "tests", "cpp", "stream_trim_driver")
SR_EINVAL, SR_ELIMIT = -1, -4
DIM = 39
WP = ref.WP
# (seeds, words each, frames per state) of the sampled utterances that make one long one: 248 frames (w6x3), 306 frames (w5x9)
UTTS = {"w6x3": ((4120, 4121, 4122, 4123), 3, (2, 4)), "w5x9": ((4120, 4121, 4122), 3, (1, 2))}


class Setup:
    def __init__(self, name, tmp):
        self.name = name
        self.lex = ref.LEXICA[name]
        self.spec = synth.make_mixset(self.lex.n_states, 2, DIM, seed=4101)
        self.mp = str(tmp / (name + ".mix"))
        synth.write_mixset(self.mp, self.spec)
        self.word_off, self.automaton, self.sil_state = self.lex.flatten()
        seeds, nw, fps = UTTS[name]
        self.feats = np.concatenate([
            synth.sample_utterance(self.spec, self.lex, np.random.default_rng(seed).integers(1, self.lex.n_words, size=nw), seed=seed,
                                   frames_per_state=fps) for seed in seeds]).astype(np.float32)
        self.T = len(self.feats)
        assert 200 <= self.T <= 350
        self.model = capi.Model.from_mixset(self.mp, DIM)
        self.lexh = self.model.lexicon(self.word_off, self.automaton, self.lex.silence_idx, ref.TDP, self.sil_state)
        self.scores = self.model.score_frames(self.feats, capi.GMM_DEFAULT)
        assert (self.scores >= 0).all()  # the restatement's premise
        self.net = ref.make_net(self.lex)
        self._runs, self._batch = {}, {}

    def run(self, beam, piece):
        """ref.run with a trim after every push, computed once per (beam, piece) and left unchanged"""
        if (beam, piece) not in self._runs:
            per, tr, _ = ref.run(self.net, beam, WP, self.scores, piece)
            self._runs[(beam, piece)] = (per, ref.window_needed(per), tr.base)
        return self._runs[(beam, piece)]

    def batch(self, beam):
        if beam not in self._batch:
            c = self.model.upload(self.feats, np.array([0, self.T], np.uint64))
            words, _, tb = c.recognize(self.lexh, beam, WP, capi.GMM_DEFAULT, traceback=True)
            c.close()
            self._batch[beam] = (words, tb)
        return self._batch[beam]

    def stream(self, beam, max_frames, max_streams=1):
        return self.model.stream(self.lexh, beam, WP, capi.GMM_DEFAULT, max_streams=max_streams, max_frames=max_frames)

    def close(self):
        self.lexh.close()
        self.model.close()


@pytest.fixture(scope="module", params=sorted(ref.LEXICA))
def setup(request, tmp_path_factory):
    s = Setup(request.param, tmp_path_factory.mktemp("trim"))
    yield s
    s.close()


def _code(excinfo):
    return excinfo.value.code


# ---- 1. past the old limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [60.0, math.inf])
def test_a_window_far_below_the_utterance_serves_it_whole(setup, beam):
    s = setup
    bwords, _ = s.batch(beam)
    assert len(bwords) >= 8
    for piece in (1, 3, 7):
        per, W, base = s.run(beam, piece)
        assert W < s.T / 2 and base > s.T / 2, (piece, W, base)  # a condition on the fixture, met by the reference alone
        assert {r["dropped"] & 1 for r in per if r["dropped"]} == {0, 1}  # frames dropped of both parities: both buffer moves
        with s.stream(beam, W) as st:
            sid = st.begin()
            for n, r in enumerate(per):
                st.push({sid: s.feats[n * piece:(n + 1) * piece]})
                words, commit, _ = st.stable([sid])
                assert np.array_equal(words[0], r["want_stable"]) and int(commit[0]) == r["want_commit"], (piece, r["frames"])
                dropped = st.trim([sid])
                assert int(dropped[0]) == r["dropped"], (piece, r["frames"], int(dropped[0]), r["dropped"])
                partial, frames = st.partial(sid, frames=True)
                assert frames == r["frames"] == min((n + 1) * piece, s.T)
                assert np.array_equal(partial, r["partial"]) and np.array_equal(partial, r["want_partial"]), (piece, r["frames"])
            words, commit, _ = st.stable([sid])  # after the trim: the archive leads, the commit frame counts from the start
            assert np.array_equal(words[0], per[-1]["want_stable"]) and int(commit[0]) == per[-1]["want_commit"]
            assert np.array_equal(st.end(sid), bwords), piece


# ---- 2. a window one too small, and a trim that makes room ------------------------------------------------------------------------------
def _replay(st, sid, feats, events):
    """holds the stream against ref.limited_run's events one by one; -> how many refused pushes a trim rescued"""
    rescued = 0
    for i, e in enumerate(events):
        if e[0] == "refused":
            before = st.partial(sid, frames=True)
            with pytest.raises(capi.SrError) as ei:
                st.push({sid: feats[e[1]:e[2]]})
            assert _code(ei) == SR_ELIMIT
            after = st.partial(sid, frames=True)
            assert before[1] == after[1] and np.array_equal(before[0], after[0])  # a refused push changes nothing
            rescued += i + 2 < len(events) and events[i + 2][0] == "push"
        elif e[0] == "push":
            st.push({sid: feats[e[1]:e[2]]})
            partial, frames = st.partial(sid, frames=True)
            assert frames == e[3] and np.array_equal(partial, e[4]), e[:4]
        elif e[0] == "trim":
            assert int(st.trim([sid])[0]) == e[1], (i, e[1])
            assert np.array_equal(st.partial(sid), e[2])
    return rescued


@pytest.mark.parametrize("beam", [60.0, math.inf])
def test_a_window_one_too_small_is_elimit_and_a_trim_helps_where_the_reference_says_so(setup, beam):
    s = setup
    for piece in (1, 3, 7):
        _, W, _ = s.run(beam, piece)
        # the same schedule, one frame short: some push is refused, and refused again after a trim of nothing
        events = ref.limited_run(s.net, beam, WP, s.scores, piece, 1, W - 1)
        assert events[-1] == ("gave_up",) and events[-3][0] == "trim" and events[-3][1] == 0
        with s.stream(beam, W - 1) as st:
            sid = st.begin()
            _replay(st, sid, s.feats, events)
            st.end(sid)
    # a trim every third push in the window that a trim every push needs: pushes are refused, a trim makes room, the push goes through
    piece = 7
    _, W, _ = s.run(beam, piece)
    events = ref.limited_run(s.net, beam, WP, s.scores, piece, 3, W)
    kinds = [e[0] for e in events]
    assert "gave_up" not in kinds and kinds.count("refused") >= 2
    with s.stream(beam, W) as st:
        sid = st.begin()
        assert _replay(st, sid, s.feats, events) == kinds.count("refused")
        assert np.array_equal(st.end(sid), s.batch(beam)[0])


# ---- 3. never trimmed, and a trim of nothing -----------------------------------------------------------------------------------------
def test_untrimmed_streams_and_trims_of_nothing_return_the_batch_s_bits(setup):
    s = setup
    beam = 60.0
    bwords, (btb_s, btb_w, btb_b) = s.batch(beam)
    per, _, _ = s.run(beam, 7)
    assert per[0]["want_commit"] == 0  # the commit point has not left frame 0 after the first piece: a trim there drops nothing
    got = []
    for trims in (False, True):
        with s.stream(beam, s.T) as st:
            sid = st.begin()
            if trims:
                assert int(st.trim([sid])[0]) == 0  # before any push
                assert st.partial(sid, frames=True)[1] == 0
            st.push({sid: s.feats[:7]})
            if trims:
                assert int(st.trim([sid])[0]) == 0
                assert int(st.trim([sid])[0]) == 0  # right after a trim
            for t in range(7, s.T, 7):
                st.push({sid: s.feats[t:t + 7]})
            got.append(st.end(sid, traceback=True))  # base == 0: the traceback is there
    for words, (tb_s, tb_w, tb_b) in got:
        assert np.array_equal(words, bwords)
        assert np.array_equal(tb_s.view(np.uint64), btb_s[: s.T + 1].view(np.uint64))
        assert np.array_equal(tb_w, btb_w[: s.T + 1]) and np.array_equal(tb_b, btb_b[: s.T + 1])


# ---- 4. two ids in one call, slot reuse ------------------------------------------------------------------------------------------------
def test_two_ids_in_one_call_with_both_parities_and_slot_reuse(setup):
    s = setup
    beam = 60.0
    bwords, _ = s.batch(beam)
    # frames pushed -> (frames the trim then drops, partial after it), from the reference: one id drops an odd count, one an even one
    ds = {}
    for t in range(20, 60):
        tr = ref.TrimSearch(s.net, beam, WP)
        for row in s.scores[:t]:
            tr.push(row)
        ds[t] = (tr.trim(), tr.partial())
    ta = min(t for t, (d, _) in ds.items() if d & 1)
    tb = min(t for t, (d, _) in ds.items() if d and not d & 1)
    assert max(ta, tb) + 7 < s.T // 2
    with s.stream(beam, s.T // 2, max_streams=2) as st:  # (the ids' pushes fall elsewhere than run()'s: a window with room to spare)
        a, b = st.begin(), st.begin()
        st.push({a: s.feats[:ta], b: s.feats[:tb]})
        dropped = st.trim([b, a])
        assert [int(x) for x in dropped] == [ds[tb][0], ds[ta][0]]
        assert np.array_equal(st.partial(a), ds[ta][1]) and np.array_equal(st.partial(b), ds[tb][1])
        assert st.partial(a, frames=True)[1] == ta and st.partial(b, frames=True)[1] == tb
        at = {a: ta, b: tb}
        while min(at.values()) < s.T:
            push = {i: s.feats[t:t + 7] for i, t in at.items() if t < s.T}
            st.push(push)
            st.trim(list(push))
            at = {i: min(t + 7, s.T) if i in push else t for i, t in at.items()}
        assert np.array_equal(st.end(a), bwords)
        # the slot's next utterance starts with an empty archive and base 0
        c = st.begin()
        assert c % 2 == a % 2 and c != a
        assert int(st.trim([c])[0]) == 0
        partial, frames = st.partial(c, frames=True)
        assert frames == 0 and len(partial) == 0
        st.push({c: s.feats[:ta]})
        partial, frames = st.partial(c, frames=True)
        assert frames == ta
        assert int(st.trim([c, b])[0]) == ds[ta][0]
        assert np.array_equal(st.partial(c), ds[ta][1])
        for t in range(ta, s.T, 7):
            st.push({c: s.feats[t:t + 7]})
            st.trim([c])
        assert np.array_equal(st.end(c), bwords) and np.array_equal(st.end(b), bwords)


# ---- 5. audio ids and row ids ------------------------------------------------------------------------------------------------------------
def test_a_row_id_through_a_projection_trims(setup):
    """context 1: the search runs a row behind the rows received; M picks the centre row, so the rows searched are the rows pushed"""
    s = setup
    beam = 60.0
    bwords, _ = s.batch(beam)
    piece = 5
    _, W, _ = s.run(beam, piece)
    M = np.zeros((DIM, 3 * DIM + 1))
    M[:, DIM:2 * DIM] = np.eye(DIM)
    # the window is bounded by the rows received: a row more than the rows searched, and the trims fall a row earlier than in run()
    with s.stream(beam, W + piece + 1) as st:
        st.set_projection(DIM, 1, M)
        sid = st.begin()
        tr = ref.TrimSearch(s.net, beam, WP)
        dropped_any = 0
        for t in range(0, s.T, piece):
            last = t + piece >= s.T
            st.push_rows({sid: s.feats[t:t + piece]}, finish=last)
            for row in s.scores[tr.frames():(s.T if last else t + piece - 1)]:
                tr.push(row)
            d = tr.trim()
            assert int(st.trim([sid])[0]) == d, t
            dropped_any += d > 0
            partial, frames = st.partial(sid, frames=True)
            assert frames == tr.frames() and np.array_equal(partial, tr.partial()), t
        assert dropped_any >= 5 and tr.base > W + piece + 1
        assert np.array_equal(st.end(sid), bwords)


def test_an_audio_id_trims(tmp_path):
    """PCM in uneven pieces, a trim every few pushes, in a window below the utterance's frame count: the words of the batch decoder
    on sr_corpus_from_audio.  The window is measured, not assumed: an untrimmed id fed the same pieces says where the commit point is
    after every push (sr_stream_stable), and from that follows the largest count of frames the trimmed id holds at a push."""
    p = FR.params(preemphasis=0.9)
    post = dict(n_static=12, n_first=12, n_second=1, deriv_step=3, energy_max_norm=0)
    lex = ref.LEXICA["w6x3"]
    word_off, automaton, sil = lex.flatten()
    mp = str(tmp_path / "a.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 3, 25, seed=42))
    T = 250
    x = np.concatenate(FR.signals(p["sample_rate"]))[8000:8000 + p["window"] + (T - 1) * p["shift"] + 56].astype(np.int16)
    rng = np.random.default_rng(77)
    cuts = [0]
    while cuts[-1] < len(x):
        cuts.append(min(cuts[-1] + int(rng.integers(200, 1400)), len(x)))
    every = 3
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post) as fe:
        lexh = m.lexicon(word_off, automaton, lex.silence_idx, ref.TDP, sil)
        corpus = fe.from_audio(x, np.array([0, len(x)], np.uint64))
        assert int(corpus.frame_off[1]) == T
        bwords, _ = corpus.recognize(lexh, 500.0, WP, capi.GMM_DEFAULT)[:2]
        corpus.close()
        assert len(bwords) >= 8
        # the untrimmed id: the commit frame after every push, and its partial results
        with m.stream(lexh, 500.0, WP, capi.GMM_DEFAULT, max_streams=1, max_frames=T) as st:
            st.set_frontend(fe)
            sid = st.begin()
            commits, partials = [], []
            for i in range(len(cuts) - 1):
                st.push_audio({sid: x[cuts[i]:cuts[i + 1]]})
                commits.append(int(st.stable([sid])[1][0]))
                partials.append(st.partial(sid, frames=True))
            st.finish_audio([sid])
            assert np.array_equal(st.end(sid), bwords)
        base, need = 0, 0
        for i in range(len(cuts) - 1):
            need = max(need, fe.frames(cuts[i + 1]) - base)  # the frames the samples so far make, less the frames dropped
            if (i + 1) % every == 0:
                base = commits[i]
        assert need < T // 2 and base > T // 2, (need, base)  # a condition on the fixture
        with m.stream(lexh, 500.0, WP, capi.GMM_DEFAULT, max_streams=1, max_frames=need) as st:
            st.set_frontend(fe)
            sid = st.begin()
            total = 0
            for i in range(len(cuts) - 1):
                st.push_audio({sid: x[cuts[i]:cuts[i + 1]]})
                if (i + 1) % every == 0:
                    total += int(st.trim([sid])[0])
                    assert total == commits[i], i
                partial, frames = st.partial(sid, frames=True)
                assert frames == partials[i][1] and np.array_equal(partial, partials[i][0]), i
            st.finish_audio([sid])
            assert np.array_equal(st.end(sid), bwords)
        if need > 1:  # one frame less: the same pushes overflow
            with m.stream(lexh, 500.0, WP, capi.GMM_DEFAULT, max_streams=1, max_frames=need - 1) as st:
                st.set_frontend(fe)
                sid = st.begin()
                with pytest.raises(capi.SrError) as ei:
                    for i in range(len(cuts) - 1):
                        st.push_audio({sid: x[cuts[i]:cuts[i + 1]]})
                        if (i + 1) % every == 0:
                            st.trim([sid])
                assert _code(ei) == SR_ELIMIT
        lexh.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_outputs_untouched(setup):
    s = setup
    L = capi.lib()
    beam = 60.0
    with s.stream(beam, 64, max_streams=3) as st:
        a, b, gone = st.begin(), st.begin(), st.begin()
        st.push({a: s.feats[:60], b: s.feats[:50]})
        st.end(gone)
        before = (st.partial(a, frames=True), st.partial(b, frames=True))
        for ids in ([a, 9999], [a, gone], [a, b, a]):  # unknown, ended, repeated
            ids = np.asarray(ids, np.uint32)
            dropped = np.full(len(ids), 0xABCD, np.uint32)
            assert L.sr_stream_trim(st.h, len(ids), ids.ctypes.data, dropped.ctypes.data) == SR_EINVAL
            assert (dropped == 0xABCD).all()
        # ... and nothing was trimmed: the next trim drops what the reference drops from frame 0
        tr = ref.TrimSearch(s.net, beam, WP)
        for row in s.scores[:60]:
            tr.push(row)
        d = tr.trim()
        assert d > 0
        ids = np.asarray([a], np.uint32)
        assert L.sr_stream_trim(st.h, 1, ids.ctypes.data, None) == 0  # out_dropped may be NULL
        after = st.partial(a, frames=True)
        assert after[1] == before[0][1] == 60 and np.array_equal(after[0], before[0][0]) and np.array_equal(after[0], tr.partial())
        assert int(st.trim([a])[0]) == 0
        # the dropped traceback entries are gone: a trimmed id ends without them, and the refusal leaves it open
        with pytest.raises(capi.SrError) as ei:
            st.end(a, traceback=True)
        assert _code(ei) == SR_EINVAL
        st.push({a: s.feats[60:60 + d]})  # still open, and the window has room for the frames dropped
        assert st.partial(a, frames=True)[1] == 60 + d
        with pytest.raises(capi.SrError) as ei:
            st.push({a: s.feats[60 + d:60 + d + 5]})
        assert _code(ei) == SR_ELIMIT
        st.end(a)
        words, tb = st.end(b, traceback=True)  # never trimmed: its traceback is there
        assert len(tb[0]) == 51


# ---- 7. real speech ------------------------------------------------------------------------------------------------------------------
def test_real_speech_negative_costs_trimmed_equals_untrimmed(tmp_path):
    """the sequential boundary replay is live here (negative emission costs) and the numpy restatement does not cover it: a trimmed id
    is held against an untrimmed id fed the same pushes, at every push, and against the batch words at the end"""
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
            bwords = c.recognize(lexh, beam, wp, capi.GMM_DEFAULT)[0]
            c.close()
            with m.stream(lexh, beam, wp, capi.GMM_DEFAULT, max_streams=2, max_frames=len(feats)) as st:
                a, b = st.begin(), st.begin()
                total = 0
                for t in range(0, len(feats), 3):
                    st.push({a: feats[t:t + 3], b: feats[t:t + 3]})
                    words, commit, silence = st.stable([a, b])
                    assert np.array_equal(words[0], words[1]) and commit[0] == commit[1] and silence[0] == silence[1], (u, t)
                    d = int(st.trim([a])[0])
                    assert total + d == int(commit[1]), (u, t)  # the frames dropped so far are the untrimmed id's commit frame
                    total += d
                    pa, pb = st.partial(a, frames=True), st.partial(b, frames=True)
                    assert pa[1] == pb[1] and np.array_equal(pa[0], pb[0]), (u, t)
                assert np.array_equal(st.end(a), bwords) and np.array_equal(st.end(b), bwords)
                moved += total > 0
        assert moved  # the commit point does leave frame 0 on real speech
        lexh.close()


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_the_mirror_s_trim_agrees_with_the_c_calls(setup, tmp_path):
    s = setup  # (its model came from the built library: the driver links against that)
    src = os.path.join(ROOT, "tests", "cpp", "stream_trim_driver.cpp")
    hdrs = [os.path.join(ROOT, "include", "sr_sietill.hpp"), os.path.join(ROOT, "include", "srgpu.h")]
    if not os.path.exists(DRIVER) or os.path.getmtime(DRIVER) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER,
                               "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                               "-Wl,-rpath,$ORIGIN/../../speechrecognition_amd", "-Wl,-rpath,/opt/rocm/lib"])
    beam, piece = 60.0, 7
    per, W, base = s.run(beam, piece)
    blob = struct.pack("<I", s.lex.n_words)
    for n, r in zip(s.lex.word_states, s.lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<I5dI", s.lex.silence_idx, *ref.TDP, beam, WP, capi.GMM_DEFAULT)
    blob += struct.pack("<III", W, piece, s.T) + np.ascontiguousarray(s.feats, "<f4").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.check_output([DRIVER, "run", s.mp, str(DIM), str(case)], text=True).splitlines()
    assert not out[0].startswith("error"), out
    pushes = [[int(x) for x in l.split()[1:]] for l in out if l.startswith("push")]
    assert len(pushes) == len(per)
    for got, r in zip(pushes, per):
        assert got[0] == r["frames"] and got[1] == r["dropped"] and got[2:] == [int(w) for w in r["partial"]], got[:2]
    assert [int(x) for x in [l for l in out if l.startswith("final")][0].split()[1:]] == [int(w) for w in s.batch(beam)[0]]
    assert int([l for l in out if l.startswith("dropped")][0].split()[1]) == base
    assert out[-1] == "same", out[-1]
