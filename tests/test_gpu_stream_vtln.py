"""A VTLN warp per utterance of a stream set (sr_stream_set_warp, sr_bigram_stream_set_warp; stream_frontend_kernel): utterances fed as
PCM samples in pieces of every kind, several per push with different warps among them, at most five open at once.  No tolerance
anywhere: with energy_max_norm == 0 the rows of an id with warp w must carry the bits of sr_corpus_from_audio_warped on the whole
utterance under w (those of sr_corpus_from_audio without a warp), so the words and the traceback must be the batch's on that corpus;
behind a projection and a transform they must be the batch chain's; with the energy maximum on they must be the warped no-maximum
rows with the causal maximum of tests/stream_audio_reference.py applied.

The warps are alpha = 0.88, 1.0, 1.12 (break 0.875) on the parameter sets of tests/test_gpu_vtln.py, where every warp has a valid
filterbank.  Warp 1 is alpha == 1.0, whose filters are the unwarped ones (tests/test_gpu_vtln.py), so one sr_corpus_from_audio_warped
call with warp 1 in the place of "no warp" is the batch corpus of a mixed run; every case that relies on it asserts those rows
against sr_corpus_from_audio first.  Where a test must tell warp 1 from no warp (slot reuse) the middle alpha is 0.94."""
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import frontend_reference as R
from tests import stream_audio_reference as SR
from tests import vtln_reference as V
from tests.test_gpu_stream import _check_against_batch
from tests.test_gpu_stream_audio import MODES as AUDIO_MODES
from tests.test_gpu_stream_audio import assert_rows, net, stream_audio, utterances  # noqa: F401  (net: the fixture)
from tests.test_gpu_vtln import MFCC16, MFCC64, batch, placeholder, post_of, u32

pytestmark = pytest.mark.gpu

FRAMES = [0, 1, 2, 3, 4, 7, 17, 60]
MODES = AUDIO_MODES[:len(FRAMES)]          # one sample, whole, one shift, 37 samples, random sizes
OTHER_MODES = ["whole", "whole", "37", "shift", "random", "37", "shift", "random"]
VTLN3 = dict(alpha=[0.88, 1.0, 1.12], break_frac=V.BREAK)
VTLN3_APART = dict(alpha=[0.88, 0.94, 1.12], break_frac=V.BREAK)   # no warp is the unwarped bank
IDENTITY = 1
WARPS = [[None, 0, 1, 2][u % 4] for u in range(len(FRAMES))]
SR_EINVAL = -1


def utts_of(p):
    utts = utterances(p)[:len(FRAMES)]
    assert [R.n_frames(len(x), p) for x in utts] == FRAMES
    return utts


class PerUtteranceWarps:
    """a stream set whose begin() gives the next utterance its warp -- and its transform, if there are any -- (stream_audio begins the
    utterances in order), and which counts the pushes that carried two or more distinct warps"""

    def __init__(self, st, warps, Ws=None):
        self.st, self.warps, self.Ws, self.n, self.by_id, self.mixed = st, warps, Ws, 0, {}, 0

    def begin(self):
        sid = self.st.begin()
        w = self.warps[self.n % len(self.warps)]
        if w is not None:
            self.st.set_warp(sid, w)
        if self.Ws is not None:
            self.st.set_transform(sid, self.Ws[self.n % len(self.Ws)])
        self.by_id[sid] = w
        self.n += 1
        return sid

    def push_audio(self, samples, feats=False):
        if len({self.by_id[int(sid)] for sid in samples}) >= 2:
            self.mixed += 1
        return self.st.push_audio(samples, feats=feats)

    def __getattr__(self, name):
        return getattr(self.st, name)


def warped_batch(fe, utts, warps):
    """-> (the batch corpus of utterance u under warps[u], its rows, its frame offsets).  None goes in as the identity warp, after the
    assertion that the identity warp's rows are sr_corpus_from_audio's."""
    samples, soff = batch(utts)
    corpus = fe.from_audio_warped(samples, soff, np.array([IDENTITY if w is None else w for w in warps], np.uint32))
    rows, off = corpus.download(), corpus.frame_off.astype(np.int64)
    plain = fe.from_audio(samples, soff)
    plain_rows = plain.download()
    assert np.array_equal(plain.frame_off, corpus.frame_off)
    plain.close()
    for u, w in enumerate(warps):
        if w is None or w == IDENTITY:
            assert np.array_equal(u32(rows[off[u]:off[u + 1]]), u32(plain_rows[off[u]:off[u + 1]])), u
    return corpus, rows, off, plain_rows


def a_warp_does_something(rows, plain_rows, off, warps, which):
    """the guard against a vacuous pass: each warp of `which` changes the bits of at least one utterance that carries it"""
    for w in which:
        assert any(warps[u] == w and off[u + 1] > off[u] and not np.array_equal(u32(rows[off[u]:off[u + 1]]), u32(plain_rows[off[u]:off[u + 1]]))
                   for u in range(len(warps))), w


# ---- 1. rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [MFCC16, MFCC64], ids=["400-160", "64-32"])
def test_streamed_rows_are_the_warped_batch_front_end_s(net, p):
    dim = 2 * p["n_cepstra"] + 1
    mp, lexparts = net(dim)
    utts = utts_of(p)
    with capi.Model.from_mixset(mp, dim) as m, m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN3) as fe:
        assert fe.n_warps == 3
        lexh = m.lexicon(*lexparts)
        corpus, rows, off, plain_rows = warped_batch(fe, utts, WARPS)
        assert np.array_equal(np.diff(off), FRAMES)
        corpus.close()
        a_warp_does_something(rows, plain_rows, off, WARPS, (0, 2))
        end = lambda st, sid: st.end(sid)  # noqa: E731
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe)
            w = PerUtteranceWarps(st, WARPS)
            first, _, pushes = stream_audio(w, utts, MODES, p, 21, end)
            assert pushes > 100 and w.mixed >= 1, (pushes, w.mixed)        # ids with different warps shared pushes
            assert_rows(first, rows, off, utts)
            again, _, _ = stream_audio(PerUtteranceWarps(st, WARPS), utts, MODES, p, 21, end)
            for u in range(len(utts)):
                assert np.array_equal(u32(again[u]), u32(first[u])), u
            # another assignment of the cuts, and another interleaving: the same bits
            w = PerUtteranceWarps(st, WARPS)
            other, _, _ = stream_audio(w, utts, OTHER_MODES, p, 22, end, max_open=3)
            assert w.mixed >= 1
            assert_rows(other, rows, off, utts)
        lexh.close()


# ---- 2. words and traceback ------------------------------------------------------------------------------------------------------
def three_warps_in_one_push(st, x, finish):
    """recipe (b): the same samples to three ids, each under its own warp, every push carrying all three -> [finish(st, id)] by warp"""
    ids = [st.begin() for _ in range(3)]
    for w, sid in enumerate(ids):
        st.set_warp(sid, w)
    for at in range(0, len(x), 2500):
        st.push_audio({sid: x[at:at + 2500] for sid in ids})
    st.finish_audio(ids)
    return [finish(st, sid) for sid in ids]


def normalising_post(m, p, utts):
    """post-processing parameters whose mean and deviation are those of the utterances' own unwarped rows: the synthetic models' means
    are N(0, 1), and on raw cepstra (component 0 is in the tens) every search ends with no word end inside the beam -- the results
    would agree with the batch's as +inf agrees with +inf"""
    with m.frontend(p, post_of(p, energy_max_norm=0)) as raw:
        c = raw.from_audio(*batch(utts))
        rows = c.download().astype(np.float64)
        c.close()
    return post_of(p, energy_max_norm=0, mean=rows.mean(axis=0), stddev=rows.std(axis=0) + 1e-3)


def test_streamed_words_and_traceback_are_the_warped_batch_s(net):
    p = MFCC16
    mp, lexparts = net(25)
    utts = utts_of(p)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, normalising_post(m, p, utts), vtln=VTLN3) as fe:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off, _ = warped_batch(fe, utts, WARPS)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        c3, _, off3, _ = warped_batch(fe, [utts[7]] * 3, [0, 1, 2])
        words3, woff3, tb3 = c3.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe)
            w = PerUtteranceWarps(st, WARPS)
            got_rows, got, _ = stream_audio(w, utts, MODES, p, 31, lambda st, sid: st.end(sid, traceback=True))
            assert w.mixed >= 1
            assert_rows(got_rows, rows, off, utts)
            assert sorted(got) == list(range(len(utts)))
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
            three = three_warps_in_one_push(st, utts[7], lambda st, sid: st.end(sid, traceback=True))
            _check_against_batch(dict(enumerate(three)), words3, woff3, tb3, c3.frame_off)
            finals = [res[1][0][-1] for res in three]
            for wi in range(3):   # the score recipe (b) compares: each id's final tb_score is the batch's under that warp
                assert finals[wi].view(np.uint64) == tb3[0][int(off3[wi + 1]) + wi].view(np.uint64), wi
            print("final tb_score by warp:", [float(s) for s in finals])
            assert np.isfinite(finals).all() and len({float(s) for s in finals}) == 3   # ... and it tells the warps apart
            assert any(len(w_) for w_, _ in got.values())
        corpus.close()
        c3.close()
        lexh.close()


def test_streamed_bigram_items_are_the_warped_batch_s(tmp_path):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    p = MFCC16
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=25)
    utts = utts_of(p)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, normalising_post(m, p, utts), vtln=VTLN3) as fe:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        corpus, rows, off, _ = warped_batch(fe, utts, WARPS)
        gw, gs, gt, goff = corpus.recognize_bigram(bg, 60.0, 30.0, capi.GMM_PREFILTER)
        corpus.close()
        c3, _, _, _ = warped_batch(fe, [utts[7]] * 3, [0, 1, 2])
        w3, s3, t3, o3 = c3.recognize_bigram(bg, 60.0, 30.0, capi.GMM_PREFILTER)
        c3.close()
        with m.bigram_stream(bg, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES) + 1) as st:
            st.set_frontend(fe)
            w = PerUtteranceWarps(st, WARPS)
            got_rows, got, _ = stream_audio(w, utts, MODES, p, 41, lambda st, sid: st.end(sid))
            assert w.mixed >= 1
            three = three_warps_in_one_push(st, utts[7], lambda st, sid: st.end(sid))
        assert_rows(got_rows, rows, off, utts)
        for u in range(len(utts)):
            a, b = int(goff[u]), int(goff[u + 1])
            assert _same(got[u], (gw[a:b], gs[a:b], gt[a:b])), u
        for wi in range(3):
            a, b = int(o3[wi]), int(o3[wi + 1])
            assert b > a and _same(three[wi], (w3[a:b], s3[a:b], t3[a:b])), wi
        bg.close()


# ---- 3. slot reuse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zerogram", "bigram"])
def test_a_reused_slot_does_not_inherit_a_warp(net, tmp_path, kind):
    from tests.test_bigram import _setup
    p = MFCC16
    utts = utts_of(p)
    order = [(6, 2, False), (5, None, False), (7, 0, False), (6, 1, True)]     # (utterance, warp set, cleared again)
    if kind == "zerogram":
        mp, lexparts = net(25)
    else:
        lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=25)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN3_APART) as fe:
        samples, soff = batch([utts[u] for u, _, _ in order])
        plain = fe.from_audio(samples, soff)
        plain_rows, off = plain.download(), plain.frame_off.astype(np.int64)
        plain.close()
        per_warp = []
        for w in range(3):
            c = fe.from_audio_warped(samples, soff, np.full(len(order), w, np.uint32))
            per_warp.append(c.download())
            c.close()
            assert not np.array_equal(u32(per_warp[w]), u32(plain_rows))       # here every warp differs from no warp
        net_h = m.lexicon(*lexparts) if kind == "zerogram" else m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        open_ = (lambda: m.stream(net_h, 500.0, 10.0, capi.GMM_EXACT, max_streams=1, max_frames=60)) if kind == "zerogram" else \
            (lambda: m.bigram_stream(net_h, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=1, max_frames=61))
        with open_() as st:
            st.set_frontend(fe)
            for i, (u, w, cleared) in enumerate(order):
                sid = st.begin()
                assert sid == i                                                 # the one slot, a new id every time
                if w is not None:
                    st.set_warp(sid, w)
                if cleared:
                    st.set_warp(sid, capi.STREAM_NO_WARP)
                x = utts[u]
                got = [st.push_audio({sid: x[:1111]}, feats=True)[sid], st.push_audio({sid: x[1111:]}, feats=True)[sid],
                       st.finish_audio([sid], feats=True)[sid]]
                st.end(sid)
                want = plain_rows if (w is None or cleared) else per_warp[w]
                assert np.array_equal(u32(np.concatenate(got)), u32(want[off[i]:off[i + 1]])), (i, u, w, cleared)
        net_h.close()


# ---- 4. the pipeline -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zerogram", "bigram"])
def test_warped_audio_through_the_pipeline_is_the_batch_chain_s(net, tmp_path, kind):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    from tests.test_gpu_stream_pipeline import batch_route, make_case
    mfcc, c, dim = MFCC64, 2, 25
    D = 2 * mfcc["n_cepstra"] + 1
    utts = utts_of(mfcc)
    _, M, Ws = make_case(D, c, dim, 61, frames=FRAMES)
    if kind == "zerogram":
        mp, lexparts = net(dim)
    else:
        lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=dim)
    with placeholder(D) as src, capi.Model.from_mixset(mp, dim) as m, src.frontend(mfcc, post_of(mfcc, energy_max_norm=0), vtln=VTLN3) as fe:
        inp, in_rows, in_off, plain_in = warped_batch(fe, utts, WARPS)
        a_warp_does_something(in_rows, plain_in, in_off, WARPS, (0, 2))
        corpus, rows, off = batch_route(inp, m, c, M, Ws)       # from_audio_warped -> splice_transform -> transform
        inp.close()
        assert np.array_equal(np.diff(off), FRAMES)
        if kind == "zerogram":
            net_h = m.lexicon(*lexparts)
            words, woff, tb = corpus.recognize(net_h, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
            st = m.stream(net_h, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES))
            end = lambda st, sid: st.end(sid, traceback=True)  # noqa: E731
        else:
            net_h = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
            gw, gs, gt, goff = corpus.recognize_bigram(net_h, 60.0, 30.0, capi.GMM_PREFILTER)
            st = m.bigram_stream(net_h, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES) + 1)
            end = lambda st, sid: st.end(sid)  # noqa: E731
        with st:
            st.set_projection(D, c, M)
            st.set_frontend(fe)
            w = PerUtteranceWarps(st, WARPS, Ws)
            got_rows, got, _ = stream_audio(w, utts, MODES, mfcc, 51, end)
            assert w.mixed >= 1
        assert_rows(got_rows, rows, off, utts)
        assert sorted(got) == list(range(len(utts)))
        if kind == "zerogram":
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
        else:
            for u in range(len(utts)):
                a, b = int(goff[u]), int(goff[u + 1])
                assert _same(got[u], (gw[a:b], gs[a:b], gt[a:b])), u
        corpus.close()
        net_h.close()


# ---- 5. the energy maximum -------------------------------------------------------------------------------------------------------
def test_the_energy_maximum_is_the_causal_one_of_the_warped_rows(net):
    p = MFCC16
    mp, lexparts = net(25)
    utts = utts_of(p)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN3) as fe0, \
            m.frontend(p, post_of(p, energy_max_norm=1), vtln=VTLN3) as fe1:
        lexh = m.lexicon(*lexparts)
        c0, warped_rows, off, plain_rows = warped_batch(fe0, utts, WARPS)
        c0.close()
        a_warp_does_something(warped_rows, plain_rows, off, WARPS, (0, 2))
        want = np.concatenate([SR.causal_max(warped_rows[off[u]:off[u + 1]], 3) for u in range(len(utts))])
        assert not np.array_equal(u32(want), u32(warped_rows))                  # (the maximum does something)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_frontend(fe1)
            w = PerUtteranceWarps(st, WARPS)
            got, _, _ = stream_audio(w, utts, MODES, p, 51, lambda st, sid: st.end(sid))
            assert w.mixed >= 1
        assert_rows(got, want, off, utts)
        lexh.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zerogram", "bigram"])
def test_refusals_leave_the_set_and_the_warp_as_they_were(net, tmp_path, kind):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    p = MFCC16
    utt = utts_of(p)[6]                              # 17 frames
    L = capi.lib()
    fn = "sr_stream" if kind == "zerogram" else "sr_bigram_stream"
    if kind == "zerogram":
        mp, lexparts = net(25)
    else:
        lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=25)
    post = post_of(p, energy_max_norm=0)
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post) as plain_fe, m.frontend(p, post, vtln=VTLN3) as fe:
        corpus, rows, off, plain_rows = warped_batch(fe, [utt, utt], [2, None])
        assert not np.array_equal(u32(rows[:17]), u32(rows[17:]))
        if kind == "zerogram":
            net_h = m.lexicon(*lexparts)
            words, woff, tb = corpus.recognize(net_h, 500.0, 10.0, capi.GMM_EXACT, traceback=True)
            st = m.stream(net_h, 500.0, 10.0, capi.GMM_EXACT, max_streams=2, max_frames=17)

            def ends_as_the_batch(sid, u):
                _check_against_batch({u: st.end(sid, traceback=True)}, words, woff, tb, corpus.frame_off)
        else:
            net_h = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
            gw, gs, gt, goff = corpus.recognize_bigram(net_h, 60.0, 30.0, capi.GMM_PREFILTER)
            st = m.bigram_stream(net_h, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=2, max_frames=18)

            def ends_as_the_batch(sid, u):
                a, b = int(goff[u]), int(goff[u + 1])
                assert _same(st.end(sid), (gw[a:b], gs[a:b], gt[a:b])), u

        def set_warp(sid, warp):
            return getattr(L, fn + "_set_warp")(st.h, sid, warp)

        def refused(call):
            with pytest.raises(capi.SrError) as e:
                call()
            assert e.value.code == SR_EINVAL, e.value

        def audio(sid, cuts, want):
            """the utterance's samples in pieces, finished: its rows must be `want`"""
            got = [st.push_audio({sid: utt[a:b]}, feats=True)[sid] for a, b in zip(cuts[:-1], cuts[1:])]
            got.append(st.finish_audio([sid], feats=True)[sid])
            assert np.array_equal(u32(np.concatenate(got)), u32(want))

        with st:
            # no front end attached
            sid = st.begin()
            assert set_warp(sid, 0) == SR_EINVAL and b"no front end" in L.sr_last_error()
            assert set_warp(sid, capi.STREAM_NO_WARP) == SR_EINVAL
            st.push({sid: plain_rows[:17]})                                     # ... and the id goes on as a row id
            ends_as_the_batch(sid, 1)
            # a front end without warps
            st.set_frontend(plain_fe)
            sid = st.begin()
            assert set_warp(sid, 0) == SR_EINVAL and b"no warps" in L.sr_last_error()
            assert set_warp(sid, capi.STREAM_NO_WARP) == SR_EINVAL
            audio(sid, [0, 1000, len(utt)], plain_rows[:17])
            ends_as_the_batch(sid, 1)
            # a warped front end
            st.set_frontend(fe)
            a, b = st.begin(), st.begin()
            assert getattr(L, fn + "_set_frontend")(st.h, plain_fe.h) == SR_EINVAL   # ids are open: no warp can outlive its front end
            assert set_warp(a, 3) == SR_EINVAL and b"n_warps" in L.sr_last_error()   # warp == n_warps
            assert set_warp(a + 2, 0) == SR_EINVAL and set_warp(77, 0) == SR_EINVAL  # ids that are not open
            st.set_warp(a, 2)
            assert set_warp(a, 3) == SR_EINVAL and set_warp(a, 0xFFFFFFFE) == SR_EINVAL   # refused: warp 2 stays
            refused(lambda: st.push({a: rows[:2]}))                             # a warped id takes no feature rows ...
            refused(lambda: st.push_rows({a: rows[:2]}, finish=True))
            refused(lambda: st.push({b: rows[17:19], a: rows[:2]}))             # ... and a push that names one changes no other id
            st.set_warp(a, 0)                                                   # (still fresh: the refused pushes did not count as its first)
            st.set_warp(a, 2)
            st.set_warp(b, 1)
            st.set_warp(b, None)                                                # b: set and cleared, a row id after all
            first = st.push_audio({a: utt[:1000]}, feats=True)[a]               # 4 statics, 1 row
            assert len(first) == 1
            refused(lambda: st.set_warp(a, 0))                                  # after the first push
            refused(lambda: st.set_warp(a, None))
            refused(lambda: st.push({a: rows[:2]}))
            st.push({b: rows[17:20]})
            refused(lambda: st.set_warp(b, 1))                                  # ... of either kind
            rest = [st.push_audio({a: utt[1000:1500]}, feats=True)[a], st.push_audio({a: utt[1500:]}, feats=True)[a]]
            st.push({b: rows[20:]})
            rest.append(st.finish_audio([a], feats=True)[a])
            assert np.array_equal(u32(np.concatenate([first] + rest)), u32(rows[:17]))   # warp 2's rows through all of it
            refused(lambda: st.set_warp(a, 0))                                  # a finished id
            ends_as_the_batch(a, 0)
            ends_as_the_batch(b, 1)
            refused(lambda: st.set_warp(a, 0))                                  # an ended id
            # the slot that carried warp 2 takes rows again: the warp ended with its utterance
            c = st.begin()
            assert c % 2 == a % 2
            st.push({c: plain_rows[:17]})
            ends_as_the_batch(c, 1)
        corpus.close()
        net_h.close()


# ---- 7. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror_streams_under_a_warp_to_its_batch_call_s_words(net, tmp_path):
    """sr::StreamingRecognizer::set_warp (include/sr_sietill.hpp) through tests/cpp/stream_vtln_driver.cpp"""
    from tests.test_stream_vtln_cpu import compile_driver
    exe = str(tmp_path / "stream_vtln_driver")
    compile_driver(exe)
    p = MFCC16
    mp, (word_off, automaton, silence_idx, tdp, sil_state) = net(25)
    utt = utts_of(p)[7]
    beam, wp, piece, warp = 500.0, 10.0, 1111, 0
    blob = struct.pack("<5I3d2f", p["window"], p["shift"], p["n_fft"], p["n_mel"], p["n_cepstra"], p["sample_rate"], p["f_low"], p["f_high"],
                       p["preemphasis"], p["energy_floor"])
    blob += struct.pack("<I3dd", 3, *VTLN3["alpha"], VTLN3["break_frac"])
    blob += struct.pack("<I", len(word_off) - 1) + np.asarray(word_off, "<u4").tobytes() + np.asarray(automaton, "<u2").tobytes()
    blob += struct.pack("<I5d", silence_idx, *tdp, beam, wp) + struct.pack("<4I", capi.GMM_PREFILTER, piece, warp, len(utt))
    blob += np.ascontiguousarray(utt, "<i2").tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    out = subprocess.run([exe, mp, "25", str(case)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    line = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines()}
    assert line["words"] == line["batch"]
    with capi.Model.from_mixset(mp, 25) as m, m.frontend(p, post_of(p, energy_max_norm=0), vtln=VTLN3) as fe:
        lexh = m.lexicon(word_off, automaton, silence_idx, tdp, sil_state)
        corpus, _, _, _ = warped_batch(fe, [utt, utt], [warp, None])
        words, woff = corpus.recognize(lexh, beam, wp, capi.GMM_PREFILTER)
        corpus.close()
        assert line["words"] == list(words[int(woff[0]):int(woff[1])]) and line["plain"] == list(words[int(woff[1]):int(woff[2])])
        lexh.close()
