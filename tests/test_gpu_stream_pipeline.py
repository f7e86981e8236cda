"""The pipeline of a stream set (sr_stream_set_projection, sr_stream_set_transform, sr_stream_push_rows and the bigram twins;
stream_pipeline_kernel): utterances fed as rows or as audio in pieces of every kind, several per push, at most five open at once, each
with its own transform.  No tolerance anywhere: the rows searched must carry the bits of the batch route on the whole utterances --
sr_corpus_upload (or sr_corpus_from_audio), sr_corpus_splice_transform, sr_corpus_transform -- so the words and the traceback must be
the batch search's on that corpus."""
import os

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests.test_gpu_frontend import MFCC16, MFCC64, batch, placeholder, post_of, u32
from tests.test_gpu_stream import _check_against_batch
from tests.test_gpu_stream_audio import MODES as AUDIO_MODES
from tests.test_gpu_stream_audio import stream_audio, utterances

pytestmark = pytest.mark.gpu

TDP = (3.0, 0.0, 30.0)
FRAMES = [0, 1, 2, 3, 4, 7, 17, 60, 250]
MODES = ["one", "one", "whole", "one", "one", "one", "3", "one", "37"]         # by utterance
OTHER_MODES = ["whole", "whole", "one", "whole", "random", "random", "37", "random", "3"]
SR_EINVAL, SR_ELIMIT = -1, -4


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """a six-word lexicon and a 3-density mixset per dimension -> make(dim) = (mixset path, lexicon parts)"""
    tmp = tmp_path_factory.mktemp("streampipeline")
    lex = synth.make_lexicon(6, 3, 1)
    word_off, automaton, sil = lex.flatten()

    def make(dim):
        mp = os.path.join(str(tmp), f"e{dim}.mix")
        if not os.path.exists(mp):
            synth.write_mixset(mp, synth.make_mixset(lex.n_states, 3, dim, seed=41))
        return mp, (word_off, automaton, lex.silence_idx, TDP, sil)
    return make


def make_case(D, c, p, seed, frames=FRAMES, with_w=True):
    """-> (utterances float32[T, D], M, one W per utterance or None)"""
    rng = np.random.default_rng(seed)
    utts = [(rng.normal(size=(T, D)) * 3.0).astype(np.float32) for T in frames]
    E = (2 * c + 1) * D
    M = np.hstack([rng.normal(size=(p, E)) / np.sqrt(E), rng.normal(size=(p, 1))])
    Ws = [np.hstack([np.eye(p) + 0.1 * rng.normal(size=(p, p)), rng.normal(size=(p, 1))]) if with_w else None for _ in frames]
    return utts, M, Ws


def batch_route(src_corpus, target, c, M, Ws):
    """an input corpus (on its placeholder model) through splice_transform [and transform] -> (corpus on target, rows, off)"""
    proj = src_corpus if M is None else src_corpus.splice_transform(target, c, M)
    out = proj
    if Ws is not None and Ws[0] is not None:
        out = proj.transform(np.arange(len(Ws)), np.stack(Ws))
        if proj is not src_corpus:
            proj.close()
    return out, out.download(), out.frame_off.astype(np.int64)


def upload(model, utts):
    off = np.concatenate([[0], np.cumsum([len(x) for x in utts])]).astype(np.uint64)
    return model.upload(np.concatenate(utts), off)


def piece(mode, rng, left):
    k = {"whole": left, "one": 1, "3": 3, "37": 37, "random": int(rng.integers(0, 41))}[mode]
    return min(k, left)


def stream_rows(st, utts, modes, seed, finish, Ws=None, max_open=5):
    """Every utterance through `st` as rows: at most max_open open at once, each push carries a random subset of the open ones with a
    piece by the utterance's mode; the finish rides on an utterance's last rows or follows in a later push without rows; an
    utterance is ended a random number of pushes after it.  -> ({u: its rows, concatenated}, {u: finish(st, id)}, pushes)"""
    rng = np.random.default_rng(seed)
    todo, open_, done = list(range(len(utts))), {}, {}
    rows = {u: [] for u in todo}
    out, pushes = {}, 0
    while todo or open_ or done:
        while todo and len(open_) + len(done) < max_open:
            u = todo.pop(0)
            sid = st.begin()
            if Ws is not None and Ws[u] is not None:
                st.set_transform(sid, Ws[u])
            open_[u] = (sid, 0)
        push, last = {}, {}
        for u in list(open_):
            sid, at = open_[u]
            if rng.random() < 0.75 and at < len(utts[u]):
                k = piece(modes[u], rng, len(utts[u]) - at)
                push[sid] = (u, utts[u][at:at + k])
                open_[u] = (sid, at + k)
                if at + k == len(utts[u]) and rng.random() < 0.5:
                    last[sid] = u
            elif at == len(utts[u]) and rng.random() < 0.6:
                last[sid] = u
        if push or last:
            got = st.push_rows({sid: x for sid, (u, x) in push.items()}, finish=list(last), feats=True)
            pushes += 1
            for sid, u in list({s: u for s, (u, _) in push.items()}.items()) + [(s, u) for s, u in last.items() if s not in push]:
                rows[u].append(got[sid])
            for sid, u in last.items():
                del open_[u]
                done[u] = sid
        for u in list(done):
            if rng.random() < 0.5:
                out[u] = finish(st, done.pop(u))
    return {u: np.concatenate(r) for u, r in rows.items()}, out, pushes


def assert_rows(got, rows, off, n):
    for u in range(n):
        want = rows[off[u]:off[u + 1]]
        assert got[u].shape == want.shape, (u, got[u].shape, want.shape)
        assert np.array_equal(u32(got[u]), u32(want)), (u, int(np.argmax((u32(got[u]) != u32(want)).any(axis=1))))


# ---- 1. row pushes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_w", [False, True], ids=["projection", "projection+W"])
@pytest.mark.parametrize("D,c,p", [(3, 0, 2), (3, 1, 3), (25, 4, 17), (39, 6, 39)])
def test_streamed_rows_words_and_traceback_are_the_batch_route_s(net, D, c, p, with_w):
    mp, lexparts = net(p)
    utts, M, Ws = make_case(D, c, p, 7 + D, with_w=with_w)
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m:
        lexh = m.lexicon(*lexparts)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        assert np.array_equal(np.diff(off), FRAMES)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_projection(D, c, M)
            got_rows, got, pushes = stream_rows(st, utts, MODES, 21, lambda st, sid: st.end(sid, traceback=True), Ws)
            assert pushes > 50
            assert_rows(got_rows, rows, off, len(utts))
            assert sorted(got) == list(range(len(utts)))
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
            # another assignment of the cuts, and another interleaving: the same bits
            other, _, _ = stream_rows(st, utts, OTHER_MODES, 22, lambda st, sid: st.end(sid), Ws, max_open=3)
            assert_rows(other, rows, off, len(utts))
        corpus.close()
        inp.close()
        lexh.close()


def test_the_plain_push_feeds_the_pipeline_and_counts_the_rows_searched(net, tmp_path):
    """sr_stream_push / sr_bigram_stream_push under a projection with context > 0: the binding's count of rows searched (the length
    of end()'s traceback, the capacity of a later push_rows) follows the delay"""
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    D, c, p = 25, 4, 17
    mp, lexparts = net(p)
    utts, M, Ws = make_case(D, c, p, 33, frames=[60, 3])
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m:
        lexh = m.lexicon(*lexparts)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=2, max_frames=60) as st:
            st.set_projection(D, c, M)
            a, b = st.begin(), st.begin()
            st.set_transform(a, Ws[0])
            st.set_transform(b, Ws[1])
            st.push({a: utts[0][:7], b: utts[1]})                      # b: 3 rows, fewer than the context
            assert st.frames[a] == 3 and st.frames[b] == 0
            assert st.partial(a, frames=True)[1] == 3 and st.partial(b, frames=True)[1] == 0
            got = [st.push_rows({a: utts[0][7:20]}, feats=True)[a]]     # the capacity follows from the count: 13 rows
            assert len(got[0]) == 13
            st.push({a: utts[0][20:]})
            assert st.frames[a] == 56
            tail = st.push_rows({}, finish=[a, b], feats=True)
            assert np.array_equal(u32(tail[a]), u32(rows[56:60])) and np.array_equal(u32(got[0]), u32(rows[3:16]))
            assert np.array_equal(u32(tail[b]), u32(rows[60:63]))
            res = {0: st.end(a, traceback=True), 1: st.end(b, traceback=True)}
            assert len(res[0][1][0]) == 61 and len(res[1][1][0]) == 4
            _check_against_batch(res, words, woff, tb, corpus.frame_off)
        corpus.close()
        inp.close()
        lexh.close()
    # the bigram twin
    lex, spec, bmp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 52, 9, 2, D=p)
    with placeholder(D) as src, capi.Model.from_mixset(bmp, p) as m:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        gw, gs, gt, goff = corpus.recognize_bigram(bg, 60.0, 30.0, capi.GMM_PREFILTER)
        with m.bigram_stream(bg, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=1, max_frames=61) as st:
            st.set_projection(D, c, M)
            a = st.begin()
            st.set_transform(a, Ws[0])
            st.push({a: utts[0][:30]})
            st.push({a: utts[0][30:]})
            assert st.frames[a] == 56 and st.partial(a, frames=True)[1] == 56
            assert np.array_equal(u32(st.push_rows({}, finish=[a], feats=True)[a]), u32(rows[56:60]))
            assert _same(st.end(a), (gw[:int(goff[1])], gs[:int(goff[1])], gt[:int(goff[1])]))
        corpus.close()
        inp.close()
        bg.close()


def test_the_largest_transform_beside_the_widest_projection(net):
    """p = 63 with E = 507: W (32.3 KB), the group's projected rows and the history beside the static tiles, the kernel's largest LDS need"""
    D, c, p = 39, 6, 63
    mp, lexparts = net(p)
    frames = [1, 7, 80]
    utts, M, Ws = make_case(D, c, p, 35, frames=frames)
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m:
        lexh = m.lexicon(*lexparts)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=3, max_frames=80) as st:
            st.set_projection(D, c, M)
            got_rows, got, _ = stream_rows(st, utts, ["one", "3", "37"], 24, lambda st, sid: st.end(sid, traceback=True), Ws)
            assert_rows(got_rows, rows, off, len(utts))
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
        corpus.close()
        inp.close()
        lexh.close()


# ---- 2. a transform alone --------------------------------------------------------------------------------------------------------
def test_a_transform_alone_has_no_delay(net):
    p = 17
    mp, lexparts = net(p)
    utts, _, Ws = make_case(p, 0, p, 31)
    Ws[5] = None                                  # one utterance without a transform among the others: its rows pass unchanged
    ident = np.hstack([np.eye(p), np.zeros((p, 1))])
    with capi.Model.from_mixset(mp, p) as m:
        lexh = m.lexicon(*lexparts)
        inp = upload(m, utts)
        corpus, rows, off = batch_route(inp, m, 0, None, [ident if w is None else w for w in Ws])
        assert np.array_equal(u32(rows[off[5]:off[6]]), u32(utts[5]))
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES)) as st:
            got_rows, got, _ = stream_rows(st, utts, MODES, 23, lambda st, sid: st.end(sid, traceback=True), Ws)
            assert_rows(got_rows, rows, off, len(utts))
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
            # every push gives its own rows back at once, sr_stream_push feeds the same pipeline, and end needs no finish
            a, b = st.begin(), st.begin()
            st.set_transform(a, Ws[7])
            st.set_transform(b, Ws[6])
            st.set_transform(b, None)             # cleared again
            r = st.push_rows({a: utts[7][:10], b: utts[6][:4]}, feats=True)
            assert np.array_equal(u32(r[a]), u32(rows[off[7]:off[7] + 10])) and np.array_equal(u32(r[b]), u32(utts[6][:4]))
            assert st.partial(a, frames=True)[1] == 10
            st.push({a: utts[7][10:], b: utts[6][4:]})
            wa, wb = st.end(a, traceback=True), st.end(b)
            _check_against_batch({7: wa}, words, woff, tb, corpus.frame_off)
            plain = upload(m, [utts[6]])
            assert np.array_equal(wb, plain.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER)[0])
            plain.close()
        corpus.close()
        inp.close()
        lexh.close()


# ---- 3. audio --------------------------------------------------------------------------------------------------------------------
class PerUtteranceTransforms:
    """a stream set whose begin() gives the next utterance its transform (stream_audio begins the utterances in order)"""

    def __init__(self, st, Ws):
        self.st, self.Ws, self.n = st, Ws, 0

    def begin(self):
        sid = self.st.begin()
        self.st.set_transform(sid, self.Ws[self.n % len(self.Ws)])
        self.n += 1
        return sid

    def __getattr__(self, name):
        return getattr(self.st, name)


def audio_batch(fe, utts, target, c, M, Ws):
    samples, soff = batch(utts)
    inp = fe.from_audio(samples, soff)
    corpus, rows, off = batch_route(inp, target, c, M, Ws)
    inp.close()
    return corpus, rows, off


@pytest.mark.parametrize("mfcc,c,p", [(MFCC16, 4, 17), (MFCC64, 2, 7)], ids=["400-160", "64-32"])
def test_audio_through_the_pipeline_is_the_batch_route_s(net, mfcc, c, p):
    D = 2 * mfcc["n_cepstra"] + 1
    mp, lexparts = net(p)
    utts = utterances(mfcc)
    _, M, Ws = make_case(D, c, p, 41)
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m, src.frontend(mfcc, post_of(mfcc, energy_max_norm=0)) as fe:
        lexh = m.lexicon(*lexparts)
        corpus, rows, off = audio_batch(fe, utts, m, c, M, Ws)
        assert np.array_equal(np.diff(off), FRAMES)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_projection(D, c, M)
            st.set_frontend(fe)
            seen = []

            def after_push(u, sid, n_samples):
                if u >= 6 and len(seen) < 5:
                    seen.append(st.partial(sid, frames=True)[1] == max(fe.frames(n_samples) - 3 - c, 0))

            got_rows, got, pushes = stream_audio(PerUtteranceTransforms(st, Ws), utts, AUDIO_MODES, mfcc, 51,
                                                 lambda st, sid: st.end(sid, traceback=True), after_push=after_push)
            assert pushes > 100 and seen and all(seen)             # the delay is deriv_step + context frames
            assert_rows(got_rows, rows, off, len(utts))
            _check_against_batch(got, words, woff, tb, corpus.frame_off)
        corpus.close()
        lexh.close()


# ---- 4. the bigram twin ----------------------------------------------------------------------------------------------------------
def test_the_bigram_stream_set_carries_the_same_pipeline(tmp_path):
    from tests.test_bigram import _setup
    from tests.test_gpu_bigram_stream import _same
    mfcc, c, p = MFCC64, 2, 25
    D = 2 * mfcc["n_cepstra"] + 1
    lex, spec, mp, word_off, mixtures, lm, tdp, _ = _setup(tmp_path, 51, 9, 2, D=p)
    utts, M, Ws = make_case(D, c, p, 61)
    audio = utterances(mfcc)
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m, src.frontend(mfcc, post_of(mfcc, energy_max_norm=0)) as fe:
        bg = m.bigram(word_off, mixtures, lex.silence_idx, lm, tdp)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        acorpus, arows, aoff = audio_batch(fe, audio, m, c, M, Ws)
        want = [c_.recognize_bigram(bg, 60.0, 30.0, capi.GMM_PREFILTER) for c_ in (corpus, acorpus)]
        with m.bigram_stream(bg, 60.0, 30.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES) + 1) as st:
            st.set_projection(D, c, M)
            got_rows, got, _ = stream_rows(st, utts, MODES, 71, lambda st, sid: st.end(sid), Ws)
            st.set_frontend(fe)
            agot_rows, agot, _ = stream_audio(PerUtteranceTransforms(st, Ws), audio, AUDIO_MODES, mfcc, 72, lambda st, sid: st.end(sid))
        assert_rows(got_rows, rows, off, len(utts))
        assert_rows(agot_rows, arows, aoff, len(audio))
        for g, (gw, gs, gt, goff) in ((got, want[0]), (agot, want[1])):
            for u in range(len(FRAMES)):
                a, b = int(goff[u]), int(goff[u + 1])
                assert _same(g[u], (gw[a:b], gs[a:b], gt[a:b])), u
        corpus.close()
        acorpus.close()
        inp.close()
        bg.close()


# ---- 5. independence and reuse ---------------------------------------------------------------------------------------------------
def test_an_utterance_s_bits_do_not_depend_on_its_company_or_its_slot_s_past(net):
    D, c, p = 25, 4, 17
    mp, lexparts = net(p)
    utts, M, Ws = make_case(D, c, p, 81)
    with placeholder(D) as src, capi.Model.from_mixset(mp, p) as m:
        lexh = m.lexicon(*lexparts)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        bare, bare_rows, _ = batch_route(inp, m, c, M, None)       # the projection alone
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=5, max_frames=max(FRAMES)) as st:
            st.set_projection(D, c, M)
            first, w1, _ = stream_rows(st, utts, MODES, 91, lambda st, sid: st.end(sid, traceback=True), Ws)
            again, w2, _ = stream_rows(st, utts, MODES, 91, lambda st, sid: st.end(sid, traceback=True), Ws)
            for u in range(len(utts)):                            # two identical runs: identical bits
                assert np.array_equal(u32(first[u]), u32(again[u])), u
                assert np.array_equal(w1[u][0], w2[u][0]) and np.array_equal(w1[u][1][0].view(np.uint64), w2[u][1][0].view(np.uint64)), u
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=1, max_frames=max(FRAMES)) as st:
            st.set_projection(D, c, M)
            for u in (7, 6):                                      # alone in a set of one slot: the bits it had among others
                alone, _, _ = stream_rows(st, [utts[u]], ["random"], 92, lambda st, sid: st.end(sid), [Ws[u]])
                assert np.array_equal(u32(alone[0]), u32(first[u])), u
            # the slot again, after an utterance with another transform and another history: nothing of either shows
            sid = st.begin()
            r = [st.push_rows({sid: utts[5][:3]}, feats=True)[sid], st.push_rows({sid: utts[5][3:]}, finish=True, feats=True)[sid]]
            assert len(r[0]) == 0 and np.array_equal(u32(np.concatenate(r)), u32(bare_rows[off[5]:off[6]]))
            st.end(sid)
            sid = st.begin()                                      # ... and a one-row utterance splices 2c + 1 copies of its row
            r = st.push_rows({sid: utts[1]}, finish=True, feats=True)[sid]
            assert np.array_equal(u32(r), u32(bare_rows[off[1]:off[2]]))
            st.end(sid)
        corpus.close()
        bare.close()
        inp.close()
        lexh.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_as_it_was(net):
    D, c, p = 25, 2, 17
    mp, lexparts = net(p)
    utts, M, Ws = make_case(D, c, p, 95, frames=[17])
    x, W = utts[0], Ws[0]
    L = capi.lib()
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    with placeholder(D) as src, placeholder(13) as src13, capi.Model.from_mixset(mp, p) as m, \
            src.frontend(MFCC16, post_of(MFCC16, energy_max_norm=0)) as fe, src13.frontend(MFCC64, post_of(MFCC64, energy_max_norm=0)) as fe13:
        lexh = m.lexicon(*lexparts)
        inp = upload(src, utts)
        corpus, rows, off = batch_route(inp, m, c, M, Ws)
        words, woff, tb = corpus.recognize(lexh, 500.0, 10.0, capi.GMM_PREFILTER, traceback=True)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_PREFILTER, max_streams=2, max_frames=17) as st:
            def raw_push(ids, feats, foff, finish=0, out=None, cap=0, ooff=None):
                ids = np.asarray(ids, np.uint32)
                return L.sr_stream_push_rows(st.h, len(ids), P(ids), P(feats), P(foff), finish, P(out), cap, P(ooff))

            def refused(code, call):
                with pytest.raises(capi.SrError) as e:
                    call()
                assert e.value.code == code, e.value

            big = np.zeros((p, 514))
            assert L.sr_stream_set_projection(st.h, 27, 9, P(big)) == SR_ELIMIT               # E = 513
            assert L.sr_stream_set_projection(st.h, 0, 0, P(big)) == SR_EINVAL                # in_dim == 0
            assert L.sr_stream_set_frontend(st.h, fe.h) == SR_EINVAL                          # no projection: another model's front end
            st.set_projection(D, c, M)
            assert L.sr_stream_set_frontend(st.h, fe13.h) == SR_EINVAL                        # a front end of the wrong dimension
            st.set_frontend(fe)
            assert L.sr_stream_set_projection(st.h, 13, 1, P(np.zeros((p, 40)))) == SR_EINVAL  # ... and the projection against the front end
            assert L.sr_stream_set_projection(st.h, 0, 0, None) == SR_EINVAL                  # detaching under a foreign front end
            a = st.begin()
            assert L.sr_stream_set_projection(st.h, D, c, P(M)) == SR_EINVAL                  # an id is open
            assert L.sr_stream_set_projection(st.h, 0, 0, None) == SR_EINVAL
            st.set_transform(a, W)
            parts = [st.push_rows({a: x[:5]}, feats=True)[a]]
            assert len(parts[0]) == 3 and st.partial(a, frames=True)[1] == 3
            # every refusal below is followed by the same valid pushes; the rows must still be the batch's
            refused(SR_EINVAL, lambda: st.set_transform(a, Ws[0] * 2.0))                      # after the first push
            refused(SR_EINVAL, lambda: st.set_transform(a, None))
            refused(SR_EINVAL, lambda: st.end(a))                                             # rows pending: the id stays open
            four = np.array([0, 4], np.uint64)
            ooff = np.full(2, 99, np.uint64)
            out = np.full((3, p), 7.5, np.float32)
            assert raw_push([a], x[5:9], four, 0, out, 3, ooff) == SR_EINVAL                  # 4 rows, room for 3
            assert ooff[1] == 4 and b"4 rows" in L.sr_last_error() and (out == 7.5).all()
            assert raw_push([a], np.zeros((13, D), np.float32), np.array([0, 13], np.uint64)) == SR_ELIMIT   # 5 + 13 rows received
            assert raw_push([a, a], x[5:9], np.array([0, 2, 4], np.uint64)) == SR_EINVAL      # an id twice
            assert raw_push([a], None, four) == SR_EINVAL                                     # rows without feats
            refused(SR_EINVAL, lambda: st.push_audio({a: np.zeros(500, np.int16)}))           # audio on a row id
            parts.append(st.push_rows({a: x[5:9]}, feats=True)[a])
            assert st.partial(a, frames=True)[1] == 7
            parts.append(st.push_rows({a: x[9:]}, finish=True, feats=True)[a])
            assert np.array_equal(u32(np.concatenate(parts)), u32(rows))
            refused(SR_EINVAL, lambda: st.push_rows({a: x[:1]}))                              # rows for a finished id
            refused(SR_EINVAL, lambda: st.push_rows({}, finish=[a]))
            refused(SR_EINVAL, lambda: st.push({a: x[:1]}))
            _check_against_batch({0: st.end(a, traceback=True)}, words, woff, tb, corpus.frame_off)
            refused(SR_EINVAL, lambda: st.push_rows({a: x[:1]}))                              # an ended id
            # the same utterance again, the refusals of a fresh id in between
            b = st.begin()
            st.set_transform(b, W)
            assert raw_push([b], x, np.array([0, 17], np.uint64), 1, out, 3, ooff) == SR_EINVAL and ooff[1] == 17
            got = st.push_rows({b: x}, finish=True, feats=True)[b]
            assert np.array_equal(u32(got), u32(rows))
            _check_against_batch({0: st.end(b, traceback=True)}, words, woff, tb, corpus.frame_off)
            refused(SR_EINVAL, lambda: st.set_transform(b + 2, W))                            # an id that is not open
        corpus.close()
        inp.close()
        lexh.close()


def test_a_transform_needs_a_dimension_the_lds_holds(net):
    mp, lexparts = net(64)
    with capi.Model.from_mixset(mp, 64) as m:
        lexh = m.lexicon(*lexparts)
        with m.stream(lexh, 500.0, 10.0, capi.GMM_EXACT, max_streams=1, max_frames=4) as st:
            for projected in (False, True):
                if projected:
                    st.set_projection(3, 1, make_case(3, 1, 64, 3)[1])
                sid = st.begin()
                with pytest.raises(capi.SrError) as e:
                    st.set_transform(sid, np.hstack([np.eye(64), np.zeros((64, 1))]))
                assert e.value.code == SR_ELIMIT
                st.end(sid)
        lexh.close()
