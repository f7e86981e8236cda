"""Which check answers when an input to a streaming call breaks two: the order of the refusals of sr_stream_* and sr_bigram_stream_*,
their texts, and that a refused call changes nothing.

The table below is read off the entry points' source, check by check in the order they stand there; no figure in it is measured.  The
setting is the smallest there is: dimension 4, 6 single-density states in 3 words of 2, two slots, a window of 4 frames.  Two ids are
open, a with 3 frames (by the CPU oracle enough for a word in either search) and b with 2; after every refused call the partial results
and frame counts of both are what they were, and at the end both still take the frames that fill their windows and end with a result.
Raw calls through capi.lib(): the binding's own checks must not answer first."""
import ctypes as C

import numpy as np
import pytest

from speechrecognition_amd import capi, synth

pytestmark = pytest.mark.gpu

OK, EINVAL, ELIMIT = 0, -1, -4
DIM, MAX_STREAMS, MAX_FRAMES = 4, 2, 4
GONE = 9999      # never an id of a set of two slots that has begun two utterances
MARK = 0xABCD    # what the output arrays hold before a call


class Setting:
    def __init__(self, tmp):
        self.lex = synth.LexiconSpec(np.full(3, 2, np.uint16), np.ones(3, np.uint16), 0)
        spec = synth.make_mixset(self.lex.n_states, 1, DIM, seed=71)
        mp = str(tmp / "refusals.mix")
        synth.write_mixset(mp, spec)
        # a frame per state along sil w1 sil w2 sil: silence's two frames, then word 1's
        self.feats = synth.sample_utterance(spec, self.lex, [1, 2], seed=72, frames_per_state=(1, 1)).astype(np.float32)[:MAX_FRAMES]
        assert self.feats.shape == (MAX_FRAMES, DIM)
        self.model = capi.Model.from_mixset(mp, DIM)
        word_off, automaton, sil_state = self.lex.flatten()
        self.lexh = self.model.lexicon(word_off, automaton, self.lex.silence_idx, (3.0, 0.0, 30.0), sil_state)
        lm = (-np.log(np.random.default_rng(73).dirichlet(np.ones(3), size=3))).T.astype(np.float32).copy()
        tdp = np.array([[3.0, 0.0, 30.0, 5.0], [1.0, 0.0, 40.0, 2.0]], np.float32)
        self.bigram = self.model.bigram(word_off, automaton, 0, lm, tdp)

    def open(self, kind):
        if kind == "sr_stream":
            return self.model.stream(self.lexh, 200.0, 1.0, capi.GMM_DEFAULT, max_streams=MAX_STREAMS, max_frames=MAX_FRAMES)
        return self.model.bigram_stream(self.bigram, None, None, capi.GMM_DEFAULT, max_streams=MAX_STREAMS, max_frames=MAX_FRAMES)

    def close(self):
        self.bigram.close()
        self.lexh.close()
        self.model.close()


@pytest.fixture(scope="module")
def setting(tmp_path_factory):
    s = Setting(tmp_path_factory.mktemp("refusals"))
    yield s
    s.close()


def u32(*v):
    return np.asarray(v, np.uint32)


def u64(*v):
    return np.asarray(v, np.uint64)


def marked(n, dtype=np.uint32):
    return np.full(n, MARK, dtype)


def p(a):
    return None if a is None else a.ctypes.data


def pu32(a):
    """for the parameters the binding declares as uint32_t* (the others are void*)"""
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def snapshot(st, i):
    got, frames = st.partial(i, frames=True)
    parts = got if isinstance(got, tuple) else (got,)
    return frames, tuple(x.tobytes() for x in parts)


def refusals(L, fn, st, a, b, x):
    """(name, call -> status, status wanted, a piece of the message that only this check words, -> the outputs are as they must be)"""
    h = st.h
    push, rows, audio, stable = (getattr(L, fn + s) for s in ("_push", "_push_rows", "_push_audio", "_stable"))
    zerogram = fn == "sr_stream"
    T = []

    def case(name, call, status, piece, outputs=lambda: True):
        T.append((name, call, status, piece, outputs))

    def stable_call(n, ids, cap, off, commit, arrays=True, hole=None):
        """the set's stable call with output arrays of `cap` entries (hole: the index of one passed as NULL)"""
        outs = [np.zeros(max(cap, 1), t) for t in ((np.uint32,) if zerogram else (np.uint32, np.float32, np.uint32))]
        ptrs = [p(o) if arrays and k != hole else None for k, o in enumerate(outs)]
        tail = (p(off), p(commit), None) if zerogram else (p(off), p(commit))
        return lambda: stable(h, n, p(ids), *ptrs, cap, *tail)

    # ---- n == 0: nothing is looked at, the first offset is written
    case("push, n == 0", lambda: push(h, 0, None, None, None), OK, None)
    off0 = marked(1, np.uint64)
    case("push_rows, n == 0", lambda: rows(h, 0, None, None, None, 0, None, 0, p(off0)), OK, None, lambda: off0[0] == 0)
    off1 = marked(1, np.uint64)
    case("stable, n == 0", stable_call(0, None, 0, off1, None, arrays=False), OK, None, lambda: off1[0] == 0)
    # ---- the audio push asks for the front end before it looks at n
    off2 = marked(1, np.uint64)
    case("push_audio without a front end, n == 0", lambda: audio(h, 0, None, None, None, None, 0, p(off2)), EINVAL, "has no front end",
         lambda: off2[0] == MARK)
    # ---- row pushes: the arguments, then entry by entry the id, then its offsets, then its window; the capacity after all entries
    ids = u32(GONE)
    case("null frame_off before any id", lambda: rows(h, 1, p(ids), p(x), None, 0, None, 0, None), EINVAL, "null argument")
    bad0 = u64(1, 2)
    case("frame_off[0] != 0 before any id", lambda: rows(h, 1, p(ids), p(x), p(bad0), 0, None, 0, None), EINVAL, "frame_off[0] must be 0")
    twice, first, both, down = u32(a, a), u32(a, GONE), u32(a, b), u64(0, 1, 0)
    case("an id named twice before that entry's offsets", lambda: push(h, 2, p(twice), p(x), p(down)), EINVAL,
         f"push entry 1: stream id {a} appears twice in one push")
    case("an unopened id before that entry's offsets", lambda: push(h, 2, p(first), p(x), p(down)), EINVAL,
         f"push entry 1: stream id {GONE} is not open")
    case("descending offsets of an open id", lambda: push(h, 2, p(both), p(x), p(down)), EINVAL, "frame_off is not ascending at entry 1")
    wide = u64(0, 2, 3)
    case("entry 0's window before entry 1's id", lambda: push(h, 2, p(first), p(x), p(wide)), ELIMIT, f"stream id {a}: 3 + 2 frames exceed max_frames 4")
    only_b, three = u32(b), u64(0, 3)
    out0, off3 = np.zeros((1, DIM), np.float32), marked(2, np.uint64)
    case("over the window and over out_feats: the window", lambda: rows(h, 1, p(only_b), p(x), p(three), 0, p(out0), 0, p(off3)), ELIMIT,
         f"stream id {b}: 2 + 3 frames exceed max_frames 4", lambda: (off3 == MARK).all())
    only_a, one = u32(a), u64(0, 1)
    off4 = marked(2, np.uint64)
    case("over out_feats and null feats: out_feats", lambda: rows(h, 1, p(only_a), None, p(one), 0, p(out0), 0, p(off4)), EINVAL,
         "this push readies 1 rows, out_feats holds 0", lambda: off4[0] == MARK and off4[1] == 1)
    off5 = marked(2, np.uint64)
    case("null feats alone", lambda: rows(h, 1, p(only_a), None, p(one), 0, p(out0), 1, p(off5)), EINVAL, "null feats", lambda: (off5 == MARK).all())
    # ---- stable: the arguments before any id, then entry by entry
    off6, commit = marked(3, np.uint64), marked(2)
    gone = u32(GONE)
    case("an unopened id beside a null output array", stable_call(1, gone, 4, off6, commit, hole=0), EINVAL, "null argument",
         lambda: (off6 == MARK).all() and (commit == MARK).all())
    if not zerogram:
        case("an unopened id beside a null score array", stable_call(1, gone, 4, off6, commit, hole=1), EINVAL, "null argument")
    case("an unopened id beside a null out_commit", stable_call(1, gone, 4, off6, None), EINVAL, "null argument")
    case("an unopened id, no capacity and no arrays", stable_call(1, gone, 0, off6, commit, arrays=False), EINVAL,
         f"entry 0: stream id {GONE} is not open", lambda: (off6 == MARK).all() and (commit == MARK).all())
    case("stable, an id named twice", stable_call(2, twice, 8, off6, commit), EINVAL, f"entry 1: stream id {a} appears twice in one call",
         lambda: (off6 == MARK).all() and (commit == MARK).all())
    case("stable, named twice before the unopened id", stable_call(3, u32(b, b, GONE), 8, marked(4, np.uint64), marked(3)), EINVAL,
         f"entry 1: stream id {b} appears twice in one call")
    # ---- trim (the zerogram set alone has one)
    if zerogram:
        trim = L.sr_stream_trim
        dropped = marked(2)
        case("trim, n == 0", lambda: trim(h, 0, None, p(dropped)), OK, None, lambda: (dropped == MARK).all())
        case("trim, null ids", lambda: trim(h, 1, None, p(dropped)), EINVAL, "null argument", lambda: (dropped == MARK).all())
        case("trim, [a, a]", lambda: trim(h, 2, p(twice), p(dropped)), EINVAL, f"entry 1: stream id {a} appears twice in one call",
             lambda: (dropped == MARK).all())
        case("trim, an unopened id after an open one", lambda: trim(h, 2, p(first), p(dropped)), EINVAL, f"entry 1: stream id {GONE} is not open",
             lambda: (dropped == MARK).all())
    # ---- one id at a time
    count = marked(1)
    if zerogram:
        case("end of an unopened id", lambda: L.sr_stream_end(h, GONE, None, 0, pu32(count), None, None, None), EINVAL, f"stream id {GONE} is not open")
        case("partial without count", lambda: L.sr_stream_partial(h, a, None, 0, None, None), EINVAL, "null argument")
    else:
        case("end of an unopened id", lambda: L.sr_bigram_stream_end(h, GONE, None, None, None, 0, pu32(count)), EINVAL, f"stream id {GONE} is not open")
        case("partial without count", lambda: L.sr_bigram_stream_partial(h, a, None, None, None, 0, None, None), EINVAL, "null argument")
    new_id = marked(1)
    case("begin with every slot open", lambda: getattr(L, fn + "_begin")(h, pu32(new_id)), ELIMIT, "all 2 streams are open", lambda: new_id[0] == MARK)
    case("a transform after the first push", lambda: getattr(L, fn + "_set_transform")(h, a, None), EINVAL, "has been pushed to")
    case("a warp for an unopened id", lambda: getattr(L, fn + "_set_warp")(h, GONE, 0), EINVAL, f"stream id {GONE} is not open")
    case("a front end while ids are open", lambda: getattr(L, fn + "_set_frontend")(h, None), EINVAL, "the front end changes only while none is")
    return T


@pytest.mark.parametrize("fn", ["sr_stream", "sr_bigram_stream"])
def test_the_first_failing_check_answers_and_a_refusal_changes_nothing(setting, fn):
    L = capi.lib()
    x = setting.feats
    with setting.open(fn) as st:
        a, b = st.begin(), st.begin()
        assert (a, b) == (0, 1)
        st.push({a: x[:3], b: x[:2]})
        before = (snapshot(st, a), snapshot(st, b))
        assert before[0][0] == 3 and before[1][0] == 2
        table = refusals(L, fn, st, a, b, x)
        assert len(table) >= 25
        for name, call, status, piece, outputs in table:
            rc = call()
            text = L.sr_last_error().decode(errors="replace")
            assert rc == status, (name, rc, text)
            assert piece is None or piece in text, (name, text)
            assert outputs(), name
            assert (snapshot(st, a), snapshot(st, b)) == before, name
        # a buffer too small in _end leaves the id open (its count says what it takes), and the other id is as it was
        size = {i: len(snap[1][0]) // 4 for i, snap in zip((a, b), before)}
        assert max(size.values()) >= 1  # a condition on the fixture: an id has a result to be too long for no buffer
        for i in (i for i in (a, b) if size[i]):
            count = marked(1)
            if fn == "sr_stream":
                rc = L.sr_stream_end(st.h, i, None, 0, pu32(count), None, None, None)
            else:
                rc = L.sr_bigram_stream_end(st.h, i, None, None, None, 0, pu32(count))
            text = L.sr_last_error().decode(errors="replace")
            assert rc == EINVAL and f"stream {i}: {size[i]} " in text and "hold" in text and count[0] == size[i], (rc, text)
            assert (snapshot(st, a), snapshot(st, b)) == before
        # both ids are still served: each takes the frames that fill its window, a no further one, both end with a result
        st.push({a: x[3:4], b: x[2:4]})
        assert snapshot(st, a)[0] == 4 and snapshot(st, b)[0] == 4
        ids, off = u32(a), u64(0, 1)
        assert getattr(L, fn + "_push")(st.h, 1, p(ids), p(x), p(off)) == ELIMIT
        assert f"stream id {a}: 4 + 1 frames exceed max_frames 4" in L.sr_last_error().decode(errors="replace")
        st.end(a)
        st.end(b)
        c = st.begin()  # slot 0 again, its next generation
        assert c == MAX_STREAMS
        st.end(c)
