"""sr_bigram_stream_stable (bigram_stream_commit_kernel): the stable prefix of a bigram stream's items after every push, on lexica
of tests/bigram_cases.py whose batch route is the register layout, the dense LDS image and the global layout (the stream itself
always keeps its states in device memory), and on one whose entries live in device memory too (GSM 2).

Safety: the items stable() returned after t frames are a prefix -- word, score bits and time -- of partial() at t and at every
later frame whose count is not 0, and of the final result; the commit time is the last stable item's (0: none) and never
decreases; asking changes nothing (the final items equal sr_recognize_bigram_corpus'); a reused slot starts from the start entry
and then answers what a fresh stream set answers.

Exactness: neither CPU restatement the bigram stream tests use (oracle/sr_oracle.c::orc_bigram_decode,
tests/test_bigram.py::linear_search_py) exposes its hypotheses and word ends without being changed, so
tests/bigram_commit_reference.py carries linear_search_py's statements as a class that does.  It must first reproduce the library's
final items bit for bit; then commit time and stable items must equal what tests/commit_reference.py gives on its alive set after
every push.  This is the check that catches reading the image's other (stale) buffer, which is safe but late.  The fixtures were
chosen on the CPU so that the commit entry has left the start entry at a quarter of the frames at least: asserted."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import bigram_cases as bc
from tests import bigram_commit_reference as bcr

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
D = 12
# (lexicon of bigram_cases, its batch route, acoustic beam, LM beam, sampled words)
CASES = [
    ("r40m1", "registers", 40.0, 6.0, 4),
    ("r40m1", "registers", FLT_MAX, FLT_MAX, 4),
    ("l1p4097", "lds", 60.0, 8.0, 3),
    ("glong", "global", 60.0, 8.0, 2),
    ("g4723", "global", 40.0, 6.0, 6),   # entries in device memory (GSM 2)
]


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            and np.array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32)))


def _is_prefix(a, b):
    n = len(a[0])
    return n <= len(b[0]) and _same(a, tuple(x[:n] for x in b))


def _setup(tmp_path, name):
    spec = bc.LEXICA[name]
    word_off, mixtures, _ = bc.lexicon(name)
    ms = synth.make_mixset(spec.model_states, 2, D, seed=8100 + spec.seed)
    mp = str(tmp_path / (name + ".mix"))
    synth.write_mixset(mp, ms)
    lex = synth.ExplicitLexicon(np.array(word_off), np.array(mixtures), spec.sil_idx)
    return spec, ms, mp, lex, np.array(bc.lm_table("dyadic", name))


def _stream(st, feats, piece):
    """-> [(t, partial items, stable items, commit time)] after every push, and the final items"""
    sid = st.begin()
    items, commit = st.stable([sid])
    assert len(items[0][0]) == 0 and commit[0] == 0  # nothing pushed: the start entry
    rec = []
    for t in range(0, len(feats), piece):
        st.push({sid: feats[t:t + piece]})
        items, commit = st.stable([sid])
        rec.append((min(t + piece, len(feats)), st.partial(sid), items[0], int(commit[0])))
    return rec, st.end(sid)


def _check_safety(rec, final):
    for i, (t, _, stable, commit) in enumerate(rec):
        assert commit <= t
        assert commit == (int(stable[2][-1]) if len(stable[2]) else 0)  # the book time of the commit entry
        if i:
            assert commit >= rec[i - 1][3], (t, commit, rec[i - 1][3])
            assert _is_prefix(rec[i - 1][2], stable), t
        for t2, partial2, _, _ in rec[i:]:
            if len(partial2[0]):
                assert _is_prefix(stable, partial2), (t, t2, stable, partial2)
        if len(final[0]):
            assert _is_prefix(stable, final), t


@pytest.mark.parametrize("name,route,acp,lmp,n_words", CASES)
def test_stable_items_are_safe_and_monotone(tmp_path, name, route, acp, lmp, n_words):
    spec, ms, mp, lex, lm = _setup(tmp_path, name)
    rng = np.random.default_rng(8200 + spec.seed)
    words = rng.choice([w for w in range(spec.W) if w != spec.sil_idx], size=n_words)
    feats = synth.sample_utterance(ms, lex, words, seed=8300 + spec.seed, frames_per_state=(1, 2))[:120]
    assert len(feats) >= 12
    with capi.Model.from_mixset(mp, D) as m:
        bg = m.bigram(lex.word_off, lex.automaton, spec.sil_idx, lm, spec.tdp)
        assert bg.describe() == route
        c = m.upload(feats, np.array([0, len(feats)], np.uint64))
        gw, gs, gt, goff = c.recognize_bigram(bg, acp, lmp, capi.GMM_DEFAULT)
        c.close()
        batch = (gw[: int(goff[1])], gs[: int(goff[1])], gt[: int(goff[1])])
        by_piece = {}
        for piece in (1, 3) if spec.W < 1000 else (1,):
            with m.bigram_stream(bg, acp, lmp, capi.GMM_DEFAULT, max_streams=1, max_frames=len(feats)) as st:
                rec, final = _stream(st, feats, piece)
            assert _same(final, batch)  # asking changed nothing
            _check_safety(rec, final)
            by_piece[piece] = {t: (stable, commit) for t, _, stable, commit in rec}
        if 3 in by_piece:  # the commit entry does not depend on how old the previous call's is
            for t, (stable, commit) in by_piece[3].items():
                assert commit == by_piece[1][t][1] and _same(stable, by_piece[1][t][0]), t
        if acp < FLT_MAX and spec.W < 1000:
            # under a beam the first words of a sampled utterance are settled long before its end: the answer is not "nothing, ever"
            assert max(commit for _, commit in by_piece[1].values()) > 0
        bg.close()


@pytest.mark.parametrize("name,acp,lmp,n_words,frames", [("r40m1", 40.0, 6.0, 8, 60), ("l1p4097", 60.0, 8.0, 3, 45)])
def test_commit_entry_equals_the_reference_at_every_push(tmp_path, name, acp, lmp, n_words, frames):
    spec, ms, mp, lex, lm = _setup(tmp_path, name)
    rng = np.random.default_rng(8500 + spec.seed)
    words = rng.choice([w for w in range(spec.W) if w != spec.sil_idx], size=n_words)
    feats = synth.sample_utterance(ms, lex, words, seed=8600 + spec.seed, frames_per_state=(1, 2))[:frames]
    with capi.Model.from_mixset(mp, D) as m:
        bg = m.bigram(lex.word_off, lex.automaton, spec.sil_idx, lm, spec.tdp)
        dense = m.score_frames(feats, capi.GMM_DEFAULT)
        ref = bcr.Search(lex.word_off, lex.automaton, spec.sil_idx, lm, spec.tdp, acp, lmp)
        want, floor = {}, 1
        for t, row in enumerate(dense, 1):
            ref.push(row)
            floor, ctime, items = ref.commit(floor)
            want[t] = (ctime, items)
        assert sum(want[t][0] > 0 for t in want) * 4 >= len(want)
        for piece in (1, 3):
            with m.bigram_stream(bg, acp, lmp, capi.GMM_DEFAULT, max_streams=1, max_frames=len(feats)) as st:
                rec, final = _stream(st, feats, piece)
            assert _same(final, ref.result())  # the reference follows the library's search, or its alive sets mean nothing
            _check_safety(rec, final)
            for t, _, stable, commit in rec:
                assert commit == want[t][0], (piece, t, commit, want[t][0])
                assert _same(stable, want[t][1]), (piece, t)
        bg.close()


def test_two_streams_in_one_call_slot_reuse_and_errors(tmp_path):
    name, acp, lmp = "r40m1", 40.0, 6.0
    spec, ms, mp, lex, lm = _setup(tmp_path, name)
    rng = np.random.default_rng(8400)
    utts = [synth.sample_utterance(ms, lex, rng.choice(np.arange(1, spec.W), size=8), seed=8401 + i, frames_per_state=(1, 2)) for i in range(2)]
    L = capi.lib()
    with capi.Model.from_mixset(mp, D) as m:
        bg = m.bigram(lex.word_off, lex.automaton, spec.sil_idx, lm, spec.tdp)
        alone = []
        for f in utts:  # each utterance alone in a fresh stream set, frame by frame
            with m.bigram_stream(bg, acp, lmp, capi.GMM_DEFAULT, max_streams=1, max_frames=len(f)) as st:
                rec, _ = _stream(st, f, 1)
            alone.append({t: (stable, commit) for t, _, stable, commit in rec})
        with m.bigram_stream(bg, acp, lmp, capi.GMM_DEFAULT, max_streams=2, max_frames=max(len(f) for f in utts)) as st:
            a, b = st.begin(), st.begin()
            ta, tb = len(utts[0]), len(utts[1]) // 2
            st.push({a: utts[0], b: utts[1][:tb]})
            items, commit = st.stable([b, a])
            assert _same(items[0], alone[1][tb][0]) and _same(items[1], alone[0][ta][0])
            assert [int(x) for x in commit] == [alone[1][tb][1], alone[0][ta][1]]
            assert alone[0][ta][1] > 0
            # errors: unknown and repeated ids, too small a capacity -- nothing but the offsets is written
            n0, n1 = len(items[0][0]), len(items[1][0])
            for ids, cap, want_off in (([a, 777], 64, None), ([a, a], 64, None), ([b, a], n0 + n1 - 1, [0, n0, n0 + n1])):
                ids = np.asarray(ids, np.uint32)
                ow, osc, ot = np.full(64, 0xABCD, np.uint32), np.full(64, 7.0, np.float32), np.full(64, 0xABCD, np.uint32)
                off, cm = np.full(3, 0xABCD, np.uint64), np.full(2, 0xABCD, np.uint32)
                rc = L.sr_bigram_stream_stable(st.h, 2, ids.ctypes.data, ow.ctypes.data, osc.ctypes.data, ot.ctypes.data, cap, off.ctypes.data, cm.ctypes.data)
                assert rc == -1
                assert (ow == 0xABCD).all() and (osc == 7.0).all() and (ot == 0xABCD).all() and (cm == 0xABCD).all()
                assert [int(x) for x in off] == (want_off or [0xABCD] * 3)
            st.end(a)
            # the slot's next utterance starts from the start entry, then answers what a fresh stream set answers
            c = st.begin()
            assert c % 2 == a % 2 and c != a
            items, commit = st.stable([c])
            assert len(items[0][0]) == 0 and commit[0] == 0
            for t in range(1, len(utts[1]) + 1):
                st.push({c: utts[1][t - 1:t]})
                items, commit = st.stable([c])
                assert int(commit[0]) == alone[1][t][1] and _same(items[0], alone[1][t][0]), t
            st.end(b), st.end(c)
        bg.close()
