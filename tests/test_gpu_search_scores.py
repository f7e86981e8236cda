"""The zerogram search kernels alone (viterbi_words.hip, viterbi_fast.hip, the two replay kernels of viterbi_decode.hip) on score tables
the test supplies through sr_recognize_corpus_scores, against the oracle on the same table (tests/search_cases.py; the conditions that
keep a case from passing vacuously are checked in test_search_cases_cpu.py).  Integers and bits throughout: the words, word_off, tb_word,
tb_bkp are equal, tb_score is equal as uint64 (positions where both sides hold a NaN count as equal).

Before a case runs, sr_lexicon_describe must report the route the case was written for ("words NW x NT plain L [general]", "slots",
"big"): which instantiation of the word-per-lane kernel, which launch shape of the replay ran is a checked fact.  Flags: no kFlagCorrupt;
kFlagReplay for no utterance whose rows hold no negative and no NaN value; in the hand-off cases (exact_negative 0, negative or NaN
entries) some utterance is flagged and some is not, and the flagged ones equal the oracle like the others."""
import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import search_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(oracle_lib):
    """model and lexicon handles by name, made on first use and shared by the cases of this module"""
    models, lexica = {}, {}

    def get(name):
        if name not in lexica:
            spec = sc.LEXICA[name]
            if spec.model_states not in models:
                models[spec.model_states] = capi.Model.from_mixset(sc.model_file(spec.model_states), sc.MODEL_DIM, device=0)
            m = models[spec.model_states]
            word_off, automaton, sil_state = sc.lexicon(name).flatten()
            lexica[name] = (m, m.lexicon(word_off, automaton, sc.lexicon(name).silence_idx, sc.TDP, sil_state))
        return lexica[name]

    yield get
    for _, lexh in lexica.values():
        lexh.close()
    for m in models.values():
        m.close()


def _check_route(name, lexh):
    spec, text = sc.LEXICA[name], lexh.describe()
    if spec.describe.endswith("("):  # "slots (" / "big (": the position count follows
        assert text.startswith(spec.describe), f"{name}: {text!r}, wanted {spec.describe!r}..."
    elif spec.describe == "words ":  # short-word lexica of the slot-kernel rows: the word-per-lane kernel by default
        assert text.startswith("words ") and "replay" not in text, f"{name}: {text!r}"
    else:
        assert text == spec.describe, f"{name}: {text!r}, wanted {spec.describe!r}"


RUNS = [(c, r) for c in sc.CASES for r in c.runs]


def _run_id(p):
    if isinstance(p, sc.Case):
        return p.id
    en, general, slots = p
    return f"neg{en}" + ("-general" if general else "-slots" if slots else "")


def _run_and_compare(m, lexh, case, run):
    """runs the case on the device and holds everything it returns against the oracle -> (flags, replayed, clean)"""
    exact_negative, general, slots = run
    table, off = sc.batch(case)
    ref = sc.reference(case)
    U = len(off) - 1
    corpus = m.upload(np.zeros((int(off[-1]), sc.MODEL_DIM), np.float32), off)
    try:
        words, woff, (tbs, tbw, tbb), flags = corpus.recognize_scores(lexh, table, case.am_threshold, sc.PENALTY, exact_negative,
                                                                     general_kernel=general, slot_kernel=slots)
    finally:
        corpus.close()
    assert not np.any(flags & sc.FLAG_CORRUPT), f"kFlagCorrupt: {flags}"
    clean = sc.clean_utterances(table, off)
    replayed = (flags & sc.FLAG_REPLAY) != 0
    assert not np.any(replayed & clean), f"kFlagReplay on utterances without a negative or NaN entry: flags {flags}, clean {clean}"
    assert len(woff) == U + 1 and int(woff[0]) == 0
    for u in range(U):
        want_words, (ws, ww, wb) = ref[u]
        tag = f"utterance {u} ({int(off[u + 1]) - int(off[u])} frames, flags {int(flags[u])})"
        assert np.array_equal(words[int(woff[u]):int(woff[u + 1])], want_words), f"{tag}: words"
        lo, hi = int(off[u]) + u, int(off[u + 1]) + u + 1
        assert np.array_equal(tbw[lo:hi], ww), f"{tag}: tb_word"
        assert np.array_equal(tbb[lo:hi], wb), f"{tag}: tb_bkp"
        got = np.ascontiguousarray(tbs[lo:hi])
        same = (got.view(np.uint64) == ws.view(np.uint64)) | (np.isnan(got) & np.isnan(ws))
        assert np.all(same), f"{tag}: tb_score differs at entries {np.flatnonzero(~same)[:8]}"
    return flags, replayed, clean


@pytest.mark.parametrize("case,run", RUNS, ids=_run_id)
def test_search_equals_oracle(handles, case, run):
    exact_negative, general, slots = run
    m, lexh = handles(case.lex)
    _check_route(case.lex, lexh)
    flags, replayed, _ = _run_and_compare(m, lexh, case, run)
    if case.handoff and exact_negative == 0 and not general and not lexh.describe().startswith("big"):
        assert np.any(replayed) and not np.all(replayed), f"hand-off: flags {flags}"
    if general:  # the replay kernel alone flags nothing for itself
        assert not np.any(replayed)
    if exact_negative == 1 and not general and not slots and lexh.describe().startswith("words"):
        # the word-per-lane kernel's NEG variant replays the early-out in place and hands nothing on; where its arrays do not fit the
        # LDS the fast variant ran instead, and it has flagged what it met
        if sc.LEXICA[case.lex].neg_fits:
            assert not np.any(replayed), f"the NEG variant did not run: flags {flags}"
        elif case.kind in ("negative", "nan"):
            assert np.any(replayed), f"the fast variant did not run: flags {flags}"


def test_chunked_pass_equals_oracle(monkeypatch, oracle_lib):
    """The hook runs the production chunk loop: with 1 MiB of score workspace a chunk of the 10 104-state model holds 12 frames, so
    every long utterance is a chunk of its own and the two short ones at the end share one -- five copies into alternating tables,
    each search at its chunk's frame base.  Same answers."""
    case = next(c for c in sc.CASES if c.lex == "w1edge" and c.kind == "negative")
    spec = sc.LEXICA[case.lex]
    monkeypatch.setenv("SRGPU_SCORE_CHUNK_MB", "1")
    with capi.Model.from_mixset(sc.model_file(spec.model_states), sc.MODEL_DIM, device=0) as m:
        word_off, automaton, sil_state = sc.lexicon(case.lex).flatten()
        lexh = m.lexicon(word_off, automaton, sc.lexicon(case.lex).silence_idx, sc.TDP, sil_state)
        try:
            _check_route(case.lex, lexh)
            for run in (sc.WORDS_FIRST, sc.SLOTS, sc.REPLAY):
                _, replayed, _ = _run_and_compare(m, lexh, case, run)
                assert np.any(replayed) != run[1]
        finally:
            lexh.close()


def test_argument_checks(handles):
    m, lexh = handles("w1l3")
    case = next(c for c in sc.CASES if c.lex == "w1l3" and c.kind == "dyadic")
    table, off = sc.batch(case)
    corpus = m.upload(np.zeros((int(off[-1]), sc.MODEL_DIM), np.float32), off)
    try:
        with pytest.raises(capi.SrError):  # the element count
            corpus.recognize_scores(lexh, table[:-1], 4.0, 1.0, 0)
        with pytest.raises(capi.SrError):  # exact_negative is 0 or 1
            corpus.recognize_scores(lexh, table, 4.0, 1.0, 2)
    finally:
        corpus.close()
