"""The bigram search kernels alone (viterbi_bigram.hip: the register layout, the dense LDS layout, the global-states layout) on score
tables the test supplies through sr_recognize_bigram_corpus_scores, against the oracle on the same table (tests/bigram_cases.py; the
conditions that keep a case from passing vacuously are checked in test_bigram_cases_cpu.py).  Integers and bits throughout: words, times
and offsets are equal, scores are equal as uint32, per utterance; a zero-frame utterance gives nothing.

Before a case runs, sr_bigram_route must report the kernel the case was written for ("registers 3 rows4 0b100", "lds 2 x 12", "global 8
entries global"): which instantiation ran is a checked fact, and every instantiation the launcher has is named by some case.

Budget, measured once on an MI355X: the module's 384 tests (371 device runs of 143 cases) take about 23 s, the oracle's answers
included; about half of that is the oracle on the seven cases of 4 200 to 8 192 words (3 s for the slowest, W = 8 192 at 6 to 8 frames);
every other case takes less than 0.3 s."""
import ctypes as C

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import bigram_cases as bc

pytestmark = pytest.mark.gpu

SR_EINVAL, SR_ELIMIT = -1, -4


class Handles:
    """models by state count and bigram nets by (lexicon, LM), made on first use and shared by the cases of this module"""

    def __init__(self):
        self.models, self.nets = {}, {}

    def model(self, n_states):
        if n_states not in self.models:
            self.models[n_states] = capi.Model.from_mixset(bc.model_file(n_states), bc.MODEL_DIM, device=0)
        return self.models[n_states]

    def net(self, name, lm_kind, beam=0.0):
        key = (name, lm_kind, beam if lm_kind == "wide" else 0.0)
        if key not in self.nets:
            spec = bc.LEXICA[name]
            word_off, mixtures, _ = bc.lexicon(name)
            self.nets[key] = self.model(spec.model_states).bigram(word_off, mixtures, spec.sil_idx, bc.lm_table(lm_kind, name, key[2]), spec.tdp)
        return self.model(bc.LEXICA[name].model_states), self.nets[key]

    def close(self):
        for bg in self.nets.values():
            bg.close()
        for m in self.models.values():
            m.close()


@pytest.fixture(scope="module")
def handles(oracle_lib):
    h = Handles()
    yield h
    h.close()


def _flag_args(flags):
    return dict(dense_states=flags == "dense", global_states=flags == "global")


def _compare(res, ref, off, tag):
    gw, gs, gt, goff = res
    U = len(off) - 1
    assert len(goff) == U + 1 and int(goff[0]) == 0
    for u in range(U):
        w, s, t = ref[u][:3]
        a, b = int(goff[u]), int(goff[u + 1])
        where = f"{tag}: utterance {u} ({int(off[u + 1]) - int(off[u])} frames)"
        assert b - a == len(w), f"{where}: {b - a} items, the oracle has {len(w)}"
        assert np.array_equal(gw[a:b], w), f"{where}: words"
        assert np.array_equal(gt[a:b], t), f"{where}: times"
        assert np.array_equal(gs[a:b].view(np.uint32), s.view(np.uint32)), f"{where}: score bits"
        if int(off[u + 1]) == int(off[u]):
            assert a == b, f"{where}: items for no frame"


def _run(handles, case, flags, **kw):
    m, bg = handles.net(case.lex, case.lm, case.ac)
    want = bc.LEXICA[case.lex].route_for(flags)
    got = bg.route(**_flag_args(flags))
    assert got == want, f"{case.lex} [{flags}]: route {got!r}, the case was written for {want!r}"
    table, off = bc.batch(case)
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    try:
        return corpus.recognize_bigram_scores(bg, table, case.ac, case.lmb, **_flag_args(flags), **kw)
    finally:
        corpus.close()


RUNS = [(c, f) for c in bc.CASES for f in c.flags]


@pytest.mark.parametrize("case,flags", RUNS, ids=lambda p: p.id if isinstance(p, bc.Case) else (p or "default"))
def test_bigram_search_equals_oracle(handles, case, flags):
    _, off = bc.batch(case)
    _compare(_run(handles, case, flags), bc.reference(case), off, f"{case.id} [{flags}]")


def test_every_route_is_named_by_a_case():
    assert {r for c, f in RUNS for r in [bc.LEXICA[c.lex].route_for(f)]} == set(bc.ROUTES)


@pytest.mark.parametrize("case,flags", [(c, f) for c in bc.CASES if "book" in c.conditions for f in c.flags],
                         ids=lambda p: p.id if isinstance(p, bc.Case) else (p or "default"))
def test_book_holds_k_and_not_k_minus_one(handles, case, flags):
    """The book of an utterance holds 2 + min(max_word_ends, W) T entries and the search writes 2 + stats[0]: the smallest
    max_word_ends that fits must pass (for r40one it fits exactly), one less is SR_ELIMIT, and the handle survives the error."""
    k, T = bc.book_k(case)
    _, off = bc.batch(case)
    ref = bc.reference(case)
    _compare(_run(handles, case, flags, max_word_ends=k), ref, off, f"{case.id} [{flags}] max_word_ends {k}")
    with pytest.raises(capi.SrError) as ei:
        _run(handles, case, flags, max_word_ends=k - 1)
    assert ei.value.code == SR_ELIMIT
    _compare(_run(handles, case, flags, max_word_ends=k), ref, off, f"{case.id} [{flags}] after the error")


def test_two_chunk_pass_equals_oracle(monkeypatch, oracle_lib):
    """The hook runs the production chunk loop: with 1 MiB of score workspace a chunk of the 11 136-state model holds 11 frames, so
    every long utterance is a chunk of its own: copies into alternating tables, each search at its chunk's frame base.  Same answers."""
    case = bc.case("r2100rowfit-dyadic-dyadic")
    monkeypatch.setenv("SRGPU_SCORE_CHUNK_MB", "1")
    h = Handles()
    try:
        _, off = bc.batch(case)
        for flags in case.flags:
            _compare(_run(h, case, flags), bc.reference(case), off, f"{case.id} [{flags}] in chunks")
    finally:
        h.close()


def test_persistent_grid_leaves_its_images_clean(handles, oracle_lib):
    """Global states at W = 60: 640 utterances of 0 .. 8 frames, more than the persistent grid has workgroups, so a workgroup decodes
    several in its one state image; every third utterance's rows are all +inf or all NaN (nothing survives its first frame) and its
    neighbours are ordinary: each workgroup must leave the image at +inf for its next utterance.  All held against the oracle."""
    name = "g60"
    spec = bc.LEXICA[name]
    rng = np.random.default_rng(77)
    N = 640
    lens = [int(t) for t in rng.integers(0, 9, size=N)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    table = (rng.integers(0, 24, size=(int(off[-1]), spec.model_states)) * 0.25).astype(np.float64)
    for u in range(0, N, 3):
        table[int(off[u]):int(off[u + 1])] = np.inf if u % 2 else np.nan
    lm = bc.lm_table("dyadic", name)
    m, bg = handles.net(name, "dyadic")
    assert bg.route(global_states=True) == spec.route_global
    want = [bc.decode(name, lm, table[int(off[u]):int(off[u + 1])], 12.0, 6.0) for u in range(N)]
    assert sum(len(w[0]) > 0 for w in want) > N // 3 and all(len(want[u][0]) == 0 for u in range(0, N, 3))
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    try:
        _compare(corpus.recognize_bigram_scores(bg, table, 12.0, 6.0, global_states=True), want, off, "persistent grid")
        _compare(corpus.recognize_bigram_scores(bg, table, 12.0, 6.0), want, off, "the same batch on the LDS layout")
    finally:
        corpus.close()


def test_argument_checks(handles):
    case = bc.case("r40m1-dyadic-dyadic")
    m, bg = handles.net(case.lex, case.lm)
    table, off = bc.batch(case)
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    try:
        with pytest.raises(capi.SrError) as ei:  # the element count
            corpus.recognize_bigram_scores(bg, table[:-1], case.ac, case.lmb)
        assert ei.value.code == SR_EINVAL
        with pytest.raises(capi.SrError) as ei:  # both layout flags
            corpus.recognize_bigram_scores(bg, table, case.ac, case.lmb, dense_states=True, global_states=True)
        assert ei.value.code == SR_EINVAL
        L = capi.lib()
        n = int(off[-1]) + len(off)
        ow, osc, ot, oo = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(len(off), np.uint64)
        t = np.ascontiguousarray(table)
        p = capi.BigramParams(case.ac, case.lmb, capi.GMM_DEFAULT, 0, 0)
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        call = lambda scores=t, p_=C.byref(p), outs=(ow, osc, ot, oo), net=bg.h: L.sr_recognize_bigram_corpus_scores(  # noqa: E731
            m.h, corpus.h, net, p_, P(scores), t.size, *[P(a) for a in outs])
        assert call() == 0
        assert call(scores=None) == SR_EINVAL and call(p_=None) == SR_EINVAL and call(net=None) == SR_EINVAL
        for i in range(4):
            assert call(outs=tuple(None if j == i else a for j, a in enumerate((ow, osc, ot, oo)))) == SR_EINVAL
        assert call() == 0
        _compare((ow[: int(oo[-1])], osc[: int(oo[-1])], ot[: int(oo[-1])], oo), bc.reference(case), off, "after the refusals")
        buf = C.create_string_buffer(64)
        assert L.sr_bigram_route(bg.h, 3, buf, len(buf)) == SR_EINVAL and L.sr_bigram_route(bg.h, 4, buf, len(buf)) == SR_EINVAL
        assert L.sr_bigram_route(None, 0, buf, len(buf)) == SR_EINVAL and L.sr_bigram_route(bg.h, 0, None, 0) == SR_EINVAL
        assert bg.describe() == "registers" and bg.route() == "registers 1 rows4 0b1"
    finally:
        corpus.close()
