"""The cases of tests/bigram_cases.py without a GPU: every lexicon has the shape it was written for and gets, by the restated route
rules, the kernel its route texts name; every case's conditions hold, so that none passes vacuously; every instantiation the launcher has is
reached by a dyadic and by a real case whose answer is more than silence; and on a few small cases the oracle agrees with the
independent Python transcription of tests/test_bigram.py."""
import numpy as np
import pytest

from tests import bigram_cases as bc
from tests.test_bigram import linear_search_py


def test_lexica_have_the_shapes_they_were_written_for():
    for name, spec in bc.LEXICA.items():
        word_off, mixtures, n = bc.lexicon(name)
        W, P2, ld, mss, sil, mask = bc.shape(name)
        assert len(word_off) == W + 1 and len(mixtures) == word_off[-1] and mixtures.max() < bc.POOL <= spec.model_states
        assert list(mixtures[word_off[spec.sil_idx]:word_off[spec.sil_idx + 1]]) == list(range(spec.sil_states))
        assert not np.any(mixtures[np.repeat(np.arange(W), n) != spec.sil_idx] < spec.sil_states)   # the silence's states are its own
        if spec.p2 is not None:
            assert P2 == spec.p2
        assert sorted(int(w) for w in np.flatnonzero(n == 4)) == sorted(spec.four) or spec.lens[1] >= 4
        if spec.route.startswith("registers"):
            assert set(int(x) for x in n) >= {1, 2, 3} or spec.lens == (1, 1)   # one-state and two-state words mixed in
            assert mask == int(spec.route.split("0b")[1], 2)
    # the four-state words sit at the edges of the 1024-word rows
    assert bc.LEXICA["r1100m3"].four == (1023, 1024, 1099) and bc.LEXICA["r2100m7"].four == (1023, 1024, 2047, 2048, 2099)
    assert bc.LEXICA["r2100m2"].four == (1024, 2047) and bc.LEXICA["r2100m4"].four == (2048, 2099)
    # the rows of the register layout's DMA: bytes = 8 x the model's states rounded up to 8
    rows = {name: 8 * bc.shape(name)[2] for name in ("r40m1", "r40row2048", "r1100row2432", "r40row18k", "r2100rowfit", "r2100rowover")}
    assert rows == {"r40m1": 128, "r40row2048": 2048, "r1100row2432": 2048 + 384, "r40row18k": 18 * 1024 + 64,
                    "r2100rowfit": 8 * bc.ld_fit(2100), "r2100rowover": 8 * bc.ld_fit(2100) + 64}
    assert bc.lds_regs(2100, bc.ld_fit(2100)) == bc.LDS_BYTES
    # the positions at the break points of the dense layout
    assert [bc.shape(n)[1] for n in ("l1p4096", "l1p4097", "l1p12288", "l1p12289", "l2p4096", "l2p4097", "l2p12288", "l2p12289", "l4p12288",
                                     "l4p12289")] == [4096, 4097, 12288, 12289] + [4096, 4097, 12288, 12289] + [12288, 12289]
    for name, W in (("l1fit", 500), ("l4fit", 2100)):
        assert bc.lds_dense(W, bc.shape(name)[1]) <= bc.LDS_BYTES < bc.lds_dense(W, bc.shape(name)[1] + 1)
    assert sorted(bc.LEXICA[n].W for n in ("g4200", "g4722", "g4723", "g8192")) == [4200, 4722, 4723, 8192]
    assert bc.lexicon("glong")[2][1:].min() >= 18 and bc.lexicon("glong")[2].max() <= 24 and bc.LEXICA["g4200"].sil_states == 3
    assert {bc.LEXICA[n].sil_states for n in bc.LEXICA if bc.LEXICA[n].route.startswith("lds")} >= {2, 3}


@pytest.mark.parametrize("name", list(bc.LEXICA))
def test_route_texts_follow_from_the_rules(name):
    spec = bc.LEXICA[name]
    sh = bc.shape(name)
    assert bc.route(*sh) == spec.route
    assert bc.route(*sh, dense=True) == spec.route_dense
    assert bc.route(*sh, glob=True) == spec.route_global
    assert spec.route in bc.ROUTES and spec.route_global in bc.ROUTES and spec.route_dense in bc.ROUTES + ("none",)


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_case_conditions(case):
    table, off = bc.batch(case)
    finite = table[np.isfinite(table)]
    assert np.all(np.abs(finite) < bc.FLT_MAX)        # beyond it the search's cast to float is undefined
    if case.kind == "real":
        assert np.mean(table != table.astype(np.float32)) > 0.99   # doubles that are not floats: the cast rounds
    elif case.kind != "neginf":
        assert np.all((finite * 4) == np.round(finite * 4))
    if case.lens is None:
        lens = np.diff(off.astype(np.int64))
        assert set(lens[lens <= 3]) == {0, 1, 2, 3} and np.sum(lens > 3) >= 2
        assert all(len(r[0]) == 0 for r, n in zip(bc.reference(case), lens) if n == 0)
    for f in case.flags:
        assert bc.LEXICA[case.lex].route_for(f) != "none"
    for name in case.conditions:
        assert bc.CONDITIONS[name](case), f"{case.id}: condition {name} does not hold"


def test_every_route_has_a_dyadic_and_a_real_case_that_counts():
    have = {}
    for c in bc.CASES:
        if c.kind in ("dyadic", "real") and bc.counts(c):
            for r in c.routes():
                have.setdefault(r, set()).add(c.kind)
    missing = {r: {"dyadic", "real"} - have.get(r, set()) for r in bc.ROUTES}
    assert not any(missing.values()), {r: m for r, m in missing.items() if m}


def test_every_kind_of_table_and_lm_is_used():
    assert {c.kind for c in bc.CASES} == set(bc.KINDS) and {c.lm for c in bc.CASES} == set(bc.LM_KINDS)
    for cond in bc.CONDITIONS:
        assert any(cond in c.conditions for c in bc.CASES), cond
    # beams off, and multiples of 0.125
    assert any(c.ac >= bc.FLT_MAX and c.lmb >= bc.FLT_MAX for c in bc.CASES)
    assert all(b >= bc.FLT_MAX or b * 8 == round(b * 8) for c in bc.CASES for b in (c.ac, c.lmb))
    # the W >= 4200 cases keep their beams on
    assert all(c.ac < bc.FLT_MAX for c in bc.CASES if bc.LEXICA[c.lex].W >= 4200)


def test_the_exact_book_fit_exists():
    """r40one: every word has one state, so with the beams off every word ends in every frame and the merged list holds W entries:
    stats[0] == W T, the book is exactly full at max_word_ends = W"""
    c = next(c for c in bc.CASES if "book_exact" in c.conditions)
    k, T = bc.book_k(c)
    assert k == bc.LEXICA[c.lex].W and int(bc.reference(c)[0][3][0]) == k * T
    assert int(bc.reference(c)[0][3][3]) == 2 + k * T      # the oracle's book: the sentinel, the start entry, the word ends


SMALL = [("r40m1", "flat", "dyadic", (6.0, 2.0)), ("r40m1", "tightr", "dyadic", (12.0, 6.0)), ("r40m1", "forbid", "inf", (bc.FLT_MAX, bc.FLT_MAX)),
         ("r40m1", "dyadic", "neginf", (bc.FLT_MAX, bc.FLT_MAX)), ("r40m1", "dyadic", "nan", (12.0, 6.0)), ("r40one", "wide", "negative", (4.0, bc.FLT_MAX))]


@pytest.mark.parametrize("name,lm_kind,kind,beams", SMALL, ids=lambda p: str(p) if isinstance(p, str) else None)
def test_oracle_agrees_with_the_python_transcription(name, lm_kind, kind, beams):
    """ties, NaN and infinities on both sides of a comparison: the C restatement and the Python transcription of LinearSearch.cc take
    them the same way"""
    spec = bc.LEXICA[name]
    word_off, mixtures, _ = bc.lexicon(name)
    lm = bc.lm_table(lm_kind, name, beams[0] if lm_kind == "wide" else 0.0)
    table, _ = bc._batch(name, kind, 3, (10, 4))
    rows = table[:10]
    w, s, t, _ = bc.decode(name, lm, rows, *beams)
    with np.errstate(all="ignore"):
        pw, ps, pt = linear_search_py(rows, word_off, mixtures, spec.sil_idx, lm, spec.tdp, np.float32(beams[0]), np.float32(beams[1]))
    assert list(w) == list(pw) and list(t) == list(pt)
    assert np.array_equal(s.view(np.uint32), np.asarray(ps, np.float32).view(np.uint32))
