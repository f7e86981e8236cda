"""The cases of tests/search_cases.py, checked with the oracle alone: every case of the GPU matrix (test_gpu_search_scores.py) meets the
conditions declared for it -- so none of them passes vacuously on the device --, the lexica have the shapes their names promise, and
the oracle is deterministic on tables with NaN and +inf (the device is compared with it bit for bit)."""
import numpy as np
import pytest

from tests import search_cases as sc


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def test_case_ids_are_unique():
    ids = [c.id for c in sc.CASES]
    assert len(set(ids)) == len(ids)
    assert set(sc.SEEDS) <= set(ids)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_case_meets_its_conditions(case):
    for name in case.conditions:
        assert sc.CONDITIONS[name](case), f"{case.id}: {name} does not hold"
    table, off = sc.batch(case)
    lens = np.diff(off.astype(np.int64))
    assert 6 <= len(lens) <= 8 and {0, 1, 2, 3} <= set(lens.tolist()) and np.sum(lens >= 40) >= 2
    if case.handoff:  # some utterance may be flagged, and some must not be
        clean = sc.clean_utterances(table, off)
        assert np.any(clean[lens > 3]) and not np.all(clean)


@pytest.mark.parametrize("name", sorted(sc.LEXICA))
def test_lexicon_shape(name):
    lex = sc.lexicon(name)
    n = np.diff(lex.word_off.astype(np.int64))
    assert lex.n_states <= sc.LEXICA[name].model_states and lex.n_words <= 65535
    assert n[lex.silence_idx] in (1, 2, 3) and lex.automaton[lex.word_off[lex.silence_idx]] == 0
    if sc.LEXICA[name].describe.startswith("words"):
        assert n.max() <= 4 and lex.n_words <= 3072
    else:
        assert n.max() > 4 or sc.LEXICA[name].model_states > 10104
    if name in sc.P_RANGES:
        lo, hi = sc.P_RANGES[name]
        assert lo <= int(lex.word_off[-1]) <= hi
    if "clone" in name:
        assert sc.clone_words(lex).mean() > 0.2


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_oracle_is_deterministic_on_inf_and_nan(kind):
    case = next(c for c in sc.CASES if c.lex == "w1l3g" and c.kind == kind)
    table, _ = sc.batch(case)
    assert np.isinf(table).any() if kind == "inf" else np.isnan(table).any()
    first = sc.reference(case)
    sc._reference.cache_clear()
    second = sc.reference(case)
    assert first is not second
    for (wa, ta), (wb, tb) in zip(first, second):
        assert np.array_equal(wa, wb)
        for a, b in zip(ta, tb):
            assert a.tobytes() == b.tobytes()
