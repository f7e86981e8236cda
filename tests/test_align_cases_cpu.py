"""The cases of tests/align_cases.py, on the references alone: no case passes vacuously.  What the GPU tests then hold the kernels to
(tests/test_gpu_align_scores.py, tests/test_gpu_fb_scores.py) is the oracle and tests/fb_reference.py on these same tables."""
import math

import numpy as np
import pytest

from tests import align_cases as ac
from tests import fb_reference as fbr


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.conditions], ids=ac.case_id)
def test_case_conditions(case, oracle_lib):
    for name in case.conditions:
        assert ac.CONDITIONS[name](case), f"{ac.case_id(case)}: condition {name} does not hold"


def test_every_dyadic_case_of_some_size_is_a_tie_case():
    for c in ac.CASES:
        if "ties" in c.conditions:
            assert ac.tie_fraction(c) >= 0.05, ac.case_id(c)
    assert sum("ties" in c.conditions for c in ac.CASES) >= 4


@pytest.mark.parametrize("case,thr", ac.pruning_runs(), ids=lambda p: ac.case_id(p) if isinstance(p, ac.Case) else f"thr{p:g}")
def test_the_beam_prunes_some_and_not_all(case, thr):
    share = ac.prune_share(case, thr)
    assert 0.10 < share < 0.90, f"{ac.case_id(case)} at {thr:g}: {share:.3f} of the created nodes pruned"


def test_the_counting_restatement_is_the_oracle(oracle_lib):
    """pruned_stats counts for the conditions above; its end position and cost are the oracle's"""
    for case in ac.CASES:
        if case.table in ("nan", "neginf") or "pruned" not in case.kinds or case.batch in ("chunky", "b600", "b257"):
            continue
        _, _, auts = ac.batch(case)
        for thr in case.thresholds:
            ref = ac.align_reference(case, thr)
            for u, aut in enumerate(auts):
                _, _, hi, cost = ac.pruned_stats(ac.rows(case, u), aut, case.tdp, thr)
                assert ac.same_cost(cost, ref[u][1]), f"{ac.case_id(case)} thr {thr:g} utterance {u}: {cost} vs {ref[u][1]}"
                if len(ref[u][0]) > 1:
                    assert ref[u][0][-1] == aut[hi]


def test_full_aligner_oracle_is_the_min_recursion(oracle_lib):
    """Oracle.align_full and fb_reference.viterbi agree wherever a path of finite cost exists (T >= 2)"""
    n = 0
    for case in ac.CASES:
        if "full" not in case.kinds or case.table in ("nan", "neginf") or case.batch == "chunky":
            continue
        _, off, auts = ac.batch(case)
        ref = ac.align_reference(case, None)
        for u, aut in enumerate(auts):
            if len(ac.rows(case, u)) < 2:
                assert ref[u][1] == math.inf  # (the reference never writes a cost for T = 1)
                continue
            states, cost = fbr.viterbi(ac.rows(case, u), aut, case.tdp, ac.SIL)
            assert ac.same_cost(cost, ref[u][1]), f"{ac.case_id(case)} utterance {u}"
            if math.isfinite(cost):
                assert np.array_equal(states, ref[u][0]), f"{ac.case_id(case)} utterance {u}"
                n += 1
    assert n > 100


def test_no_path_is_defined(oracle_lib):
    """An utterance without a path of finite cost: cost +inf.  From the frame of +inf on every cell loops in place, so the back-trace
    stands on the last position down to that frame -- the window has long moved past it -- and follows the cheapest way into it from
    there.  (It did read unset back pointers before the oracle said what stands there: test_oracle_outside_the_window.)"""
    for case in ac.CASES:
        if case.table != "inf_frame":
            continue
        _, _, auts = ac.batch(case)
        states, cost = ac.align_reference(case, None)[ac.HOSTILE_UTT]
        assert cost == math.inf
        assert np.all(states[len(states) // 2:] == auts[ac.HOSTILE_UTT][-1])


def test_oracle_outside_the_window(oracle_lib):
    """Five positions, six frames, every cost +inf: every cell loops in place, so the walk from position 4 stands outside the window
    at frame 1 (positions 0 .. 2) and at frame 0, and stays: the last state in every frame, cost +inf."""
    table = np.full((6, ac.N_STATES), np.inf)
    states, cost = ac.oracle_align(table, np.array([3, 4, 5, 6, 7], np.uint16), ac.TDP)
    assert cost == math.inf and np.array_equal(states, [7] * 6)


def test_batches_cover_the_shapes():
    shapes = {s for b in ac.BATCHES.values() for s in b}
    for want in ((1, 1), (1, 5), (2, 2), (3, 2), (5, 3), (64, 70), (65, 70), (257, 300), (600, 301)):
        assert want in shapes
    assert len(ac.BATCHES["ragged70"]) == 70 and {t for _, t in ac.BATCHES["ragged70"]} <= set(range(1, 41))
    assert ac.BATCHES["b64_65"] == ac.BATCHES["b64"] + ac.BATCHES["b65"]
    assert ac.kinds_of("tiny_wide") == ("pruned", "fb") and ac.kinds_of("b600") == ("pruned", "fb") and ac.kinds_of("tiny") == ("full", "pruned", "fb")
    # chunky: more frames than a 1 MiB score chunk of this model holds (40 states, 320 bytes a row), and more trellis than 1 MiB
    assert sum(t for _, t in ac.BATCHES["chunky"]) > (1 << 20) // (8 * ac.N_STATES)
    assert max(8 * n * t for n, t in ac.BATCHES["chunky"]) <= 1 << 20 < sum(8 * n * t for n, t in ac.BATCHES["chunky"]) // 3


def test_reference_dtype():
    """the float64 recursion is the default and unchanged; the longdouble one carries more bits where the platform has them"""
    case = next(c for c in ac.CASES if c.batch == "b64_65" and c.table == "random" and c.scale == 1.0 and not c.offset and c.tdp == ac.TDP and not c.sil)
    (F64, _, g64), (F80, _, g80) = ac.fb_reference(case, "float64")[0], ac.fb_reference(case, "longdouble")[0]
    assert isinstance(F64, float) and g64.dtype == np.float64 and g80.dtype == np.longdouble
    assert abs(float(F80 - F64)) < 1e-11 and float(np.max(np.abs(g80 - g64))) < 1e-11
    if np.finfo(np.longdouble).nmant > 52:
        assert float(F80 - np.longdouble(F64)) != 0.0 or float(np.max(np.abs(g80 - g64))) != 0.0
