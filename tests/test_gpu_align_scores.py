"""The forced aligners alone (align_full_kernel, align_pruned_kernel of viterbi_align.hip) on score tables the test supplies through
sr_align_corpus_scores, against the oracle on the same table (tests/align_cases.py; the conditions that keep a case from passing
vacuously are checked in test_align_cases_cpu.py).  Integers and bits: the states are equal, the cost is equal as uint64 (both sides
NaN counts as equal) -- for every case, with the default score chunks and with chunks of 1 MiB (the `chunky` batch then takes two,
the second at a frame base other than 0; every other batch still fits one)."""
import math
import os

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import align_cases as ac

pytestmark = pytest.mark.gpu

SR_EINVAL, SR_ELIMIT = -1, -4


@pytest.fixture(scope="module")
def models(oracle_lib):
    """model handles by score-chunk setting (read when a model is created), made on first use"""
    made = {}

    def get(chunk_mb):
        if chunk_mb not in made:
            old = os.environ.get("SRGPU_SCORE_CHUNK_MB")
            if chunk_mb:
                os.environ["SRGPU_SCORE_CHUNK_MB"] = str(chunk_mb)
            try:
                made[chunk_mb] = capi.Model.from_mixset(ac.model_file(), ac.MODEL_DIM, device=0)
            finally:
                if chunk_mb:
                    if old is None:
                        del os.environ["SRGPU_SCORE_CHUNK_MB"]
                    else:
                        os.environ["SRGPU_SCORE_CHUNK_MB"] = old
        return made[chunk_mb]

    yield get
    for m in made.values():
        m.close()


def _upload(m, off):
    return m.upload(np.zeros((int(off[-1]), ac.MODEL_DIM), np.float32), off)


def _compare(tag, auts, off, got, want):
    states, cost = got
    for u in range(len(auts)):
        f0, f1 = int(off[u]), int(off[u + 1])
        where = f"{tag} utterance {u} (N {len(auts[u])}, T {f1 - f0})"
        assert ac.same_cost(cost[u], want[u][1]), f"{where}: cost {cost[u]!r}, the oracle's {want[u][1]!r}"
        assert np.array_equal(states[f0:f1], want[u][0]), f"{where}: states differ at frames {np.flatnonzero(states[f0:f1] != want[u][0])[:8]}"


RUNS = [(c, thr) for c in ac.CASES for thr in ((None,) if "full" in c.kinds else ()) + (c.thresholds if "pruned" in c.kinds else ())]


def _run_id(p):
    if isinstance(p, ac.Case):
        return ac.case_id(p)
    return "full" if p is None else f"thr{p:g}"


@pytest.mark.parametrize("chunk_mb", [0, 1], ids=["chunks_default", "chunks_1mb"])
@pytest.mark.parametrize("case,thr", RUNS, ids=_run_id)
def test_aligner_equals_oracle(models, case, thr, chunk_mb):
    m = models(chunk_mb)
    table, off, auts = ac.batch(case)
    corpus = _upload(m, off)
    try:
        got = corpus.align_scores(auts, case.tdp, ac.SIL, table, pruning_threshold=thr)
    finally:
        corpus.close()
    _compare(ac.case_id(case), auts, off, got, ac.align_reference(case, thr))


def _dyadic():
    return next(c for c in ac.CASES if c.batch == "b64_65" and c.table == "dyadic" and not c.sil)


@pytest.mark.parametrize("thr", [-0.0, math.nan], ids=["minus_zero", "nan"])
def test_thresholds_that_stay_legal(models, thr):
    """-0.0 prunes what 0 prunes, a NaN limit prunes nothing: both sides, the same answer"""
    case = _dyadic()
    table, off, auts = ac.batch(case)
    want = tuple(ac.oracle_align(ac.rows(case, u), auts[u], case.tdp, thr) for u in range(len(auts)))
    corpus = _upload(models(0), off)
    try:
        got = corpus.align_scores(auts, case.tdp, ac.SIL, table, pruning_threshold=thr)
    finally:
        corpus.close()
    _compare(f"threshold {thr}", auts, off, got, want)


def test_negative_threshold_is_refused(models):
    """A negative threshold prunes the best node of frame 1 with the rest; nothing is left to trace back.  Refused on the host, by the
    hook and by sr_align_corpus_pruned -- never run."""
    case = _dyadic()
    table, off, auts = ac.batch(case)
    corpus = _upload(models(0), off)
    try:
        for thr in (-0.25, -1e-300, -math.inf):
            with pytest.raises(capi.SrError):
                corpus.align_scores(auts, case.tdp, ac.SIL, table, pruning_threshold=thr)
            with pytest.raises(capi.SrError):
                corpus.align(auts, case.tdp, ac.SIL, pruning_threshold=thr)
    finally:
        corpus.close()


def test_argument_checks(models):
    case = _dyadic()
    table, off, auts = ac.batch(case)
    corpus = _upload(models(0), off)
    try:
        with pytest.raises(capi.SrError) as e:  # the element count
            corpus.align_scores(auts, case.tdp, ac.SIL, table[:-1])
        assert e.value.code == SR_EINVAL
    finally:
        corpus.close()


def _limit_batch(N, T, seed):
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 17, size=(T, ac.N_STATES)).astype(np.float64) * 0.25
    ref = (np.arange(N) % 3 + 1).astype(np.uint16)  # three states
    return table, np.array([0, T], np.uint64), [ref]


def test_pruned_aligner_at_its_position_limit(models):
    """20 bytes a position and 48 more in 160 KiB: 8189 positions run and equal the oracle; 8190 and 8192 -- within the 8192 of
    sr_align_corpus -- are SR_ELIMIT on the host, for the hook and for sr_align_corpus_pruned, not a failed launch."""
    m = models(0)
    for N in (8190, 8192):
        table, off, auts = _limit_batch(N, 2, 1)
        corpus = _upload(m, off)
        try:
            for call in (lambda: corpus.align_scores(auts, ac.TDP_DYADIC, ac.SIL, table, pruning_threshold=0.25),
                         lambda: corpus.align(auts, ac.TDP_DYADIC, ac.SIL, pruning_threshold=0.25)):
                with pytest.raises(capi.SrError) as e:
                    call()
                assert e.value.code == SR_ELIMIT and "8189" in str(e.value)
        finally:
            corpus.close()
    table, off, auts = _limit_batch(8189, 2, 2)
    corpus = _upload(m, off)
    try:
        got = corpus.align_scores(auts, ac.TDP_DYADIC, ac.SIL, table, pruning_threshold=0.25)
    finally:
        corpus.close()
    _compare("pruned 8189 x 2", auts, off, got, (ac.oracle_align(table, auts[0], ac.TDP_DYADIC, 0.25),))


def test_full_aligner_at_its_position_limit(models):
    """8192 positions in 8192 frames (one path: forward in every frame) and in 8200 (a choice of eight loops), on three states"""
    m = models(0)
    for T in (8192, 8200):
        table, off, auts = _limit_batch(8192, T, 3)
        corpus = _upload(m, off)
        try:
            got = corpus.align_scores(auts, ac.TDP_DYADIC, ac.SIL, table)
            with pytest.raises(capi.SrError) as e:
                corpus.align_scores([np.concatenate([auts[0], auts[0][:1]])], ac.TDP_DYADIC, ac.SIL, table)
            assert e.value.code in (SR_ELIMIT, SR_EINVAL)  # (8193 positions: over the limit, and at T = 8192 more than the frames)
        finally:
            corpus.close()
        _compare(f"full 8192 x {T}", auts, off, got, (ac.oracle_align(table, auts[0], ac.TDP_DYADIC),))
