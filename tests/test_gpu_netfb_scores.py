"""The word-posterior pass alone (netfb_forward_kernel, netfb_backward_kernel, netfb_words_kernel, netfb_top_kernel of
viterbi_netfb.hip) on score tables the test supplies through sr_word_posteriors_corpus_scores, against tests/net_fb_reference.py run in
np.longdouble on the same table with NaN set to +inf (tests/netfb_cases.py).  max_items is the number of words and the floor 0, so every
positive posterior comes back: a listed word carries the reference's value, an unlisted one has a reference value within tolerance of 0.

The tolerance is measured, not fixed (netfb_cases.bound): the float64 run of the same reference rounds as the kernels do, so its
distance from the longdouble run is the error the number format forces on this table; the kernels get 8 times that plus 4 ulp of the
value.  Every case prints its distances and the kernels' (lines `TOL ...`; profiles/netfb_scores_tolerance.txt holds a run's).

Device against device, bit for bit: a shorter list is the head of the full one, two calls agree, the floor only drops items, and the run
in several score chunks and launch groups equals the run in one."""
import math

import numpy as np
import pytest

from tests import netfb_cases as nc

pytestmark = pytest.mark.gpu

POST = [c for c in nc.CASES if "post" in c.passes and c.name != "chunks"]


@pytest.fixture(scope="module")
def models(oracle_lib):
    made = {}

    def get(S):
        if S not in made:
            made[S] = nc.open_model(S)
        return made[S]

    yield get
    for m in made.values():
        m.close()


def _model(models, case):
    return models(nc.LEXICA[case.lex].S)


def check(case, got, utts=None):
    """the call's outputs against the longdouble reference and the contract -> the case's TOL line"""
    cost, count, word, weight = got
    off = nc.frame_off(case)
    W = nc.net(case.lex).W
    r64, r80 = nc.post_reference(case, "float64"), nc.post_reference(case, "longdouble")
    assert not np.any(np.isnan(weight)) and np.all(weight >= 0.0), "a NaN or negative weight"
    worst = {}
    for u in (range(len(case.lens)) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} utterance {u} (T {f1 - f0})"
        dev = nc.dense(count[f0:f1], word[f0:f1], weight[f0:f1], W)
        if case.table == "neginf" and u == nc.HOSTILE:  # no reference: F as computed, and no items beside it
            assert cost[u] == -math.inf and not np.any(count[f0:f1]), f"{tag}: F {cost[u]}, {count[f0:f1].sum()} items"
            continue
        F80, p80 = r80[u]
        if not np.isfinite(F80):
            assert F80 == math.inf and cost[u] == math.inf and not np.any(count[f0:f1]), f"{tag}: F {cost[u]}, the reference's {F80}"
            continue
        nc.hold(tag, (cost[u], dev), r64[u], (F80, p80), 1.0, worst)
        assert np.all(dev[np.asarray(p80 == 0)] == 0.0), f"{tag}: a posterior where no path goes"
    return nc.tol_line("post", case, worst)


@pytest.mark.parametrize("case", POST, ids=nc.case_id)
def test_posteriors_equal_longdouble_reference(models, case):
    check(case, nc.run(_model(models, case), case, "post"))


@pytest.mark.parametrize("name", ["ragged-d", "w130", "twins", "nan_first1-a", "inf_frame-d"])
def test_lists_floors_and_repeats(models, name):
    case = nc.by_name(name)
    m = _model(models, case)
    full = nc.run(m, case, "post")
    assert nc.same_bytes(full, nc.run(m, case, "post")), "two identical calls differ"
    cost, count, word, weight = full
    for K in (1, 3):
        c2, n2, w2, p2 = nc.run(m, case, "post", max_items=K)
        assert nc.same_bytes((c2,), (cost,)) and np.array_equal(n2, np.minimum(count, K))
        assert nc.same_bytes((w2, p2), (word[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    floor = float(np.median(weight[weight > 0]))
    c3, n3, w3, p3 = nc.run(m, case, "post", floor=floor)
    keep = (weight > 0) & (weight >= floor)  # (each frame's list is descending: what the floor keeps is a head)
    assert 0 < keep.sum() < (weight > 0).sum()
    assert nc.same_bytes((c3,), (cost,)) and np.array_equal(n3, keep.sum(axis=1))
    assert nc.same_bytes((w3, p3), (np.where(keep, word, 0), np.where(keep, weight, 0.0)))


def test_exact_ties_list_the_smaller_word_first(models):
    case = nc.by_name("twins")
    _, count, word, weight = nc.run(_model(models, case), case, "post")
    pairs = 0
    for t in range(len(count)):
        ids, w = word[t, :count[t]].tolist(), weight[t, :count[t]]
        for a in range(1, 9, 2):  # word a and its twin a + 1: both listed or neither, equal bits, a first and a + 1 right behind
            assert (a in ids) == (a + 1 in ids)
            if a in ids:
                i = ids.index(a)
                assert ids[i + 1] == a + 1 and w[i] == w[i + 1], (t, ids, w)
                pairs += 1
    assert pairs > len(count)


def test_clean_utterances_beside_a_hostile_one(models):
    """the utterances that share a call with the NaN, the -inf or the frame of +inf return the bits they return without it"""
    for name in ("nan_first1-a", "nan_pos0-d", "neginf-a", "inf_frame-a"):
        case = nc.by_name(name)
        off = nc.frame_off(case)
        clean = nc.Case(name + "-clean", case.lex, "random", lens=case.lens)
        assert np.array_equal(np.delete(nc.table(case), slice(int(off[1]), int(off[2])), axis=0),
                              np.delete(nc.table(clean), slice(int(off[1]), int(off[2])), axis=0))
        m = _model(models, case)
        a, b = nc.run(m, case, "post"), nc.run(m, clean, "post")
        for u in (0, 2):
            f0, f1 = int(off[u]), int(off[u + 1])
            assert nc.same_bytes([x[f0:f1] for x in a[1:]] + [a[0][u:u + 1]], [x[f0:f1] for x in b[1:]] + [b[0][u:u + 1]]), (name, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` (P = 1025, S = 512) in three score chunks and six launch groups, the trellis and score offsets at work: the bits of the
    run in one chunk and one group, which four utterances hold against the reference"""
    case = nc.by_name("chunks")
    one = nc.run(_model(models, case), case, "post")
    check(case, one, utts=case.sample)
    cut = nc.run_in_child(case, ["post"], tmp_path / "cut.npz")["post"]
    assert nc.same_bytes(cut, one)


def test_argument_checks(models):
    from speechrecognition_amd import capi

    case = nc.by_name("t123-a")
    m = _model(models, case)
    word_off, aut, sil, sil_state = nc.lexicon(case.lex)
    off = nc.frame_off(case)
    lexh = m.lexicon(word_off, aut, sil, case.tdp, sil_state)
    corpus = m.upload(np.zeros((int(off[-1]), nc.MODEL_DIM), np.float32), off)
    try:
        with pytest.raises(capi.SrError):  # the element count
            corpus.word_posteriors_scores(lexh, case.wp, nc.table(case)[:-1])
        with pytest.raises(capi.SrError):  # a negative floor
            corpus.word_posteriors_scores(lexh, case.wp, nc.table(case), floor=-0.5)
    finally:
        corpus.close()
        lexh.close()
