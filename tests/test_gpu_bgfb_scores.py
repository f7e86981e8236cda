"""The word-posterior pass over the bigram search network alone (bgfb_table_kernel, bgfb_forward_kernel, bgfb_product_kernel,
bgfb_backward_kernel, bgfb_words_kernel of viterbi_bigram_fb.hip; netfb_top_kernel through bgfb_top) on score tables the test supplies
through sr_bigram_word_posteriors_corpus_scores, against tests/bigram_fb_reference.py run in np.longdouble on the same table with NaN
set to +inf and the device's underflow rule stated in log space (tests/bigram_fb_cases.py).  max_items is the number of words and the
floor 0, so every positive posterior comes back: a listed word carries the reference's value, an unlisted one has a reference value
within tolerance of 0.

The tolerance is measured, not fixed (netfb_cases.bound): the kernels may lie 8 times as far from the longdouble run as the farther of
two float64 restatements does -- the log-space reference, and the one that takes the word entry in the linear domain like the device --
plus 4 ulp of the value.  Every case prints its distances and the kernels' (lines `TOL ...`; profiles/bgfb_scores_tolerance.txt holds
a run's).

Device against device, bit for bit: a shorter list is the head of the full one, two calls agree, the floor only drops items, twins carry
equal bits, another kappa in between rebuilds the cached table and leaves the first kappa's bits alone, clean utterances do not see a
hostile one beside them, and the run in several score chunks and launch groups equals the run in one."""
import math

import numpy as np
import pytest

from tests import bigram_fb_cases as bc

pytestmark = pytest.mark.gpu

POST = [c for c in bc.CASES if "post" in c.passes and c.name != "chunks"]


@pytest.fixture(scope="module")
def models(oracle_lib):
    made = {}

    def get(S):
        if S not in made:
            made[S] = bc.open_model(S)
        return made[S]

    yield get
    for m in made.values():
        m.close()


def _model(models, case):
    return models(bc.LEXICA[case.lex].S)


def check(case, got, utts=None):
    """the call's outputs against the longdouble reference and the contract -> the case's TOL line"""
    cost, count, word, weight = got
    off = bc.frame_off(case)
    W = bc.net(case.lex).W
    assert not np.any(np.isnan(weight)) and np.all(weight >= 0.0) and not np.any(np.isnan(cost)), "a NaN or negative weight, or a NaN cost"
    worst = {}
    for u in (bc.sampled(case) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} utterance {u} (T {f1 - f0})"
        dev = bc.dense(count[f0:f1], word[f0:f1], weight[f0:f1], W)
        F80, p80 = bc.reference(case, "post", u)
        if not np.isfinite(F80):
            assert u in case.hostile and F80 == math.inf and cost[u] == math.inf and not np.any(count[f0:f1]), \
                f"{tag}: F {cost[u]}, {count[f0:f1].sum()} items, the reference's F {F80}"
            continue
        bc.hold(tag, (cost[u], dev), bc.restatements(case, "post", u), (F80, p80), 1.0, worst)
        assert np.all(dev[np.asarray(p80 == 0)] == 0.0), f"{tag}: a posterior where no path goes"
    return bc.tol_line("post", case, worst)


@pytest.mark.parametrize("case", POST, ids=bc.case_id)
def test_posteriors_equal_longdouble_reference(models, case):
    check(case, bc.run(_model(models, case), case, "post"))


@pytest.mark.parametrize("name", ["ragged17", "w65", "w513", "twins", "nan_first-r6", "inf_frame-b5", "gap_far"])
def test_lists_floors_and_repeats(models, name):
    case = bc.by_name(name)
    m = _model(models, case)
    full = bc.run(m, case, "post")
    assert bc.same_bytes(full, bc.run(m, case, "post")), "two identical calls differ"
    cost, count, word, weight = full
    for K in (1, 3):
        c2, n2, w2, p2 = bc.run(m, case, "post", max_items=K)
        assert bc.same_bytes((c2,), (cost,)) and np.array_equal(n2, np.minimum(count, K))
        assert bc.same_bytes((w2, p2), (word[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    floor = float(np.median(weight[weight > 0]))
    c3, n3, w3, p3 = bc.run(m, case, "post", floor=floor)
    keep = (weight > 0) & (weight >= floor)  # (each frame's list is descending: what the floor keeps is a head)
    assert 0 < keep.sum() < (weight > 0).sum()
    assert bc.same_bytes((c3,), (cost,)) and np.array_equal(n3, keep.sum(axis=1))
    assert bc.same_bytes((w3, p3), (np.where(keep, word, 0), np.where(keep, weight, 0.0)))


def test_twins_carry_equal_bits_and_list_the_smaller_word_first(models):
    case = bc.by_name("twins")
    _, count, word, weight = bc.run(_model(models, case), case, "post")
    pairs = 0
    for t in range(len(count)):
        ids, w = word[t, :count[t]].tolist(), weight[t, :count[t]]
        for a in range(1, 7, 2):  # word a and its twin a + 1: both listed or neither, equal bits, a first and a + 1 right behind
            assert (a in ids) == (a + 1 in ids)
            if a in ids:
                i = ids.index(a)
                assert ids[i + 1] == a + 1 and w[i] == w[i + 1], (t, ids, w)
                pairs += 1
    assert pairs > len(count)


def test_another_kappa_rebuilds_the_table_and_the_first_comes_back(models):
    case = bc.by_name("w65")
    m = _model(models, case)
    bg = bc.open_net(m, case)
    try:
        first = bc.run(m, case, "post", bg=bg, kappa=0.3)
        other = bc.run(m, case, "post", bg=bg, kappa=2.5)
        again = bc.run(m, case, "post", bg=bg, kappa=0.3)
        fresh = bc.run(m, case, "post", kappa=2.5)
    finally:
        bg.close()
    assert bc.same_bytes(first, again) and bc.same_bytes(other, fresh) and not np.array_equal(first[0], other[0])


def test_clean_utterances_beside_a_hostile_one(models):
    """the utterances that share a call with the NaN, the frame of +inf or the word that is not entered return the bits they return
    without it"""
    for name in ("nan_first-r6", "nan_sil-b5", "inf_frame-r6", "gap_far"):
        case = bc.by_name(name)
        off = bc.frame_off(case)
        f0, f1 = int(off[bc.HOSTILE]), int(off[bc.HOSTILE + 1])
        calm = np.array(bc.table(case))
        calm[f0:f1] = 3.0
        m = _model(models, case)
        a, b = bc.run(m, case, "post"), bc.run(m, case, "post", tab=calm)
        assert not bc.same_bytes(a, b), name
        for u in (0, 2):
            g0, g1 = int(off[u]), int(off[u + 1])
            assert bc.same_bytes([x[g0:g1] for x in a[1:]] + [a[0][u:u + 1]], [x[g0:g1] for x in b[1:]] + [b[0][u:u + 1]]), (name, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` (P = 1000, S = 768) in four score chunks and seven launch groups, the trellis, score, order and double-buffer offsets at
    work: the bits of the run in one chunk and one group, which holds against the reference"""
    case = bc.by_name("chunks")
    one = bc.run(_model(models, case), case, "post")
    check(case, one)
    cut = bc.run_in_child(case, ["post"], tmp_path / "cut.npz")["post"]
    assert bc.same_bytes(cut, one)


def test_argument_checks(models):
    from speechrecognition_amd import capi

    case = bc.by_name("dyadic-r6")
    m = _model(models, case)
    off = bc.frame_off(case)
    bg = bc.open_net(m, case)
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    tab = bc.table(case)
    EINVAL = -1

    def code(fn):
        with pytest.raises(capi.SrError) as ei:
            fn()
        return ei.value.code

    try:
        assert code(lambda: corpus.bigram_word_posteriors_scores(bg, tab[:-1])) == EINVAL      # the element count
        neg = np.array(tab)
        neg[3, 2] = -np.inf
        assert code(lambda: corpus.bigram_word_posteriors_scores(bg, neg)) == EINVAL           # a -inf entry
        assert code(lambda: corpus.bigram_word_posteriors_scores(bg, tab, floor=-0.5)) == EINVAL
        with bc.open_model(bc.LEXICA[case.lex].S) as m2:                                       # a net of another model
            other = bc.open_net(m2, case)
            assert code(lambda: corpus.bigram_word_posteriors_scores(other, tab)) == EINVAL
            other.close()
        assert np.isfinite(corpus.bigram_word_posteriors_scores(bg, tab)[0]).all()             # the handles survive the errors
    finally:
        corpus.close()
        bg.close()
