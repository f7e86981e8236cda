"""The occupancy passes over the bigram search network alone (the free network: viterbi_bigram_fb.hip's forward, product and backward
kernels; the transcripts' chains: bgchain_forward_kernel and bgchain_backward_kernel of viterbi_bigram_mmi.hip; items_kernel at
kBgItemsSerial) on score tables the test supplies through sr_bigram_occupancies_corpus_scores, against tests/bigram_mmi_reference.py run
in np.longdouble on the same table with NaN set to +inf (tests/bigram_fb_cases.py).  max_items is the model's number of states and the
floor 0, so every positive occupancy comes back.  The tolerance is test_gpu_bgfb_scores.py's rule; the `TOL` lines go to
profiles/bgfb_scores_tolerance.txt.

Device against device: F_den is the word-posterior hook's F bit for bit (include/srgpu.h promises it), F_num >= F_den, lists, floors,
repeats, clean utterances beside a hostile one and the run in several score chunks and launch groups."""
import math

import numpy as np
import pytest

from tests import bigram_fb_cases as bc
from tests.test_gpu_bgfb_scores import _model, models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

OCC = [c for c in bc.CASES if "occ" in c.passes and c.name != "chunks"]


def check(case, got, chain, utts=None):
    cost, count, state, weight = got
    off = bc.frame_off(case)
    S = bc.LEXICA[case.lex].S
    kind = "chain" if chain else "occ"
    assert not np.any(np.isnan(weight)) and np.all(weight >= 0.0) and not np.any(np.isnan(cost)), "a NaN or negative weight, or a NaN cost"
    worst = {}
    for u in (bc.sampled(case) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} {'chain' if chain else 'free'} utterance {u} (T {f1 - f0})"
        dev = bc.dense(count[f0:f1], state[f0:f1], weight[f0:f1], S)
        F80, o80 = bc.reference(case, kind, u)
        if not np.isfinite(F80):
            assert u in case.hostile and F80 == math.inf and cost[u] == math.inf and not np.any(count[f0:f1]), \
                f"{tag}: F {cost[u]}, {count[f0:f1].sum()} items, the reference's F {F80}"
            continue
        bc.hold(tag, (cost[u], dev), bc.restatements(case, kind, u), (F80, o80), 1.0, worst)
        assert np.all(dev[np.asarray(o80 == 0)] == 0.0), f"{tag}: an occupancy where no path goes"
    return bc.tol_line(kind, case, worst), worst


@pytest.mark.parametrize("case", OCC, ids=bc.case_id)
def test_occupancies_equal_longdouble_reference(models, case):
    m = _model(models, case)
    if case.trans not in bc.CHAINS:  # (the chain-* cases: the transcripts' network only)
        den = bc.run(m, case, "occ")
        check(case, den, False)
        assert bc.same_bytes((den[0],), (bc.run(m, case, "post", max_items=1)[0],)), "F_den is not the word posteriors' F"
    if case.trans is None:
        return
    num = bc.run(m, case, "chain")
    _, worst = check(case, num, True)
    if case.trans in bc.CHAINS:
        return
    for u in range(len(case.lens)):  # the chain's paths are paths of the free network
        slack = bc.bound(worst.get("dF", 0.0), den[0][u]) if math.isfinite(den[0][u]) else 0.0
        assert num[0][u] >= den[0][u] - 2 * slack, (u, num[0][u], den[0][u])


@pytest.mark.parametrize("name,kind", [("ragged70", "occ"), ("ragged70", "chain"), ("w513", "occ"), ("chain-shapes", "chain"),
                                       ("nan_sil-b5", "occ"), ("p513", "chain")])
def test_lists_floors_and_repeats(models, name, kind):
    case = bc.by_name(name)
    m = _model(models, case)
    full = bc.run(m, case, kind)
    assert bc.same_bytes(full, bc.run(m, case, kind)), "two identical calls differ"
    cost, count, state, weight = full
    for K in (1, 3):
        c2, n2, s2, w2 = bc.run(m, case, kind, max_items=K)
        assert bc.same_bytes((c2,), (cost,)) and np.array_equal(n2, np.minimum(count, K))
        assert bc.same_bytes((s2, w2), (state[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    floor = float(np.median(weight[weight > 0]))
    c3, n3, s3, w3 = bc.run(m, case, kind, floor=floor)
    keep = (weight > 0) & (weight >= floor)
    assert 0 < keep.sum() < (weight > 0).sum()
    assert bc.same_bytes((c3,), (cost,)) and np.array_equal(n3, keep.sum(axis=1))
    assert bc.same_bytes((s3, w3), (np.where(keep, state, 0), np.where(keep, weight, 0.0)))


def test_clean_utterances_beside_a_hostile_one(models):
    for name in ("nan_first-b5", "nan_sil-r6", "inf_frame-b5"):
        case = bc.by_name(name)
        off = bc.frame_off(case)
        f0, f1 = int(off[bc.HOSTILE]), int(off[bc.HOSTILE + 1])
        calm = np.array(bc.table(case))
        calm[f0:f1] = 3.0
        m = _model(models, case)
        for kind in ("occ", "chain"):
            a, b = bc.run(m, case, kind), bc.run(m, case, kind, tab=calm)
            assert not bc.same_bytes(a, b), (name, kind)
            for u in (0, 2):
                g0, g1 = int(off[u]), int(off[u + 1])
                assert bc.same_bytes([x[g0:g1] for x in a[1:]] + [a[0][u:u + 1]], [x[g0:g1] for x in b[1:]] + [b[0][u:u + 1]]), (name, kind, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` in four score chunks and seven launch groups -- the chains' trellis offsets count from the group's first utterance --:
    the bits of the run in one chunk and one group, which holds against the reference"""
    case = bc.by_name("chunks")
    m = _model(models, case)
    one = {k: bc.run(m, case, k) for k in ("occ", "chain")}
    check(case, one["occ"], False)
    check(case, one["chain"], True)
    cut = bc.run_in_child(case, ["occ", "chain"], tmp_path / "cut.npz")
    assert bc.same_bytes(cut["occ"], one["occ"]) and bc.same_bytes(cut["chain"], one["chain"])


def test_argument_checks(models):
    from speechrecognition_amd import capi

    case = bc.by_name("dyadic-r6")
    m = _model(models, case)
    off = bc.frame_off(case)
    bg = bc.open_net(m, case)
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    tab = bc.table(case)
    neg = np.array(tab)
    neg[0, 0] = -np.inf

    def code(fn):
        with pytest.raises(capi.SrError) as ei:
            fn()
        return ei.value.code

    try:
        for trans in (None, [list(t) for t in bc.transcripts(case)]):
            assert code(lambda: corpus.bigram_occupancies_scores(bg, tab[:-1], transcripts=trans)) == -1   # the element count
            assert code(lambda: corpus.bigram_occupancies_scores(bg, neg, transcripts=trans)) == -1        # a -inf entry
            assert code(lambda: corpus.bigram_occupancies_scores(bg, tab, transcripts=trans, floor=-1.0)) == -1
        with bc.open_model(bc.LEXICA[case.lex].S) as m2:                                                   # a net of another model
            other = bc.open_net(m2, case)
            assert code(lambda: corpus.bigram_occupancies_scores(other, tab)) == -1
            other.close()
    finally:
        corpus.close()
        bg.close()
