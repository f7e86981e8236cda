"""The occupancy pass alone (netfb_forward_kernel with netocc_backward_kernel, chain_forward_kernel and chain_backward_kernel of
viterbi_mmi.hip; the item path of posterior_items.hip) on score tables the test supplies through sr_net_occupancies_corpus_scores:
the free network and the transcripts' chains, against tests/mmi_reference.py run in np.longdouble on the same table with NaN set to
+inf (tests/netfb_cases.py).  max_items is the model's number of states and the floor 0, so every positive occupancy comes back.  The
tolerance is test_gpu_netfb_scores.py's rule (netfb_cases.bound); the `TOL` lines go to profiles/netfb_scores_tolerance.txt.

Device against device: F_den is the word-posterior hook's F bit for bit (the same forward kernel), F_num >= F_den, lists, floors, repeats
and the run in several score chunks and launch groups."""
import math

import numpy as np
import pytest

from tests import netfb_cases as nc
from tests.test_gpu_netfb_scores import _model, models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

OCC = [c for c in nc.CASES if "occ" in c.passes and c.name != "chunks"]


def check(case, got, chain, utts=None):
    cost, count, state, weight = got
    off = nc.frame_off(case)
    S = nc.LEXICA[case.lex].S
    r64, r80 = nc.occ_reference(case, "float64", chain), nc.occ_reference(case, "longdouble", chain)
    assert not np.any(np.isnan(weight)) and np.all(weight >= 0.0), "a NaN or negative weight"
    worst = {}
    for u in (nc.sampled(case) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} {'chain' if chain else 'free'} utterance {u} (T {f1 - f0})"
        dev = nc.dense(count[f0:f1], state[f0:f1], weight[f0:f1], S)
        if case.table == "neginf" and u == nc.HOSTILE and not (chain and math.isfinite(cost[u])):
            assert cost[u] in (-math.inf, math.inf) and not np.any(count[f0:f1]), f"{tag}: F {cost[u]}, {count[f0:f1].sum()} items"
            continue
        # (a chain that cannot reach the -inf cell keeps a finite F: the reference is defined for it, and the rule holds it)
        F80, o80 = r80[u]
        if not np.isfinite(F80):
            assert F80 == math.inf and cost[u] == math.inf and not np.any(count[f0:f1]), f"{tag}: F {cost[u]}, the reference's {F80}"
            continue
        nc.hold(tag, (cost[u], dev), r64[u], (F80, o80), 1.0, worst)
        assert np.all(dev[np.asarray(o80 == 0)] == 0.0), f"{tag}: an occupancy where no path goes"
    return nc.tol_line("chain" if chain else "occ", case, worst), worst


@pytest.mark.parametrize("case", OCC, ids=nc.case_id)
def test_occupancies_equal_longdouble_reference(models, case):
    m = _model(models, case)
    den = nc.run(m, case, "occ")
    check(case, den, False)
    if "post" in case.passes:  # the same forward kernel on the same table
        assert nc.same_bytes((den[0],), (nc.run(m, case, "post", max_items=1)[0],)), "F_den is not the word posteriors' F"
    if case.trans is None:
        return
    num = nc.run(m, case, "chain")
    _, worst = check(case, num, True)
    # the chain's paths are paths of the free network
    for u in range(len(case.lens)):
        if case.table == "neginf" and u == nc.HOSTILE:
            continue
        slack = nc.bound(worst.get("dF", 0.0), den[0][u]) if math.isfinite(den[0][u]) else 0.0
        assert num[0][u] >= den[0][u] - 2 * slack, (u, num[0][u], den[0][u])


@pytest.mark.parametrize("name,kind", [("ragged-a", "occ"), ("ragged-a", "chain"), ("p513", "occ"), ("chain-mixed", "chain"),
                                       ("nan_own1-a", "occ")])
def test_lists_floors_and_repeats(models, name, kind):
    case = nc.by_name(name)
    m = _model(models, case)
    full = nc.run(m, case, kind)
    assert nc.same_bytes(full, nc.run(m, case, kind)), "two identical calls differ"
    cost, count, state, weight = full
    for K in (1, 3):
        c2, n2, s2, w2 = nc.run(m, case, kind, max_items=K)
        assert nc.same_bytes((c2,), (cost,)) and np.array_equal(n2, np.minimum(count, K))
        assert nc.same_bytes((s2, w2), (state[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    floor = float(np.median(weight[weight > 0]))
    c3, n3, s3, w3 = nc.run(m, case, kind, floor=floor)
    keep = (weight > 0) & (weight >= floor)
    assert 0 < keep.sum() < (weight > 0).sum()
    assert nc.same_bytes((c3,), (cost,)) and np.array_equal(n3, keep.sum(axis=1))
    assert nc.same_bytes((s3, w3), (np.where(keep, state, 0), np.where(keep, weight, 0.0)))


def test_clean_utterances_beside_a_hostile_one(models):
    for name in ("nan_first1-a", "neginf-a", "inf_frame-a"):
        case = nc.by_name(name)
        off = nc.frame_off(case)
        clean = nc.Case(name + "-clean", case.lex, "random", lens=case.lens, trans=case.trans)
        m = _model(models, case)
        for kind in ("occ", "chain"):
            a, b = nc.run(m, case, kind), nc.run(m, clean, kind)
            for u in (0, 2):
                f0, f1 = int(off[u]), int(off[u + 1])
                assert nc.same_bytes([x[f0:f1] for x in a[1:]] + [a[0][u:u + 1]], [x[f0:f1] for x in b[1:]] + [b[0][u:u + 1]]), (name, kind, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` in three score chunks and six launch groups -- the chains' trellis offsets count from the group's first utterance --:
    the bits of the run in one chunk and one group, which four utterances hold against the reference"""
    case = nc.by_name("chunks")
    m = _model(models, case)
    one = {k: nc.run(m, case, k) for k in ("occ", "chain")}
    check(case, one["occ"], False)
    check(case, one["chain"], True)
    cut = nc.run_in_child(case, ["occ", "chain"], tmp_path / "cut.npz")
    assert nc.same_bytes(cut["occ"], one["occ"]) and nc.same_bytes(cut["chain"], one["chain"])


def test_argument_checks(models):
    from speechrecognition_amd import capi

    case = nc.by_name("t123-a")
    m = _model(models, case)
    word_off, aut, sil, sil_state = nc.lexicon(case.lex)
    off = nc.frame_off(case)
    lexh = m.lexicon(word_off, aut, sil, case.tdp, sil_state)
    corpus = m.upload(np.zeros((int(off[-1]), nc.MODEL_DIM), np.float32), off)
    try:
        for trans in (None, [[1], [], [2]]):
            with pytest.raises(capi.SrError):  # the element count
                corpus.net_occupancies_scores(lexh, case.wp, nc.table(case)[:-1], transcripts=trans)
    finally:
        corpus.close()
        lexh.close()
