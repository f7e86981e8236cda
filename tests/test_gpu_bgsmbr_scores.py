"""The accuracy pass over the bigram search network alone (bgsmbr_forward_kernel, bgsmbr_backward_kernel of viterbi_bigram_smbr.hip on
bgfb_product_kernel at two operand vectors per utterance; items_kernel at kBgItemsSerial) on score tables the test supplies through
sr_bigram_accuracies_corpus_scores, against tests/bigram_smbr_reference.py run in np.longdouble on the same table with NaN set to +inf
(tests/bigram_fb_cases.py).  max_items is the model's number of states and the floor 0, so every gamma that is not 0 comes back, ranked
on |gamma|.  The tolerance is test_gpu_bgfb_scores.py's rule for F, Abar, every gamma and a frame's sum of gamma (0); the `TOL` lines
go to profiles/bgfb_scores_tolerance.txt.

Device against device: F is the word-posterior hook's F bit for bit (include/srgpu.h promises it), 0 <= Abar <= T, |gamma| <= T, lists,
floors, repeats, clean utterances beside a hostile one and the run in several score chunks and launch groups."""
import math

import numpy as np
import pytest

from tests import bigram_fb_cases as bc
from tests.test_gpu_bgfb_scores import _model, models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SMBR = [c for c in bc.CASES if "smbr" in c.passes and c.name != "chunks"]


def check(case, got, utts=None):
    cost, acc, count, state, weight = got
    off = bc.frame_off(case)
    S = bc.LEXICA[case.lex].S
    assert not np.any(np.isnan(weight)) and not np.any(np.isnan(acc)) and not np.any(np.isnan(cost)), "a NaN weight, accuracy or cost"
    worst = {}
    eps = np.finfo(np.float64).eps
    for u in range(len(case.lens)):
        f0, f1 = int(off[u]), int(off[u + 1])
        T = f1 - f0
        assert 0.0 <= acc[u] <= T * (1.0 + 64 * eps), f"utterance {u}: Abar {acc[u]} of {T} frames"
        assert np.all(np.abs(weight[f0:f1]) <= T * (1.0 + 64 * eps)), f"utterance {u}: |gamma| above T"
        if not math.isfinite(cost[u]):
            assert acc[u] == 0.0 and not np.any(count[f0:f1]), f"utterance {u}: F {cost[u]}, Abar {acc[u]}, {count[f0:f1].sum()} items"
    for u in (bc.sampled(case) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} utterance {u} (T {f1 - f0})"
        dev = bc.dense(count[f0:f1], state[f0:f1], weight[f0:f1], S, key=np.abs)
        F80, A80, g80 = bc.reference(case, "smbr", u)
        if not np.isfinite(F80):
            assert u in case.hostile and F80 == math.inf and cost[u] == math.inf, f"{tag}: F {cost[u]}, the reference's {F80}"
            continue
        r64 = bc.restatements(case, "smbr", u)
        bc.hold(tag, (cost[u], dev), [(r[0], r[2]) for r in r64], (F80, g80), 0.0, worst)
        # Abar is the sum over the frames of the occupancy of the frame's label, and gamma = occ (c - Abar) carries its error: like a
        # frame's sum it is held to the larger of its own float64 distance and the weights' (test_gpu_smbr_scores.py)
        dA, kA = max(bc.dist(r[1], A80) for r in r64), bc.dist(acc[u], A80)
        dw = max(bc.dist(r[2], g80) for r in r64)
        assert kA <= bc.bound(max(dA, dw), max(float(A80), 1.0)), f"{tag}: Abar off by {kA:.3e}; float64 reference {dA:.3e}, weights {dw:.3e}"
        worst["dA"], worst["kA"] = max(worst.get("dA", 0.0), dA), max(worst.get("kA", 0.0), kA)
    return bc.tol_line("smbr", case, worst)


@pytest.mark.parametrize("case", SMBR, ids=bc.case_id)
def test_accuracies_equal_longdouble_reference(models, case):
    m = _model(models, case)
    got = bc.run(m, case, "smbr")
    check(case, got)
    if "post" in case.passes:
        assert bc.same_bytes((got[0],), (bc.run(m, case, "post", max_items=1)[0],)), "F is not the word posteriors' F"


@pytest.mark.parametrize("name", ["ragged49", "w512", "labels_first", "nan_first-b5", "gap_far_k"])
def test_lists_floors_and_repeats(models, name):
    case = bc.by_name(name)
    m = _model(models, case)
    full = bc.run(m, case, "smbr")
    assert bc.same_bytes(full, bc.run(m, case, "smbr")), "two identical calls differ"
    cost, acc, count, state, weight = full
    for K in (1, 3):
        c2, a2, n2, s2, w2 = bc.run(m, case, "smbr", max_items=K)
        assert bc.same_bytes((c2, a2), (cost, acc)) and np.array_equal(n2, np.minimum(count, K))
        assert bc.same_bytes((s2, w2), (state[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    mag = np.abs(weight)
    floor = float(np.median(mag[mag > 0]))
    c3, a3, n3, s3, w3 = bc.run(m, case, "smbr", floor=floor)
    keep = (mag > 0) & (mag >= floor)
    assert 0 < keep.sum() < (mag > 0).sum()
    assert bc.same_bytes((c3, a3), (cost, acc)) and np.array_equal(n3, keep.sum(axis=1))
    assert bc.same_bytes((s3, w3), (np.where(keep, state, 0), np.where(keep, weight, 0.0)))


def test_clean_utterances_beside_a_hostile_one(models):
    for name in ("nan_first-r6", "nan_sil-b5", "inf_frame-r6", "gap_far"):
        case = bc.by_name(name)
        off = bc.frame_off(case)
        f0, f1 = int(off[bc.HOSTILE]), int(off[bc.HOSTILE + 1])
        calm = np.array(bc.table(case))
        calm[f0:f1] = 3.0
        m = _model(models, case)
        a, b = bc.run(m, case, "smbr"), bc.run(m, case, "smbr", tab=calm)
        assert not bc.same_bytes(a, b), name
        for u in (0, 2):
            g0, g1 = int(off[u]), int(off[u + 1])
            assert bc.same_bytes([x[g0:g1] for x in a[2:]] + [a[0][u:u + 1], a[1][u:u + 1]],
                                 [x[g0:g1] for x in b[2:]] + [b[0][u:u + 1], b[1][u:u + 1]]), (name, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` at 16 bytes a cell and two operand vectors per utterance: four score chunks and fourteen launch groups; the bits of the
    run in one chunk and one group, which holds against the reference"""
    case = bc.by_name("chunks")
    one = bc.run(_model(models, case), case, "smbr")
    check(case, one)
    cut = bc.run_in_child(case, ["smbr"], tmp_path / "cut.npz")["smbr"]
    assert bc.same_bytes(cut, one)


def test_argument_checks(models):
    from speechrecognition_amd import capi

    case = bc.by_name("dyadic-r6")
    m = _model(models, case)
    off = bc.frame_off(case)
    bg = bc.open_net(m, case)
    corpus = m.upload(np.zeros((int(off[-1]), bc.MODEL_DIM), np.float32), off)
    tab, lab = bc.table(case), bc.labels(case)
    neg = np.array(tab)
    neg[-1, -1] = -np.inf

    def code(fn):
        with pytest.raises(capi.SrError) as ei:
            fn()
        return ei.value.code

    try:
        assert code(lambda: corpus.bigram_accuracies_scores(bg, lab, tab[:-1])) == -1      # the element count
        assert code(lambda: corpus.bigram_accuracies_scores(bg, lab, neg)) == -1           # a -inf entry
        assert code(lambda: corpus.bigram_accuracies_scores(bg, lab, tab, floor=-0.5)) == -1
        with bc.open_model(bc.LEXICA[case.lex].S) as m2:                                   # a net of another model
            other = bc.open_net(m2, case)
            assert code(lambda: corpus.bigram_accuracies_scores(other, lab, tab)) == -1
            other.close()
    finally:
        corpus.close()
        bg.close()
