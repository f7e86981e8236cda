"""The accuracy pass alone (smbr_forward_kernel, smbr_backward_kernel of viterbi_smbr.hip; the item path of posterior_items.hip) on
score tables the test supplies through sr_net_accuracies_corpus_scores, against tests/smbr_reference.py run in np.longdouble on the same
table with NaN set to +inf (tests/netfb_cases.py).  max_items is the model's number of states and the floor 0, so every gamma that is
not 0 comes back, ranked on |gamma|.  The tolerance is test_gpu_netfb_scores.py's rule (netfb_cases.bound) for F, Abar, every gamma and
a frame's sum of gamma (0); the `TOL` lines go to profiles/netfb_scores_tolerance.txt.

Device against device: 0 <= Abar <= T, |gamma| <= T, lists, floors, repeats and the run in several score chunks and launch groups.  (F
is not the word posteriors' F bit for bit: la_add* give nf_ladd*'s cost bits for the same operands, but smbr_forward_kernel adds the
emission to each source before its three-way sum where netfb_forward_kernel adds it to the sum.)"""
import math

import numpy as np
import pytest

from tests import netfb_cases as nc
from tests.test_gpu_netfb_scores import _model, models  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SMBR = [c for c in nc.CASES if "smbr" in c.passes and c.name != "chunks"]


def check(case, got, utts=None):
    cost, acc, count, state, weight = got
    off = nc.frame_off(case)
    S = nc.LEXICA[case.lex].S
    r64, r80 = nc.smbr_reference(case, "float64"), nc.smbr_reference(case, "longdouble")
    assert not np.any(np.isnan(weight)) and not np.any(np.isnan(acc)), "a NaN weight or accuracy"
    worst = {}
    for u in range(len(case.lens)):
        f0, f1 = int(off[u]), int(off[u + 1])
        T = f1 - f0
        assert 0.0 <= acc[u] <= T * (1.0 + 64 * np.finfo(np.float64).eps), f"utterance {u}: Abar {acc[u]} of {T} frames"
        assert np.all(np.abs(weight[f0:f1]) <= T * (1.0 + 64 * np.finfo(np.float64).eps)), f"utterance {u}: |gamma| above T"
        if not math.isfinite(cost[u]):
            assert acc[u] == 0.0 and not np.any(count[f0:f1]), f"utterance {u}: F {cost[u]}, Abar {acc[u]}, {count[f0:f1].sum()} items"
    for u in (nc.sampled(case) if utts is None else utts):
        f0, f1 = int(off[u]), int(off[u + 1])
        tag = f"{case.name} utterance {u} (T {f1 - f0})"
        dev = nc.dense(count[f0:f1], state[f0:f1], weight[f0:f1], S, key=np.abs)
        if case.table == "neginf" and u == nc.HOSTILE:
            assert cost[u] == -math.inf, f"{tag}: F {cost[u]}"
            continue
        F80, A80, g80 = r80[u]
        if not np.isfinite(F80):
            assert F80 == math.inf and cost[u] == math.inf, f"{tag}: F {cost[u]}, the reference's {F80}"
            continue
        nc.hold(tag, (cost[u], dev), (r64[u][0], r64[u][2]), (F80, g80), 0.0, worst)
        dA, kA = nc.dist(r64[u][1], A80), nc.dist(acc[u], A80)
        # Abar is the sum over the frames of the occupancy of the frame's label, and gamma = occ (c - Abar) carries its error: like a
        # frame's sum it is held to the larger of its own float64 distance and the weights' (in the float64 run the errors of a sum
        # may cancel by chance: dA lies up to 50 times below dw in single utterances, the kernels' distance within dw).  Held to
        # 8 dA + 4 ulp alone, three utterances miss: ragged-b utterance 6 (T 18; kernel 9.07e-15, dA 1.88e-16, dw 9.44e-15),
        # labels_best-c utterance 5 (T 33; 2.22e-14, 8.40e-16, 4.27e-14), plus1e8-d utterance 6 (T 18; 3.68e-08, 2.09e-09, 8.76e-08).
        dw = nc.dist(r64[u][2], g80)
        assert kA <= nc.bound(max(dA, dw), max(float(A80), 1.0)), f"{tag}: Abar off by {kA:.3e}; float64 reference {dA:.3e}, weights {dw:.3e}"
        worst["dA"], worst["kA"] = max(worst.get("dA", 0.0), dA), max(worst.get("kA", 0.0), kA)
    return nc.tol_line("smbr", case, worst)


@pytest.mark.parametrize("case", SMBR, ids=nc.case_id)
def test_accuracies_equal_longdouble_reference(models, case):
    check(case, nc.run(_model(models, case), case, "smbr"))


@pytest.mark.parametrize("name", ["ragged-b", "p513", "labels_first-d", "nan_first1-d"])
def test_lists_floors_and_repeats(models, name):
    case = nc.by_name(name)
    m = _model(models, case)
    full = nc.run(m, case, "smbr")
    assert nc.same_bytes(full, nc.run(m, case, "smbr")), "two identical calls differ"
    cost, acc, count, state, weight = full
    for K in (1, 3):
        c2, a2, n2, s2, w2 = nc.run(m, case, "smbr", max_items=K)
        assert nc.same_bytes((c2, a2), (cost, acc)) and np.array_equal(n2, np.minimum(count, K))
        assert nc.same_bytes((s2, w2), (state[:, :K], weight[:, :K])), f"the list of {K} is not the head of the full one"
    mag = np.abs(weight)
    floor = float(np.median(mag[mag > 0]))
    c3, a3, n3, s3, w3 = nc.run(m, case, "smbr", floor=floor)
    keep = (mag > 0) & (mag >= floor)
    assert 0 < keep.sum() < (mag > 0).sum()
    assert nc.same_bytes((c3, a3), (cost, acc)) and np.array_equal(n3, keep.sum(axis=1))
    assert nc.same_bytes((s3, w3), (np.where(keep, state, 0), np.where(keep, weight, 0.0)))


def test_clean_utterances_beside_a_hostile_one(models):
    for name in ("nan_first1-a", "nan_own1-d", "neginf-a", "inf_frame-a"):
        case = nc.by_name(name)
        off = nc.frame_off(case)
        clean = nc.Case(name + "-clean", case.lex, "random", lens=case.lens)
        m = _model(models, case)
        a, b = nc.run(m, case, "smbr"), nc.run(m, clean, "smbr")
        for u in (0, 2):
            f0, f1 = int(off[u]), int(off[u + 1])
            assert nc.same_bytes([x[f0:f1] for x in a[2:]] + [a[0][u:u + 1], a[1][u:u + 1]],
                                 [x[f0:f1] for x in b[2:]] + [b[0][u:u + 1], b[1][u:u + 1]]), (name, u)


def test_score_chunks_and_launch_groups_of_1mb(models, tmp_path):
    """`chunks` at 16 bytes a cell: three score chunks and twelve launch groups of one to three utterances; the bits of the run in
    one chunk and one group, which four utterances hold against the reference"""
    case = nc.by_name("chunks")
    one = nc.run(_model(models, case), case, "smbr")
    check(case, one)
    cut = nc.run_in_child(case, ["smbr"], tmp_path / "cut.npz")["smbr"]
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
            corpus.net_accuracies_scores(lexh, case.wp, nc.labels(case), nc.table(case)[:-1])
    finally:
        corpus.close()
        lexh.close()
