"""The Baum-Welch pass alone (fb_forward_kernel, fb_backward_kernel of viterbi_fb.hip; items_by_frame_kernel, items_top_kernel of
posterior_items.hip) on score tables the test supplies through sr_state_posteriors_corpus_scores, against tests/fb_reference.py run in
np.longdouble on the same table (tests/align_cases.py).  max_items is the largest number of distinct mixtures of the call's automata
and the floor 0, so every positive posterior comes back: automata of distinct states give the posteriors of positions, the others sums.

The tolerance is measured, not fixed.  The float64 run of the same reference rounds as the kernels do (one rounding per operation, the
same recursion), so its distance from the longdouble run is the size of error the number format forces on this table -- d_F for F, d_g
for the largest posterior error, d_s for the largest error of a frame's sum (a frame's sum is held to the larger of d_s and d_g: in
the float64 run the errors of a frame's posteriors may cancel by chance).  The kernels get 8 times that plus 4 ulp of the value: the
device's exp and log1p are not glibc's, and logadd3 adds three costs at once where numpy chains two logaddexp.  Every case prints
its distances and the kernels' (lines `TOL ...`; profiles/fb_scores_tolerance.txt holds a run's)."""
import math
import os

import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import align_cases as ac
from tests import fb_reference as fbr

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def models(oracle_lib):
    """model handles by (SRGPU_SCORE_CHUNK_MB, SRGPU_FB_MB) -- read when a model is created -- made on first use"""
    made = {}

    def get(chunk_mb=0, fb_mb=0):
        key = (chunk_mb, fb_mb)
        if key not in made:
            env = {k: str(v) for k, v in (("SRGPU_SCORE_CHUNK_MB", chunk_mb), ("SRGPU_FB_MB", fb_mb)) if v}
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[key] = capi.Model.from_mixset(ac.model_file(), ac.MODEL_DIM, device=0)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _n_mix(auts):
    return max(len(np.unique(a)) for a in auts)


def _run(m, case, floor=0.0, max_items=None):
    table, off, auts = ac.batch(case)
    corpus = m.upload(np.zeros((int(off[-1]), ac.MODEL_DIM), np.float32), off)
    try:
        return corpus.state_posteriors_scores(auts, case.tdp, ac.SIL, table, floor=floor, max_items=max_items or _n_mix(auts))
    finally:
        corpus.close()


def _dense(mix, count, state, weight):
    """the items of an utterance's frames as [T, M] over its mixtures `mix` (ascending); checks the order of each frame's items"""
    col = {int(k): j for j, k in enumerate(mix)}
    out = np.zeros((len(count), len(mix)))
    for t in range(len(count)):
        n = int(count[t])
        ids, w = state[t, :n], weight[t, :n]
        assert len(set(ids.tolist())) == n and all(int(k) in col for k in ids), f"frame {t}: mixtures {ids}"
        assert all(w[i] > w[i + 1] or (w[i] == w[i + 1] and ids[i] < ids[i + 1]) for i in range(n - 1)), f"frame {t}: order {w} {ids}"
        assert np.all(weight[t, n:] == 0) and np.all(state[t, n:] == 0)
        out[t, [col[int(k)] for k in ids]] = w
    return out


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


def _check(case, got, viterbi=None):
    """holds the call's outputs against the longdouble reference -> the case's TOL line"""
    cost, count, state, weight = got
    table, off, auts = ac.batch(case)
    r64, r80 = ac.fb_reference(case, "float64"), ac.fb_reference(case, "longdouble")
    assert not np.any(np.isnan(weight)), "a NaN weight"
    worst = dict(dF=0.0, dg=0.0, ds=0.0, kF=0.0, kg=0.0, ks=0.0)
    for u, ref in enumerate(auts):
        f0, f1 = int(off[u]), int(off[u + 1])
        T, N = f1 - f0, len(ref)
        tag = f"{ac.case_id(case)} utterance {u} (N {N}, T {T})"
        (F64, mix, g64), (F80, _, g80) = r64[u], r80[u]
        if case.table in ("nan", "neginf") and u == ac.HOSTILE_UTT:
            # outside the contract for entries; what must hold: F as computed, items only beside a finite F, no weight above 1
            if not math.isfinite(cost[u]):
                assert not np.any(count[f0:f1]), f"{tag}: items beside F = {cost[u]}"
            assert np.all(weight[f0:f1] <= 1.0 + 64 * np.finfo(np.float64).eps), f"{tag}: a weight of {weight[f0:f1].max()}"
            continue
        if not np.isfinite(F80):
            assert F80 == math.inf and cost[u] == math.inf, f"{tag}: F {cost[u]}, the reference's {F80}"
            assert not np.any(count[f0:f1]), f"{tag}: items without a path"
            continue
        dF = abs(float(LD(F64) - F80))
        kF = abs(float(LD(cost[u]) - F80))
        assert kF <= 8 * dF + 4 * _ulp(float(F80)), f"{tag}: F off by {kF:.3e}; float64 reference {dF:.3e}"
        dev = _dense(mix, count[f0:f1], state[f0:f1], weight[f0:f1])
        dg = float(np.max(np.abs(g64 - g80)))
        err = np.abs(dev.astype(LD) - g80).astype(np.float64)
        tol = 8 * dg + 4 * _ulp(g80.astype(np.float64))
        assert np.all(err <= tol), f"{tag}: posterior off by {err.max():.3e} at {np.argwhere(err > tol)[:4].tolist()}; float64 reference {dg:.3e}"
        # unreachable through +inf entries, forbidden jumps or the window: exactly 0, that is no item
        assert np.all(dev[np.asarray(g80 == 0)] == 0.0), f"{tag}: a posterior where no path goes"
        ds = float(np.max(np.abs(g64.sum(axis=1).astype(LD) - g80.sum(axis=1))))
        ks = float(np.max(np.abs(dev.astype(LD).sum(axis=1) - g80.sum(axis=1))))
        assert ks <= 8 * max(ds, dg) + 4 * _ulp(1.0), f"{tag}: a frame's posteriors add up to 1 -+ {ks:.3e}; float64 reference {ds:.3e}"
        assert count[f1 - 1] == 1 and state[f1 - 1, 0] == ref[-1] and weight[f1 - 1, 0] == 1.0, f"{tag}: the last frame's item"
        if viterbi is not None and T >= 2 and N <= T:
            V = float(viterbi[u])
            slack = 8 * dF + 4 * _ulp(V)
            assert V - math.log(fbr.n_paths(T, N)) - slack <= cost[u] <= V + slack, f"{tag}: F {cost[u]} against V {V}"
        for k, v in (("dF", dF), ("dg", dg), ("ds", ds), ("kF", kF), ("kg", float(err.max())), ("ks", ks)):
            worst[k] = max(worst[k], v)
    line = (f"TOL {ac.case_id(case):34s} float64-longdouble F {worst['dF']:.2e} gamma {worst['dg']:.2e} sum {worst['ds']:.2e} | "
            f"kernel-longdouble F {worst['kF']:.2e} gamma {worst['kg']:.2e} sum {worst['ks']:.2e}")
    print(line)
    return line


FB_CASES = [c for c in ac.CASES if "fb" in c.kinds]


@pytest.mark.parametrize("case", FB_CASES, ids=ac.case_id)
def test_posteriors_equal_longdouble_reference(models, case):
    m = models()
    got = _run(m, case)
    viterbi = None
    if "full" in case.kinds:  # V from the aligner on the same table
        table, off, auts = ac.batch(case)
        corpus = m.upload(np.zeros((int(off[-1]), ac.MODEL_DIM), np.float32), off)
        try:
            _, viterbi = corpus.align_scores(auts, case.tdp, ac.SIL, table)
        finally:
            corpus.close()
    _check(case, got, viterbi)


def _pick(batch, table):
    return next(c for c in ac.CASES if c.batch == batch and c.table == table and c.scale == 1.0 and not c.offset and not c.sil
                and c.tdp in (ac.TDP, ac.TDP_DYADIC) and "fb" in c.kinds)


@pytest.mark.parametrize("batch", ["chunky", "ragged70"])
def test_score_chunks_of_1mb(models, batch):
    """`chunky` takes two score chunks, the second at a frame base other than 0; same answers, bit for bit"""
    case = _pick(batch, "random")
    got = _run(models(chunk_mb=1), case)
    _check(case, got)
    for a, b in zip(got, _run(models(), case)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("batch,table", [("chunky", "random"), ("chunky", "dyadic"), ("ragged70", "random"), ("ragged70", "inf_frame")])
def test_launch_groups_of_1mb(models, batch, table):
    """SRGPU_FB_MB=1: `chunky` (4.5 MiB of trellis, none above 0.6) runs in several launch groups.  (The 70 ragged utterances have some
    0.13 MiB of trellis together: no budget splits them, and they run here as one group beside it.)"""
    case = next(c for c in ac.CASES if c.batch == batch and c.table == "inf_frame") if table == "inf_frame" else _pick(batch, table)
    got = _run(models(fb_mb=1), case)
    _check(case, got)
    for a, b in zip(got, _run(models(), case)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_floor_on_a_posterior(models):
    """Two positions, three frames, all costs 0: two paths of equal cost, the middle frame's posteriors are 0.5 and 0.5.  A floor of 0.5
    keeps both (smaller id first), the next double above drops both, max_items = 1 keeps the smaller id."""
    case = next(c for c in ac.CASES if c.batch == "floor")
    m = models()
    _, _, auts = ac.batch(case)
    lo, hi = sorted(int(k) for k in auts[0])
    cost, count, state, weight = _run(m, case, floor=0.5)
    assert abs(cost[0] + math.log(2.0)) <= 4 * _ulp(math.log(2.0))
    assert count[1] == 2 and state[1].tolist()[:2] == [lo, hi] and weight[1].tolist()[:2] == [0.5, 0.5]
    assert count[0] == 1 and count[2] == 1 and weight[0, 0] == 1.0 and weight[2, 0] == 1.0
    _, count, state, weight = _run(m, case, floor=float(np.nextafter(0.5, 1.0)))
    assert count[1] == 0 and np.all(weight[1] == 0)
    assert count[0] == 1 and count[2] == 1
    _, count, state, weight = _run(m, case, floor=0.0, max_items=1)
    assert count[1] == 1 and state[1, 0] == lo and weight[1, 0] == 0.5
    assert state.shape[1] == 1 and np.all(count[:3] == 1)


def test_argument_checks(models):
    case = _pick("b64_65", "random")
    table, off, auts = ac.batch(case)
    corpus = models().upload(np.zeros((int(off[-1]), ac.MODEL_DIM), np.float32), off)
    try:
        with pytest.raises(capi.SrError):  # the element count
            corpus.state_posteriors_scores(auts, case.tdp, ac.SIL, table[:-1])
        with pytest.raises(capi.SrError):  # a negative floor
            corpus.state_posteriors_scores(auts, case.tdp, ac.SIL, table, floor=-0.5)
    finally:
        corpus.close()
