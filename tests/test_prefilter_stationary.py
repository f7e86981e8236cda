"""The fp16 prefilter's two routes write the same candidate masks, word for word: `staged` keeps a workgroup's frames
stationary and streams the model through LDS (gmm_prefilter16_kernel), `stationary` keeps a 4-state group's A operand in a wave's
registers and streams the frames' operands, built once per launch, past it (gmm_prefilter_stationary_kernel).  Compared through
sr_prefilter_masks, which runs the prefilter alone by the route it is given and poisons the mask array first, so a word a route
leaves unwritten shows as well.  Every (frame, state slot) entry is compared: the masks are integers, there is no tolerance."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth

pytestmark = pytest.mark.gpu

STAGED, STATIONARY = 0, 1


def _frame_counts():
    r = capi.prefilter_range_frames()
    return [1, 15, 16, 17, 63, 65, r + 1, 2 * r + 17]


def _model(tmp_path, S, M, D, seed):
    """S states of M densities; density 1 of state 0 := a copy of density 0 (an exact tie) where the mixture has two"""
    spec = synth.make_mixset(S, M, D, seed=seed)
    dl = spec.mixtures[0]
    if len(dl) > 1:
        spec.mean_acc[dl[1]] = spec.mean_acc[dl[0]]; spec.var_acc[dl[1]] = spec.var_acc[dl[0]]
        spec.mean_w[dl[1]] = spec.mean_w[dl[0]]; spec.var_w[dl[1]] = spec.var_w[dl[0]]
    mp = str(tmp_path / f"m{S}_{M}_{D}.mix")
    synth.write_mixset(mp, spec)
    return mp, spec


def _features(spec, T, D, seed):
    """T random frames; from 5 frames on, the first five are: a NaN, an inf, one beyond fp16's range (every density a candidate),
    all zeros, and the mean of state 0's first density (the tie decides there)"""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((T, D)).astype(np.float32)
    if T >= 5:
        feats[0, D // 2] = np.nan
        feats[1, 0] = np.inf
        feats[2, D - 1] = 300.0
        feats[3] = 0.0
        d0 = spec.mixtures[0][0]
        feats[4] = (spec.mean_acc[d0] / spec.mean_w[d0]).astype(np.float32)
    return feats


def _compare(m, spec, D, seed, counts):
    tied = len(spec.mixtures[0]) > 1
    for T in counts:
        feats = _features(spec, T, D, seed + T)
        want = m.prefilter_masks(feats, STAGED)
        got = m.prefilter_masks(feats, STATIONARY)
        assert got.shape == want.shape and got.shape[1:] == (T, 4)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"T={T}: {len(bad)} mask words differ, first (group, frame, slot) {bad[0]}: {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x}"
        if tied:  # state 0 = slot 0 of group 0, its densities 0 and 1 = bits 0 and 1: identical scores, identical fate
            w = got[0, :, 0]
            assert np.array_equal(w & 1, (w >> 1) & 1), f"T={T}: tied densities with different bits"
            if T >= 5:
                assert w[4] & 3 == 3, f"T={T}: the frame on the tied densities' mean must keep both ({w[4]:#x})"
                assert got[0, 2, 0] & 3 == 3  # beyond fp16's range: everything stays


@pytest.mark.parametrize("D", [39, 9, 25])
@pytest.mark.parametrize("S", [5, 16, 37])
@pytest.mark.parametrize("M", [1, 7, 32])
def test_masks_equal_the_staged_route(tmp_path, S, M, D):
    mp, spec = _model(tmp_path, S, M, D, seed=100 * S + M + D)
    with capi.Model.from_mixset(mp, D) as m:
        _compare(m, spec, D, S * M + D, _frame_counts())


@pytest.mark.parametrize("M", [64, 128])
def test_masks_equal_the_staged_route_wide_mixtures(tmp_path, M):
    """6 states of 64 / 128 densities: 2 / 4 consecutive state slots per state, the candidate limit relative to the minimum over all
    of them (the cross-lane minima of the epilogue)"""
    mp, spec = _model(tmp_path, 6, M, 39, seed=M)
    with capi.Model.from_mixset(mp, 39) as m:
        _compare(m, spec, 39, M, _frame_counts())


def test_default_route_scores_equal_the_exact_kernel_and_refine_what_the_staged_route_refines(tmp_path, monkeypatch):
    """sr_score_corpus end to end: the default (stationary) route gives SR_GMM_EXACT's bits, and its refinement evaluates exactly the
    densities the staged route's does -- the masks are the same, so the counts are."""
    S, M, D = 37, 32, 39
    mp, spec = _model(tmp_path, S, M, D, seed=7)
    T = capi.prefilter_range_frames() + 333
    feats = _features(spec, T, D, 11)
    counts = {}
    for route in ("default", "staged", "stationary"):
        if route == "default":
            monkeypatch.delenv("SRGPU_PREFILTER", raising=False)
        else:
            monkeypatch.setenv("SRGPU_PREFILTER", route)
        with capi.Model.from_mixset(mp, D) as m:  # (the knob is read when the model is created)
            m.profile(True)
            got = m.score_frames(feats, capi.GMM_PREFILTER)
            prof = m.profile_read()
            m.profile(False)
            if route == "default":
                exact = m.score_frames(feats, capi.GMM_EXACT)
        assert np.array_equal(got.view(np.uint64), exact.view(np.uint64)), route
        assert prof["prefilter_ms"] > 0 and prof["refined_pairs"] == T * S
        counts[route] = (prof["refined_densities"], prof["refined_pairs"])
    assert counts["default"] == counts["staged"] == counts["stationary"], counts


def test_unknown_route_name_is_refused(tmp_path, monkeypatch):
    mp, _ = _model(tmp_path, 5, 7, 9, seed=3)
    monkeypatch.setenv("SRGPU_PREFILTER", "sideways")
    with pytest.raises(capi.SrError):
        capi.Model.from_mixset(mp, 9)
