"""The fp16 prefilter's candidate limit (gmm_prefilter.hip header), restated in numpy: the host's per-state norms of the
fp16 coefficients and their rounding residuals (pack_prefilter), the kernel's per-frame |b| and |b^ - b| and its limit.  On
random and adversarial models and frames, every fp16-emulated score lies within eps of the exact one, the limit is never
above the norm-only limit the kernel used before, and the exact arg-min of every (frame, state) stays a candidate."""
from __future__ import annotations

import numpy as np
import pytest

from tests.prefilter_reference import F32, KRES16, emulated_scores, frame_side, limits, midpoints, pack_model

# (the restatement itself -- bound_consts, to_f16, up, pack_model, frame_side, limits, emulated_scores, midpoints -- lives in
# tests/prefilter_reference.py, shared with the tests that hold the device's masks against it)


def check(A, konst, states, X):
    """states: list of density index arrays.  Returns (candidates per pair with the residual form, with the norm-only form)."""
    T, D = X.shape
    ks32 = (2 * D + 3 + 31) // 32
    As, ks, Ah, kexp, norms = pack_model(A, konst)
    bh, bex, bnorm, dbn = frame_side(X)
    approx = emulated_scores(Ah, kexp, bh)
    exact = ks[None] + bex @ As.T
    nst = np.stack([np.max(norms[s], 0) for s in states])  # per-state maxima
    new, old, res = limits(nst, bnorm, dbn, ks32)
    assert np.all(res), "every state of these models takes the residual form"
    assert np.all(new <= old)
    cand_new = cand_old = 0
    for si, s in enumerate(states):
        err = np.abs(approx[:, s].astype(np.float64) - exact[:, s])
        assert np.all(err <= 0.5 * new[:, si:si + 1]), float(np.max(err / (0.5 * new[:, si:si + 1])))
        amin = np.min(approx[:, s], 1)
        mask_new = approx[:, s] <= (amin + new[:, si]).astype(F32)[:, None]
        mask_old = approx[:, s] <= (amin + old[:, si]).astype(F32)[:, None]
        assert np.all(mask_old | ~mask_new)
        assert np.all(mask_new[np.arange(T), np.argmin(exact[:, s], 1)])
        cand_new += int(mask_new.sum())
        cand_old += int(mask_old.sum())
    return cand_new / (T * len(states)), cand_old / (T * len(states))


def model(rng, S, M, D, tie=False):
    """a = [1/(2 var); -mu/var] and konst of a synth.make_mixset-like model (mu ~ N(0,1), var = 0.5 + |N(0,1)|)."""
    mu = rng.standard_normal((S * M, D))
    var = 0.5 + np.abs(rng.standard_normal((S * M, D)))
    if tie:
        var = np.repeat(var[::M], M, 0)
    A = np.empty((S * M, 2 * D))
    A[:, 0::2], A[:, 1::2] = 0.5 / var, -mu / var
    konst = 0.5 * np.sum(np.log(2 * np.pi * var) + mu * mu / var, 1) + np.log(M)
    return A, konst, [np.arange(s * M, (s + 1) * M) for s in range(S)]


def test_bench_distribution_halves_the_second_candidates():
    rng = np.random.default_rng(1)
    A, konst, states = model(rng, 200, 32, 39)
    X = rng.standard_normal((600, 39)).astype(F32)
    new, old = check(A, konst, states, X)
    assert 1.07 < old < 1.11, old        # the norm-only bound: 1.087 on the bench model
    assert new < 1.05 and (new - 1.0) < 0.6 * (old - 1.0), (new, old)


@pytest.mark.parametrize("D", [9, 39, 47, 62])
@pytest.mark.parametrize("tie", [False, True])
def test_adversarial_frames(D, tie):
    rng = np.random.default_rng(D + 100 * tie)
    A, konst, states = model(rng, 24, 32, D, tie)
    T = 360
    X = rng.standard_normal((T, D))
    X[0:60] = midpoints(rng, (60, D))                              # x and (often) x^2 on fp16 midpoints
    X[60:120] = rng.standard_normal((60, D)) * 1e-6                # fp16 subnormals (x) and underflowing x^2
    X[120:150] = rng.integers(-2**13, 2**13, size=(30, D)) * 2.0**-24  # exactly representable subnormals
    X[150:210] = rng.uniform(250.0, 255.9, size=(60, D)) * rng.choice([-1.0, 1.0], size=(60, D))  # x^2 near fp16's top
    X[210:240] = 0.0
    X[240:270, : D // 2] = 0.0
    check(A, konst, states, X.astype(F32))


@pytest.mark.parametrize("D", [9, 62])
def test_adversarial_models(D):
    """Coefficients on fp16 midpoints after scaling, and a model whose largest coefficient sits just below a power of two."""
    rng = np.random.default_rng(7 * D)
    S, M = 16, 32
    A = midpoints(rng, (S * M, 2 * D), -3, 4) * 2.0**-13
    A[:, 0::2] = np.abs(A[:, 0::2])
    A[0, 0] = 2.0**-1 * (2 - 2.0**-11)
    konst = rng.uniform(5.0, 60.0, size=S * M)
    states = [np.arange(s * M, (s + 1) * M) for s in range(S)]
    X = np.concatenate([rng.standard_normal((150, D)), midpoints(rng, (50, D))]).astype(F32)
    check(A, konst, states, X)


def test_norm_only_form_for_a_state_of_subnormal_coefficients():
    """A state whose scaled coefficients are all in fp16's subnormal range keeps the norm-only limit exactly."""
    nk = np.array([[1e-6, 100.0, 3e-7, 1.2e-6], [8000.0, 100.0, 2.0, 8000.0]])
    bnorm = np.array([6.0, 40.0], F32)
    new, old, res = limits(nk, bnorm, (KRES16 * bnorm).astype(F32), 3)
    assert list(res) == [False, True]
    assert np.array_equal(new[:, 0], old[:, 0]) and np.all(new[:, 1] < old[:, 1])
