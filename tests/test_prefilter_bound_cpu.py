"""The fp16 prefilter's candidate limit (gmm_prefilter.hip header), restated in numpy: the host's per-state norms of the
fp16 coefficients and their rounding residuals (pack_prefilter), the kernel's per-frame |b| and |b^ - b| and its limit.  On
random and adversarial models and frames, every fp16-emulated score lies within eps of the exact one, the limit is never
above the norm-only limit the kernel used before, and the exact arg-min of every (frame, state) stays a candidate."""
from __future__ import annotations

import numpy as np
import pytest

F32, F16 = np.float32, np.float16
KAPPA16, KRES16 = F32(1.05e-3), F32(4.8835e-4)


def bound_consts(ks32):
    """(acc, abs, sub) of pf_bound(ks32) (kernels.h)."""
    return (F32(1.6e-5), F32(7.0e-7), F32(3.38e-7)) if ks32 == 4 else (F32(1.1e-5), F32(6.0e-7), F32(2.92e-7))


def to_f16(v):
    """double -> float -> _Float16, as the host packs (and float -> _Float16, as the kernel packs)."""
    return np.asarray(v, dtype=np.float64).astype(F32).astype(F16).astype(np.float64)


def up(v):
    """The host's rounding up of a norm to float."""
    return np.nextafter((np.asarray(v, dtype=np.float64) * (1.0 + 1e-6)).astype(F32), F32(np.inf))


def pack_model(A, konst):
    """Scaled fp16 coefficients, the 3-term konst expansion and the per-density norms the host computes (pack_prefilter)."""
    big = max(np.max(np.abs(A)), np.max(np.abs(konst)))
    sA = 2.0 ** (13 - int(np.floor(np.log2(big))))
    As, ks = A * sA, konst * sA
    Ah = to_f16(As)
    kexp, rest = [], ks.copy()
    for _ in range(3):
        c = to_f16(rest)
        kexp.append(c)
        rest = rest - c
    norms = np.stack([up(np.sqrt(np.sum(As * As, 1))), up(np.abs(ks)), up(np.sqrt(np.sum((Ah - As) ** 2, 1))),
                      up(np.sqrt(np.sum(Ah * Ah, 1)))], 1)
    return As, ks, Ah, np.stack(kexp, 1), norms


def frame_side(X):
    """b = [x^2; x] interleaved, its fp16 image, and the kernel's bnorm and dbnorm (fp32, rounded up, dbnorm capped)."""
    T, D = X.shape
    X = X.astype(F32)
    b32 = np.empty((T, 2 * D), F32)
    b32[:, 0::2], b32[:, 1::2] = X * X, X
    bh = b32.astype(F16).astype(np.float64)
    bex = np.empty((T, 2 * D))
    bex[:, 0::2], bex[:, 1::2] = X.astype(np.float64) ** 2, X
    e = (bex - bh).astype(F32)  # fmaf(x, x, -b^) rounds the exact residual once; x - b^ is exact
    n2, e2 = np.zeros(T, F32), np.zeros(T, F32)
    for k in range(2 * D):
        n2 = (n2 + b32[:, k] * b32[:, k]).astype(F32)
        e2 = (e2 + e[:, k] * e[:, k]).astype(F32)
    bnorm = (np.sqrt(n2) * F32(1.0001)).astype(F32)
    dbn = np.minimum((np.sqrt(e2) * F32(1.0001)).astype(F32), (KRES16 * bnorm).astype(F32))
    return bh, bex, bnorm, dbn


def limits(nk, bnorm, dbn, ks32):
    """2 eps per (frame, state): (residual form, norm-only form) -- the host's folding of the state's norms into
    (lim1, limD, lim0) (pack_prefilter) and the kernel's limD |b^ - b| + lim1 |b| + lim0 in fp32."""
    kacc, kabs, ksub = bound_consts(ks32)
    na, nko, nd, nh = (nk[:, i].astype(F32) for i in range(4))
    lim0 = F32(2) * (kacc * nko + kabs * na)
    lim1_norm = F32(2) * (KAPPA16 * na + kabs)
    lim1_res = up(2.0 * (nd.astype(np.float64) + float(kacc) * nh + float(kabs)))
    limd_res = up(2.0 * (1.0 + float(kacc)) * nh.astype(np.float64))
    res = ((limd_res.astype(np.float64) * float(KRES16) + lim1_res <= lim1_norm * (1.0 - 2.0**-12))
           & ((1.0 + float(kacc)) * float(ksub) * nh.astype(np.float64) <= float(kabs) * na.astype(np.float64)))
    lim1, limd = np.where(res, lim1_res, lim1_norm), np.where(res, limd_res, F32(0))
    new = (limd[None] * dbn[:, None] + (lim1[None] * bnorm[:, None] + lim0[None])).astype(F32)
    old = (lim1_norm[None] * bnorm[:, None] + lim0[None]).astype(F32)
    return new, old, res


def check(A, konst, states, X):
    """states: list of density index arrays.  Returns (candidates per pair with the residual form, with the norm-only form)."""
    T, D = X.shape
    ks32 = (2 * D + 3 + 31) // 32
    As, ks, Ah, kexp, norms = pack_model(A, konst)
    bh, bex, bnorm, dbn = frame_side(X)
    approx = np.zeros((T, len(A)), F32)  # products of two fp16 values are exact in fp32; fp32 accumulation in k order
    for k in range(2 * D):
        approx = (approx + (bh[:, k:k + 1] * Ah[None, :, k]).astype(F32)).astype(F32)
    for t in range(3):
        approx = (approx + kexp[None, :, t].astype(F32)).astype(F32)
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


def midpoints(rng, shape, lo=-6, hi=3):
    """Values exactly halfway between two neighbouring fp16 numbers (fp16 rounding's worst case)."""
    m = rng.integers(1024, 2048, size=shape) + 0.5
    return m * np.exp2(rng.integers(lo, hi, size=shape) - 10.0) * rng.choice([-1.0, 1.0], size=shape)


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
