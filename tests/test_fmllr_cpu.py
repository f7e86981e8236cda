"""fMLLR without a GPU: the binding, and sr_fmllr_estimate (host code) on statistics made by the numpy restatement
(tests/fmllr_reference.py) from random models and features.

Rounding bounds.  u = 2^-53; every bound below is a multiple of 2^-52 = 2u times a sum of absolute values the reference computes.
Q(W) is a sum of D (E^2 + E) + 1 products, E = D + 1.  An evaluation adds them in chains of at most E (a row of G_i times w) + E (that
vector times w) + D (over the rows) + 3 additions and multiplications, so it errs by at most (2E + D + 3) u times the sum of the terms'
absolute values (the standard bound for a sum of products); log|det A| comes from D pivots of an elimination whose entries carry up
to D u relative error each, D^2 u absolute in the logarithm, times beta -- and beta D <= 2 x the quadratic terms' sum at any W the
update leaves (w_i G_i w_i^T ~ beta), so at most 2 D u of the same sum.  One evaluation: (2E + 3D + 3) u < 5E u; a comparison of two
evaluations (the library's and the reference's, or two sweeps'): 10E u = 5E 2^-52.  The tests use Q_MULT = 8 E."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import fmllr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
NEW = ["sr_fmllr_statistics_corpus", "sr_fmllr_statistics_bw_corpus", "sr_fmllr_estimate", "sr_corpus_transform"]


def q_mult(D):
    return 8 * (D + 1)


@pytest.fixture(scope="module")
def capi():
    from speechrecognition_amd import build, capi
    build.build()
    return capi


def make_statistics(D, S=3, seed=0, frames=None):
    """random model, features drawn around its means and bent by a per-speaker affine map, hard pairs -> reference statistics"""
    rng = np.random.default_rng(1000 * D + seed)
    model = R.random_model(rng, 12, 3, D)
    frames = frames or max(60, 12 * (D + 1))
    feats, states, off, spk = [], [], [0], []
    for s in range(S):
        A = np.eye(D) + 0.15 * rng.normal(size=(D, D)) / np.sqrt(D)
        b = 0.3 * rng.normal(size=D)
        for _ in range(2):
            st = rng.integers(0, 12, size=frames // 2)
            d = np.array([rng.integers(model[0][k], model[0][k + 1]) for k in st])
            y = model[1][d] + rng.normal(size=(len(st), D)) / np.sqrt(model[2][d])
            feats.append(((y - b) @ np.linalg.inv(A).T).astype(np.float32))
            states.append(st)
            off.append(off[-1] + len(st))
            spk.append(s)
    feats, states = np.concatenate(feats), np.concatenate(states)
    pairs = R.alignment_pairs(feats, model, states, True)
    beta, k, G, _, _, _ = R.statistics(feats, model, pairs, off, spk, S)
    return beta, k, G


def test_symbols_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "srgpu.h")).read()
    declared = set(re.findall(r"SR_API\s+[\w\s\*]+?\b(sr_\w+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(capi.lib(), name), name
    assert capi.lib().sr_abi_version() == 4 and capi.SR_ABI_VERSION == 4
    assert "#define SR_ABI_VERSION 4" in hdr


@pytest.mark.parametrize("D", [1, 2, 13, 39])
def test_auxiliary_is_monotone_and_matches_the_reference(capi, D):
    beta, k, G = make_statistics(D)
    for sweeps in (1, 2, 5):
        W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=sweeps)
        assert status.tolist() == [0, 0, 0]
        for s in range(3):
            q, mag = R.aux(beta[s], k[s], G[s], W[s])
            tol = q_mult(D) * EPS * mag
            print(f"D={D} sweeps={sweeps} s={s}: Q={q:.6f} lib-ref={aux[s, -1] - q:.3e} tol={tol:.3e} steps={np.diff(aux[s]).min():.3e}")
            assert abs(aux[s, -1] - q) <= tol
            q0, mag0 = R.aux(beta[s], k[s], G[s], np.hstack([np.eye(D), np.zeros((D, 1))]))
            assert abs(aux[s, 0] - q0) <= q_mult(D) * EPS * mag0
            for j in range(sweeps):
                assert aux[s, j + 1] >= aux[s, j] - q_mult(D) * EPS * max(mag, mag0)
            assert aux[s, -1] > aux[s, 0]   # the fixture is bent: there is something to gain
            sign, ld = np.linalg.slogdet(W[s][:, :D])
            # D pivots, each with up to D u relative error on either side
            assert abs(logdet[s] - ld) <= 2 * D * D * EPS + EPS * abs(ld)


@pytest.mark.parametrize("D", [1, 2, 13, 39])
def test_last_row_is_stationary_after_a_sweep(capi, D):
    """The row update solves dQ/dw_i = 0.  The computed w_i comes from a Cholesky solve with G_i (backward stable: it solves a system
    with G_i perturbed by at most ~E u ||G_i||, so the residual is at most E u kappa(G_i) of ||w_i G_i||) and from the cofactor row of A
    (the inverse: D u kappa(A) relative).  Margin: 16 E 2^-52 (kappa(G_i) + kappa(A)), both condition numbers from numpy."""
    beta, k, G = make_statistics(D, seed=1)
    W, _, _, status = capi.fmllr_estimate(beta, k, G, n_sweeps=1)
    assert status.tolist() == [0, 0, 0]
    i = D - 1
    for s in range(3):
        g, scale = R.row_gradient(beta[s], k[s], G[s], W[s], i)
        margin = 16 * (D + 1) * EPS * (np.linalg.cond(G[s][i]) + np.linalg.cond(W[s][:, :D]))
        print(f"D={D} s={s}: |grad|/scale={np.linalg.norm(g) / scale:.3e} margin={margin:.3e}")
        assert np.linalg.norm(g) / scale <= margin


def test_one_dimension_has_a_closed_form(capi):
    """D = 1: W = [a b], Q = beta log|a| - 1/2 w G w^T + w k^T.  Stationarity: w = G^-1 (k + (beta / a) e_0), so with H = G^-1 and
    m = H_0 . k:  a^2 - m a - beta H_00 = 0; of the two roots the one with the larger Q.  One sweep reaches it."""
    beta, k, G = make_statistics(1, seed=2)
    W, aux, _, status = capi.fmllr_estimate(beta, k, G, n_sweeps=1)
    for s in range(3):
        H = np.linalg.inv(G[s][0])
        m = H[0] @ k[s][0]
        best = None
        for sign in (1.0, -1.0):
            a = (m + sign * np.sqrt(m * m + 4 * beta[s] * H[0, 0])) / 2
            w = H @ (k[s][0] + beta[s] / a * np.array([1.0, 0.0]))
            q = R.aux(beta[s], k[s], G[s], w[None, :])[0]
            if best is None or q > best[0]:
                best = (q, w)
        tol = 64 * EPS * np.linalg.cond(G[s][0])   # two solves with G, a handful of operations each
        assert np.abs(W[s][0] - best[1]).max() <= tol * np.abs(best[1]).max(), (W[s][0], best[1])
        W2, aux2, _, _ = capi.fmllr_estimate(beta, k, G, n_sweeps=3)
        assert np.abs(W2[s][0] - W[s][0]).max() <= tol * np.abs(best[1]).max()


def test_status_and_errors(capi):
    D = 5
    beta, k, G = make_statistics(D, seed=3)
    rng = np.random.default_rng(9)
    W0 = np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), (3, 1, 1)) + 0.01 * rng.normal(size=(3, D, D + 1))
    # too little data: left as given, bit for bit
    W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=2, min_count=float(beta[1]) + 0.5, W=W0)
    assert status[1] == 1 and np.array_equal(W[1].view(np.uint64), W0[1].view(np.uint64))
    assert [int(status[s]) for s in (0, 2)] == [0 if beta[s] >= beta[1] + 0.5 else 1 for s in (0, 2)]
    # a singular G_i: restored
    Gs = G.copy()
    Gs[2, 3, :, 1] = 0.0
    Gs[2, 3, 1, :] = 0.0
    W, aux, logdet, status = capi.fmllr_estimate(beta, k, Gs, n_sweeps=2, W=W0)
    assert status.tolist() == [0, 0, 2]
    assert np.array_equal(W[2].view(np.uint64), W0[2].view(np.uint64))
    assert not np.array_equal(W[0], W0[0])
    # argument errors
    L = capi.lib()
    st = np.zeros(3, np.int32)
    Wc = W0.copy()
    P = lambda a: a.ctypes.data  # noqa: E731
    assert L.sr_fmllr_estimate(0, 3, P(beta), P(k), P(G), 1, 0.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, None, P(k), P(G), 1, 0.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), None, P(G), 1, 0.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), None, 1, 0.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 1, 0.0, None, None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 1, 0.0, P(Wc), None, None, None) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 0, 0.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 1, -1.0, P(Wc), None, None, P(st)) == -1
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 1, float("nan"), P(Wc), None, None, P(st)) == -1
    assert np.array_equal(Wc, W0)
    assert L.sr_fmllr_estimate(D, 3, P(beta), P(k), P(G), 1, 0.0, P(Wc), None, None, P(st)) == 0   # optional outputs may be NULL


def test_reference_row_update_agrees_with_the_library(capi):
    """the restatement's own update (explicit inverses) lands on the same transform: a check of the reference, at the conditioning's level"""
    D = 6
    beta, k, G = make_statistics(D, seed=4)
    W, _, _, _ = capi.fmllr_estimate(beta, k, G, n_sweeps=3)
    for s in range(3):
        Wr = R.estimate(beta[s], k[s], G[s], 3)
        kappa = max(np.linalg.cond(G[s][i]) for i in range(D))
        assert np.abs(W[s] - Wr).max() <= 1e3 * (D + 1) * EPS * kappa * np.abs(Wr).max()


def test_cpp_driver_compiles_and_estimates(capi, tmp_path):
    drv = str(tmp_path / "fmllr_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fmllr_driver.cpp"), "-o", drv,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    D, sweeps = 4, 3
    beta, k, G = make_statistics(D, seed=5)
    p = tmp_path / "stats.bin"
    p.write_bytes(struct.pack("<IIId", D, 3, sweeps, 0.0) + beta.tobytes() + k.tobytes() + G.tobytes())
    out = subprocess.check_output([drv, "estimate", str(p)], text=True).splitlines()
    W, aux, logdet, status = capi.fmllr_estimate(beta, k, G, n_sweeps=sweeps)
    for s in range(3):
        head = out[2 * s].split()
        assert head[:4] == ["speaker", str(s), "status", "0"]
        assert int(head[5], 16) == int(logdet[s:s + 1].view(np.uint64)[0]) and int(head[7], 16) == int(aux[s, -1:].view(np.uint64)[0])
        got = np.array([int(x, 16) for x in out[2 * s + 1].split()[2:]], dtype=np.uint64)
        assert np.array_equal(got, W[s].reshape(-1).view(np.uint64))
