"""MLLR mean adaptation without a GPU: the binding, and sr_mllr_estimate (host code) on statistics made with the numpy restatement
(tests/mllr_reference.py).

The solve bound.  u = 2^-53, gamma_m = m u / (1 - m u), n = D + 1.  Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.),
Theorem 10.4: the computed solution of a Cholesky solve satisfies (G + dG) w = k with |dG| <= gamma_{3n+1} |R^T| |R|, R the computed
factor, and (10.7) || |R^T| |R| ||_2 <= n (1 - n gamma_{n+1})^-1 ||G||_2.  Hence the residual
    ||w G - k||_2 = ||w dG||_2 <= CHOL(n) ||G||_2 ||w||_2,    CHOL(n) = n gamma_{3n+1} / (1 - n gamma_{n+1}),
the constant the tests use as it stands; ||G||_2 and ||w||_2 come from numpy, the residual itself is formed in numpy.longdouble.

Exact recovery.  Statistics of observations that equal W* xi_d exactly satisfy k_i = w*_i G_i in exact arithmetic.  They reach the
library rounded to FP64: k + dk with ||dk||_2 <= u ||k||_2 <= u ||G||_2 ||w*||_2 and G + dG' with ||dG'||_2 <= u || |G| ||_2 <=
u sqrt(n) ||G||_2.  With the solve's own dG: G (w - w*) = dk - w dG - w* dG', so
    ||w - w*||_2 <= cond_2(G) (CHOL(n) ||w||_2 + u (1 + sqrt(n)) ||w*||_2),
the solve bound scaled by numpy's cond(G_i), plus the rounding of the statistics handed in."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import mllr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
NEW = ["sr_mllr_statistics_corpus", "sr_mllr_statistics_bw_corpus", "sr_mllr_estimate", "sr_model_transform_means"]
TREE = np.array([4, 4, 5, 5, 6, 6, -1], np.int32)   # leaves 0 .. 3; 4 = {0, 1}, 5 = {2, 3}, 6 = the root


def gamma(m):
    return m * U / (1 - m * U)


def chol_const(n):
    return n * gamma(3 * n + 1) / (1 - n * gamma(n + 1))


@pytest.fixture(scope="module")
def capi():
    from speechrecognition_amd import build, capi
    build.build()
    return capi


def make_statistics(D, S=2, n_classes=3, seed=0, per_class=None, w_star=None, noise=0.3):
    """statistics of random densities and occupancies, summed in longdouble and rounded once: x_acc[s][d] = occ (W*_{s,r} xi_d + noise)
    -> (beta [S, R], k, G)"""
    rng = np.random.default_rng(977 * D + seed)
    E = D + 1
    per_class = per_class or 3 * E
    beta = np.zeros((S, n_classes), LD); k = np.zeros((S, n_classes, D, E), LD); G = np.zeros((S, n_classes, D, E, E), LD)
    for s in range(S):
        for r in range(n_classes):
            for _ in range(per_class):
                mu = rng.normal(0.0, 2.0, size=D)
                iv = (1.0 / rng.uniform(0.5, 2.0, size=D)).astype(LD)
                occ = LD(rng.uniform(0.5, 20.0))
                xi = np.concatenate([mu, [1.0]]).astype(LD)
                W = (w_star[s, r] if w_star is not None else R.identity(D) + 0.1 * rng.normal(size=(D, E))).astype(LD)
                x = W @ xi + (noise * rng.normal(size=D) if noise else 0.0)
                beta[s, r] += occ
                k[s, r] += np.outer(iv * (occ * x), xi)
                G[s, r] += (occ * iv)[:, None, None] * np.outer(xi, xi)[None]
    return beta.astype(np.float64), k.astype(np.float64), G.astype(np.float64)


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
def test_solve_residual_and_auxiliary(capi, D):
    beta, k, G = make_statistics(D)
    W, node, aux = capi.mllr_estimate(beta, k, G)
    S, Rn = beta.shape
    assert np.array_equal(node, np.tile(np.arange(Rn, dtype=np.int32), (S, 1)))
    worst = 0.0
    for s in range(S):
        for r in range(Rn):
            for i in range(D):
                res = W[s, r, i].astype(LD) @ G[s, r, i].astype(LD) - k[s, r, i].astype(LD)
                lim = chol_const(D + 1) * np.linalg.norm(G[s, r, i], 2) * np.linalg.norm(W[s, r, i])
                worst = max(worst, float(np.linalg.norm(res.astype(np.float64)) / lim))
                assert np.linalg.norm(res.astype(np.float64)) <= lim, (s, r, i)
            # the auxiliary function: at the result it is no smaller than at the start, and both match the restatement
            assert aux[s, r, 1] >= aux[s, r, 0]
            q0, m0 = R.aux(k[s, r], G[s, r], R.identity(D))
            q1, m1 = R.aux(k[s, r], G[s, r], W[s, r])
            # a sum of D (E^2 + E) products in chains of at most 2 E + D + 3 operations, on either side
            tol = 2 * (2 * (D + 1) + D + 3) * 2 * U
            assert abs(aux[s, r, 0] - q0) <= tol * m0 and abs(aux[s, r, 1] - q1) <= tol * m1
    print(f"D={D}: worst residual / bound = {worst:.3e}")


@pytest.mark.parametrize("D", [1, 2, 13, 39])
def test_exact_observations_recover_the_transform(capi, D):
    rng = np.random.default_rng(5 + D)
    S, Rn, E = 2, 2, D + 1
    w_star = R.identity(D, S, Rn) + 0.2 * rng.normal(size=(S, Rn, D, E))
    beta, k, G = make_statistics(D, S=S, n_classes=Rn, seed=1, w_star=w_star, noise=0.0)
    W, node, aux = capi.mllr_estimate(beta, k, G)
    assert (node >= 0).all()
    worst = 0.0
    for s in range(S):
        for r in range(Rn):
            for i in range(D):
                lim = np.linalg.cond(G[s, r, i]) * (chol_const(E) * np.linalg.norm(W[s, r, i]) +
                                                    U * (1 + np.sqrt(E)) * np.linalg.norm(w_star[s, r, i]))
                err = np.linalg.norm(W[s, r, i] - w_star[s, r, i])
                worst = max(worst, float(err / lim))
                assert err <= lim, (s, r, i, err, lim)
    print(f"D={D}: worst |W - W*| / bound = {worst:.3e}")


def test_tree_backs_off_to_the_lowest_node_that_qualifies(capi):
    D, S = 5, 2
    beta, k, G = make_statistics(D, S=S, n_classes=4, seed=2)
    rng = np.random.default_rng(3)
    W0 = R.identity(D, S, 4) + 0.01 * rng.normal(size=(S, 4, D, D + 1))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
    # leaf 0 of speaker 0 is too small: it takes node 4 = {0, 1}; every other leaf qualifies by itself
    beta2, k2, G2 = beta.copy(), k.copy(), G.copy()
    scale = 0.01
    beta2[0, 0] *= scale; k2[0, 0] *= scale; G2[0, 0] *= scale
    min_count = float(beta2[0, 0]) * 2
    assert beta2[0, 1:].min() > min_count and beta2[1].min() > min_count
    W, node, aux = capi.mllr_estimate(beta2, k2, G2, parent=TREE, min_count=min_count, W=W0)
    assert node.tolist() == [[4, 1, 2, 3], [0, 1, 2, 3]]
    summed = (beta2[0, 0] + beta2[0, 1], k2[0, 0] + k2[0, 1], G2[0, 0] + G2[0, 1])
    Wn, _, _ = capi.mllr_estimate(summed[0][None, None], summed[1][None, None], summed[2][None, None])
    assert np.array_equal(bits(W[0, 0]), bits(Wn[0, 0])), "the parent's transform is the estimate from its leaves' summed statistics"
    assert np.array_equal(bits(R.node_statistics(beta2[0], k2[0], G2[0], TREE, 4)[2]), bits(summed[2]))
    alone, _, _ = capi.mllr_estimate(beta2, k2, G2)
    assert np.array_equal(bits(W[0, 1:]), bits(alone[0, 1:])) and np.array_equal(bits(W[1]), bits(alone[1]))
    q0, m0 = R.aux(summed[1], summed[2], W0[0, 0])
    assert abs(aux[0, 0, 0] - q0) <= 2 * (2 * (D + 1) + D + 3) * 2 * U * m0 and aux[0, 0, 1] >= aux[0, 0, 0]
    # further up: only the root holds enough for speaker 0
    big = float(beta2[0].sum()) * 0.9
    W, node, _ = capi.mllr_estimate(beta2, k2, G2, parent=TREE, min_count=big, W=W0)
    assert node[0].tolist() == [6, 6, 6, 6]
    root = R.node_statistics(beta2[0], k2[0], G2[0], TREE, 6)
    Wr, _, _ = capi.mllr_estimate(np.array([[root[0]]]), root[1][None, None], root[2][None, None])
    for r in range(4):
        assert np.array_equal(bits(W[0, r]), bits(Wr[0, 0]))
    # the root too small: node -1, W as given bit for bit, the auxiliary values NaN
    W, node, aux = capi.mllr_estimate(beta2, k2, G2, parent=TREE, min_count=float(beta2.sum()) * 2, W=W0)
    assert (node == -1).all() and np.array_equal(bits(W), bits(W0)) and np.isnan(aux).all()
    # without a tree a small leaf has nowhere to go
    W, node, _ = capi.mllr_estimate(beta2, k2, G2, min_count=min_count, W=W0)
    assert node[0].tolist() == [-1, 1, 2, 3] and np.array_equal(bits(W[0, 0]), bits(W0[0, 0]))
    # a G_i that is not positive definite backs off too: leaf 2 of speaker 1 goes to node 5, whose sum factorises
    G3 = G.copy()
    G3[1, 2, 3, :, 1] = 0.0
    G3[1, 2, 3, 1, :] = 0.0
    W, node, _ = capi.mllr_estimate(beta, k, G3, parent=TREE, W=W0)
    assert node.tolist() == [[0, 1, 2, 3], [0, 1, 5, 3]]
    W, node, _ = capi.mllr_estimate(beta, k, G3, W=W0)
    assert node[1].tolist() == [0, 1, -1, 3] and np.array_equal(bits(W[1, 2]), bits(W0[1, 2]))
    # a forest: two roots, nothing above them
    forest = np.array([4, 4, 5, 5, -1, -1], np.int32)
    assert max(beta2[0, 0] + beta2[0, 1], beta2[0, 2] + beta2[0, 3]) < big
    W, node, _ = capi.mllr_estimate(beta2, k2, G2, parent=forest, min_count=big, W=W0)
    assert node[0].tolist() == [-1, -1, -1, -1]
    W, node, _ = capi.mllr_estimate(beta2, k2, G2, parent=forest, min_count=min_count, W=W0)
    assert node[0].tolist() == [4, 1, 2, 3]


def test_argument_errors(capi):
    D, S = 3, 2
    beta, k, G = make_statistics(D, S=S, n_classes=4, seed=4)
    W0 = R.identity(D, S, 4)
    W = W0.copy()
    node = np.zeros((S, 4), np.int32)
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(dim=D, n_classes=4, parent=TREE, b=beta, kk=k, g=G, mc=0.0, w=W, nd=node, n_nodes=None):
        parent = None if parent is None else np.ascontiguousarray(parent, np.int32)
        n_nodes = (len(parent) if parent is not None else 4) if n_nodes is None else n_nodes
        return L.sr_mllr_estimate(dim, S, n_classes, n_nodes, None if parent is None else P(parent), None if b is None else P(b),
                                  None if kk is None else P(kk), None if g is None else P(g), mc, None if w is None else P(w),
                                  None if nd is None else P(nd), None)

    assert call() == 0                      # out_aux may be NULL
    W[:] = W0
    assert call(dim=0) == -1
    assert call(parent=None) == -1 and call(b=None) == -1 and call(kk=None) == -1 and call(g=None) == -1
    assert call(w=None) == -1 and call(nd=None) == -1
    assert call(mc=-1.0) == -1 and call(mc=float("nan")) == -1
    assert call(n_classes=0) == -1
    assert call(n_nodes=3) == -1            # fewer nodes than classes
    for bad in ([4, 4, 5, 5, 6, 6, 6],      # a node that is its own parent
                [4, 4, 5, 5, 6, 6, 5],      # a parent below its child
                [4, 4, 5, 5, 6, 7, -1],     # a parent beyond the nodes
                [1, 4, 5, 5, 6, 6, -1],     # a leaf as a parent
                [4, 4, 5, 5, 6, 6, -2]):    # neither a node nor -1
        assert call(parent=bad) == -1, bad
    assert np.array_equal(W, W0)
    assert b"malformed tree" in L.sr_last_error()


def test_standalone_driver_under_the_sanitizers(capi, tmp_path):
    """tests/cpp/mllr_driver.cpp and mllr.cpp alone, built with -fsanitize=address,undefined and run as a plain program on a small tree
    case: the same bits as the library's estimate, and no report."""
    drv = str(tmp_path / "mllr_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "mllr_driver.cpp"),
                           os.path.join(ROOT, "speechrecognition_amd", "csrc", "mllr.cpp"), "-o", drv])
    D, S = 4, 2
    beta, k, G = make_statistics(D, S=S, n_classes=4, seed=6)
    beta[0, 0] *= 0.01; k[0, 0] *= 0.01; G[0, 0] *= 0.01
    G[1, 2, 1, :, 0] = 0.0
    G[1, 2, 1, 0, :] = 0.0
    min_count = float(beta[0, 0]) * 2
    W0 = R.identity(D, S, 4) + 0.01 * np.random.default_rng(8).normal(size=(S, 4, D, D + 1))
    case = tmp_path / "case.bin"
    case.write_bytes(struct.pack("<IIIId", D, S, 4, len(TREE), min_count) + TREE.tobytes() + beta.tobytes() + k.tobytes() + G.tobytes() +
                     W0.tobytes())
    p = subprocess.run([drv, str(case)], text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:], p.stderr[-2000:])
    out = p.stdout.splitlines()
    W, node, aux = capi.mllr_estimate(beta, k, G, parent=TREE, min_count=min_count, W=W0)
    assert node.tolist() == [[4, 1, 2, 3], [0, 1, 5, 3]]
    for s in range(S):
        for r in range(4):
            head = out[2 * (s * 4 + r)].split()
            assert head[:4] == ["leaf", str(s), str(r), "node"] and int(head[4]) == node[s, r]
            assert [int(x, 16) for x in head[6:8]] == aux[s, r].view(np.uint64).tolist()
            got = np.array([int(x, 16) for x in out[2 * (s * 4 + r) + 1].split()[1:]], dtype=np.uint64)
            assert np.array_equal(got, W[s, r].reshape(-1).view(np.uint64))
