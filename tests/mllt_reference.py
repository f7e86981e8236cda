"""numpy restatement of MLLT, the global semi-tied covariance transform (Gales 1999, one transform class), as include/srgpu.h
states it: the statistics from (features, model tables, pairs), the auxiliary function Q(A), the row update and the sweep loop.
Plain FP64 sums; beside every sum the same sum over absolute values, which is what the tests' rounding bounds are multiples of.
The pairs come from tests/fmllr_reference.py (random_model, alignment_pairs, posterior_pairs)."""
import numpy as np


def statistics(feats, model, pairs):
    """-> (beta, G [D, D, D], Gabs, n): G[i][j][k] = sum (gamma iv_di) z_j z_k with z = (double) x_t - mu_d, one matrix product
    (gamma iv)^T @ (z_j z_k); Gabs the same product over absolute values; n the number of pairs (all of them live: the pair
    walks of fmllr_reference leave the dropped ones out)"""
    _, means, inv_vars, _, _ = model
    D = feats.shape[1]
    if not pairs:
        return 0.0, np.zeros((D, D, D)), np.zeros((D, D, D)), 0
    t = np.array([p[0] for p in pairs]); d = np.array([p[1] for p in pairs]); w = np.array([p[2] for p in pairs], dtype=np.float64)
    z = feats[t].astype(np.float64) - means[d]
    a = w[:, None] * inv_vars[d]
    zz = (z[:, :, None] * z[:, None, :]).reshape(len(pairs), D * D)
    G = (a.T @ zz).reshape(D, D, D)
    Gabs = (np.abs(a).T @ np.abs(zz)).reshape(D, D, D)
    beta = 0.0
    for v in w:
        beta += v
    return beta, G, Gabs, len(pairs)


def aux(beta, G, A):
    """Q(A) = beta log|det A| - 1/2 sum_i a_i G_i a_i^T -> (Q, sum of the absolute values of its terms)"""
    D = A.shape[0]
    _, logdet = np.linalg.slogdet(A)
    q = beta * logdet
    mag = abs(beta * logdet)
    for i in range(D):
        q += -0.5 * (A[i] @ G[i] @ A[i])
        mag += 0.5 * (np.abs(A[i]) @ np.abs(G[i]) @ np.abs(A[i]))
    return q, mag


def cofactor_row(A, i):
    return np.linalg.det(A) * np.linalg.inv(A)[:, i]


def row_gradient(beta, G, A, i):
    """dQ/da_i = beta (A^-T)_i - a_i G_i"""
    return beta * np.linalg.inv(A)[:, i] - A[i] @ G[i]


def row_update(beta, G, A, i):
    """a_i = alpha p_i G_i^-1 in place, alpha = +sqrt(beta / (p_i G_i^-1 p_i^T))"""
    p = cofactor_row(A, i)
    pg = np.linalg.solve(G[i], p)
    A[i] = np.sqrt(beta / (p @ pg)) * pg


def estimate(beta, G, n_sweeps, A=None):
    """-> (A, [Q after 0 .. n_sweeps sweeps])"""
    D = G.shape[0]
    A = np.eye(D) if A is None else A.copy()
    qs = [aux(beta, G, A)[0]]
    for _ in range(n_sweeps):
        for i in range(D):
            row_update(beta, G, A, i)
        qs.append(aux(beta, G, A)[0])
    return A, qs
