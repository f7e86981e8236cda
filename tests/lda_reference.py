"""numpy restatement of the LDA calls (include/srgpu.h: sr_lda_statistics_corpus, sr_lda_estimate, sr_corpus_splice_transform).

Splicing with clamping at the utterance's edges; the three sums in plain FP64 and, beside every sum, the same sum over absolute
values (the scale of the rounding bounds in tests/test_gpu_lda.py); the estimate with numpy's Cholesky and symmetric
eigendecomposition; the projection as the specified loop, vectorised over frames one column at a time, where numpy rounds every
multiplication and every addition."""
import numpy as np

SKIP = 0xFFFFFFFF


def splice(feats, off, context):
    """-> f64[F, (2 context + 1) D]: row t stacks frames t - context .. t + context of t's utterance, edge frames repeated"""
    feats = np.asarray(feats, dtype=np.float32)
    F, D = feats.shape
    c = int(context)
    src = np.empty((F, 2 * c + 1), dtype=np.int64)
    for u in range(len(off) - 1):
        a, b = int(off[u]), int(off[u + 1])
        if b > a:
            t = np.arange(a, b)[:, None] + np.arange(-c, c + 1)[None, :]
            src[a:b] = np.clip(t, a, b - 1)
    return feats[src].astype(np.float64).reshape(F, (2 * c + 1) * D)


def frame_classes(states, class_of_state=None):
    """-> i64[F]: the class of every frame, -1 where it is skipped"""
    states = np.asarray(states, dtype=np.int64)
    k = states if class_of_state is None else np.asarray(class_of_state, dtype=np.int64)[states]
    return np.where(k == SKIP, -1, k)


def statistics(feats, off, states, context, class_of_state=None, n_classes=None):
    """-> (count f64[K], sum f64[K, E], scatter f64[E, E], sum_abs, scatter_abs)"""
    Z = splice(feats, off, context)
    k = frame_classes(states, class_of_state)
    K = int(n_classes) if n_classes is not None else int(k.max()) + 1
    E = Z.shape[1]
    count, total, total_abs = np.zeros(K), np.zeros((K, E)), np.zeros((K, E))
    for q in range(K):
        rows = Z[k == q]
        count[q] = len(rows)
        total[q] = rows.sum(axis=0)
        total_abs[q] = np.abs(rows).sum(axis=0)
    kept = Z[k >= 0]
    return count, total, kept.T @ kept, total_abs, np.abs(kept).T @ np.abs(kept)


def covariances(count, total, scatter):
    """-> (W, B, mu): within-class and between-class covariance and the global mean, as sr_lda_estimate defines them"""
    N = count.sum()
    live = count > 0
    muk = total[live] / count[live][:, None]
    between = (muk * count[live][:, None]).T @ muk
    mu = total.sum(axis=0) / N
    return (scatter - between) / N, between / N - np.outer(mu, mu), mu


def estimate(count, total, scatter, p, remove_mean=False):
    """-> (M f64[p, E+1], eig f64[E] descending, W, B, mu)"""
    W, B, mu = covariances(count, total, scatter)
    L = np.linalg.cholesky(W)
    Li = np.linalg.inv(L)
    Cm = Li @ B @ Li.T
    w, V = np.linalg.eigh(0.5 * (Cm + Cm.T))
    order = np.argsort(-w, kind="stable")
    w, V = w[order], V[:, order]
    A = np.linalg.solve(L.T, V[:, :p]).T   # rows q^T L^-1
    for i in range(p):
        if A[i, np.argmax(np.abs(A[i]))] < 0:
            A[i] = -A[i]
    b = -(A @ mu) if remove_mean else np.zeros(p)
    return np.hstack([A, b[:, None]]), w, W, B, mu


def project(feats, off, context, M):
    """-> f32[F, p]: acc = M[i][E]; acc = acc + M[i][n] * z[n], n ascending, every operation rounded"""
    Z = splice(feats, off, context)
    M = np.asarray(M, dtype=np.float64)
    p, E = M.shape[0], M.shape[1] - 1
    out = np.empty((Z.shape[0], p), dtype=np.float32)
    for i in range(p):
        acc = np.full(Z.shape[0], M[i, E])
        for n in range(E):
            acc = acc + M[i, n] * Z[:, n]
        out[:, i] = acc.astype(np.float32)
    return out
