"""numpy restatement of MLLR mean adaptation as include/srgpu.h states it: the per-(speaker, regression class) statistics from
(features, model tables, pairs), the auxiliary function Q(W), the closed-form estimate over a regression-class tree and the mean
transform loop.  The statistics are summed in numpy.longdouble (64-bit significands: their own error is 2^-11 of an FP64 rounding
per term, negligible beside the tests' bounds); beside every sum the same sum over absolute values, which is what the bounds are
multiples of.  The pairs come from tests/fmllr_reference.py (alignment_pairs, posterior_pairs): MLLR takes exactly fMLLR's."""
import numpy as np

LD = np.longdouble


def identity(D, *lead):
    return np.tile(np.hstack([np.eye(D), np.zeros((D, 1))]), tuple(lead) + (1, 1))


def entries(feats, pairs, frame_off, utt_speaker):
    """-> {(speaker, density): [occ, x_acc [D], |x|_acc [D], n_pairs]} in longdouble, a key's pairs in the order given"""
    F, D = feats.shape
    spk_of = np.zeros(F, dtype=np.int64)
    for u, s in enumerate(utt_speaker):
        spk_of[int(frame_off[u]):int(frame_off[u + 1])] = int(s)
    out = {}
    for t, d, w in pairs:
        e = out.setdefault((int(spk_of[t]), int(d)), [LD(0), np.zeros(D, LD), np.zeros(D, LD), 0])
        x = feats[t].astype(LD)
        e[0] += LD(w)
        e[1] += LD(w) * x
        e[2] += LD(abs(w)) * np.abs(x)
        e[3] += 1
    return out


def statistics(feats, model, pairs, frame_off, utt_speaker, n_speakers, dens_class, n_classes):
    """-> (beta [S, R], k [S, R, D, E], G [S, R, D, E, E]) rounded to FP64 from longdouble sums, the same sums over absolute values
    (kabs, Gabs), n [S, R] = the group's pairs + entries, n_entries [S, R]"""
    _, means, inv_vars, _, _ = model
    D = feats.shape[1]
    E = D + 1
    S, R = n_speakers, n_classes
    ent = entries(feats, pairs, frame_off, utt_speaker)
    beta = np.zeros((S, R), LD); k = np.zeros((S, R, D, E), LD); G = np.zeros((S, R, D, E, E), LD)
    kabs = np.zeros_like(k); Gabs = np.zeros_like(G)
    n = np.zeros((S, R), dtype=np.int64); n_ent = np.zeros((S, R), dtype=np.int64)
    for (s, d) in sorted(ent):
        occ, x, xa, cnt = ent[(s, d)]
        r = int(dens_class[d])
        iv = inv_vars[d].astype(LD)
        xi = np.concatenate([means[d], [1.0]]).astype(LD)
        outer = np.outer(xi, xi)
        beta[s, r] += occ
        k[s, r] += np.outer(iv * x, xi)
        kabs[s, r] += np.outer(iv * xa, np.abs(xi))
        G[s, r] += (occ * iv)[:, None, None] * outer[None]
        Gabs[s, r] += (abs(occ) * iv)[:, None, None] * np.abs(outer)[None]
        n[s, r] += cnt + 1
        n_ent[s, r] += 1
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    return f64(beta), f64(k), f64(G), f64(kabs), f64(Gabs), n, n_ent


def aux(k, G, W):
    """Q(W) = -1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T) of one node -> (Q, sum of the absolute values of its terms)"""
    q, mag = 0.0, 0.0
    for i in range(W.shape[0]):
        w = W[i]
        q += -0.5 * (w @ G[i] @ w) + w @ k[i]
        mag += 0.5 * (np.abs(w) @ np.abs(G[i]) @ np.abs(w)) + np.abs(w) @ np.abs(k[i])
    return q, mag


def solve(k, G):
    """w_i = k_i G_i^-1 per row, numpy's LU"""
    return np.stack([np.linalg.solve(G[i], k[i]) for i in range(k.shape[0])])


def node_statistics(beta, k, G, parent, v):
    """the statistics of node v of one speaker (beta [R], k [R, D, E], G [R, D, E, E]): the sum over its leaves, ascending"""
    R = len(beta)
    if v < R:
        return beta[v], k[v], G[v]
    b, kk, GG = 0.0, np.zeros_like(k[0]), np.zeros_like(G[0])
    for r in range(R):
        a = int(parent[r])
        while a != -1 and a != v:
            a = int(parent[a])
        if a == v:
            b, kk, GG = b + beta[r], kk + k[r], GG + G[r]
    return b, kk, GG


def transform_means(means, dens_class, W):
    """mu'_di = acc, acc from b_i taking acc = acc + A_ij * mu_dj for j ascending, one operation after the other"""
    C, D = means.shape
    cls = np.asarray(dens_class, dtype=np.int64)
    acc = W[cls][:, :, D].copy()
    for j in range(D):
        acc = acc + W[cls][:, :, j] * means[:, j][:, None]
    return acc
