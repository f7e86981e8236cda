"""numpy restatement of fMLLR (constrained MLLR, Gales 1998) as include/srgpu.h states it: the per-speaker statistics from
(features, model tables, pairs), the auxiliary function Q(W), the row update and the transform loop.  Plain FP64 sums; beside
every sum the same sum over absolute values, which is what the tests' rounding bounds are multiples of."""
import numpy as np


def random_model(rng, S, M, D, ragged=True):
    """-> (dens_off u32[S+1], means [C, D], inv_vars [C, D], norm [C], logw [C]): S mixtures of 1..M densities"""
    n = rng.integers(1, M + 1, size=S) if ragged else np.full(S, M)
    dens_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    C = int(dens_off[-1])
    means = rng.normal(0.0, 2.0, size=(C, D))
    var = rng.uniform(0.5, 2.0, size=(C, D))
    inv_vars = 1.0 / var
    norm = 0.5 * (D * np.log(2 * np.pi) + np.log(var).sum(axis=1))
    logw = np.concatenate([np.log(w / w.sum()) for w in (rng.uniform(0.5, 1.5, size=k) for k in n)])
    return dens_off, means, inv_vars, norm, logw


def density_scores(x, model, s):
    """the costs of mixture s' densities for the float frame x: norm + dist / 2 - logw, two partial sums like the kernels"""
    dens_off, means, inv_vars, norm, logw = model
    c0, c1 = int(dens_off[s]), int(dens_off[s + 1])
    D = len(x)
    p = ((x.astype(np.float64) - means[c0:c1]) ** 2) * inv_vars[c0:c1]
    D2 = D - (D & 1)
    l0 = np.zeros(c1 - c0)
    l1 = np.zeros(c1 - c0)
    for d in range(0, D2, 2):
        l0 = l0 + p[:, d]
        l1 = l1 + p[:, d + 1]
    dist = l0 + l1
    if D & 1:
        dist = dist + p[:, D - 1]
    return norm[c0:c1] + dist / 2 - logw[c0:c1]


def mixture_pairs(x, model, s, max_approx):
    """the (density, membership) pairs of frame x in mixture s: the arg-min at 1, or the soft memberships with the < 1e-8 drop"""
    c0 = int(model[0][s])
    sc = density_scores(x, model, s)
    if len(sc) == 0:
        return []
    if max_approx:
        return [(c0 + int(np.argmin(sc)), 1.0)]
    p = np.exp(-sc)
    tot = 0.0
    for v in p:
        tot += v
    p = p / tot
    return [(c0 + j, float(v)) for j, v in enumerate(p) if not v < 1e-8]


def alignment_pairs(feats, model, states, max_approx):
    """-> list of (frame, density, weight) in frame order"""
    out = []
    for t, s in enumerate(states):
        out += [(t, d, w) for d, w in mixture_pairs(feats[t], model, int(s), max_approx)]
    return out


def posterior_pairs(feats, model, count, state, weight, max_approx):
    """pairs of per-frame posterior items (count[t] items (state[t, j], weight[t, j])), mixtures in ascending id"""
    out = []
    for t in range(len(feats)):
        items = sorted(zip(state[t, :int(count[t])].tolist(), weight[t, :int(count[t])].tolist()))
        for s, g in items:
            out += [(t, d, g * w) for d, w in mixture_pairs(feats[t], model, int(s), max_approx)]
    return out


def statistics(feats, model, pairs, frame_off, utt_speaker, n_speakers):
    """-> (beta [S], k [S, D, E], G [S, D, E, E]), the same sums over absolute values (kabs, Gabs), pairs per speaker n [S]"""
    _, means, inv_vars, _, _ = model
    F, D = feats.shape
    E = D + 1
    xi = np.concatenate([feats.astype(np.float64), np.ones((F, 1))], axis=1)
    spk_of = np.zeros(F, dtype=np.int64)
    for u, s in enumerate(utt_speaker):
        spk_of[int(frame_off[u]):int(frame_off[u + 1])] = int(s)
    a = np.zeros((F, D)); c = np.zeros((F, D)); cabs = np.zeros((F, D)); g = np.zeros(F)
    n = np.zeros(n_speakers, dtype=np.int64)
    for t, d, w in pairs:
        a[t] += w * inv_vars[d]
        c[t] += w * inv_vars[d] * means[d]
        cabs[t] += abs(w) * inv_vars[d] * np.abs(means[d])
        g[t] += w
        n[spk_of[t]] += 1
    beta = np.zeros(n_speakers); k = np.zeros((n_speakers, D, E)); G = np.zeros((n_speakers, D, E, E))
    kabs = np.zeros_like(k); Gabs = np.zeros_like(G)
    for s in range(n_speakers):
        sel = spk_of == s
        if not sel.any():
            continue
        x, ax = xi[sel], np.abs(xi[sel])
        beta[s] = g[sel].sum()
        k[s] = c[sel].T @ x
        kabs[s] = cabs[sel].T @ ax
        G[s] = np.einsum("ti,tj,tk->ijk", a[sel], x, x, optimize=True)
        Gabs[s] = np.einsum("ti,tj,tk->ijk", np.abs(a[sel]), ax, ax, optimize=True)
    return beta, k, G, kabs, Gabs, n


def aux(beta, k, G, W):
    """Q(W) = beta log|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T) of one speaker -> (Q, sum of the absolute values of its terms)"""
    D = W.shape[0]
    _, logdet = np.linalg.slogdet(W[:, :D])
    q = beta * logdet
    mag = abs(beta * logdet)
    for i in range(D):
        w = W[i]
        q += -0.5 * (w @ G[i] @ w) + w @ k[i]
        mag += 0.5 * (np.abs(w) @ np.abs(G[i]) @ np.abs(w)) + np.abs(w) @ np.abs(k[i])
    return q, mag


def cofactor_row(A, i):
    return np.linalg.det(A) * np.linalg.inv(A)[:, i]


def row_gradient(beta, k, G, W, i):
    """dQ/dw_i = beta p_i / (p_i . w_i) - w_i G_i + k_i -> (gradient, ||w_i G_i|| + ||k_i||)"""
    D = W.shape[0]
    p = np.concatenate([cofactor_row(W[:, :D], i), [0.0]])
    wg = W[i] @ G[i]
    return beta * p / (p @ W[i]) - wg + k[i], np.linalg.norm(wg) + np.linalg.norm(k[i])


def row_update(beta, k, G, W, i):
    """Gales' update of row i in place"""
    D = W.shape[0]
    p = np.concatenate([cofactor_row(W[:, :D], i), [0.0]])
    Gi = np.linalg.inv(G[i])
    a, b = p @ Gi @ p, p @ Gi @ k[i]
    best = None
    for sign in (1.0, -1.0):
        alpha = (-b + sign * np.sqrt(b * b + 4 * a * beta)) / (2 * a)
        w = (alpha * p + k[i]) @ Gi
        f = beta * np.log(abs(alpha * a + b)) - 0.5 * (w @ G[i] @ w) + w @ k[i]
        if best is None or f > best[0]:
            best = (f, w)
    W[i] = best[1]


def estimate(beta, k, G, n_sweeps, W=None):
    D = k.shape[0]
    W = np.hstack([np.eye(D), np.zeros((D, 1))]) if W is None else W.copy()
    for _ in range(n_sweeps):
        for i in range(D):
            row_update(beta, k, G, W, i)
    return W


def transform(feats, frame_off, utt_speaker, W):
    """y_ti = (float)(b_i + sum_j A_ij (double) x_tj), j ascending, one addition after the other"""
    F, D = feats.shape
    out = np.empty_like(feats)
    for u, s in enumerate(utt_speaker):
        f0, f1 = int(frame_off[u]), int(frame_off[u + 1])
        x = feats[f0:f1].astype(np.float64)
        acc = np.tile(W[s][:, D], (f1 - f0, 1))
        for j in range(D):
            acc = acc + W[s][:, j][None, :] * x[:, j][:, None]
        out[f0:f1] = acc.astype(np.float32)
    return out
