"""Forward-backward over the aligner's automata, restated in numpy (log space, FP64, np.logaddexp): the reference the Baum-Welch
tests hold sr_state_posteriors_corpus / sr_baum_welch_corpus against.  Emission costs come in as a dense [T, S] table -- from
pyoracle.Oracle.score_matrix, so the reference never touches the GPU.

Topology (align_full's): s_0 = 0, s_{T-1} = N-1, s_t - s_{t-1} in {0, 1, 2}; the transition penalty is keyed on the SOURCE
position's state, and any jump out of silence costs `forward`.  With semiring="min" the same recursion is the Viterbi
alignment (ties: loop before forward before skip, as the aligner's strict `<`).

The recursions take a `dtype` (default float64, the kernels' own precision): with np.longdouble (x87: 64 bits of mantissa) the same
recursion is the yardstick the float64 one, and the kernels, are measured against (tests/test_gpu_fb_scores.py)."""
from __future__ import annotations

import numpy as np

INF = np.inf


def _jump_costs(ref, tdp, sil, dtype=np.float64):
    """c[j, s]: penalty of jump j out of position s."""
    ref = np.asarray(ref)
    c = np.empty((3, len(ref)), dtype=dtype)
    for j in range(3):
        c[j] = tdp[j]
    c[:, ref == sil] = tdp[1]
    return c


def _shift(v, j):
    """out[s] = v[s - j] (INF where s < j)."""
    if j == 0:
        return v
    out = np.full_like(v, INF)
    out[j:] = v[:-j]
    return out


def _ladd(*xs):
    """-log sum exp(-x)."""
    acc = -xs[0]
    for x in xs[1:]:
        acc = np.logaddexp(acc, -x)
    return -acc


def forward(e, ref, tdp, sil, semiring="log", dtype=np.float64):
    """alpha [T, N] (and, for semiring="min", the taken jumps [T, N])."""
    E = np.asarray(e)[:, np.asarray(ref, dtype=np.int64)].astype(dtype)
    T, N = E.shape
    c = _jump_costs(ref, tdp, sil, dtype)
    A = np.full((T, N), INF, dtype=dtype)
    bp = np.zeros((T, N), dtype=np.int64)
    A[0, 0] = E[0, 0]
    for t in range(1, T):
        cand = [_shift(A[t - 1] + c[j], j) for j in range(3)]
        if semiring == "min":
            st = np.stack(cand)
            bp[t] = np.argmin(st, axis=0)
            A[t] = E[t] + st.min(axis=0)
        else:
            A[t] = E[t] + _ladd(*cand)
    return (A, bp) if semiring == "min" else A


def viterbi(e, ref, tdp, sil):
    """-> (state per frame, cost) -- align_full's result for T >= 2."""
    A, bp = forward(e, ref, tdp, sil, "min")
    T, N = A.shape
    ref = np.asarray(ref)
    out = np.zeros(T, dtype=np.uint16)
    s = N - 1
    for t in range(T - 1, -1, -1):
        out[t] = ref[s]
        if t > 0:
            s -= int(bp[t, s])
    return out, float(A[T - 1, N - 1])


def backward(e, ref, tdp, sil, dtype=np.float64):
    E = np.asarray(e)[:, np.asarray(ref, dtype=np.int64)].astype(dtype)
    T, N = E.shape
    c = _jump_costs(ref, tdp, sil, dtype)
    B = np.full((T, N), INF, dtype=dtype)
    B[T - 1, N - 1] = 0.0
    for t in range(T - 2, -1, -1):
        nxt = E[t + 1] + B[t + 1]
        cand = []
        for j in range(3):
            v = np.full(N, INF, dtype=dtype)
            if j < N:
                v[: N - j] = nxt[j:]
            cand.append(c[j] + v)
        B[t] = _ladd(*cand)
    return B


def posteriors(e, ref, tdp, sil, dtype=np.float64):
    """-> (F = -log P(X | automaton), gamma [T, N] per position); F a Python float for float64, else a scalar of dtype."""
    A = forward(e, ref, tdp, sil, dtype=dtype)
    B = backward(e, ref, tdp, sil, dtype=dtype)
    T, N = A.shape
    F = float(A[T - 1, N - 1]) if dtype is np.float64 else A[T - 1, N - 1]
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.exp(F - (A + B)) if np.isfinite(F) else np.zeros_like(A)
    g[~np.isfinite(A + B)] = 0.0
    return F, g


def mixture_posteriors(gamma, ref):
    """-> (mixtures ascending, [T, M] posterior per distinct mixture of the automaton)."""
    ref = np.asarray(ref, dtype=np.int64)
    mix = np.unique(ref)
    out = np.zeros((gamma.shape[0], len(mix)), dtype=gamma.dtype)
    for j, k in enumerate(mix):
        out[:, j] = gamma[:, ref == k].sum(axis=1)
    return mix, out


def items(mix, gm, floor):
    """per frame [(mixture, gamma)] with gamma > 0 and >= floor, ascending mixture id"""
    return [[(int(mix[j]), float(gm[t, j])) for j in range(len(mix)) if gm[t, j] > 0 and gm[t, j] >= floor] for t in range(gm.shape[0])]


def top_items(frame_items, max_items):
    """largest first, ties: smaller id first, at most max_items"""
    return [sorted(it, key=lambda kv: (-kv[1], kv[0]))[:max_items] for it in frame_items]


def n_paths(T, N):
    """number of 0-1-2 paths from position 0 at frame 0 to position N-1 at frame T-1 (a Python int)"""
    cnt = [0] * N
    cnt[0] = 1
    for _ in range(1, T):
        cnt = [cnt[s] + (cnt[s - 1] if s > 0 else 0) + (cnt[s - 2] if s > 1 else 0) for s in range(N)]
    return cnt[N - 1]


def density_scores(x, tables, dens):
    """-log(weight * N(x)) of densities `dens` (norm + dist / 2 - log weight; pyoracle.Oracle.tables() layout)"""
    mi, vi = tables["mix_mean"][dens], tables["mix_var"][dens]
    d = (x[None, :].astype(np.float64) - tables["means"][mi]) ** 2 * tables["vars_inv"][vi]
    return tables["norm"][vi] + d.sum(axis=1) / 2 - tables["logw"][mi]


def accumulate(feats, frame_items, tables, n_mean, n_var, first_pass=False, max_approx=False):
    """The Baum-Welch statistics of per-frame items: w = gamma * p_d as sr_baum_welch_corpus defines it.
    -> (mean_acc, mean_w, var_acc, var_w, scale_mean, scale_var): the scales are sum |w x| and sum w x^2 per row element (for a
    relative tolerance that survives cancellation)."""
    D = feats.shape[1]
    off = tables["mix_off"]
    ma, mw, va, vw = np.zeros((n_mean, D)), np.zeros(n_mean), np.full((n_var, D), 1e-4), np.zeros(n_var)
    sm, sv = np.zeros((n_mean, D)), np.zeros((n_var, D))
    for t, it in enumerate(frame_items):
        x = feats[t].astype(np.float64)
        for k, g in it:
            dens = np.arange(off[k], off[k + 1])
            if len(dens) == 0:
                continue
            if first_pass:
                ws = [(dens[0], g)]
            elif max_approx:
                ws = [(int(dens[np.argmin(density_scores(feats[t], tables, dens))]), g)]
            else:
                sc = density_scores(feats[t], tables, dens)
                p = np.exp(-sc)
                p = p / p.sum()
                ws = [(d, g * pd) for d, pd in zip(dens, p) if not pd < 1e-8]
            for d, w in ws:
                r, q = tables["mix_mean"][d], tables["mix_var"][d]
                ma[r] += w * x
                mw[r] += w
                sm[r] += np.abs(w * x)
                va[q] += (w * x) * x
                vw[q] += w
                sv[q] += (w * x) * x
    return ma, mw, va, vw, sm, sv
