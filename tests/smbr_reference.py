"""sMBR over the recognition network, restated in numpy (log space for the costs, linear for the accuracies, FP64): the reference the
sMBR tests hold sr_net_accuracies_corpus / sr_smbr_statistics_corpus against.

The network, its penalties and its start hypothesis are tests/mmi_reference.py's free graph.  A path pi of probability
P(pi) = exp(-kappa cost(pi)) / sum scores A(pi) = the number of frames whose emission is the reference's mixture (an entry into
position 1 of a word emits, and is scored as, the word's FIRST state).  Beside alpha and beta run

  abar_t(s)  the expected accuracy of frames 0 .. t over the paths reaching s at t
  bbar_t(s)  the expected accuracy of frames t + 1 .. over the continuations of s at t

both as posterior-weighted means of their sources.  Abar = the mean of abar_{T-1} over the final slots, and

  gamma_t(k) = sum over the occupancy parts of (t, k) of part * (c_part - Abar),   c_part = abar-side + [k == ref_t] + bbar-side
             = occ_t(k) (c_t(k) - Abar) = -(1 / kappa) d Abar / d e(t, k).

smbr() takes a `dtype` as net_fb_reference's recursions do (np.longdouble: the yardstick of tests/test_gpu_smbr_scores.py)."""
from __future__ import annotations

import numpy as np

from tests import mmi_reference as M

INF = np.inf


def _wmean(xs, vals, dtype=np.float64):
    """-> (-log sum exp(-x), the mean of vals weighted with exp(-x)); (+inf, 0) without a finite x"""
    xs, vals = np.asarray(xs, dtype=dtype), np.asarray(vals, dtype=dtype)
    ok = np.isfinite(xs)
    if not ok.any():
        return INF, 0.0
    m = xs[ok].min()
    w = np.exp(m - xs[ok])
    return m - np.log(w.sum()), dtype((w * vals[ok]).sum() / w.sum())


def smbr(e, gr, tdp, wp, ref, scale=1.0, dtype=np.float64):
    """e [T, S] emission costs, gr a mmi_reference.Graph, ref [T] reference mixtures (>= S: none)
    -> (F, Abar, gamma [T, S]); F = +inf (or T = 0): Abar = 0, gamma = 0"""
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    T, S = e.shape
    P = gr.P
    ref = np.asarray(ref, dtype=np.int64)
    gamma = np.zeros((T, S), dtype=dtype)
    if T == 0:
        return INF, 0.0, gamma
    into, ent = M._penalties(gr, tdp, wp, scale, dtype)
    scale = dtype(scale)
    wm = lambda xs, vals: _wmean(xs, vals, dtype)
    hit = lambda k, t: 1.0 if k == ref[t] else 0.0
    G = len(gr.src)
    # rows 1 .. T are the frames, row 0 the virtual row
    A, Aa = np.full((T + 1, P), INF, dtype=dtype), np.zeros((T + 1, P), dtype=dtype)
    A[0, 0] = 0.0
    Es, Ea = np.full((T + 1, G), INF, dtype=dtype), np.zeros((T + 1, G), dtype=dtype)
    inw, inwa = np.full((T + 1, P), INF, dtype=dtype), np.zeros((T + 1, P), dtype=dtype)
    for t in range(1, T + 1):
        em = scale * e[t - 1]
        cache = {}
        for g, srcs in enumerate(gr.src):
            if srcs not in cache:
                cache[srcs] = wm(A[t - 1, list(srcs)], Aa[t - 1, list(srcs)])
            Es[t - 1, g], Ea[t - 1, g] = cache[srcs]
        for s in range(P):
            xs, vs = [], []
            for j in range(3):
                if gr.pos[s] >= j and not (j == 0 and gr.end[s]):
                    xs.append(A[t - 1, s - j] + into[j, s])
                    vs.append(Aa[t - 1, s - j])
            inw[t, s], inwa[t, s] = wm(xs, vs)
            k = gr.state[s]
            xs, vs = [inw[t, s] + em[k]], [inwa[t, s] + hit(k, t - 1)]
            if gr.pos[s] <= 1:
                kf = k if gr.pos[s] == 0 else gr.first[s]
                xs.append(Es[t - 1, gr.seg[s]] + ent[s] + em[kf])
                vs.append(Ea[t - 1, gr.seg[s]] + hit(kf, t - 1))
            A[t, s], Aa[t, s] = wm(xs, vs)
    F, Abar = wm(A[T, gr.final], Aa[T, gr.final])
    if not np.isfinite(F):
        return INF, 0.0, gamma
    B, Bb = np.full((T + 1, P), INF, dtype=dtype), np.zeros((T + 1, P), dtype=dtype)
    B[T, gr.final] = 0.0
    for t in range(T, 0, -1):
        em = scale * e[t - 1]
        if t < T:
            en = scale * e[t]
            X = []  # the entries into segment g at frame t + 1 (row t + 1 of B): (cost, accuracy of frames t + 1 ..)
            for g in range(G):
                b = gr.beg[g]
                k = gr.state[b]
                xs, vs = [ent[b] + en[k] + B[t + 1, b]], [Bb[t + 1, b] + hit(k, t)]
                if not gr.end[b]:
                    xs.append(ent[b + 1] + en[k] + B[t + 1, b + 1])
                    vs.append(Bb[t + 1, b + 1] + hit(k, t))
                X.append(wm(xs, vs))
            cache = {}
            for s in range(P):
                if gr.end[s]:
                    key = tuple(gr.dst[gr.seg[s]])
                    if key not in cache:
                        cache[key] = wm([X[g][0] for g in key], [X[g][1] for g in key])
                    B[t, s], Bb[t, s] = cache[key]
                else:
                    xs, vs = [], []
                    for j in range(3):
                        if j == 2 and gr.end[s + 1]:
                            break
                        k = gr.state[s + j]
                        xs.append(into[j, s + j] + en[k] + B[t + 1, s + j])
                        vs.append(Bb[t + 1, s + j] + hit(k, t))
                    B[t, s], Bb[t, s] = wm(xs, vs)
        for s in range(P):
            if not np.isfinite(B[t, s]):
                continue
            k = gr.state[s]
            own = inw[t, s] + em[k] + B[t, s]
            if np.isfinite(own):
                gamma[t - 1, k] += np.exp(F - own) * (inwa[t, s] + hit(k, t - 1) + Bb[t, s] - Abar)
            if gr.pos[s] <= 1:
                kf = k if gr.pos[s] == 0 else gr.first[s]
                x = Es[t - 1, gr.seg[s]] + ent[s] + em[kf] + B[t, s]
                if np.isfinite(x):
                    gamma[t - 1, kf] += np.exp(F - x) * (Ea[t - 1, gr.seg[s]] + hit(kf, t - 1) + Bb[t, s] - Abar)
    return F / scale, Abar, gamma


def signed_items(gamma, sign, floor=0.0):
    """per frame [(mixture, sign * gamma)] with sign * gamma > 0 and >= floor, ascending mixture id (mmi_reference.frame_items' shape)"""
    g = sign * np.asarray(gamma)
    return [[(int(k), float(row[k])) for k in np.flatnonzero((row > 0) & (row >= floor))] for row in g]
