"""sMBR over the bigram-LM search network, restated in numpy (log space for the costs, linear for the accuracies, FP64): the reference
the bigram sMBR tests hold sr_bigram_accuracies_corpus / sr_bigram_smbr_statistics_corpus against.

The network, its penalties and its start are tests/bigram_fb_reference.py's (Net, every history kept, no beams, every cost times
kappa).  A path pi of probability P(pi) = exp(-kappa cost(pi)) / sum scores A(pi) = the number of frames at which the mixture of the
position it occupies is the reference's.  An entry emits the mixture of the state it moves TO, so every source of a position scores
the same [state(s) == ref_t].  Beside alpha and beta run

  abar_t(s)  the expected accuracy of frames 0 .. t over the paths reaching s at t
  bbar_t(s)  the expected accuracy of frames t + 1 .. over the continuations of s at t

both as posterior-weighted means of their sources (_wmean).  Abar = the mean over the word ends after the last frame, and

  gamma_t(k) = sum over the positions s carrying k of occ_t(s) (abar_t(s) + bbar_t(s) - Abar)
             = occ_t(k) (c_t(k) - Abar) = -(1 / kappa) d Abar / d e(t, k).

Nothing here multiplies probabilities across words in the linear domain: the word entry is a weighted mean per word over the
histories' costs in log space, the independent statement of what the device computes as two matrix products."""
from __future__ import annotations

import numpy as np

from tests import bigram_fb_reference as R

INF = np.inf


def _wmean(xs, vals, axis=0):
    """-> (-log sum exp(-x), the mean of vals weighted with exp(-x)) along axis; (+inf, 0) where no x is finite"""
    xs = R._arr(xs)
    dt = xs.dtype.type
    vals = np.broadcast_to(np.asarray(vals).astype(xs.dtype), xs.shape)
    if xs.shape[axis] == 0:
        shape = np.delete(xs.shape, axis)
        return np.full(shape, INF, dtype=xs.dtype)[()], np.zeros(shape, dtype=xs.dtype)[()]
    m = xs.min(axis=axis, keepdims=True)
    ok = np.isfinite(m)
    ms = np.where(ok, m, dt(0.0))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w = np.where(np.isfinite(xs), np.exp(ms - xs), dt(0.0))
        s = w.sum(axis=axis, keepdims=True)
        s1 = np.where(ok, s, dt(1.0))
        cost = np.where(ok, ms - np.log(s1), dt(INF))
        acc = np.where(ok, (w * np.where(np.isfinite(xs), vals, dt(0.0))).sum(axis=axis, keepdims=True) / s1, dt(0.0))
    return np.squeeze(cost, axis)[()], np.squeeze(acc, axis)[()]


def _entry_mean(vec, vals, klm, axis):
    """the W x W weighted mean of the word entry: over the histories (axis 1: vec = their costs) or over the words (axis 0), in log
    space"""
    return _wmean((vec[None, :] if axis == 1 else vec[:, None]) + klm, vals[None, :] if axis == 1 else vals[:, None], axis=axis)


def _shift(v, j, fill):
    out = np.full_like(v, fill)
    if j == 0:
        return v.copy()
    if j > 0:
        out[j:] = v[:-j]
    else:
        out[:j] = v[-j:]
    return out


def smbr(e, net, lm, tdp, ref, scale=1.0, shift=0.0, dtype=np.float64, entry_sum=None):
    """e [T, S] emission costs, net a bigram_fb_reference.Net, lm [W, W] (lm[w, h]; NaN / +inf: forbidden), tdp [2][4], ref [T]
    reference mixtures (>= S: none) -> (F, Abar, gamma [T, S]); T = 0: F = 0; T = 0 or F = +inf: Abar = 0, gamma = 0.
    shift: every frame of every path scores that much more.  Abar (returned without it) and gamma do not depend on it in exact
    arithmetic; in FP64 the difference between two shifts shows this restatement's own rounding error.
    dtype as bigram_fb_reference's.  entry_sum(vec, values, klm, axis) -> (cost, mean) replaces the W x W weighted mean of the word
    entry, as bigram_fb_reference's entry_sum does the sum (tests: the linear-domain evaluation and the underflow cut)."""
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    T, S = e.shape
    W, P, sil = net.W, net.P, net.sil
    ref = np.asarray(ref, dtype=np.int64)
    gamma = np.zeros((T, S), dtype=dtype)
    if T == 0:
        return dtype(0.0), dtype(0.0), gamma
    klm, td = R._klm(net, lm, scale, dtype), R._tdp(tdp, scale, dtype)
    scale, shift = dtype(scale), dtype(shift)
    wsum = entry_sum or _entry_mean
    pt = td[net.is_sil]  # [P, 4]
    hit = lambda t: (net.state == ref[t]).astype(dtype) + shift  # noqa: E731
    k, n = net.k, net.n
    is_last = k == n - 1
    two = (net.slot_off[1:] - net.slot_off[:-1]) >= 2

    A, Aa = np.full((T, P), INF, dtype=dtype), np.zeros((T, P), dtype=dtype)
    we, wea = R.start_ends(net, dtype), np.zeros(2 * W, dtype=dtype)
    prev, preva = np.full(P, INF, dtype=dtype), np.zeros(P, dtype=dtype)
    for t in range(T):
        # histories and entries: word w from every history through the LM, the copy h + W from word h's end, silence from its own
        hist, hista = _wmean([we[:W], we[W:]], [wea[:W], wea[W:]])
        hist[sil], hista[sil] = we[sil], wea[sil]
        ent, enta = np.full(2 * W, INF, dtype=dtype), np.zeros(2 * W, dtype=dtype)
        ent[:W], enta[:W] = wsum(hist, hista, klm, 1)
        ent[W:], enta[W:] = we[:W], wea[:W]
        ent[sil], enta[sil] = we[sil], wea[sil]
        ent[sil + W], enta[sil + W] = INF, 0.0
        zero = dtype(0.0)
        ep, epa = ent[net.slot], enta[net.slot]
        xs = [prev + pt[:, 0],
              np.where(k >= 1, _shift(prev, 1, INF) + pt[:, 1], INF),
              np.where(k >= 2, _shift(prev, 2, INF) + pt[:, 2], INF),
              np.where(k == 0, ep, INF),
              np.where(k == 1, ep + pt[:, 2], INF)]
        vs = [preva, _shift(preva, 1, 0.0), _shift(preva, 2, 0.0), epa, epa]
        cur, cura = _wmean(np.where(np.isnan(xs), dtype(INF), xs), vs)
        ok = np.isfinite(cur)
        cur = np.where(ok, cur + scale * e[t, net.state], dtype(INF))
        cura = np.where(ok, cura + hit(t), zero)
        A[t], Aa[t] = cur, cura
        we, wea = cur[net.last] + td[net.slot_sil, 3], cura[net.last]
        prev, preva = cur, cura
    kF, Abar = _wmean(we, wea)
    if not np.isfinite(kF):
        return dtype(INF), dtype(0.0), gamma

    zero = dtype(0.0)
    B, Bb = np.full(P, INF, dtype=dtype), np.zeros(P, dtype=dtype)
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            cur, cura = np.where(is_last, pt[:, 3], dtype(INF)), np.zeros(P, dtype=dtype)
        else:
            x = scale * e[t + 1, net.state] + B          # the successor's emission and beta
            xa = np.where(np.isfinite(x), hit(t + 1) + Bb, zero)   # the accuracy of frames t + 1 ..
            f1 = np.minimum(net.first + 1, P - 1)
            bent, benta = _wmean([x[net.first], np.where(two, td[net.slot_sil, 2] + x[f1], INF)], [xa[net.first], xa[f1]])
            Y, Ya = wsum(bent[:W], benta[:W], klm, 0)  # [h]: into every word through the LM
            Rc, Ra = np.empty(2 * W, dtype=dtype), np.empty(2 * W, dtype=dtype)
            Rc[:W], Ra[:W] = _wmean([Y, bent[W:]], [Ya, benta[W:]])
            Rc[sil], Ra[sil] = _wmean([Y[sil], bent[sil]], [Ya[sil], benta[sil]])
            Rc[W:], Ra[W:] = Y, Ya
            xs = [pt[:, 0] + x,
                  np.where(k + 1 < n, _shift(pt[:, 1] + x, -1, INF), INF),
                  np.where(k + 2 < n, _shift(pt[:, 2] + x, -2, INF), INF),
                  np.where(is_last, pt[:, 3] + Rc[net.slot], INF)]
            vs = [xa, _shift(xa, -1, 0.0), _shift(xa, -2, 0.0), Ra[net.slot]]
            cur, cura = _wmean(np.where(np.isnan(xs), dtype(INF), xs), vs)
        B, Bb = cur, cura
        y = A[t] + B
        ok = np.isfinite(y)
        with np.errstate(invalid="ignore", over="ignore"):
            g = np.where(ok, np.exp(kF - np.where(ok, y, zero)) * (Aa[t] + Bb - Abar), zero)
        gamma[t] = R.collect(g[None, :], net.state, S)[0, :S]
    return kF / scale, dtype(Abar) - T * shift, gamma
