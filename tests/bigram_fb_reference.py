"""Forward-backward over the bigram-LM search network, restated in numpy (log space, FP64): the reference the bigram word-posterior
tests hold sr_bigram_word_posteriors_corpus / sr_recognize_bigram_confidence_corpus against.  Emission costs come in as a dense
[T, S] table.

The network is the one orc_bigram_decode (oracle/sr_oracle.c) searches, every path summed, no beams, every cost times kappa:
  * slots 0 .. W-1 are the words, slot h + W the silence copy entered after word h != silence (the silence word's states, the
    silence penalties tdp[1]); positions = the slots' states back to back.
  * before frame 1 there is one word end: the silence word, cost 0.
  * a word end of slot x has history x (a word), h (the copy h + W) or silence (the silence word); the cost of a history is the
    sum (min) of its word ends -- the decoder's merge WITHOUT the positional cut of mergeSilenceToBigramNodes: every history is kept.
  * word w != silence is entered from every history h at hist_h + lm[w, h] (NaN = +inf: forbidden); the copy h + W from the word
    end of word h alone, the silence word from its own word end, both at no LM cost.
  * an entry moves to the word's first state at no penalty or to its second at the skip penalty; from a state the moves are to the
    same, the next and the one after at tdp[isSilence][0..2]; the destination's mixture is emitted; a word end is the last state
    plus tdp[isSilence][3].
F = -(1/kappa) log sum over the word ends after frame T of exp(-kappa cost); T = 0: F = 0.  Nothing here multiplies probabilities
in the linear domain: the entry is a log-sum-exp per word, the independent statement of what the device computes as a matrix
product.

forward, backward and posteriors take a `dtype` (default float64, the kernels' own precision): with np.longdouble (x87: 64 bits of
mantissa) the same recursion is the yardstick the float64 one, and the kernels, are measured against (tests/bigram_fb_cases.py)."""
from __future__ import annotations

import numpy as np

INF = np.inf


class Net:
    def __init__(self, word_off, mixtures, silence):
        word_off = np.asarray(word_off, dtype=np.int64)
        mixtures = np.asarray(mixtures, dtype=np.int64)
        self.W = W = len(word_off) - 1
        self.sil = int(silence)
        ac = np.concatenate([np.arange(W), np.full(W, self.sil)])  # acoustic word of every slot
        n = (word_off[1:] - word_off[:-1])[ac]
        self.slot_off = np.concatenate([[0], np.cumsum(n)])
        self.P = int(self.slot_off[-1])
        self.slot = np.repeat(np.arange(2 * W), n)
        self.k = np.arange(self.P) - self.slot_off[self.slot]
        self.n = n[self.slot]
        self.state = mixtures[word_off[ac[self.slot]] + self.k]
        self.is_sil = ((self.slot >= W) | (self.slot == self.sil)).astype(np.int64)
        self.first = self.slot_off[:-1]
        self.last = self.slot_off[1:] - 1
        self.slot_sil = ((np.arange(2 * W) >= W) | (np.arange(2 * W) == self.sil)).astype(np.int64)
        self.word = np.where(self.slot < W, self.slot, self.sil)  # the word a position's posterior counts for
        self.hist = np.where(np.arange(2 * W) < W, np.arange(2 * W), np.arange(2 * W) - W)  # (the silence word: itself)


def _arr(x):
    """x as an array: longdouble stays, everything else is float64"""
    x = np.asarray(x)
    return x if x.dtype == np.longdouble else x.astype(np.float64)


def _lsum(x, axis=None, semiring="log"):
    """-log sum exp(-x) (or the minimum); +inf where nothing is finite"""
    x = _arr(x)
    if axis is None:
        x, axis = x.reshape(-1), 0
    if x.shape[axis] == 0:
        return np.full(np.delete(x.shape, axis), INF, dtype=x.dtype)[()]
    m = x.min(axis=axis, keepdims=True)
    if semiring == "min":
        return np.squeeze(m, axis)[()]
    ms = np.where(np.isfinite(m), m, x.dtype.type(0.0))
    with np.errstate(divide="ignore", over="ignore"):
        s = np.exp(ms - x).sum(axis=axis, keepdims=True)
        out = np.where(np.isfinite(m), ms - np.log(s), INF)
    return np.squeeze(out, axis)[()]


def _comb(xs, semiring):
    return _lsum(np.stack([_arr(x) for x in xs]), axis=0, semiring=semiring)


def _shift(v, j):
    out = np.full_like(v, INF)
    if j == 0:
        return v.copy()
    if j > 0:
        out[j:] = v[:-j]
    else:
        out[:j] = v[-j:]
    return out


def _klm(net, lm, scale, dtype=np.float64):
    klm = dtype(scale) * np.asarray(lm, dtype=np.float64).astype(dtype)
    klm = np.where(np.isnan(klm), dtype(INF), klm)
    klm[net.sil, :] = INF  # no transition into silence through the LM
    return klm


def _tdp(tdp, scale, dtype=np.float64):
    return dtype(scale) * np.asarray(tdp, dtype=np.float64).reshape(2, 4).astype(dtype)


def histories(net, we, semiring="log"):
    """word-end costs [2W] -> cost per history [W]"""
    W = net.W
    h = _comb([we[:W], we[W:]], semiring)
    h[net.sil] = we[net.sil]
    return h


def _entry_sum(vec, klm, axis, semiring="log"):
    """the W x W sum of the word entry: over the histories (axis 1: vec = their costs) or over the words (axis 0: vec = their
    entry costs), in log space"""
    return _lsum((vec[None, :] if axis == 1 else vec[:, None]) + klm, axis=axis, semiring=semiring)


def entries(net, we, klm, semiring="log", entry_sum=None):
    """word-end costs [2W] after a frame -> entry costs [2W] of the next"""
    W = net.W
    ent = np.full(2 * W, INF, dtype=we.dtype)
    hist = histories(net, we, semiring)
    ent[:W] = entry_sum(hist, klm, 1) if entry_sum else _entry_sum(hist, klm, 1, semiring)
    ent[W:] = we[:W]
    ent[net.sil] = we[net.sil]
    ent[net.sil + W] = INF
    return ent


def start_ends(net, dtype=np.float64):
    we = np.full(2 * net.W, INF, dtype=dtype)
    we[net.sil] = 0.0
    return we


def forward(e, net, lm, tdp, semiring="log", scale=1.0, entry_sum=None, dtype=np.float64):
    """-> (alpha [T, P], WE [T + 1, 2W]): WE[t] = the word-end costs after frame t (row 0: the start), all times kappa.
    entry_sum(vec, klm, axis) replaces the log-space W x W sum (tests: a second, linear-domain evaluation to measure its spread)."""
    E = np.asarray(e, dtype=np.float64).astype(dtype)
    T = E.shape[0]
    klm, td = _klm(net, lm, scale, dtype), _tdp(tdp, scale, dtype)
    scale = dtype(scale)
    pt = td[net.is_sil]  # [P, 4]
    A = np.full((T, net.P), INF, dtype=dtype)
    WE = np.full((T + 1, 2 * net.W), INF, dtype=dtype)
    WE[0] = start_ends(net, dtype)
    prev = np.full(net.P, INF, dtype=dtype)
    for t in range(T):
        ent = entries(net, WE[t], klm, semiring, entry_sum)[net.slot]
        c0 = prev + pt[:, 0]
        c1 = np.where(net.k >= 1, _shift(prev, 1) + pt[:, 1], INF)
        c2 = np.where(net.k >= 2, _shift(prev, 2) + pt[:, 2], INF)
        e0 = np.where(net.k == 0, ent, INF)
        e1 = np.where(net.k == 1, ent + pt[:, 2], INF)
        cur = _comb([c0, c1, c2, e0, e1], semiring) + scale * E[t, net.state]
        cur = np.where(np.isnan(cur), INF, cur)
        A[t] = cur
        WE[t + 1] = cur[net.last] + td[net.slot_sil, 3]
        prev = cur
    return A, WE


def backward(e, net, lm, tdp, scale=1.0, semiring="log", entry_sum=None, dtype=np.float64):
    """beta [T, P]: the cost from after frame t at a position to a word end after frame T (scaled)."""
    E = np.asarray(e, dtype=np.float64).astype(dtype)
    T = E.shape[0]
    W = net.W
    klm, td = _klm(net, lm, scale, dtype), _tdp(tdp, scale, dtype)
    scale = dtype(scale)
    pt = td[net.is_sil]
    is_last = net.k == net.n - 1
    B = np.full((T, net.P), INF, dtype=dtype)
    if T == 0:
        return B
    B[T - 1] = np.where(is_last, pt[:, 3], INF)
    two = (net.slot_off[1:] - net.slot_off[:-1]) >= 2
    for t in range(T - 2, -1, -1):
        x = scale * E[t + 1, net.state] + B[t + 1]  # emission of the successor + its beta
        # entry into slot y before frame t + 1
        b2 = np.where(two, td[net.slot_sil, 2] + x[np.minimum(net.first + 1, net.P - 1)], INF)
        bent = _comb([x[net.first], b2], semiring)
        Y = entry_sum(bent[:W], klm, 0) if entry_sum else _entry_sum(bent[:W], klm, 0, semiring)  # [h]
        R = np.empty(2 * W, dtype=dtype)
        R[:W] = _comb([Y, bent[W:]], semiring)
        R[net.sil] = _comb([Y[net.sil], bent[net.sil]], semiring)
        R[W:] = Y
        s0 = pt[:, 0] + x
        s1 = np.where(net.k + 1 < net.n, _shift(pt[:, 1] + x, -1), INF)
        s2 = np.where(net.k + 2 < net.n, _shift(pt[:, 2] + x, -2), INF)
        ex = np.where(is_last, pt[:, 3] + R[net.slot], INF)
        cur = _comb([s0, s1, s2, ex], semiring)
        B[t] = np.where(np.isnan(cur), INF, cur)
    return B


def gammas(e, net, lm, tdp, scale=1.0, entry_sum=None, dtype=np.float64):
    """-> (kappa F, gamma [T, P]): the posterior of every position at every frame (0 where no path goes, all 0 for F = +inf)"""
    A, WE = forward(e, net, lm, tdp, "log", scale, entry_sum, dtype)
    T = A.shape[0]
    kF = _lsum(WE[T])
    if T == 0:
        return kF, np.zeros((0, net.P), dtype=dtype)
    Bt = backward(e, net, lm, tdp, scale, entry_sum=entry_sum, dtype=dtype)
    ok = np.isfinite(A) & np.isfinite(Bt) & np.isfinite(kF)
    zero = dtype(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        G = np.where(ok, np.exp(kF - np.where(ok, A + Bt, zero)), zero)
    return kF, G


def collect(G, index, n):
    """[T, P] -> [T, n]: the positions' values summed per index (np.bincount, which knows float64 only, in G's dtype)"""
    if G.dtype != np.longdouble:
        return np.stack([np.bincount(index, weights=g, minlength=n) for g in G]) if len(G) else np.zeros((0, n))
    out = np.zeros((G.shape[0], n), dtype=G.dtype)
    for t in range(G.shape[0]):
        np.add.at(out[t], index, G[t])
    return out


def posteriors(e, net, lm, tdp, scale=1.0, entry_sum=None, dtype=np.float64):
    """-> (F, word posteriors [T, W]); p[t, silence] sums the silence word and every copy."""
    kF, G = gammas(e, net, lm, tdp, scale, entry_sum, dtype)
    return kF / dtype(scale), collect(G, net.word, net.W)


def best_cost(e, net, lm, tdp):
    """min-semiring cost of the best path (kappa = 1) and the word-end lists WE [T + 1, 2W]"""
    _, WE = forward(e, net, lm, tdp, "min", 1.0)
    return float(WE[-1].min()), WE


def brute_force(e, net, lm, tdp, scale=1.0):
    """-> (F, word posteriors [T, W]) by enumerating every path (tiny T and lexica only)."""
    E = np.asarray(e, dtype=np.float64)
    T = E.shape[0]
    W = net.W
    klm, td = _klm(net, lm, scale), _tdp(tdp, scale)
    paths = []  # (cost, [word per frame])

    def enter(x, c, t, words):  # at state 0 of slot x before row t
        p0 = int(net.first[x])
        s = int(net.slot_sil[x])
        step(p0, c, t, words)
        if net.slot_off[x + 1] - p0 >= 2:
            step(p0 + 1, c + td[s, 2], t, words)

    def step(p, c, t, words):  # the path takes position p at row t
        if not np.isfinite(c):
            return
        c = c + scale * E[t, net.state[p]]
        words = words + [int(net.word[p])]
        x, s = int(net.slot[p]), int(net.is_sil[p])
        if p == net.last[x]:
            end(x, c + td[s, 3], t + 1, words)
        if t + 1 == T:
            return
        for j in range(3):
            if net.k[p] + j < net.n[p]:
                step(p + j, c + td[s, j], t + 1, words)

    def end(x, c, t, words):  # a word end of slot x after t frames
        if t == T:
            paths.append((c, words))
            return
        h = int(net.hist[x])
        for w in range(W):
            if w != net.sil and np.isfinite(klm[w, h]):
                enter(w, c + klm[w, h], t, words)
        if x == net.sil:
            enter(x, c, t, words)
        elif x < W:
            enter(x + W, c, t, words)

    end(net.sil, 0.0, 0, [])
    costs = np.array([c for c, _ in paths if np.isfinite(c)])
    p = np.zeros((T, W))
    if costs.size == 0:
        return INF, p
    kF = _lsum(costs)
    for c, words in paths:
        if np.isfinite(c):
            g = np.exp(kF - c)
            for t, w in enumerate(words):
                p[t, w] += g
    return kF / scale, p
