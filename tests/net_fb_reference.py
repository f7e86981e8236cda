"""Forward-backward over the recognition network, restated in numpy (log space, FP64): the reference the word-posterior tests hold
sr_word_posteriors_corpus / sr_recognize_confidence_corpus against.  Emission costs come in as a dense [T, S] table.

The network is the one orc_decode_pruned (oracle/sr_oracle.c) searches, over slots = the lexicon's (word, position) pairs in word
order.  Before frame 0 one hypothesis sits at slot 0 (word 0, position 0) with cost 0.  A slot that is not its word's last position
moves to positions pos + j (j = 0, 1, 2) of its word at tdp(dest state, j) + e(t, dest state); the penalty is keyed on the
DESTINATION state and a move into the silence state costs `forward`.  A word-end slot enters every word v at position 0 or 1 at
wp(v) + tdp(first_v, init + 1) + e(t, first_v) -- the first state's emission also for position 1 (the reference's quirk); an entry
into position 1 of a one-position word reaches no slot.  F = -(1/kappa) log sum over the paths ending in a word end at frame T - 1
of exp(-kappa cost).  With semiring="min" (and kappa = 1) the per-frame minimum over word ends is the decoder's tb_score[1..T] at
an infinite beam, in the oracle's order of additions: ((h + wp) + tdp) + e and (h + tdp) + e.

forward, backward and posteriors take a `dtype` (default float64, the kernels' own precision): with np.longdouble (x87: 64 bits of
mantissa) the same recursion is the yardstick the float64 one, and the kernels, are measured against (tests/test_gpu_netfb_scores.py).
A NaN entry is not defined here: the tests hand over the table with NaN set to +inf (tests/netfb_cases.sanitised)."""
from __future__ import annotations

import numpy as np

INF = np.inf


class Net:
    """Slot tables of a lexicon (word_off[W + 1], automaton[P], silence word index, silence state)."""

    def __init__(self, word_off, automaton, silence_idx, silence_state):
        self.word_off = np.asarray(word_off, dtype=np.int64)
        self.state = np.asarray(automaton, dtype=np.int64)
        self.W = len(self.word_off) - 1
        self.P = int(self.word_off[-1])
        self.word = np.repeat(np.arange(self.W), np.diff(self.word_off))
        self.pos = np.arange(self.P) - self.word_off[self.word]
        self.n_pos = np.diff(self.word_off)[self.word]
        self.end = self.pos == self.n_pos - 1
        self.first = self.state[self.word_off[self.word]]
        self.sil_word = self.word == silence_idx
        self.sil_state = silence_state


def _costs(net, tdp, wp, scale, dtype=np.float64):
    """per slot: into[j] = penalty of a jump of j INTO the slot; entry = wp + tdp(first, init + 1) for positions 0 / 1 (inf else)"""
    scale = dtype(scale)
    tl, tf, ts = (scale * dtype(x) for x in tdp)
    into = np.empty((3, net.P), dtype=dtype)
    for j, v in enumerate((tl, tf, ts)):
        into[j] = np.where(net.state == net.sil_state, tf, v)
    w = np.where(net.sil_word, dtype(0.0), scale * dtype(wp))
    t_init = np.where(net.pos == 0, tf, np.where(net.first == net.sil_state, tf, ts))
    return into, w, t_init


def _shift(v, j):
    """out[s] = v[s - j], INF where s - j falls outside"""
    if j == 0:
        return v
    out = np.full_like(v, INF)
    if j > 0:
        out[j:] = v[:-j]
    else:
        out[:j] = v[-j:]
    return out


def _ladd(*xs):
    acc = -np.asarray(xs[0])
    for x in xs[1:]:
        acc = np.logaddexp(acc, -np.asarray(x))
    return -acc


def _lsum(x):
    """-log sum exp(-x) over a vector (+inf if empty or all +inf)"""
    x = np.asarray(x)
    if x.dtype != np.longdouble:
        x = x.astype(np.float64)
    if x.size == 0 or not np.isfinite(x).any():
        return INF
    m = x.min()
    return m - np.log(np.exp(m - x[np.isfinite(x)]).sum())


def forward(e, net, tdp, wp, semiring="log", scale=1.0, dtype=np.float64):
    """-> (alpha [T, P], E [T]): E[t] = the word-end sum (min) at frame t."""
    E_tab = np.asarray(e, dtype=np.float64).astype(dtype)
    T = E_tab.shape[0]
    into, w, t_init = _costs(net, tdp, wp, scale, dtype)
    scale = dtype(scale)
    A = np.full((T, net.P), INF, dtype=dtype)
    Es = np.full(T, INF, dtype=dtype)
    prev = np.full(net.P, INF, dtype=dtype)
    prev[0] = 0.0
    Eprev = dtype(0.0 if net.end[0] else INF)
    p0, p1 = net.pos == 0, net.pos == 1
    with np.errstate(invalid="ignore"):
        for t in range(T):
            em = scale * E_tab[t, net.state]
            ef = scale * E_tab[t, net.first]
            c0 = np.where(net.end, INF, prev + into[0])
            c1 = np.where(net.pos >= 1, _shift(prev, 1) + into[1], INF)
            c2 = np.where(net.pos >= 2, _shift(prev, 2) + into[2], INF)
            ent = (Eprev + w) + t_init
            if semiring == "min":
                inw = np.minimum(np.minimum(c0, c1), c2)
                inw = np.where(p0, np.minimum(c0, ent), inw)
                cur = inw + em
                cur = np.where(p1, np.minimum(cur, ent + ef), cur)
                Eprev = cur[net.end].min() if net.end.any() else INF
            else:
                inw = _ladd(c0, c1, c2)
                inw = np.where(p0, _ladd(c0, ent), inw)
                cur = inw + em
                cur = np.where(p1, _ladd(cur, ent + ef), cur)
                Eprev = _lsum(cur[net.end])
            cur = np.where(np.isnan(cur), INF, cur)
            A[t] = cur
            Es[t] = Eprev
            prev = cur
    return A, Es


def backward(e, net, tdp, wp, scale=1.0, dtype=np.float64):
    """beta [T, P]: the cost from after frame t to a word end at T - 1 (log semiring, scaled)."""
    E_tab = np.asarray(e, dtype=np.float64).astype(dtype)
    T = E_tab.shape[0]
    into, w, t_init = _costs(net, tdp, wp, scale, dtype)
    scale = dtype(scale)
    B = np.full((T, net.P), INF, dtype=dtype)
    B[T - 1, net.end] = 0.0
    entry = (net.pos == 0) | (net.pos == 1)
    nxt_end1 = np.append(net.end[1:], True)  # slot s + 1 is a word end (or does not exist)
    for t in range(T - 2, -1, -1):
        en = scale * E_tab[t + 1, net.state]
        ef = scale * E_tab[t + 1, net.first]
        b1 = B[t + 1]
        x_entry = np.where(net.pos == 0, w + t_init + en + b1, w + t_init + ef + b1)
        Bend = _lsum(x_entry[entry])
        x0 = into[0] + en + b1
        x1 = _shift(into[1] + en + b1, -1)
        x2 = _shift(into[2] + en + b1, -2)
        x2 = np.where(nxt_end1, INF, x2)
        B[t] = np.where(net.end, Bend, _ladd(x0, x1, x2))
    return B


def posteriors(e, net, tdp, wp, scale=1.0, dtype=np.float64):
    """-> (F, word posteriors [T, W]): F = -(1/kappa) log P(X); p[t, w] = sum over w's slots of gamma_t."""
    A, Es = forward(e, net, tdp, wp, "log", scale, dtype)
    T = A.shape[0]
    if T == 0:
        return INF, np.zeros((0, net.W), dtype=dtype)
    F = Es[T - 1]
    B = backward(e, net, tdp, wp, scale, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        G = np.exp(F - A - B)
    G = np.where(np.isfinite(A) & np.isfinite(B) & np.isfinite(F), G, dtype(0.0))
    p = np.zeros((T, net.W), dtype=dtype)
    for wd in range(net.W):
        a, b = net.word_off[wd], net.word_off[wd + 1]
        p[:, wd] = G[:, a:b].sum(axis=1)
    return F / dtype(scale), p


def best_ends(e, net, tdp, wp):
    """the decoder's tb_score[1..T] at an infinite beam (min semiring)"""
    return forward(e, net, tdp, wp, "min")[1]


def brute_force(e, net, tdp, wp, scale=1.0):
    """F by enumerating every path (tiny T and lexica only)."""
    E_tab = np.asarray(e, dtype=np.float64)
    T = E_tab.shape[0]
    into, w, t_init = _costs(net, tdp, wp, scale)

    def succ(s, t):
        em = scale * E_tab[t]
        if s is None or net.end[s]:
            if s is not None or net.end[0]:  # a word end (the start hypothesis is one when word 0 has one position)
                for v in range(net.W):
                    b = int(net.word_off[v])
                    yield b, w[b] + t_init[b] + em[net.state[b]]
                    if net.word_off[v + 1] - b >= 2:
                        yield b + 1, w[b + 1] + t_init[b + 1] + em[net.state[b]]
                return
            s = 0  # the start hypothesis expands within word 0 from position 0
            for j in range(3):
                if j < net.n_pos[0]:
                    yield j, into[j, j] + em[net.state[j]]
            return
        for j in range(3):
            d = s + j
            if net.pos[s] + j < net.n_pos[s]:
                yield d, into[j, d] + em[net.state[d]]

    total = []

    def walk(s, t, c):
        if t == T:
            if s is not None and net.end[s]:
                total.append(c)
            return
        for d, x in succ(s, t):
            walk(d, t + 1, c + x)

    walk(None, 0, 0.0)
    return _lsum(np.array(total)) / scale if total else INF
