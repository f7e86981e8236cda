"""MMI training over the bigram-LM search network, restated in numpy (log space, FP64): the reference the bigram MMI tests hold
sr_bigram_occupancies_corpus / sr_bigram_mmi_statistics_corpus against.  The network is tests/bigram_fb_reference.py's.

  free network (denominator)   that file's forward / backward; occ[t, k] = the sum of gamma over the positions carrying mixture k
  transcript w_1 .. w_n        the chain of segments S w_1 c_1 .. w_n c_n, written here a second time and independently (plain
  (numerator)                  loops over segments and states): S = the silence word, entered from the start's word end before frame
                               0 and from its own word end afterwards; w_i entered from the word ends of w_{i-1} and c_{i-1} (w_1:
                               of the start and S) at kappa lm[w_i, w_{i-1}] (history silence for w_1; NaN / +inf: no path); c_i =
                               the silence copy after w_i, entered from the word end of w_i alone.  Paths end in the word end of w_n
                               or c_n (n = 0: of S).

occ[t, k] = the posterior probability that frame t emits mixture k = dF / d e(t, k).  An entry emits the mixture of the state it moves
to, so a position's gamma counts for its own mixture.  enumerate_paths() lists every path of a tiny network by its sequence of
non-silence word ENTRIES: the constrained network of a transcript is exactly the paths under that key."""
from __future__ import annotations

import numpy as np

from tests import bigram_fb_reference as R

INF = np.inf


def _lse(xs, dtype=np.float64):
    xs = [dtype(x) for x in xs if np.isfinite(x)]
    if not xs:
        return dtype(INF)
    m = min(xs)
    return m - np.log(sum(np.exp(m - x) for x in xs))


def free_occupancies(e, net, lm, tdp, scale=1.0, entry_sum=None, dtype=np.float64):
    """-> (F_den, occ [T, S]) of the free network; dtype as bigram_fb_reference's"""
    S = np.asarray(e).shape[1]
    kF, G = R.gammas(e, net, lm, tdp, scale, entry_sum, dtype)
    return kF / dtype(scale), R.collect(G, net.state, S)[:, :S]


def chain_occupancies(e, net, lm, tdp, transcript, scale=1.0, dtype=np.float64):
    """-> (F_num, occ [T, S]) of the network restricted to the transcript (word ids, silence not listed); dtype as
    bigram_fb_reference's"""
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    T, S = e.shape
    W, sil = net.W, net.sil
    scale = dtype(scale)
    td = scale * np.asarray(tdp, dtype=np.float64).reshape(2, 4).astype(dtype)
    lm = np.asarray(lm, dtype=np.float64).astype(dtype)
    lse = lambda xs: _lse(xs, dtype)  # noqa: E731
    # segments: slot, states' mixtures, isSilence, entry LM cost, sources (segments whose word end enters it)
    slots, klm, srcs = [sil], [dtype(0.0)], [[0]]
    hist = sil
    for i, w in enumerate(transcript):
        w = int(w)
        assert 0 <= w < W and w != sil
        g = len(slots)
        x = lm[w, hist]
        slots += [w, w + W]
        klm += [scale * x if np.isfinite(x) or x == -INF else dtype(INF), dtype(0.0)]
        srcs += [[0] if i == 0 else [g - 2, g - 1], [g]]
        hist = w
    G = len(slots)
    mix = [net.state[net.slot_off[x]:net.slot_off[x + 1]] for x in slots]
    isl = [int(net.slot_sil[x]) for x in slots]
    n = [len(m) for m in mix]
    dsts = [[d for d in range(G) if g in srcs[d]] for g in range(G)]
    finals = [G - 1] + ([G - 2] if G > 1 else [])
    occ = np.zeros((T, S), dtype=dtype)
    if T == 0:
        return dtype(0.0 if G == 1 else INF), occ
    A = [[np.full(n[g], INF, dtype=dtype) for g in range(G)] for _ in range(T)]
    we = [dtype(INF)] * G
    we[0] = dtype(0.0)  # the start's word end is the silence word's
    for t in range(T):
        for g in range(G):
            ent = lse(we[h] for h in srcs[g]) + klm[g]
            p = td[isl[g]]
            for k in range(n[g]):
                terms = []
                if t > 0:
                    terms += [A[t - 1][g][k - j] + p[j] for j in range(3) if k - j >= 0]
                if k == 0:
                    terms.append(ent)
                if k == 1:
                    terms.append(ent + p[2])
                A[t][g][k] = lse(terms) + scale * e[t, mix[g][k]]
        we = [A[t][g][n[g] - 1] + td[isl[g], 3] for g in range(G)]
    kF = lse(we[g] for g in finals)
    if not np.isfinite(kF):
        return dtype(INF), occ
    B = [[np.full(n[g], INF, dtype=dtype) for g in range(G)] for _ in range(T)]
    for t in range(T - 1, -1, -1):
        for g in range(G):
            p = td[isl[g]]
            for k in range(n[g]):
                terms = []
                if t == T - 1:
                    if k == n[g] - 1 and g in finals:
                        terms.append(p[3])
                else:
                    x = lambda h, j: scale * e[t + 1, mix[h][j]] + B[t + 1][h][j]
                    terms += [p[j] + x(g, k + j) for j in range(3) if k + j < n[g]]
                    if k == n[g] - 1:
                        for d in dsts[g]:
                            into = [x(d, 0)] + ([td[isl[d], 2] + x(d, 1)] if n[d] >= 2 else [])
                            terms.append(p[3] + klm[d] + lse(into))
                B[t][g][k] = lse(terms)
                y = A[t][g][k] + B[t][g][k]
                if np.isfinite(y):
                    occ[t, mix[g][k]] += np.exp(kF - y)
    return kF / scale, occ


def enumerate_paths(e, net, lm, tdp, scale=1.0):
    """Every path of the free network (tiny T and lexica only) -> {sequence of non-silence word entries: (mass = sum exp(-kappa
    cost), counts [T, S] = sum of mass over the key's paths of [frame t emits mixture k])}."""
    E = np.asarray(e, dtype=np.float64)
    T, S = E.shape
    W = net.W
    klm, td = R._klm(net, lm, scale), R._tdp(tdp, scale)
    out = {}

    def enter(x, c, t, key, emitted):
        p0 = int(net.first[x])
        s = int(net.slot_sil[x])
        step(p0, c, t, key, emitted)
        if net.slot_off[x + 1] - p0 >= 2:
            step(p0 + 1, c + td[s, 2], t, key, emitted)

    def step(p, c, t, key, emitted):
        if not np.isfinite(c):
            return
        c = c + scale * E[t, net.state[p]]
        emitted = emitted + [int(net.state[p])]
        x, s = int(net.slot[p]), int(net.is_sil[p])
        if p == net.last[x]:
            end(x, c + td[s, 3], t + 1, key, emitted)
        if t + 1 == T:
            return
        for j in range(3):
            if net.k[p] + j < net.n[p]:
                step(p + j, c + td[s, j], t + 1, key, emitted)

    def end(x, c, t, key, emitted):
        if t == T:
            if np.isfinite(c):
                m = np.exp(-c)
                mass, cnt = out.setdefault(key, [0.0, np.zeros((T, S))])
                out[key][0] = mass + m
                for tt, k in enumerate(emitted):
                    cnt[tt, k] += m
            return
        h = int(net.hist[x])
        for w in range(W):
            if w != net.sil and np.isfinite(klm[w, h]):
                enter(w, c + klm[w, h], t, key + (w,), emitted)
        if x == net.sil:
            enter(x, c, t, key, emitted)
        elif x < W:
            enter(x + W, c, t, key, emitted)

    end(net.sil, 0.0, 0, (), [])
    return {k: (v[0], v[1]) for k, v in out.items()}


def frame_items(occ, floor=0.0):
    """per frame [(mixture, occ)] with occ > 0 and >= floor, ascending mixture id (tests/fb_reference.items' shape)"""
    return [[(int(k), float(row[k])) for k in np.flatnonzero((row > 0) & (row >= floor))] for row in occ]
