"""Word lattices over the bigram-LM search network, restated in numpy: the reference the bigram lattice tests hold
sr_bigram_word_lattice_corpus / sr_bigram_lattice_nbest against.  The network and its order of additions are
tests/bigram_fb_reference.py's forward(..., "min", 1.0) and backward(..., semiring="min"), imported unchanged; here the forward also
tracks, per position, the frame at which the cheapest path entered its slot and the history it was entered from.

Equal candidates are resolved in a fixed order, the first stays: in-word from the same position, one back, two back, then the entry;
among equal entry terms the smallest history.

An arc = (slot x, end frame t) with WE[t + 1, x] finite: word, hist, pred, first, last, fwd, bwd, am -- see include/srgpu.h."""
from __future__ import annotations

import numpy as np

from tests import bigram_fb_reference as R

INF = np.inf


def tracked_forward(e, net, lm, tdp):
    """-> (WE [T + 1, 2W], ST [T + 1, 2W] first frame, PR [T + 1, 2W] predecessor history, klm): rows as R.forward's WE."""
    E = np.asarray(e, dtype=np.float64)
    T, W = E.shape[0], net.W
    klm, td = R._klm(net, lm, 1.0), R._tdp(tdp, 1.0)
    WE = np.full((T + 1, 2 * W), INF)
    WE[0] = R.start_ends(net)
    ST = np.zeros((T + 1, 2 * W), np.int64)
    PR = np.zeros((T + 1, 2 * W), np.int64)
    prev = np.full(net.P, INF)
    pst = np.zeros(net.P, np.int64)
    ppr = np.zeros(net.P, np.int64)
    for t in range(T):
        hist = R.histories(net, WE[t], "min")
        ent = np.full(2 * W, INF)
        epr = np.zeros(2 * W, np.int64)
        for w in range(W):
            c = hist + klm[w]
            h = int(np.argmin(c))  # the first of equal terms
            ent[w], epr[w] = c[h], h
            ent[w + W], epr[w + W] = WE[t][w], w
        ent[net.sil], epr[net.sil] = WE[t][net.sil], net.sil
        ent[net.sil + W] = INF
        cur = np.full(net.P, INF)
        cst = np.zeros(net.P, np.int64)
        cpr = np.zeros(net.P, np.int64)
        for p in range(net.P):
            x, s, k = int(net.slot[p]), int(net.is_sil[p]), int(net.k[p])
            cands = [(prev[p] + td[s, 0], pst[p], ppr[p])]
            if k >= 1:
                cands.append((prev[p - 1] + td[s, 1], pst[p - 1], ppr[p - 1]))
            if k >= 2:
                cands.append((prev[p - 2] + td[s, 2], pst[p - 2], ppr[p - 2]))
            if k == 0:
                cands.append((ent[x], t, epr[x]))
            if k == 1:
                cands.append((ent[x] + td[s, 2], t, epr[x]))
            b = 0
            for i in range(1, len(cands)):
                if cands[i][0] < cands[b][0]:
                    b = i
            v = cands[b][0] + E[t, net.state[p]]
            cur[p] = v if v < INF else INF
            cst[p], cpr[p] = cands[b][1], cands[b][2]
        WE[t + 1] = cur[net.last] + td[net.slot_sil, 3]
        ST[t + 1] = cst[net.last]
        PR[t + 1] = cpr[net.last]
        prev, pst, ppr = cur, cst, cpr
    return WE, ST, PR, klm


def backward_ends(e, net, lm, tdp):
    """RB [T, 2W]: the cheapest continuation from a word end of slot x after frame t to a word end after frame T - 1 -- R.backward's
    R[x], by its own statements in its own order (RB[T - 1] = 0)."""
    E = np.asarray(e, dtype=np.float64)
    T, W = E.shape[0], net.W
    klm, td = R._klm(net, lm, 1.0), R._tdp(tdp, 1.0)
    pt = td[net.is_sil]
    is_last = net.k == net.n - 1
    RB = np.full((T, 2 * W), INF)
    if T == 0:
        return RB
    RB[T - 1] = 0.0
    B = np.where(is_last, pt[:, 3], INF)
    two = (net.slot_off[1:] - net.slot_off[:-1]) >= 2
    for t in range(T - 2, -1, -1):
        x = E[t + 1, net.state] + B
        b2 = np.where(two, td[net.slot_sil, 2] + x[np.minimum(net.first + 1, net.P - 1)], INF)
        bent = R._comb([x[net.first], b2], "min")
        Y = R._entry_sum(bent[:W], klm, 0, "min")
        Rx = np.empty(2 * W)
        Rx[:W] = R._comb([Y, bent[W:]], "min")
        Rx[net.sil] = R._comb([Y[net.sil], bent[net.sil]], "min")
        Rx[W:] = Y
        RB[t] = Rx
        s0 = pt[:, 0] + x
        s1 = np.where(net.k + 1 < net.n, R._shift(pt[:, 1] + x, -1), INF)
        s2 = np.where(net.k + 2 < net.n, R._shift(pt[:, 2] + x, -2), INF)
        ex = np.where(is_last, pt[:, 3] + Rx[net.slot], INF)
        cur = R._comb([s0, s1, s2, ex], "min")
        B = np.where(np.isnan(cur), INF, cur)
    return RB


def arcs(e, net, lm, tdp, beam=INF):
    """-> (best, dict of arrays word, hist, pred, first, last, fwd, bwd, am, slot) in (last, slot) order; T = 0: best 0, no arcs"""
    WE, ST, PR, klm = tracked_forward(e, net, lm, tdp)
    RB = backward_ends(e, net, lm, tdp)
    T, W = WE.shape[0] - 1, net.W
    best = float(WE[T].min()) if T else 0.0
    limit = best + beam
    out = {k: [] for k in ("word", "hist", "pred", "first", "last", "fwd", "bwd", "am", "slot")}
    for t in range(T):
        for x in range(2 * W):
            f = WE[t + 1, x]
            tot = f + RB[t, x]
            if not (f < INF and tot < INF and tot <= limit):
                continue
            b, pr = int(ST[t + 1, x]), int(PR[t + 1, x])
            isw = x < W and x != net.sil
            if isw:
                c_in = R.histories(net, WE[b], "min")[pr]
            else:
                c_in = WE[b, x - W if x >= W else net.sil]
            lmc = klm[x, pr] if isw else 0.0
            for k, v in (("word", x if x < W else net.sil), ("hist", int(net.hist[x])), ("pred", pr), ("first", b), ("last", t),
                         ("fwd", f), ("bwd", RB[t, x]), ("am", (f - c_in) - lmc), ("slot", x)):
                out[k].append(v)
    ints = ("word", "hist", "pred", "first", "last", "slot")
    return best, {k: np.asarray(v, dtype=np.uint32 if k in ints else np.float64) for k, v in out.items()}


def slot_of(word, hist, W, sil):
    return word if word != sil else (sil if hist == sil else hist + W)


def step_cost(pw, ph, word, hist, am, klm, sil, lm_scale=1.0):
    """the cost of an arc (word, hist, am) right after an arc of (pw, ph) (the start: silence, silence); +inf: no such entry"""
    c = 0.0
    if word != sil:
        l = klm[word, ph]
        if not l < INF:
            return INF
        c = lm_scale * l
    elif hist == sil:
        if not (pw == sil and ph == sil):
            return INF
    elif pw != hist or pw == sil:
        return INF
    return c + am


def lattice_paths(A, T, sil, klm, lm_scale=1.0):
    """every lattice path -> [(cost, (arc index, ...))] (small lattices only)"""
    n = len(A["word"])
    by = {}
    for i in range(n):
        by.setdefault(int(A["first"][i]), []).append(i)
    out = []

    def walk(f, pw, ph, g, seq):
        if f == T:
            out.append((g, tuple(seq)))
            return
        for i in by.get(f, []):
            st = step_cost(pw, ph, int(A["word"][i]), int(A["hist"][i]), float(A["am"][i]), klm, sil, lm_scale)
            if st < INF:
                walk(int(A["last"][i]) + 1, int(A["word"][i]), int(A["hist"][i]), g + st, seq + [i])

    if T:
        walk(0, sil, sil, 0.0, [])
    return out


def strings_of(A, paths, sil):
    """{word string: cheapest path cost} over enumerated paths, silence removed"""
    best = {}
    for g, seq in paths:
        s = tuple(int(A["word"][i]) for i in seq if int(A["word"][i]) != sil)
        if s not in best or g < best[s]:
            best[s] = g
    return best


def nbest(A, T, sil, klm, n_best, lm_scale=1.0):
    """the n_best cheapest distinct strings, by enumeration -> [(string, cost)] (ties: by string)"""
    best = strings_of(A, lattice_paths(A, T, sil, klm, lm_scale), sil)
    return sorted(best.items(), key=lambda kv: (kv[1], kv[0]))[:n_best]


def network_paths(e, net, lm, tdp):
    """R.brute_force's enumeration extended to record slots: every network path -> (cost, ((slot, end frame), ...) its word ends)"""
    E = np.asarray(e, dtype=np.float64)
    T, W = E.shape[0], net.W
    klm, td = R._klm(net, lm, 1.0), R._tdp(tdp, 1.0)
    paths = []

    def enter(x, c, t, ends):
        p0 = int(net.first[x])
        s = int(net.slot_sil[x])
        step(p0, c, t, ends)
        if net.slot_off[x + 1] - p0 >= 2:
            step(p0 + 1, c + td[s, 2], t, ends)

    def step(p, c, t, ends):
        if not np.isfinite(c):
            return
        c = c + E[t, net.state[p]]
        x, s = int(net.slot[p]), int(net.is_sil[p])
        if p == net.last[x]:
            end(x, c + td[s, 3], t + 1, ends + ((x, t),))
        if t + 1 == T:
            return
        for j in range(3):
            if net.k[p] + j < net.n[p]:
                step(p + j, c + td[s, j], t + 1, ends)

    def end(x, c, t, ends):
        if t == T:
            paths.append((c, ends))
            return
        h = int(net.hist[x])
        for w in range(W):
            if w != net.sil and np.isfinite(klm[w, h]):
                enter(w, c + klm[w, h], t, ends)
        if x == net.sil:
            enter(x, c, t, ends)
        elif x < W:
            enter(x + W, c, t, ends)

    if T:
        end(net.sil, 0.0, 0, ())
    return [(c, ends) for c, ends in paths if np.isfinite(c)]
