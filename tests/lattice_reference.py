"""Word lattices and N-best lists over the recognition network, restated in numpy: the reference the lattice tests hold
sr_word_lattice_corpus / sr_lattice_nbest against.  Network, costs and order of additions are net_fb_reference's with
semiring="min", scale 1 and no beam.

forward_min_with_starts carries, beside the cheapest cost A_t(s) of every slot, the frame b_t(s) at which that cheapest path
entered its current word.  A slot's candidates are compared on their final values (penalties and the frame's emission added) in
the order orc_decode_pruned (oracle/sr_oracle.c) meets them -- source slots ascending, the first of equal candidates stays:
    the entry from the word ends   before the in-word moves if the best word end of the frame before (the lowest slot among
                                   equal ones) lies below the destination slot, after them otherwise
    in-word moves                  from position pos - 2, pos - 1, pos
An entry sets b = t, an in-word move carries its source's b, the start hypothesis has b = 0.

An arc per (word w, frame t) whose end slot is reachable: first = b_t(end), last = t, fwd = A_t(end), bwd = Bend_t (the cheapest
continuation after a word end at t to a word end at T - 1; the same number for every word end), cost = fwd - E_{first - 1}.
There is one arc per (word, end frame), carrying the best start only: paths through the arcs are a subset of the network's."""
from __future__ import annotations

import numpy as np

from tests import net_fb_reference as R

INF = np.inf


def _shift_int(v, j):
    out = np.zeros_like(v)
    out[j:] = v[:-j]
    return out


def forward_min_with_starts(e, net, tdp, wp):
    """-> (A [T, P], b [T, P] int, E [T], best_end [T] = the lowest word-end slot with A_t = E_t (-1: none reachable))"""
    tab = np.asarray(e, dtype=np.float64)
    T = tab.shape[0]
    into, w, t_init = R._costs(net, tdp, wp, 1.0)
    A = np.full((T, net.P), INF)
    Bk = np.zeros((T, net.P), dtype=np.int64)
    Es = np.full(T, INF)
    arg = np.full(T, -1, dtype=np.int64)
    prev = np.full(net.P, INF)
    prev[0] = 0.0
    pb = np.zeros(net.P, dtype=np.int64)
    Eprev, aprev = (0.0, 0) if net.end[0] else (INF, -1)
    p0, p1 = net.pos == 0, net.pos == 1
    slots = np.arange(net.P)
    ends = np.flatnonzero(net.end)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            em = tab[t, net.state]
            ef = tab[t, net.first]
            x0 = np.where(net.end, INF, prev + into[0]) + em
            x1 = np.where(net.pos >= 1, R._shift(prev, 1) + into[1], INF) + em
            x2 = np.where(net.pos >= 2, R._shift(prev, 2) + into[2], INF) + em
            ent = (Eprev + w) + t_init
            xe = np.where(p0, ent + em, np.where(p1, ent + ef, INF))
            xe, x2, x1, x0 = (np.where(np.isnan(x), INF, x) for x in (xe, x2, x1, x0))
            cur = np.minimum(np.minimum(x0, x1), np.minimum(x2, xe))
            early = (aprev >= 0) & (aprev < slots)
            # the first candidate of the order that reaches the minimum: assign in reverse order, so that earlier ones overwrite
            b = np.full(net.P, t, dtype=np.int64)  # the late entry comes last
            b = np.where(x0 == cur, pb, b)
            b = np.where(x1 == cur, _shift_int(pb, 1), b)
            b = np.where(x2 == cur, _shift_int(pb, 2), b)
            b = np.where(early & (xe == cur), t, b)
            A[t], Bk[t] = cur, b
            if len(ends) and np.isfinite(cur[ends]).any():
                Eprev = cur[ends].min()
                aprev = int(ends[np.flatnonzero(cur[ends] == Eprev)[0]])
            else:
                Eprev, aprev = INF, -1
            Es[t], arg[t] = Eprev, aprev
            prev, pb = cur, b
    return A, Bk, Es, arg


def backward_min(e, net, tdp, wp):
    """-> (B [T, P], Bend [T]): net_fb_reference.backward with min in place of log-add; in-word (into[j] + e) + B, entry
    ((wp + t_init) + e) + B"""
    tab = np.asarray(e, dtype=np.float64)
    T = tab.shape[0]
    into, w, t_init = R._costs(net, tdp, wp, 1.0)
    B = np.full((T, net.P), INF)
    Bend = np.full(T, INF)
    if T == 0:
        return B, Bend
    B[T - 1, net.end] = 0.0
    Bend[T - 1] = 0.0
    entry = (net.pos == 0) | (net.pos == 1)
    nxt_end1 = np.append(net.end[1:], True)
    with np.errstate(invalid="ignore"):
        for t in range(T - 2, -1, -1):
            en = tab[t + 1, net.state]
            ef = tab[t + 1, net.first]
            b1 = B[t + 1]
            x_entry = np.where(net.pos == 0, ((w + t_init) + en) + b1, ((w + t_init) + ef) + b1)
            x_entry = np.where(np.isnan(x_entry), INF, x_entry)
            be = x_entry[entry].min() if entry.any() else INF
            x0 = (into[0] + en) + b1
            x1 = R._shift((into[1] + en) + b1, -1)
            x2 = R._shift((into[2] + en) + b1, -2)
            x2 = np.where(nxt_end1, INF, x2)
            inw = np.minimum(np.minimum(x0, x1), x2)
            inw = np.where(np.isnan(inw), INF, inw)
            B[t] = np.where(net.end, be, inw)
            Bend[t] = be
    return B, Bend


ARC_KEYS = ("word", "first", "last", "fwd", "bwd", "cost")


def lattice(e, net, tdp, wp, beam):
    """-> (arcs, best): arcs = dict of arrays word, first, last (int64), fwd, bwd, cost (float64) in (last, word) order; best =
    E_{T-1} (+inf for T = 0)"""
    tab = np.asarray(e, dtype=np.float64)
    T = tab.shape[0]
    out = {k: [] for k in ARC_KEYS}
    best = INF
    if T:
        A, Bk, Es, _ = forward_min_with_starts(tab, net, tdp, wp)
        _, Bend = backward_min(tab, net, tdp, wp)
        best = Es[T - 1]
        end_slot = net.word_off[1:] - 1
        for t in range(T):
            for wd in range(net.W):
                s = int(end_slot[wd])
                fwd, bwd = A[t, s], Bend[t]
                tot = fwd + bwd
                if not (np.isfinite(fwd) and np.isfinite(tot) and tot <= best + beam):
                    continue
                first = int(Bk[t, s])
                out["word"].append(wd)
                out["first"].append(first)
                out["last"].append(t)
                out["fwd"].append(fwd)
                out["bwd"].append(bwd)
                out["cost"].append(fwd - (Es[first - 1] if first > 0 else 0.0))
    arcs = {k: np.asarray(out[k], dtype=np.int64 if k in ("word", "first", "last") else np.float64) for k in ARC_KEYS}
    return arcs, best


def lattice_paths(arcs, T):
    """every lattice path as (cost summed left to right, [arc indices])"""
    by_first = {}
    for i in range(len(arcs["word"])):
        by_first.setdefault(int(arcs["first"][i]), []).append(i)
    found = []

    def walk(f, c, path):
        if f == T:
            found.append((c, list(path)))
            return
        for i in by_first.get(f, ()):
            path.append(i)
            walk(int(arcs["last"][i]) + 1, c + float(arcs["cost"][i]), path)
            path.pop()

    if T > 0:
        walk(0, 0.0, [])
    return found


def nbest(arcs, T, silence, n):
    """the n cheapest distinct word strings (silence removed) among the lattice paths, by exhaustive enumeration:
    [(words tuple, cost of its cheapest path)], cheapest first (ties: by the words)"""
    best = {}
    for c, path in lattice_paths(arcs, T):
        ws = tuple(int(arcs["word"][i]) for i in path if int(arcs["word"][i]) != silence)
        if ws not in best or c < best[ws]:
            best[ws] = c
    return sorted(best.items(), key=lambda kv: (kv[1], kv[0]))[:n]


def network_paths(e, net, tdp, wp):
    """every path of the network (tiny T and lexica only) as (cost, [(word, first, last)]): net_fb_reference.brute_force's walk,
    recording the word segments"""
    tab = np.asarray(e, dtype=np.float64)
    T = tab.shape[0]
    into, w, t_init = R._costs(net, tdp, wp, 1.0)

    def succ(s, t):
        em = tab[t]
        if s is None or net.end[s]:
            if s is not None or net.end[0]:
                for v in range(net.W):
                    b = int(net.word_off[v])
                    yield b, w[b] + t_init[b] + em[net.state[b]], True
                    if net.word_off[v + 1] - b >= 2:
                        yield b + 1, w[b + 1] + t_init[b + 1] + em[net.state[b]], True
                return
            for j in range(3):
                if j < net.n_pos[0]:
                    yield j, into[j, j] + em[net.state[j]], False
            return
        for j in range(3):
            d = s + j
            if net.pos[s] + j < net.n_pos[s]:
                yield d, into[j, d] + em[net.state[d]], False

    found = []

    def walk(s, t, c, segs, start):
        if t == T:
            if s is not None and net.end[s]:
                found.append((c, segs + [(int(net.word[s]), start, T - 1)]))
            return
        for d, x, entry in succ(s, t):
            if entry and s is not None:
                walk(d, t + 1, c + x, segs + [(int(net.word[s]), start, t - 1)], t)
            else:  # in-word, or the first frame (the start hypothesis' word starts at frame 0 either way)
                walk(d, t + 1, c + x, segs, start)

    if T > 0:
        walk(None, 0, 0.0, [], 0)
    return found
