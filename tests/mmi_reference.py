"""MMI training over the recognition network, restated in numpy (log space, FP64): the reference the MMI tests hold
sr_net_occupancies_corpus / sr_mmi_statistics_corpus / sr_model_create_from_mmi_statistics against.

One forward-backward serves both networks.  A GRAPH is a list of segments, each with the slots of a lexicon word and the network's
in-word moves (tests/net_fb_reference.py), plus per segment the word ends that enter it:

  free network (denominator)   one segment per lexicon word, entered by every word end; paths end in any word end
  transcript w_1 .. w_n        the chain sil_0 w_1 sil_1 .. w_n sil_n: a word segment is entered by the silence segment before it and
  (numerator)                  the word segment before that, a silence segment by the word segment before it and by itself; paths
                               end in the word end of w_n or sil_n.  Silence must be word 0.

The start hypothesis sits at slot 0 (position 0 of word 0 / of sil_0) on the virtual row before frame 0; when that slot is a word
end the row enters what that word end enters.  Entries cost wp(v) + tdp(first_v, init + 1) + e(t, first_v) at position 0 or 1.

occupancies(): occ[t, k] = the posterior probability that frame t's emission is mixture k's = dF / d e(t, k).  A slot's gamma counts
for its own state, except that the ENTRY part of a position-1 slot counts for the word's first state (which the entry emits).
occupancies() takes a `dtype` as net_fb_reference's recursions do (np.longdouble: the yardstick of tests/test_gpu_netocc_scores.py)."""
from __future__ import annotations

import numpy as np

from tests import net_fb_reference as R

INF = np.inf


class Graph:
    def __init__(self, net, seg_words, seg_src, final_segs):
        """seg_words[g] = lexicon word of segment g; seg_src[g] = segments whose word end enters g; final_segs = where paths end"""
        self.net = net
        st, pos, end, first, silw, seg = [], [], [], [], [], []
        self.beg, self.last = [], []
        for g, w in enumerate(seg_words):
            a, b = int(net.word_off[w]), int(net.word_off[w + 1])
            self.beg.append(len(st))
            st += net.state[a:b].tolist()
            pos += net.pos[a:b].tolist()
            end += net.end[a:b].tolist()
            first += net.first[a:b].tolist()
            silw += net.sil_word[a:b].tolist()
            seg += [g] * (b - a)
            self.last.append(len(st) - 1)
        self.state, self.pos, self.seg = np.array(st), np.array(pos), np.array(seg)
        self.end, self.first, self.sil_word = np.array(end, bool), np.array(first), np.array(silw, bool)
        self.P = len(st)
        self.src = [tuple(self.last[h] for h in hs) for hs in seg_src]  # word-end slots entering segment g
        self.dst = [[] for _ in seg_words]                            # segments the word end of g enters
        for g, hs in enumerate(seg_src):
            for h in hs:
                self.dst[h].append(g)
        self.final = [self.last[g] for g in final_segs]


def free_graph(net):
    every = list(range(net.W))
    return Graph(net, every, [every] * net.W, every)


def chain_graph(net, transcript):
    assert net.sil_word[0], "the constrained network needs silence to be word 0"
    words = [0]
    for w in transcript:
        assert 0 < w < net.W
        words += [int(w), 0]
    G = len(words)
    src = []
    for g in range(G):
        if g % 2:
            src.append([g - 1] + ([g - 2] if g >= 2 else []))
        else:
            src.append(([g - 1] if g else []) + [g])
    return Graph(net, words, src, [G - 1] + ([G - 2] if G > 1 else []))


def _penalties(gr, tdp, wp, scale, dtype=np.float64):
    scale = dtype(scale)
    tl, tf, ts = (scale * dtype(x) for x in tdp)
    sil = gr.state == gr.net.sil_state
    into = np.array([np.where(sil, tf, v) for v in (tl, tf, ts)], dtype=dtype)
    w = np.where(gr.sil_word, dtype(0.0), scale * dtype(wp))
    t_init = np.where(gr.pos == 0, tf, np.where(gr.first == gr.net.sil_state, tf, ts))
    return into, w + t_init


def _lsum(xs, dtype=np.float64):
    return R._lsum(np.asarray(list(xs), dtype=dtype))


def occupancies(e, gr, tdp, wp, scale=1.0, dtype=np.float64):
    """-> (F = -(1/kappa) log of the graph's path mass, occ [T, S])"""
    e = np.asarray(e, dtype=np.float64).astype(dtype)
    T, S = e.shape
    P = gr.P
    into, ent = _penalties(gr, tdp, wp, scale, dtype)
    scale = dtype(scale)
    lsum = lambda xs: _lsum(xs, dtype)
    if T == 0:
        return INF, np.zeros((0, S), dtype=dtype)
    # alpha; row 0 of A is the virtual row
    A = np.full((T + 1, P), INF, dtype=dtype)
    A[0, 0] = 0.0
    Esum = np.full((T + 1, len(gr.src)), INF, dtype=dtype)  # Esum[t, g]: the entry sum of segment g from row t
    inw = np.full((T + 1, P), INF, dtype=dtype)             # in-word part of alpha before the emission
    for t in range(1, T + 1):
        em = scale * e[t - 1]
        cache = {}
        for g, srcs in enumerate(gr.src):
            if srcs not in cache:
                cache[srcs] = lsum(A[t - 1, list(srcs)])
            Esum[t - 1, g] = cache[srcs]
        for s in range(P):
            terms = []
            for j in range(3):
                if gr.pos[s] >= j and not (j == 0 and gr.end[s]):
                    terms.append(A[t - 1, s - j] + into[j, s])
            inw[t, s] = lsum(terms)
            x = [inw[t, s] + em[gr.state[s]]]
            if gr.pos[s] == 0:
                x.append(Esum[t - 1, gr.seg[s]] + ent[s] + em[gr.state[s]])
            elif gr.pos[s] == 1:
                x.append(Esum[t - 1, gr.seg[s]] + ent[s] + em[gr.first[s]])
            A[t, s] = lsum(x)
    F = lsum(A[T, gr.final])
    occ = np.zeros((T, S), dtype=dtype)
    if not np.isfinite(F):
        return INF, occ
    B = np.full((T + 1, P), INF, dtype=dtype)
    B[T, gr.final] = 0.0
    for t in range(T, 0, -1):
        em = scale * e[t - 1]
        if t < T:
            en = scale * e[t]
            X = []  # X[g]: the entries into segment g at frame t + 1 (row t + 1 of B)
            for g in range(len(gr.src)):
                b = gr.beg[g]
                x = [ent[b] + en[gr.state[b]] + B[t + 1, b]]
                if not gr.end[b]:
                    x.append(ent[b + 1] + en[gr.state[b]] + B[t + 1, b + 1])
                X.append(lsum(x))
            cache = {}
            for s in range(P):
                if gr.end[s]:
                    key = tuple(gr.dst[gr.seg[s]])
                    if key not in cache:
                        cache[key] = lsum(X[g] for g in key)
                    B[t, s] = cache[key]
                else:
                    x = [into[0, s] + en[gr.state[s]] + B[t + 1, s], into[1, s + 1] + en[gr.state[s + 1]] + B[t + 1, s + 1]]
                    if not gr.end[s + 1]:
                        x.append(into[2, s + 2] + en[gr.state[s + 2]] + B[t + 1, s + 2])
                    B[t, s] = lsum(x)
        for s in range(P):
            if not np.isfinite(B[t, s]):
                continue
            own = inw[t, s] + em[gr.state[s]] + B[t, s]
            if np.isfinite(own):
                occ[t - 1, gr.state[s]] += np.exp(F - own)
            if gr.pos[s] <= 1:
                k = gr.state[s] if gr.pos[s] == 0 else gr.first[s]
                x = Esum[t - 1, gr.seg[s]] + ent[s] + em[k] + B[t, s]
                if np.isfinite(x):
                    occ[t - 1, k] += np.exp(F - x)
    return F / scale, occ


def enumerate_paths(e, net, tdp, wp, scale=1.0):
    """Every path of the free network (tiny T and lexica only) -> {word string with silence removed: (mass = sum exp(-kappa cost),
    counts [T, S] = sum of mass over the string's paths of [frame t emits state k])}."""
    e = np.asarray(e, dtype=np.float64)
    T, S = e.shape
    gr = free_graph(net)
    into, ent = _penalties(gr, tdp, wp, scale)
    sil = int(net.word[np.flatnonzero(net.sil_word)[0]])
    out = {}

    def succ(s, t):
        em = scale * e[t]
        if gr.end[s]:
            for v in range(net.W):
                b = int(net.word_off[v])
                yield b, ent[b] + em[gr.state[b]], gr.state[b], v
                if not gr.end[b]:
                    yield b + 1, ent[b + 1] + em[gr.state[b]], gr.state[b], v
            return
        for j in range(3):
            if gr.pos[s] + j < net.n_pos[s]:
                yield s + j, into[j, s + j] + em[gr.state[s + j]], gr.state[s + j], None

    def walk(s, t, c, words, emitted):
        if t == T:
            if gr.end[s]:
                key = tuple(w for w in words if w != sil)
                m = np.exp(-c)
                mass, cnt = out.setdefault(key, [0.0, np.zeros((T, S))])
                out[key][0] = mass + m
                for tt, k in enumerate(emitted):
                    cnt[tt, k] += m
            return
        for d, x, k, v in succ(s, t):
            walk(d, t + 1, c + x, words + ([v] if v is not None else []), emitted + [k])

    walk(0, 0, 0.0, [0], [])  # the start hypothesis: in word 0
    return {k: (v[0], v[1]) for k, v in out.items()}


def frame_items(occ, floor=0.0):
    """per frame [(mixture, occ)] with occ > 0 and >= floor, ascending mixture id (tests/fb_reference.items' shape)"""
    return [[(int(k), float(row[k])) for k in np.flatnonzero((row > 0) & (row >= floor))] for row in occ]


def ebw_update(means, inv_vars, num, den, E, tau, var_floor):
    """Extended Baum-Welch, in the kernel's order of operations.  num / den = (mean_acc [C, D], w [C], var_acc [C, D]) WITH the 1e-4
    seed in var_acc.  -> (means', variances') [C, D]"""
    means, var = np.asarray(means, dtype=np.float64), 1.0 / np.asarray(inv_vars, dtype=np.float64)
    C, D = means.shape
    new_m, new_v = means.copy(), var.copy()
    for c in range(C):
        gn, gd = float(num[1][c]), float(den[1][c])
        if gn == 0.0 and gd == 0.0:
            continue
        ns = 1.0
        if tau > 0.0 and gn > 0.0:
            ns = (gn + tau) / gn
            gn = gn * ns
        xn, xd = num[0][c] * ns, den[0][c]
        sn, sd = (num[2][c] - 1e-4) * ns, den[2][c] - 1e-4
        diff = gd - gn
        Dc = max(E * gd, 2.0 * max(diff, 0.0) + 1e-10)

        def update(Dk):
            d = (gn - gd) + Dk
            m = ((xn - xd) + Dk * means[c]) / d
            return m, ((sn - sd) + Dk * (var[c] + means[c] * means[c])) / d - m * m

        for _ in range(64):
            if (update(Dc)[1] >= var_floor).all():
                break
            Dc = Dc * 2.0
        m, v = update(Dc)
        new_m[c], new_v[c] = m, np.where(v >= var_floor, v, var_floor)
    return new_m, new_v
