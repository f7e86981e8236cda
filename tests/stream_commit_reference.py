"""The zerogram stream search, frame by frame, with its hypotheses in the open: a plain restatement of big_frame
(csrc/viterbi_decode.hip) that keeps score and back pointer per trellis position and prunes with `v > best + thr`, so that a test
can read the set of alive hypotheses after every frame and hold sr_stream_stable's commit point, stable words and trailing
silence against tests/commit_reference.py on it.

Simplifications, which the fixtures of tests/test_gpu_stream_stable.py respect (the search itself is held against the oracle
elsewhere, tests/test_gpu_stream.py):
  * every word has two positions or more -- no one-position word's dead second position feeding the best score;
  * every emission cost is >= 0 -- the reference's pre-AM early-out (Recognizer.cpp:143) is inert, so the word-boundary
    candidates of a target collapse to the minimal surviving word end and the first position attaining it per (word penalty,
    tdp) class, as in big_frame's fast arm: no sequential boundary replay.
Arithmetic is IEEE double in the kernel's order of operations."""
import math

import numpy as np

from tests import commit_reference

INF = math.inf
NONE = 0xFFFFFFFF


class Net:
    """Per trellis position (words back to back, as build_decode_net lays them out): emission state, word, and the flags."""

    def __init__(self, word_off, automaton, silence_word, silence_state, tdp):
        word_off = [int(x) for x in word_off]
        self.P = word_off[-1]
        self.n_words = len(word_off) - 1
        self.silence_word = int(silence_word)
        self.tl, self.tf, self.ts = (float(x) for x in tdp)
        self.state, self.word, self.pos0, self.pos1, self.end, self.sil_state, self.sil_word, self.first_sil = ([] for _ in range(8))
        for w in range(self.n_words):
            b, n = word_off[w], word_off[w + 1] - word_off[w]
            assert n >= 2, "the restatement leaves one-position words out"
            for k in range(n):
                st = int(automaton[b + k])
                self.state.append(st); self.word.append(w)
                self.pos0.append(k == 0); self.pos1.append(k == 1); self.end.append(k == n - 1)
                self.sil_state.append(st == silence_state); self.sil_word.append(w == silence_word)
                self.first_sil.append(int(automaton[b]) == silence_state)


class _Merge:
    def __init__(self):
        self.score, self.bkp = INF, 0

    def offer(self, pre_am, am, bkp):  # Recognizer.cpp:143-157: `continue` on the early-out, then strict improvement
        n = pre_am + am
        if not (pre_am > self.score) and self.score > n:
            self.score, self.bkp = n, bkp


class Search:
    """After push(row) number t: sc / bk = the pruned hypotheses of frame t; tb_score / tb_word / tb_bkp = traceback[0 .. t]."""

    def __init__(self, net, am_threshold, word_penalty):
        self.net, self.thr, self.wp = net, float(am_threshold), float(word_penalty)
        self.sc = [INF] * net.P
        self.bk = [0] * net.P
        self.sc[0] = 0.0
        self.m_we = INF
        self.ef = [NONE] * 4
        self.t = 0
        self.tb_score, self.tb_word, self.tb_bkp = [0.0], [0], [0]

    def push(self, row):
        n, sc, bk = self.net, self.sc, self.bk
        self.t += 1
        t = self.t
        bkp_new = (t - 1) & 0xFFFF
        scn, bkn = [INF] * n.P, [0] * n.P
        best, we, we_idx = INF, INF, NONE
        for p in range(n.P):
            am = float(row[n.state[p]])
            assert am >= 0.0, "the restatement leaves the sequential boundary replay out"
            pos0, pos1 = n.pos0[p], n.pos1[p]
            entry = pos0 or pos1
            t_loop = n.tf if n.sil_state[p] else n.tl
            t_skip = n.tf if n.sil_state[p] else n.ts
            p1 = p - (0 if pos0 else 1)
            p2 = p - (0 if entry else 2)
            c_skip = INF if entry else sc[p2] + t_skip
            c_fwd = INF if pos0 else sc[p1] + n.tf
            c_loop = INF if n.end[p] else sc[p] + t_loop
            am_b = float(row[n.state[p1]]) if pos1 else am
            wp = 0.0 if n.sil_word[p] else self.wp
            b_skip = pos1 and not n.first_sil[p]
            t_b = n.ts if b_skip else n.tf
            cls = (0 if n.sil_word[p] else 2) + (1 if b_skip else 0)
            c_b = (self.m_we + wp) + t_b if entry else INF
            b_first = self.ef[cls] < p1
            mg = _Merge()
            mg.offer(c_b if b_first else INF, am_b, bkp_new)
            mg.offer(c_skip, am, bk[p2])
            mg.offer(c_fwd, am, bk[p1])
            mg.offer(c_loop, am, bk[p])
            mg.offer(INF if b_first else c_b, am_b, bkp_new)
            scn[p], bkn[p] = mg.score, mg.bkp
            if mg.score < best:
                best = mg.score
            if n.end[p] and mg.score < we:  # ascending p: the first minimal word end
                we, we_idx = mg.score, p
        limit = best + self.thr
        we_alive = not (we > limit) and we != INF
        m_we = we if we_alive else INF
        near = m_we + (abs(m_we) + abs(self.wp) + abs(n.tf) + abs(n.ts) + 1.0) * 1e-9
        ef = [NONE] * 4
        rec = (INF, 0, 0)  # no surviving word end: word 0 (Recognizer.cpp:118,191)
        for p in range(n.P):
            v = scn[p]
            if v > limit:
                scn[p] = INF
                continue
            if n.end[p] and we_alive and v <= near:
                if p == we_idx:
                    rec = (v, n.word[p], bkn[p])
                for c, (w_, t_) in enumerate(((0.0, n.tf), (0.0, n.ts), (self.wp, n.tf), (self.wp, n.ts))):
                    if v + w_ + t_ == m_we + w_ + t_:
                        ef[c] = min(ef[c], p)
        self.sc, self.bk, self.m_we, self.ef = scn, bkn, m_we, ef
        self.tb_score.append(rec[0]); self.tb_word.append(rec[1]); self.tb_bkp.append(rec[2])

    # ---- what sr_stream_stable reports after the frames so far (include/srgpu.h) --------------------------------------------
    def alive(self):
        if self.t == 0:
            return [0]
        return [self.bk[p] for p in range(self.net.P) if math.isfinite(self.sc[p])]

    def commit(self, floor=0):
        return commit_reference.commit_point(self.tb_bkp, self.alive(), floor)

    def silence(self):
        if self.t == 0:
            return 0
        best, bp = INF, None
        for p in range(self.net.P):
            if math.isfinite(self.sc[p]) and self.sc[p] < best:  # ties: the smaller position
                best, bp = self.sc[p], p
        if bp is None or not self.net.sil_word[bp]:
            return 0
        return self.t - self.bk[bp]


def walk(tb_word, tb_bkp, start, silence_word):
    """The words of the traceback walk started at frame `start` (Recognizer.cpp:222-231), silence removed, in time order."""
    out, t = [], int(start)
    while t > 0:
        if int(tb_word[t]) != silence_word:
            out.append(int(tb_word[t]))
        assert int(tb_bkp[t]) < t
        t = int(tb_bkp[t])
    return np.asarray(out[::-1], np.uint32)
