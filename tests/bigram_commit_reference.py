"""Teaching::LinearSearch frame by frame with its hypotheses in the open: tests/test_bigram.py::linear_search_py (the literal Python
transcription of LinearSearch.cc:211-436,496-515 and BookKeeping.cc that the C restatement is held against) cut into a class whose
state a test can read after every frame -- the surviving state hypotheses, the merged word-end list and the book -- so that
sr_bigram_stream_stable's commit entry can be held against tests/commit_reference.py on the reference's alive set.  The search code
is linear_search_py's, statement for statement; only the frame loop's body became `push`."""
import numpy as np

from tests import commit_reference

FLT_MAX = np.float32(np.finfo(np.float32).max)
f32 = np.float32
INV = 0xFFFFFFFF


class Search:
    def __init__(self, word_off, mixtures, silence, lm, tdp, ac_pruning=FLT_MAX, lm_pruning=FLT_MAX):
        self.word_off, self.mixtures, self.silence, self.lm, self.tdp = word_off, mixtures, int(silence), lm, tdp
        self.ac_pruning, self.lm_pruning = f32(ac_pruning), f32(lm_pruning)
        self.W = len(word_off) - 1
        self.book = [[INV, FLT_MAX, 0, 0]]
        self.we = [[self.silence, f32(0.0), 0]]
        self._book_keeping(0, self.we)
        self.sh, self.wh, self.wh_map, self.sh_map = [], [], {}, {}
        self.t = 0

    def _acw(self, w):
        return w if w < self.W else self.silence

    def _issil(self, w):
        return 1 if (w == self.silence or w >= self.W) else 0

    def _nlen(self, w):
        return int(self.word_off[self._acw(w) + 1] - self.word_off[self._acw(w)])

    def _book_keeping(self, t, we):
        book, silence = self.book, self.silence
        for h in we:
            book.append([self._acw(h[0]), h[1], h[2], t])
            nb = len(book) - 1
            h[2] = nb
            if t == 0:
                book[nb][2] = nb
            if h[0] == silence:
                cur = book[nb]
                if book[cur[2]][0] == silence:
                    cur[2] = book[cur[2]][2]

    def push(self, row):
        """one frame: row = its emission costs per model state"""
        W, silence, lm, tdp = self.W, self.silence, self.lm, self.tdp
        mapc = lambda w: w if w == silence else w % W  # noqa: E731
        silc = lambda w: w if w == silence else w + W  # noqa: E731
        self.t += 1
        t, we, sh, wh, wh_map, sh_map = self.t, self.we, self.sh, self.wh, self.wh_map, self.sh_map
        ws = [[INV, FLT_MAX, INV] for _ in range(W)]
        for e in we:
            prev = mapc(e[0])
            for w in range(W):
                if w == silence:
                    continue
                ns = f32(e[1] + lm[w, prev])
                if ns < ws[w][1]:
                    ws[w] = [w, ns, e[2]]
            if e[0] < W:
                ws.append([silc(e[0]), e[1], e[2]])
        best = min(x[1] for x in ws)
        thr = self.lm_pruning
        if thr < FLT_MAX:
            thr = f32(thr + best)
        for x in ws:
            if x[1] < thr:
                if x[0] not in wh_map:
                    wh_map[x[0]] = len(wh)
                    wh.append([x[0], INV, INV, INV])
                wh[wh_map[x[0]]][3] = len(sh)
                sh.append([0, x[1], x[2]])
        nsh = []
        for h in wh:
            first_new = len(nsh)

            def expand(word, st):
                n = self._nlen(word)
                for succ in range(max(1, st[0]), min(st[0] + 2, n) + 1):
                    ns = st[1]
                    td = succ - st[0]
                    if st[0] or td > 1:
                        ns = f32(ns + tdp[self._issil(word)][td])
                    idx = sh_map.get(succ, INV)
                    if idx < first_new or idx >= len(nsh) or nsh[idx][0] != succ:
                        sh_map[succ] = len(nsh)
                        nsh.append([succ, ns, st[2]])
                    elif nsh[idx][1] >= ns:
                        nsh[idx][1] = ns
                        nsh[idx][2] = st[2]

            if h[3] != INV:
                expand(h[0], sh[h[3]])
                h[3] = INV
            if h[1] != INV:
                for i in range(h[1], h[2]):
                    expand(h[0], sh[i])
            h[1], h[2] = first_new, len(nsh)
        sh = nsh
        best = FLT_MAX
        for h in wh:
            a = self._acw(h[0])
            for i in range(h[1], h[2]):
                sh[i][1] = f32(sh[i][1] + f32(row[self.mixtures[self.word_off[a] + sh[i][0] - 1]]))
                if sh[i][1] < best:
                    best = sh[i][1]
        thr = self.ac_pruning
        if thr < FLT_MAX:
            thr = f32(thr + best)
        we, out_sh, out_wh = [], [], []
        wh_map = {}
        for h in wh:
            b = len(out_sh)
            n = self._nlen(h[0])
            for i in range(h[1], h[2]):
                sc = f32(sh[i][1] + tdp[self._issil(h[0])][3])
                if sc < thr:
                    out_sh.append(sh[i])
                    if sh[i][0] == n:
                        we.append([h[0], sc, sh[i][2]])
            h[1], h[2] = b, len(out_sh)
            if h[2] - h[1] > 0:
                wh_map[h[0]] = len(out_wh)
                out_wh.append(h)
        sh, wh = out_sh, out_wh
        first, n_ends = {}, 0
        for i in range(len(we)):
            word = mapc(we[i][0])
            if word not in first:
                first[word] = i
                n_ends += 1
            wi = first[word]
            if we[i][1] <= we[wi][1]:
                we[wi] = list(we[i])
        we = we[:n_ends]
        self._book_keeping(t, we)
        self.we, self.sh, self.wh, self.wh_map = we, sh, wh, wh_map

    def _items(self, bp):
        res = []
        while self.book[bp][3] > 0:
            res.append(self.book[bp])
            bp = self.book[bp][2]
        res.reverse()
        return (np.asarray([r[0] for r in res], np.uint32), np.asarray([r[1] for r in res], np.float32), np.asarray([r[3] for r in res], np.uint32))

    def result(self):
        """getResult (:420-436): the traceback from the first best word end"""
        if not self.we:
            return np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint32)
        bi = min(range(len(self.we)), key=lambda i: (self.we[i][1], i))
        return self._items(self.we[bi][2])

    # ---- what sr_bigram_stream_stable reports after the frames so far (include/srgpu.h) -----------------------------------------
    def alive(self):
        """the book entries a later word end can start from: the surviving state hypotheses' and the merged word ends'; a silence
        entry as its parent (a silence word end that follows it is chained to that parent instead, :410-415)"""
        out = []
        for b in [h[2] for h in self.sh] + [h[2] for h in self.we]:
            e = self.book[b]
            out.append(e[2] if e[0] == self.silence and e[3] != 0 else b)
        return out

    def commit(self, floor=1):
        """-> (commit entry, its book time, the items from the start entry to it)"""
        parent = [e[2] for e in self.book]
        c = commit_reference.commit_point(parent, self.alive(), floor)
        return c, int(self.book[c][3]), self._items(c)
