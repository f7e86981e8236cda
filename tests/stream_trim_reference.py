"""sr_stream_trim restated on tests/stream_commit_reference.py's search: drop the frames of an open utterance up to its commit
point, keep the committed words in an archive, and go on in window numbering (stream_trim_kernel in
csrc/viterbi_decode.hip).

TrimSearch is Search with a window: after trim() the traceback lists hold entries 0 .. t - d only, entry 0 stands for the commit
point, every back pointer that survives counts from it, and `base` says how many frames the utterance has lost.  `floor` is what
the library keeps in commit[slot]: the last commit point a stable() or trim() call computed, in window numbering -- where the
set of alive hypotheses is empty the commit point stays there.

What the calls of include/srgpu.h report on a trimmed utterance is restated beside it: partial() (archive + window walk, the
archive only when the walk starts at a finite entry), stable() (archive + window stable words, base + c) and frames()."""
import math

import numpy as np

from speechrecognition_amd import synth
from tests import stream_commit_reference as scr

TDP = (3.0, 0.0, 30.0)
WP = 10.0
# the lexica of tests/test_gpu_stream_stable.py: every word has two positions or more, silence is one state held for several positions
LEXICA = {
    "w6x3": synth.LexiconSpec(np.array([1, 3, 3, 3, 3, 3], np.uint16), np.array([3, 1, 1, 1, 1, 1], np.uint16), 0),
    "w5x9": synth.LexiconSpec(np.array([1, 3, 4, 5, 11], np.uint16), np.array([9, 3, 3, 2, 1], np.uint16), 0),
}


def make_net(lex):
    word_off, automaton, sil_state = lex.flatten()
    return scr.Net(word_off, automaton, lex.silence_idx, sil_state, TDP)


class TrimSearch(scr.Search):
    def __init__(self, net, am_threshold, word_penalty):
        super().__init__(net, am_threshold, word_penalty)
        self.base = 0      # frames dropped so far
        self.archive = []  # the committed words of the dropped frames, silence removed
        self.floor = 0     # commit[slot]

    def frames(self):
        return self.base + self.t

    def trim(self):
        """-> d, the frames dropped: the commit point of the window, 0 in the new numbering afterwards"""
        c = self.commit(self.floor)
        self.floor = 0
        if c == 0:
            return 0
        t = self.t
        assert c <= t - 1, (c, t)  # a hypothesis entered at frame t carries bkp = t - 1: the window never becomes empty
        self.archive += [int(w) for w in scr.walk(self.tb_word, self.tb_bkp, c, self.net.silence_word)]
        for p in range(self.net.P):
            if math.isfinite(self.sc[p]):
                assert self.bk[p] >= c, (p, self.bk[p], c)  # the definition of c
                self.bk[p] -= c
        # entries (c, t] move to (0, t - c]; a back pointer below c belongs to the no-word-end record or to a dead node
        self.tb_score = [0.0] + self.tb_score[c + 1:]
        self.tb_word = [0] + self.tb_word[c + 1:]
        self.tb_bkp = [0] + [b - c if b >= c else 0 for b in self.tb_bkp[c + 1:]]
        self.t = t - c
        self.base += c
        return c

    def window_walk(self, start):
        return [int(w) for w in scr.walk(self.tb_word, self.tb_bkp, start, self.net.silence_word)]

    def partial(self):
        """sr_stream_partial's words: a walk that starts at an entry without a surviving word end reports no archived word"""
        if self.t == 0:
            return np.zeros(0, np.uint32)
        lead = self.archive if math.isfinite(self.tb_score[self.t]) else []
        return np.asarray(lead + self.window_walk(self.t), np.uint32)

    def stable(self):
        """sr_stream_stable's (words, out_commit); moves the floor as the call does"""
        c = self.commit(self.floor)
        self.floor = c
        return np.asarray(self.archive + self.window_walk(c), np.uint32), self.base + c


def untrimmed_partial(s):
    """partial() of a plain Search after its frames so far"""
    return scr.walk(s.tb_word, s.tb_bkp, s.t, s.net.silence_word) if s.t else np.zeros(0, np.uint32)


def run(net, am_threshold, word_penalty, scores, piece, trim_every=1):
    """The whole of `scores` through a TrimSearch in pushes of `piece` rows with a trim after every trim_every-th push, beside a plain
    Search.  -> (per push: dict(frames, dropped, partial, stable, commit, want_partial, want_stable, want_commit, window)), the
    TrimSearch, the Search.  `window` is the frames the window held right after the push: the max_frames that push needed."""
    tr, un = TrimSearch(net, am_threshold, word_penalty), scr.Search(net, am_threshold, word_penalty)
    per, c = [], 0
    for n, i in enumerate(range(0, len(scores), piece)):
        for row in scores[i:i + piece]:
            tr.push(row)
            un.push(row)
        rec = {"frames": tr.frames(), "window": tr.t}
        c = un.commit(c)  # (with nothing alive the commit point stays where the last call left it)
        rec["want_partial"], rec["want_commit"] = untrimmed_partial(un), c
        rec["want_stable"] = scr.walk(un.tb_word, un.tb_bkp, c, net.silence_word)
        rec["stable"], rec["commit"] = tr.stable()
        rec["dropped"] = tr.trim() if (n + 1) % trim_every == 0 else None
        rec["partial"] = tr.partial()
        per.append(rec)
    return per, tr, un


def limited_run(net, am_threshold, word_penalty, scores, piece, trim_every, max_frames):
    """The schedule of run() against a window of max_frames: a push that would take the window past it is refused and changes
    nothing; the caller then trims and pushes the same rows again, and gives up if that is refused too.  -> the events, for a stream
    to be held against one by one: ("refused", i0, i1), ("push", i0, i1, frames after it, partial after it), ("trim", dropped,
    partial after it), and ("gave_up",) at the end where it happened."""
    tr = TrimSearch(net, am_threshold, word_penalty)
    events, i, n = [], 0, 0
    while i < len(scores):
        k = min(piece, len(scores) - i)
        if tr.t + k > max_frames:
            events.append(("refused", i, i + k))
            events.append(("trim", tr.trim(), tr.partial()))
            if tr.t + k > max_frames:
                events.append(("refused", i, i + k))
                events.append(("gave_up",))
                return events
        for row in scores[i:i + k]:
            tr.push(row)
        i, n = i + k, n + 1
        events.append(("push", i - k, i, tr.frames(), tr.partial()))
        if n % trim_every == 0:
            events.append(("trim", tr.trim(), tr.partial()))
    return events


def window_needed(per):
    """the smallest max_frames with which no push of the run overflows"""
    return max(r["window"] for r in per)
