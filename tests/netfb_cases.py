"""Cases for the forward-backward passes over the recognition network run alone on score tables the test makes up
(sr_word_posteriors_corpus_scores, sr_net_occupancies_corpus_scores, sr_net_accuracies_corpus_scores): lexica, tables, utterance
lengths, transcripts, reference labels, the references' answers and the conditions that keep a case from passing vacuously.  No pytest in
here, and the GPU only in run() at the end: tests/test_netfb_cases_cpu.py checks every case's conditions,
tests/test_gpu_netfb_scores.py, tests/test_gpu_netocc_scores.py and tests/test_gpu_smbr_scores.py run the kernels on them.

Why tables and not features: through a mixture model a test cannot place a NaN at the first state of a word and nowhere else, a frame
that kills every path, costs of 1e6 or an exact tie between two words.  Here the table is the input.  A model (S states of one density,
dimension 2: search_cases.model_file) only carries n_states and the row stride.

Frames.  Every utterance has at most 70 frames, with one exception that the network forces: a chain of N positions needs about N / 3
frames for a path (an entry into position 1 and a skipped silence segment take three positions in a frame), so the chains of 256, 257,
300 and 514 positions get 90, 90, 105 and 175 frames -- with fewer they have no path, and a case without a path compares nothing.

The tolerance rule (profiles/netfb_scores_tolerance.txt) lives here too: bound() and the TOL lines of the three GPU files."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from tests import mmi_reference as M
from tests import net_fb_reference as R
from tests import search_cases as sc
from tests import smbr_reference as SM

MODEL_DIM = sc.MODEL_DIM
INF = math.inf
LD = np.longdouble
TDP = (3.0, 0.0, 30.0)
TDP_NO_SKIP = (3.0, 0.0, INF)
TDP_DYADIC = (0.5, 0.0, 0.75)
BLOCK = 512  # kNetFbThreads


def model_file(n_states):
    return sc.model_file(n_states)


# ---- lexica: positions per word, the silence word's index, the model's states -------------------------------------------------------
@dataclass(frozen=True)
class Lex:
    lens: tuple
    sil: int
    S: int               # the model's states; state 0 is the silence state
    twins: bool = False  # word 2 k has the states of word 2 k - 1 (k >= 1)
    sil_at: tuple = ()   # slots inside longer words that emit the silence state too (every move into them costs `forward`)


def _fill(head, P, seed):
    """head, then words of 1 .. 6 positions up to exactly P positions"""
    rng = np.random.default_rng(seed)
    lens = list(head)
    while sum(lens) < P:
        lens.append(min(int(rng.integers(1, 7)), P - sum(lens)))
    return tuple(lens)


def _run_of_ones():
    """silence, multi-position words up to slot 59, one-position words at slots 60 .. 70 (both sides of the wave boundary at 64), a tail"""
    lens = [1] + [5, 6] * 5 + [4]  # 1 + 55 + 4 = 60 positions
    assert sum(lens) == 60
    return tuple(lens + [1] * 11 + [3, 2, 4])


LEXICA = {
    # the LEXICA of test_word_posteriors_cpu.py: one- and multi-position word 0, silence not first
    "a": Lex((1, 3, 3, 2), 0, 24), "b": Lex((3, 1, 2, 4), 1, 24), "c": Lex((2, 4, 1, 6, 3), 2, 24),
    "d": Lex((5, 1, 6, 2, 3, 1, 4), 5, 24), "e": Lex((1, 2), 0, 24),
    "s": Lex((1, 4, 3, 5), 0, 24, sil_at=(2, 7, 11)),  # the silence state at positions 1, 2 and 2 of the three words
    "p511": Lex(_fill((1,), 511, 1), 0, 64), "p512": Lex(_fill((1,), 512, 2), 0, 64), "p513": Lex(_fill((1,), 513, 3), 0, 64),
    "p1025": Lex(_fill((1, 65), 1025, 4), 0, 512),   # thread 0 owns slots 0, 512 and 1024; the 65-position word spans a whole wave
    "w600": Lex((1, 600), 0, 64),                    # word ends at slots 0 and 600: waves 2 .. 7 enter the block sum empty
    "ones": Lex(_run_of_ones(), 0, 64),
    "w64": Lex((1,) + (2, 1) * 31 + (2,), 0, 64), "w65": Lex((1,) + (2, 1) * 32, 0, 64), "w130": Lex((1,) + (1, 2) * 64 + (2,), 0, 64),
    "twins": Lex((1, 3, 3, 2, 2, 1, 1, 4, 4), 0, 24, twins=True),
    "two": Lex((1,) + (2,) * 6 + (3, 4), 0, 24),     # the chains' words: two positions (three in a frame with the silence skipped)
}
assert [sum(LEXICA[k].lens) for k in ("p511", "p512", "p513", "p1025")] == [511, 512, 513, 1025]
assert [len(LEXICA[k].lens) for k in ("w64", "w65", "w130")] == [64, 65, 130]


@functools.lru_cache(maxsize=None)
def lexicon(name):
    """-> (word_off u32[W + 1], automaton u16[P], silence word, silence state 0): the silence word is its one position of state 0,
    the other positions take the states 1 .. S - 1 in turn (all distinct while they last)"""
    lx = LEXICA[name]
    assert lx.lens[lx.sil] == 1
    off = np.concatenate([[0], np.cumsum(lx.lens)]).astype(np.uint32)
    aut, nxt = [], 0
    for w, n in enumerate(lx.lens):
        if w == lx.sil:
            aut.append(0)
        elif lx.twins and w >= 2 and w % 2 == 0:
            aut += aut[int(off[w - 1]):int(off[w])]
        else:
            aut += [1 + (nxt + i) % (lx.S - 1) for i in range(n)]
            nxt += n
    aut = np.asarray(aut, dtype=np.uint16)
    aut[list(lx.sil_at)] = 0
    off.setflags(write=False)
    aut.setflags(write=False)
    return off, aut, lx.sil, 0


@functools.lru_cache(maxsize=None)
def net(name):
    return R.Net(*lexicon(name))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
RAGGED = (1, 2, 3, 70, 5, 33, 18, 41, 7, 64)   # 1 .. 70, every residue mod 4
SHORT = (5, 12, 3, 9)
HOSTILE = 1                                    # the utterance that gets the frame of +inf, the NaN, the -inf


@dataclass(frozen=True)
class Case:
    name: str
    lex: str
    table: str = "random"   # random | dyadic | signed | const | inf_band | inf_frame | nan_pos0 | nan_own1 | nan_first1 | nan_pos2 | neginf
    lens: tuple = SHORT     # frames per utterance
    scale: float = 1.0      # random: U(0, 20) * scale (the penalties scaled alike) ...
    offset: float = 0.0     # ... + offset
    kappa: float = 1.0
    tdp: tuple = TDP
    wp: float = 10.0
    trans: str = None       # None: no chains | "random" | a key of CHAINS
    labels: str = "path"    # path | best | none | first
    seed: int = 0
    passes: tuple = ("post", "occ", "smbr")
    sample: tuple = None    # the utterances held against the slow references (None: all)

    @property
    def penalties(self):
        return tuple(x * self.scale for x in self.tdp), self.wp * self.scale


def case_id(c):
    return c.name


def _cases():
    out = []
    # the small lexica: the ragged batch, both kappa, both skips, both word penalties
    for i, (lx, kappa, tdp, wp) in enumerate((("a", 1.0, TDP, 10.0), ("b", 0.3, TDP, 0.0), ("c", 1.0, TDP_NO_SKIP, 10.0),
                                              ("d", 0.3, TDP_NO_SKIP, 0.0), ("e", 1.0, TDP, 0.0))):
        out.append(Case(f"ragged-{lx}", lx, lens=RAGGED, kappa=kappa, tdp=tdp, wp=wp, seed=i,
                        trans="random" if LEXICA[lx].sil == 0 else None, labels=("path", "best", "first", "path", "best")[i]))
    out.append(Case("t123-a", "a", lens=(1, 2, 3), trans="random"))
    out.append(Case("sil_inside", "s", lens=RAGGED, trans="random", seed=3))  # (the penalty into a slot is keyed on the slot's own state)
    # tables, on the four-word lexicon (chains: silence is word 0) and on the seven-word one (silence is word 5)
    for lx in ("a", "d"):
        tr = "random" if lx == "a" else None
        out.append(Case(f"dyadic-{lx}", lx, "dyadic", lens=RAGGED, tdp=TDP_DYADIC, wp=1.25, trans=tr))
        for s in (1e-3, 1e3, 1e6):
            out.append(Case(f"x{s:g}-{lx}", lx, lens=RAGGED, scale=s, trans=tr))
        out.append(Case(f"plus1e8-{lx}", lx, lens=RAGGED, offset=1e8, trans=tr))
        out.append(Case(f"signed-{lx}", lx, "signed", lens=RAGGED, trans=tr))
        out.append(Case(f"const-{lx}", lx, "const", lens=RAGGED, trans=tr))
        out.append(Case(f"inf_band-{lx}", lx, "inf_band", lens=RAGGED, trans=tr))
        out.append(Case(f"inf_frame-{lx}", lx, "inf_frame", lens=(9, 12, 6), trans=tr))
        for k in ("nan_pos0", "nan_own1", "nan_first1", "nan_pos2", "neginf"):
            out.append(Case(f"{k}-{lx}", lx, k, lens=(9, 12, 6), trans=tr))
    out.append(Case("labels_none-a", "a", labels="none", passes=("smbr",)))
    out.append(Case("labels_first-d", "d", labels="first", lens=RAGGED, passes=("smbr",)))
    out.append(Case("labels_best-c", "c", labels="best", lens=RAGGED, passes=("smbr",)))
    # the launch shape
    for lx in ("p511", "p512", "p513", "ones", "w64", "w65", "w130"):
        out.append(Case(lx, lx, lens=SHORT, seed=7))
    out.append(Case("w600", "w600", lens=(40, 6), seed=7))
    out.append(Case("twins", "twins", "dyadic", lens=(12, 9, 30), tdp=TDP_DYADIC, wp=1.25, trans="random"))
    out.append(Case("p1025", "p1025", lens=(6, 11), seed=7))
    # chains, with the words of two positions: lengths at chain_block's edges, no path, none and one word, a mixed launch group
    for k in CHAINS:
        out.append(Case(f"chain-{k}", "two", lens=CHAINS[k][1], trans=k, passes=("occ",)))
    # several score chunks and launch groups (SRGPU_SCORE_CHUNK_MB=1 SRGPU_FB_MB=1): 24 utterances of 10 .. 40 frames
    rng = np.random.default_rng(2424)
    out.append(Case("chunks", "p1025", lens=tuple(int(t) for t in rng.integers(10, 41, size=24)), seed=9, sample=(0, 10, 16, 22),
                    trans="random"))
    assert len({c.name for c in out}) == len(out)
    return out


def _chain(n2, extra=()):
    """a transcript of n2 two-position words (lexicon `two`: words 1 .. 6) and `extra`"""
    return tuple(1 + i % 6 for i in range(n2)) + tuple(extra)


# name -> (one transcript per utterance, frames per utterance); chain positions = words + 1 silences + the words' positions
CHAINS = {
    "empty_one": (((), (3,), (7,)), (4, 3, 1)),                      # sil alone; one word; one word of three positions in one frame: no path
    "n64_65": ((_chain(21), _chain(20, (7,))), (30, 30)),            # 22 + 42 = 64; 22 + 40 + 3 = 65
    "n256_257": ((_chain(85), _chain(84, (7,))), (90, 90)),          # 86 + 170 = 256; 86 + 168 + 3 = 257
    "n514": ((_chain(171),), (175,)),                                # 172 + 342 = 514
    "mixed": ((_chain(3), _chain(98, (8,))), (8, 105)),              # 4 + 6 = 10 and 100 + 196 + 4 = 300 in one launch group
}
CHAIN_LENGTHS = {"empty_one": (1, 4, 5), "n64_65": (64, 65), "n256_257": (256, 257), "n514": (514,), "mixed": (10, 300)}

CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- tables, transcripts, labels ------------------------------------------------------------------------------------------------------
def frame_off(case):
    off = np.concatenate([[0], np.cumsum(case.lens)]).astype(np.uint64)
    off.setflags(write=False)
    return off


def _entry_word(nt):
    """a word of three or more positions other than word 0 -> its first slot"""
    w = next(w for w in range(1, nt.W) if nt.word_off[w + 1] - nt.word_off[w] >= 3)
    return int(nt.word_off[w])


def nan_cells(case):
    """(frame of the hostile utterance, state) that gets the NaN, and the slot it is named for"""
    nt = net(case.lex)
    b = _entry_word(nt)
    t = case.lens[HOSTILE] // 2
    # position 0: of the last word but the silence, where it has one position (no entry into a position 1 pays it) if the lexicon has such
    last = max(w for w in range(nt.W) if w != LEXICA[case.lex].sil)
    ones = [w for w in range(1, nt.W) if w != LEXICA[case.lex].sil and nt.word_off[w + 1] - nt.word_off[w] == 1]
    p0 = int(nt.word_off[ones[0] if ones else last])
    slot = {"nan_pos0": p0, "nan_own1": b + 1, "nan_first1": b, "nan_pos2": b + 2}[case.table]
    return t, int(nt.state[slot]), slot


@functools.lru_cache(maxsize=None)
def table(case):
    """[F, S] f64, never written to"""
    S = LEXICA[case.lex].S
    rng = np.random.default_rng(8000 + case.seed)
    off = frame_off(case)
    F = int(off[-1])
    if case.table == "dyadic":
        t = rng.integers(0, 17, size=(F, S)).astype(np.float64) * 0.25
    elif case.table == "signed":
        t = rng.uniform(-50.0, 50.0, size=(F, S))
    elif case.table == "const":
        t = np.full((F, S), 2.5)
    else:
        t = rng.uniform(0.0, 20.0, size=(F, S)) * case.scale + case.offset
    nt = net(case.lex)
    if case.table == "inf_band":  # every state but the silence's and one word's: one way through the frames of the middle third
        for u in range(len(case.lens)):
            f0, T = int(off[u]), case.lens[u]
            keep = np.zeros(S, bool)
            keep[0] = True
            t[f0 + T // 3:f0 + 2 * T // 3 + 1][:, ~keep] = INF
    elif case.table == "inf_frame":
        t[int(off[HOSTILE]) + case.lens[HOSTILE] // 2] = INF
    elif case.table.startswith("nan_"):
        tt, k, _ = nan_cells(case)
        t[int(off[HOSTILE]) + tt, k] = np.nan
    elif case.table == "neginf":
        t[int(off[HOSTILE]) + case.lens[HOSTILE] // 2, 0] = -INF  # the silence state: on a path whatever the frame
    t.setflags(write=False)
    return t


def sanitised(t):
    """NaN -> +inf: the table the references see"""
    return np.where(np.isnan(t), INF, t)


def rows(case, u, clean=True):
    off = frame_off(case)
    t = table(case)[int(off[u]):int(off[u + 1])]
    return sanitised(t) if clean else t


@functools.lru_cache(maxsize=None)
def transcripts(case):
    """one tuple of word ids per utterance (silence, word 0, not listed), or None"""
    if case.trans is None:
        return None
    if case.trans in CHAINS:
        return CHAINS[case.trans][0]
    rng = np.random.default_rng(8100 + case.seed)
    nt = net(case.lex)
    out = []
    for T in case.lens:  # few enough words for a path: a word of n positions takes at least ceil(n / 2) frames
        words, need = [], 0
        for _ in range(int(rng.integers(0, 4))):
            w = int(rng.integers(1, nt.W))
            n = int(nt.word_off[w + 1] - nt.word_off[w])
            if need + (n + 1) // 2 <= T:
                words.append(w)
                need += (n + 1) // 2
        out.append(tuple(words))
    return tuple(out)


def _best_path(e, nt, tdp, wp):
    """the states of the decoder's best path at an infinite beam, by a plain Viterbi over the slots (small lexica)"""
    into, w, t_init = R._costs(nt, tdp, wp, 1.0)
    T, P = e.shape[0], nt.P
    cost = np.full(P, INF)
    cost[0] = 0.0
    E = 0.0 if nt.end[0] else INF
    back = np.zeros((T, P), dtype=np.int64)  # source slot, or -1 - (best word end) for an entry
    emit = np.zeros((T, P), dtype=np.int64)
    e_arg = 0
    for t in range(T):
        new = np.full(P, INF)
        for s in range(P):
            cand = []
            for j in range(3):
                if nt.pos[s] >= j and not (j == 0 and nt.end[s]):
                    cand.append((cost[s - j] + into[j, s] + e[t, nt.state[s]], s - j, nt.state[s]))
            if nt.pos[s] <= 1:
                k = nt.state[s] if nt.pos[s] == 0 else nt.first[s]
                cand.append((E + w[s] + t_init[s] + e[t, k], -1 - e_arg, k))
            c, b, k = min(cand, key=lambda x: x[0])
            new[s], back[t, s], emit[t, s] = c, b, k
        cost = new
        ends = np.flatnonzero(nt.end)
        e_arg = int(ends[np.argmin(cost[ends])])
        E = cost[e_arg]
    out = np.zeros(T, dtype=np.uint16)
    s = e_arg
    for t in range(T - 1, -1, -1):
        out[t] = emit[t, s]
        b = back[t, s]
        s = int(b) if b >= 0 else -1 - int(b)
    return out


@functools.lru_cache(maxsize=None)
def labels(case):
    """u16[F]: the reference mixture of every frame"""
    nt = net(case.lex)
    S = LEXICA[case.lex].S
    off = frame_off(case)
    rng = np.random.default_rng(8200 + case.seed)
    out = np.zeros(int(off[-1]), dtype=np.uint16)
    tdp, wp = case.penalties
    for u, T in enumerate(case.lens):
        f0 = int(off[u])
        if case.labels == "none":
            out[f0:f0 + T] = S + (np.arange(T) % 3)
        elif case.labels == "first":  # the first state of a longer word: scored at its position 0 and at the entries into position 1
            out[f0:f0 + T] = nt.state[_entry_word(nt)]
        elif case.labels == "best":
            with np.errstate(invalid="ignore"):
                out[f0:f0 + T] = _best_path(rows(case, u), nt, tdp, wp)
        else:  # a random walk through the network
            s = 0
            for t in range(T):
                if nt.end[s]:
                    v = int(rng.integers(0, nt.W))
                    b = int(nt.word_off[v])
                    s = b + (1 if (nt.n_pos[b] >= 2 and rng.integers(0, 2)) else 0)
                    out[f0 + t] = nt.first[b]
                else:
                    s = s + int(rng.integers(0, min(3, int(nt.n_pos[s] - nt.pos[s]))))
                    out[f0 + t] = nt.state[s]
    out.setflags(write=False)
    return out


# ---- references: per utterance, once, shared -------------------------------------------------------------------------------------------
_DT = {"float64": np.float64, "longdouble": LD}


def sampled(case):
    return tuple(range(len(case.lens))) if case.sample is None else case.sample


@functools.lru_cache(maxsize=None)
def post_reference(case, dtype_name):
    """{u: (F, word posteriors [T, W])} of net_fb_reference on the sanitised table (every utterance: the recursion is vectorised)"""
    tdp, wp = case.penalties
    out = {}
    for u in range(len(case.lens)):
        with np.errstate(all="ignore"):
            F, p = R.posteriors(rows(case, u), net(case.lex), tdp, wp, case.kappa, dtype=_DT[dtype_name])
        p.setflags(write=False)
        out[u] = (F, p)
    return out


@functools.lru_cache(maxsize=None)
def occ_reference(case, dtype_name, chain):
    """{u: (F, occupancies [T, S])} of mmi_reference for the sampled utterances: the free network, or the transcripts' chains"""
    tdp, wp = case.penalties
    nt = net(case.lex)
    out = {}
    for u in sampled(case):
        gr = M.chain_graph(nt, transcripts(case)[u]) if chain else M.free_graph(nt)
        with np.errstate(all="ignore"):
            F, occ = M.occupancies(rows(case, u), gr, tdp, wp, case.kappa, dtype=_DT[dtype_name])
        occ.setflags(write=False)
        out[u] = (F, occ)
    return out


@functools.lru_cache(maxsize=None)
def smbr_reference(case, dtype_name):
    """{u: (F, Abar, gamma [T, S])} of smbr_reference for the sampled utterances"""
    tdp, wp = case.penalties
    gr = M.free_graph(net(case.lex))
    off = frame_off(case)
    out = {}
    for u in sampled(case):
        with np.errstate(all="ignore"):
            F, A, g = SM.smbr(rows(case, u), gr, tdp, wp, labels(case)[int(off[u]):int(off[u + 1])], case.kappa, dtype=_DT[dtype_name])
        g.setflags(write=False)
        out[u] = (F, A, g)
    return out


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------------
def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


def bound(d64, ref):
    """what the kernels may lie from the longdouble value `ref`: 8 times the float64 restatement's distance d64 plus 4 ulp of the
    value (kernel and restatement are float64 recursions of the same depth that differ in the order of their sums)"""
    return 8.0 * d64 + 4.0 * ulp(ref)


def tighter(fixed, v64, v80, tag=None):
    """For the suites that ran on fixed tolerances against the float64 restatement (test_gpu_word_posteriors.py, test_gpu_mmi.py,
    test_gpu_smbr.py): value by value the rule's bound(float64 distance, longdouble value) against the longdouble run where that is
    the tighter of the two, +inf where it is not -- there the fixed bound against the float64 run, which those suites go on asserting,
    stays what holds.  With a tag, prints which one holds."""
    v80 = np.asarray(v80, dtype=LD)
    d = dist(v64, v80)
    rule = bound(d, v80.astype(np.float64))
    out = np.where(rule <= fixed, rule, np.inf)
    if tag:
        print(f"RULE {tag}: float64-longdouble {d:.2e}, rule {float(np.max(rule)):.2e}, fixed {float(np.max(fixed)):.2e}: "
              + ("the rule" if np.all(rule <= fixed) else "the fixed bound, for the largest values" if np.any(rule <= fixed) else "the fixed bound"))
    return out


def dist(a, b):
    """largest |a - b|, taken in longdouble, as a float"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def dense(count, ids, weight, n, key=lambda w: w):
    """the items of an utterance's frames as [T, n]; checks each frame's order (key(weight) descending, then id ascending), that no id
    comes twice and that the entries past the count are 0"""
    out = np.zeros((len(count), n))
    for t in range(len(count)):
        k = int(count[t])
        i, w = ids[t, :k].astype(np.int64), weight[t, :k]
        assert len(set(i.tolist())) == k and np.all(i < n), f"frame {t}: ids {i}"
        kw = key(w)
        assert all(kw[j] > kw[j + 1] or (kw[j] == kw[j + 1] and i[j] < i[j + 1]) for j in range(k - 1)), f"frame {t}: order {w} {i}"
        assert np.all(weight[t, k:] == 0) and np.all(ids[t, k:] == 0), f"frame {t}: entries past the count"
        out[t, i] = w
    return out


# ---- the launch plan at SRGPU_SCORE_CHUNK_MB=1 SRGPU_FB_MB=1, restated (make_chunks, srplan::launch_groups) ---------------------------
def plan(case, bytes_per_cell, chunk_mb=1, fb_mb=1):
    """-> [chunk: [(u0, u1) launch groups]] of the free network's pass"""
    S, P = LEXICA[case.lex].S, net(case.lex).P
    ld = (S + 7) // 8 * 8
    off = [int(x) for x in frame_off(case)]
    U = len(case.lens)
    chunk_frames = max(1, (chunk_mb << 20) // (ld * 8))
    n_target = max(1, -(-off[-1] // chunk_frames))
    even = -(-off[-1] // n_target)
    chunks, u = [], 0
    while u < U:
        v = u + 1
        while v < U and off[v + 1] - off[u] <= chunk_frames and off[v] - off[u] < even:
            v += 1
        chunks.append((u, v))
        u = v
    cost = [bytes_per_cell * P * f for f in off]
    out = []
    for u0, u1 in chunks:
        gs, u = [], u0
        while u < u1:
            v = u + 1
            while v < u1 and cost[v + 1] - cost[u] <= (fb_mb << 20):
                v += 1
            gs.append((u, v))
            u = v
        out.append(gs)
    return out


def group_frames(case, bytes_per_cell=8, **kw):
    off = frame_off(case)
    return [int(off[v] - off[u]) for gs in plan(case, bytes_per_cell, **kw) for u, v in gs]


def hold(tag, got, r64, r80, total, worst):
    """One utterance against the rule.  got / r64 / r80 = (F, weights [T, n]) of the kernels, the float64 and the longdouble run;
    total = what a frame's weights add up to (1, or 0 for gamma).  r64 may be a list of float64 restatements: each distance is then
    the largest of theirs.  Asserts, and raises the distances in `worst` (dF dw ds kF kw ks)."""
    (F, w), (F80, w80) = got, r80
    r64s = r64 if isinstance(r64, list) else [r64]
    dF, kF = max(dist(F64, F80) for F64, _ in r64s), dist(F, F80)
    assert kF <= bound(dF, float(F80)), f"{tag}: F off by {kF:.3e}; float64 reference {dF:.3e}"
    dw = max(dist(w64, w80) for _, w64 in r64s)
    err = np.abs(w.astype(LD) - w80).astype(np.float64)
    tol = bound(dw, w80.astype(np.float64))
    assert np.all(err <= tol), f"{tag}: weight off by {err.max():.3e} at {np.argwhere(err > tol)[:4].tolist()}; float64 reference {dw:.3e}"
    if total == 1.0:  # no posterior or occupancy exceeds 1 by more than the rounding the table forces on a weight
        assert np.all(w <= 1.0 + bound(dw, 1.0)), f"{tag}: a weight of 1 + {float(w.max() - 1.0):.3e}; float64 reference {dw:.3e}"
    ds = max(dist(w64.sum(axis=1), w80.sum(axis=1)) for _, w64 in r64s)
    ks = dist(w.astype(LD).sum(axis=1), w80.sum(axis=1))
    assert ks <= bound(max(ds, dw), max(abs(total), 1.0)), f"{tag}: a frame's weights add up to {total} -+ {ks:.3e}; float64 reference {ds:.3e}"
    for k, v in (("dF", dF), ("dw", dw), ("ds", ds), ("kF", kF), ("kw", float(err.max()) if err.size else 0.0), ("ks", ks)):
        worst[k] = max(worst.get(k, 0.0), v)


def tol_line(kind, case, worst):
    g = lambda k: worst.get(k, 0.0)
    line = (f"TOL {kind:5s} {case.name:16s} float64-longdouble F {g('dF'):.2e} weight {g('dw'):.2e} sum {g('ds'):.2e}"
            + (f" Abar {g('dA'):.2e}" if "dA" in worst else "")
            + f" | kernel-longdouble F {g('kF'):.2e} weight {g('kw'):.2e} sum {g('ks'):.2e}" + (f" Abar {g('kA'):.2e}" if "kA" in worst else ""))
    print(line)
    return line


# ---- the calls (the only part that touches the GPU) -------------------------------------------------------------------------------------
def open_model(S):
    from speechrecognition_amd import capi
    return capi.Model.from_mixset(model_file(S), MODEL_DIM, device=0)


def run(m, case, kind, floor=0.0, max_items=None):
    """kind post -> (F, count, word, weight); occ / chain -> (F, count, state, weight); smbr -> (F, Abar, count, state, weight):
    the hook on the case's table, dense (max_items = the words, or the model's states) unless told otherwise"""
    word_off, aut, sil, sil_state = lexicon(case.lex)
    tdp, wp = case.penalties
    off = frame_off(case)
    lexh = m.lexicon(word_off, aut, sil, tdp, sil_state)
    corpus = m.upload(np.zeros((int(off[-1]), MODEL_DIM), np.float32), off)
    try:
        if kind == "post":
            return corpus.word_posteriors_scores(lexh, wp, table(case), case.kappa, floor, max_items or len(word_off) - 1)
        K = max_items or LEXICA[case.lex].S
        if kind == "smbr":
            return corpus.net_accuracies_scores(lexh, wp, labels(case), table(case), case.kappa, floor, K)
        trans = [list(t) for t in transcripts(case)] if kind == "chain" else None
        return corpus.net_occupancies_scores(lexh, wp, table(case), case.kappa, trans, floor, K)
    finally:
        corpus.close()
        lexh.close()


def run_in_child(case, kinds, path, chunk_mb=1, fb_mb=1):
    """the case's calls in a child process under SRGPU_SCORE_CHUNK_MB / SRGPU_FB_MB (read when a model is made) -> {kind: outputs}"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SRGPU_SCORE_CHUNK_MB=str(chunk_mb), SRGPU_FB_MB=str(fb_mb))
    r = subprocess.run([sys.executable, "-m", "tests.netfb_cases", case.name, str(path)] + list(kinds), cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(str(path)) as z:
        return {k: tuple(z[f"{k}{i}"] for i in range(5 if k == "smbr" else 4)) for k in kinds}


def same_bytes(a, b):
    return all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


if __name__ == "__main__":  # run_in_child's child: case, out.npz, kinds
    import sys

    c = by_name(sys.argv[1])
    with open_model(LEXICA[c.lex].S) as model:
        out = {f"{k}{i}": a for k in sys.argv[3:] for i, a in enumerate(run(model, c, k))}
    np.savez(sys.argv[2], **out)
