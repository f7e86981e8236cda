"""Cases for the forward-backward passes over the bigram search network run alone on score tables the test makes up
(sr_bigram_word_posteriors_corpus_scores, sr_bigram_occupancies_corpus_scores, sr_bigram_accuracies_corpus_scores): lexica, language
models, tables, utterance lengths, transcripts, reference labels, the references' answers and the conditions that keep a case from
passing vacuously.  No pytest in here, and the GPU only in run() at the end: tests/test_bigram_fb_cases_cpu.py checks every case's
conditions, tests/test_gpu_bgfb_scores.py, tests/test_gpu_bgocc_scores.py and tests/test_gpu_bgsmbr_scores.py run the kernels on them.
What is generic comes from tests/netfb_cases.py (the tolerance rule, the table kinds' meaning, dense(), same_bytes(), the model file).

The references (tests/bigram_fb_reference.py, bigram_mmi_reference.py, bigram_smbr_reference.py) stay in log space; the device takes the
word entry in the linear domain, as a matrix product relative to the frame's best history.  Two things follow.

The underflow rule.  The device does not enter word w at a frame where every term exp(-kappa lm[w, h]) exp(m - hist_h) underflows
(include/srgpu.h).  cut_entry() states that rule in log space: a term whose exponent (or one of its two factors') lies more than `cut`
below 0 is dropped.  Where exactly a double's exp gives out (-708 for normal numbers, -745 with the subnormal ones) is not for a test to
pin, so no case may have a term between -790 and -650 (exponents(), checked on the CPU): the references cut at 650 and at 790 then agree
exactly, and the device must agree with them.  `gap_far` puts a word's only permitted history 820 behind the frame's best (the word is
not entered; the plain log-space reference enters it), `gap_near` 600 behind (it is entered, and the plain reference is the yardstick).

The tolerance.  netfb_cases.bound() with the float64 distance the larger of two restatements': the log-space reference in float64, and
the same with lin_entry(), which takes the entry sum as exp() and a float64 matrix product like the device."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from tests import bigram_fb_reference as R
from tests import bigram_mmi_reference as BM
from tests import bigram_smbr_reference as BS
from tests import netfb_cases as nc
from tests.netfb_cases import bound, dense, dist, hold, same_bytes, tol_line, ulp  # noqa: F401  (the GPU files take them from here)

MODEL_DIM = nc.MODEL_DIM
INF = math.inf
LD = np.longdouble
TDP = ((3.0, 0.0, 30.0, 5.0), (1.0, 0.0, 40.0, 2.0))
TDP_DYADIC = ((0.5, 0.0, 0.75, 0.25), (0.25, 0.0, 1.5, 0.5))
BLOCK = 512       # kNetFbThreads
BAND = (-790.0, -650.0)
CUT = 720.0       # inside the band: where in it makes no difference to any case


# ---- lexica: states per word, the silence word's index, the model's states ------------------------------------------------------------
@dataclass(frozen=True)
class Lex:
    lens: tuple
    sil: int
    S: int               # the model's states; the silence word takes states 0 .. (its length - 1)
    twins: bool = False  # word 2 k has the states of word 2 k - 1 (k >= 1; silence is word 0)


def _ones_twos(W):
    """silence and W - 1 words of two and one states in turn"""
    return (1,) + tuple(2 - i % 2 for i in range(W - 1))


def _fill_to(P, seed):
    """silence and words of 1 .. 6 states: exactly P positions in the NETWORK (every word also has a silence copy of one position)"""
    rng = np.random.default_rng(seed)
    lens = [1]
    while sum(lens) + len(lens) < P:
        room = P - sum(lens) - len(lens) - 1  # what a further word may have
        n = min(int(rng.integers(1, 7)), room)
        if room - n == 1:                     # (no word of 0 states after it)
            n = room
        lens.append(n)
    return tuple(lens)


LEXICA = {
    "r6": Lex((1, 3, 2, 1, 3, 2), 0, 16),
    "b5": Lex((3, 2, 1, 2, 3), 3, 16),           # silence is word 3 and has two states
    "c3": Lex((3, 1, 2), 1, 12),                 # silence is word 1
    "u6": Lex((1, 2, 1, 2, 2, 1), 0, 16),        # the underflow cases': word 3 after word 2 alone
    "twins": Lex((1, 3, 3, 2, 2, 1, 1), 0, 16, twins=True),
    "long": Lex((1, 70, 2, 3), 0, 96),           # a word of more than 64 positions
    "p513": Lex(_fill_to(BLOCK + 1, 5), 0, 64),  # thread 0 owns positions 0 and 512
    "w63": Lex(_ones_twos(63), 0, 64), "w64": Lex(_ones_twos(64), 0, 64), "w65": Lex(_ones_twos(65), 0, 64),
    "w511": Lex(_ones_twos(511), 0, 64), "w512": Lex(_ones_twos(512), 0, 64), "w513": Lex(_ones_twos(513), 0, 64),
    "chunks": Lex(_fill_to(1000, 6), 0, 768),
}


@functools.lru_cache(maxsize=None)
def lexicon(name):
    """-> (word_off u32[W + 1], mixtures u16[sum of lens], silence word): the silence word takes the states 0 .., the other positions
    the remaining states in turn (all distinct while they last)"""
    lx = LEXICA[name]
    n_sil = lx.lens[lx.sil]
    off = np.concatenate([[0], np.cumsum(lx.lens)]).astype(np.uint32)
    mix, nxt = [], 0
    for w, n in enumerate(lx.lens):
        if w == lx.sil:
            mix += list(range(n_sil))
        elif lx.twins and w >= 2 and w % 2 == 0:
            mix += mix[int(off[w - 1]):int(off[w])]
        else:
            mix += [n_sil + (nxt + i) % (lx.S - n_sil) for i in range(n)]
            nxt += n
    mix = np.asarray(mix, dtype=np.uint16)
    off.setflags(write=False)
    mix.setflags(write=False)
    return off, mix, lx.sil


@functools.lru_cache(maxsize=None)
def net(name):
    return R.Net(*lexicon(name))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
_rng70 = np.random.default_rng(70)
RAGGED70 = tuple(int(t) for t in _rng70.permutation(np.arange(1, 71)))  # the 70 lengths 1 .. 70: n_alive takes every value 70 .. 1
HEADS = (16, 17, 48, 49, 64, 65)
SHORT = (5, 12, 3, 9)
TRIPLE = (9, 12, 6)
HOSTILE = 1  # the utterance that gets the frame of +inf, the NaN, the forced word


@dataclass(frozen=True)
class Case:
    name: str
    lex: str
    table: str = "random"   # random | dyadic | signed | const | int1e3 | inf_band | inf_frame | nan_first | nan_sil | gap
    lens: tuple = SHORT     # frames per utterance
    scale: float = 1.0      # random: U(0, 20) * scale (the transition scores scaled alike) ...
    offset: float = 0.0     # ... + offset
    kappa: float = 1.0
    tdp: tuple = TDP
    lm: str = "random"      # random | dyadic | negative | holes | twins | gap
    gap: float = 0.0        # table and lm "gap": what word 2's states cost more than the others
    trans: str = None       # None: no chains | "random" | a key of CHAINS
    labels: str = "random"  # random | best | none | first
    seed: int = 0
    passes: tuple = ("post", "occ", "smbr")
    sample: tuple = None    # the utterances held against the slow references (None: all)
    plain: bool = False     # the yardstick is the plain log-space reference, not the one with the underflow rule
    base: str = None        # the case whose first utterances these are (the same table, lm and references)
    hostile: tuple = ()     # utterances that need not have a finite F


def case_id(c):
    return c.name


# name -> (lexicon, one transcript per utterance, frames per utterance)
CHAINS = {
    # silence alone; one word; a repeated word; a chain longer than its 2 frames allow (three words of two and three states: no path)
    "shapes": ("r6", ((), (3,), (2, 2), (1, 4, 5), (5, 1)), (4, 3, 7, 2, 9)),
    # b5: silence is word 3, with two states; the second transcript's LM term is forbidden (`holes`: lm[2, 0] = +inf, lm[1, 4] = NaN)
    "forbidden": ("b5", ((0, 4), (0, 2), (4, 1), (0, 1)), (9, 9, 9, 6)),
}


def _cases():
    out = []
    out.append(Case("ragged70", "r6", lens=RAGGED70, trans="random", labels="best"))
    for n in HEADS:
        out.append(Case(f"ragged{n}", "r6", lens=RAGGED70[:n], trans="random", labels="best", base="ragged70", passes=("post", "smbr")))
    out.append(Case("t0_between", "b5", lens=(7, 0, 12, 1, 0, 3), kappa=0.3, trans="random", seed=1))
    out.append(Case("sil1-c3", "c3", lens=TRIPLE + (33,), kappa=2.5, trans="random", seed=2, labels="first"))
    for lx in ("r6", "b5"):
        tr = "random"
        out.append(Case(f"dyadic-{lx}", lx, "dyadic", lens=SHORT, tdp=TDP_DYADIC, lm="dyadic", kappa=0.5, trans=tr))
        out.append(Case(f"signed-{lx}", lx, "signed", lens=SHORT, lm="negative", trans=tr, seed=3))
        out.append(Case(f"x1e3-{lx}", lx, "int1e3", lens=SHORT, scale=1e3, trans=tr, seed=4))
        out.append(Case(f"plus1e6-{lx}", lx, lens=SHORT, offset=1e6, trans=tr, seed=5))
        out.append(Case(f"const-{lx}", lx, "const", lens=SHORT, trans=tr))
        out.append(Case(f"inf_band-{lx}", lx, "inf_band", lens=TRIPLE + (20,), trans=tr, seed=6))
        out.append(Case(f"inf_frame-{lx}", lx, "inf_frame", lens=TRIPLE, trans=tr, hostile=(HOSTILE,)))
        out.append(Case(f"nan_first-{lx}", lx, "nan_first", lens=TRIPLE, trans=tr, hostile=(HOSTILE,)))  # (the chain may be cut; the free
        out.append(Case(f"nan_sil-{lx}", lx, "nan_sil", lens=TRIPLE, trans=tr, hostile=(HOSTILE,)))      # network is not: the CPU test)
        out.append(Case(f"holes-{lx}", lx, lens=SHORT, lm="holes", kappa=0.3, seed=7))
    out.append(Case("labels_none", "r6", labels="none", passes=("smbr",)))
    out.append(Case("labels_first", "b5", labels="first", lens=TRIPLE + (25,), passes=("smbr",)))
    out.append(Case("labels_random", "c3", labels="random", lens=TRIPLE + (25,), passes=("smbr",)))
    out.append(Case("twins", "twins", "dyadic", lens=(12, 9, 30), tdp=TDP_DYADIC, lm="twins", trans="random"))
    out.append(Case("gap_far", "u6", "gap", lens=TRIPLE, scale=0.1, lm="gap", gap=820.0, hostile=(HOSTILE,)))
    out.append(Case("gap_far_k", "u6", "gap", lens=TRIPLE, scale=0.1, lm="gap", gap=328.0, kappa=2.5, hostile=(HOSTILE,), seed=1))
    out.append(Case("gap_near", "u6", "gap", lens=TRIPLE, scale=0.1, lm="gap", gap=600.0, plain=True))
    # the launch shape: the padding to Kp, the strided loops over W and P, the words kernel's lanes
    for lx in ("w63", "w64", "w65"):
        out.append(Case(lx, lx, lens=SHORT, seed=8, lm="holes" if lx == "w65" else "random"))
    for lx in ("w511", "w512", "w513"):
        out.append(Case(lx, lx, lens=(12, 3, 7, 10), seed=9, kappa=0.3))
    out.append(Case("long", "long", lens=(60, 45, 70), scale=0.1, seed=10))  # (at U(0, 20) the 70 states' ends lie up to 700 apart)
    out.append(Case("p513", "p513", lens=(12, 6, 9), seed=11, trans="random"))
    for k in CHAINS:
        out.append(Case(f"chain-{k}", CHAINS[k][0], lens=CHAINS[k][2], trans=k, passes=("occ",), lm="holes" if k == "forbidden" else "random",
                        seed=12, hostile=tuple(range(len(CHAINS[k][2])))))
    rng = np.random.default_rng(2424)
    out.append(Case("chunks", "chunks", lens=tuple(int(t) for t in rng.integers(10, 41, size=24)), seed=13, trans="random", kappa=0.3))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


def root(case):
    return by_name(case.base) if case.base else case


# ---- transition scores, language models, tables, transcripts, labels ------------------------------------------------------------------------
def tdp32(case):
    """f32[2, 4]: what the device gets, and (as float64) the references"""
    return (np.asarray(case.tdp, dtype=np.float64) * case.scale).astype(np.float32)


def frame_off(case):
    off = np.concatenate([[0], np.cumsum(case.lens)]).astype(np.uint64)
    off.setflags(write=False)
    return off


GAP_W, GAP_H = 3, 2  # u6: word 3 is entered from history 2 alone


@functools.lru_cache(maxsize=None)
def lm(case):
    """f32[W, W], lm[w, h] = the score of word w after history h (the silence row is never read)"""
    case = root(case)
    W, sil = net(case.lex).W, LEXICA[case.lex].sil
    rng = np.random.default_rng(8300 + case.seed)
    if case.lm == "dyadic" or case.lm == "twins":
        t = rng.integers(0, 17, size=(W, W)).astype(np.float64) * 0.25
    elif case.lm == "negative":
        t = rng.uniform(-3.0, 5.0, size=(W, W))
    else:
        t = rng.uniform(0.0, 8.0, size=(W, W))
    if case.lm == "twins":  # word 2 k like word 2 k - 1, as a word and as a history
        for k in range(2, W, 2):
            t[k, :] = t[k - 1, :]
        for k in range(2, W, 2):
            t[:, k] = t[:, k - 1]
    if case.lm == "holes":
        t[rng.random((W, W)) < 0.15] = INF
        words = [w for w in range(W) if w != sil]
        t[:, words[-1]] = np.nan                # a column all forbidden: after that word only its silence copy
        t[words[1], :] = INF                    # a word reachable from one history only
        t[words[1], words[0]] = 0.5
        t[words[0], sil] = 1.0                  # (some word can follow the start's silence history)
        t[words[2 % len(words)], words[0]] = INF  # (chain-forbidden's transcripts)
        t[words[-1], words[0]] = 2.0
        if W > 4:
            t[1, 4] = np.nan
    if case.lm == "gap":
        t = rng.uniform(0.0, 3.0, size=(W, W))
        t[GAP_W, :] = INF
        t[GAP_W, GAP_H] = 1.0
    t = np.ascontiguousarray(t, dtype=np.float32)
    t.setflags(write=False)
    return t


def _first_state_slot(nt):
    """the first position of a word (not the silence) of two or more states whose first state no other position carries"""
    for x in range(nt.W):
        p = int(nt.slot_off[x])
        if x != nt.sil and nt.slot_off[x + 1] - p >= 2 and np.sum(nt.state == nt.state[p]) == 1:
            return p
    raise AssertionError("no such word")


def nan_cell(case):
    """(frame of the hostile utterance, state) that gets the NaN"""
    nt = net(case.lex)
    t = case.lens[HOSTILE] // 2
    if case.table == "nan_first":
        return t, int(nt.state[_first_state_slot(nt)])
    return t, int(nt.state[nt.slot_off[nt.sil + 1] - 1])  # nan_sil: the silence's last state -- the silence word's and every copy's


@functools.lru_cache(maxsize=None)
def table(case):
    """[F, S] f64, never written to"""
    if case.base:
        t = table(root(case))[:int(frame_off(case)[-1])]
        return t
    S = LEXICA[case.lex].S
    rng = np.random.default_rng(8000 + case.seed)
    off = frame_off(case)
    F = int(off[-1])
    nt = net(case.lex)
    if case.table == "dyadic":
        t = rng.integers(0, 17, size=(F, S)).astype(np.float64) * 0.25
    elif case.table == "signed":
        t = rng.uniform(-50.0, 50.0, size=(F, S))
    elif case.table == "const":
        t = np.full((F, S), 2.5)
    elif case.table == "int1e3":  # whole thousands, like the transition scores: no two histories lie between 650 and 790 apart
        t = rng.integers(0, 21, size=(F, S)).astype(np.float64) * case.scale
    else:
        t = rng.uniform(0.0, 20.0, size=(F, S)) * case.scale + case.offset
    sil_states = np.unique(nt.state[nt.is_sil == 1])
    if case.table == "inf_band":  # every state but the silence's: one way through the frames of the middle third
        for u in range(len(case.lens)):
            f0, T = int(off[u]), case.lens[u]
            keep = np.zeros(S, bool)
            keep[sil_states] = True
            t[f0 + T // 3:f0 + 2 * T // 3 + 1][:, ~keep] = INF
    elif case.table == "inf_frame":
        t[int(off[HOSTILE]) + case.lens[HOSTILE] // 2] = INF
    elif case.table.startswith("nan_"):
        tt, k = nan_cell(case)
        t[int(off[HOSTILE]) + tt, k] = np.nan
    elif case.table == "gap":
        states = lambda w: nt.state[nt.slot_off[w]:nt.slot_off[w + 1]]  # noqa: E731
        t[:, states(GAP_H)] += case.gap
        f1 = int(off[HOSTILE + 1])  # the hostile utterance's last three frames: word GAP_W or nothing
        keep = np.zeros(S, bool)
        keep[states(GAP_W)] = True
        t[f1 - 3:f1][:, ~keep] = INF
    t.setflags(write=False)
    return t


def rows(case, u, clean=True):
    off = frame_off(case)
    t = table(case)[int(off[u]):int(off[u + 1])]
    return nc.sanitised(t) if clean else t


@functools.lru_cache(maxsize=None)
def transcripts(case):
    """one tuple of word ids per utterance (silence not listed), or None"""
    if case.trans is None:
        return None
    if case.base:
        return transcripts(root(case))[:len(case.lens)]
    if case.trans in CHAINS:
        return CHAINS[case.trans][1]
    rng = np.random.default_rng(8100 + case.seed)
    nt = net(case.lex)
    words = [w for w in range(nt.W) if w != nt.sil]
    out = []
    for T in case.lens:  # few enough words for a path: a word of n states takes at least ceil(n / 2) frames
        tr, need = [], 0
        for _ in range(int(rng.integers(0, 4))):
            w = words[int(rng.integers(0, len(words)))]
            n = int(nt.slot_off[w + 1] - nt.slot_off[w])
            if need + (n + 1) // 2 <= T:
                tr.append(w)
                need += (n + 1) // 2
        out.append(tuple(tr))
    return tuple(out)


def best_path(e, nt, lm_, tdp):
    """the mixtures of the best path (the min semiring at kappa = 1) by walking bigram_fb_reference.forward's costs back"""
    T = e.shape[0]
    out = np.zeros(T, dtype=np.uint16)
    if T == 0:
        return out
    with np.errstate(invalid="ignore"):
        A, WE = R.forward(e, nt, lm_, tdp, "min", 1.0)
    if not np.isfinite(WE[T]).any():
        return out
    klm, td = R._klm(nt, lm_, 1.0), R._tdp(tdp, 1.0)
    W = nt.W
    p = int(nt.last[int(np.argmin(WE[T]))])
    for t in range(T - 1, -1, -1):
        out[t] = nt.state[p]
        if t == 0:
            break
        s, k, x = int(nt.is_sil[p]), int(nt.k[p]), int(nt.slot[p])
        cand = [(A[t - 1, p - j] + td[s, j], p - j) for j in range(3) if k >= j]
        if k <= 1:  # an entry: from which word end
            we = WE[t]
            if x >= W:
                src, c = x - W, we[x - W]
            elif x == nt.sil:
                src, c = x, we[x]
            else:
                hist = R.histories(nt, we, "min")
                h = int(np.argmin(hist + klm[x]))
                c = hist[h] + klm[x, h]
                src = h if (h == nt.sil or we[h] <= we[h + W]) else h + W
            cand.append((c + (td[s, 2] if k == 1 else 0.0), int(nt.last[src])))
        p = min(cand, key=lambda v: v[0])[1]
    return out


@functools.lru_cache(maxsize=None)
def labels(case):
    """u16[F]: the reference mixture of every frame"""
    if case.base:
        return labels(root(case))[:int(frame_off(case)[-1])]
    nt = net(case.lex)
    S = LEXICA[case.lex].S
    off = frame_off(case)
    rng = np.random.default_rng(8200 + case.seed)
    out = np.zeros(int(off[-1]), dtype=np.uint16)
    for u, T in enumerate(case.lens):
        f0 = int(off[u])
        if case.labels == "none":
            out[f0:f0 + T] = S + (np.arange(T) % 3)
        elif case.labels == "first":
            out[f0:f0 + T] = nt.state[_first_state_slot(nt)]
        elif case.labels == "best":
            out[f0:f0 + T] = best_path(rows(case, u), nt, lm(case), tdp32(case))
        else:
            out[f0:f0 + T] = rng.choice(np.unique(nt.state), size=T)
    out.setflags(write=False)
    return out


# ---- the word entry, restated: the underflow rule in log space, and the linear domain in float64 ---------------------------------------------
def _entry_terms(vec, klm, axis, sil, cut, seen):
    """the W x W terms of an entry sum with those dropped that underflow against the best of `vec`, or None where that is +inf"""
    v = np.array(vec)
    if axis == 0:
        v[sil] = INF  # (backward: the LM enters no silence, and its own entry cost is not among the minimum's)
    m = v.min()
    if not np.isfinite(m):
        return None
    col = v[None, :] if axis == 1 else v[:, None]
    with np.errstate(invalid="ignore"):
        terms = col + klm
        ex = np.minimum(np.minimum(m - terms, np.broadcast_to(m - col, terms.shape)), -klm)  # the product's exponent, and its factors'
    live = np.isfinite(terms)
    if seen is not None:
        x = ex[live].astype(np.float64)
        seen["band"] = seen.get("band", 0) + int(np.sum((x > BAND[0]) & (x < BAND[1])))
        seen["dropped"] = seen.get("dropped", 0) + int(np.sum(x <= BAND[0]))
    return np.where(live & (ex > -cut), terms, terms.dtype.type(INF))


def cut_entry(sil, cut=CUT, seen=None):
    """bigram_fb_reference's entry_sum with the device's underflow rule"""
    def f(vec, klm, axis):
        terms = _entry_terms(vec, klm, axis, sil, cut, seen)
        return np.full(klm.shape[1 - axis], INF, dtype=klm.dtype) if terms is None else R._lsum(terms, axis=axis)
    return f


def cut_entry_mean(sil, cut=CUT, seen=None):
    """bigram_smbr_reference's entry_sum with the device's underflow rule"""
    def f(vec, vals, klm, axis):
        terms = _entry_terms(vec, klm, axis, sil, cut, seen)
        if terms is None:
            return np.full(klm.shape[1 - axis], INF, dtype=klm.dtype), np.zeros(klm.shape[1 - axis], dtype=klm.dtype)
        return BS._wmean(terms, vals[None, :] if axis == 1 else vals[:, None], axis=axis)
    return f


def _lin(vec, klm, axis, sil):
    v = np.array(vec, dtype=np.float64)
    if axis == 0:
        v[sil] = INF
    m = v.min()
    if not np.isfinite(m):
        return None
    with np.errstate(under="ignore"):
        a = np.where(np.isfinite(v), np.exp(m - np.where(np.isfinite(v), v, m)), 0.0)
        Lk = np.exp(-klm)
    return m, a, (Lk if axis == 1 else Lk.T)


def lin_entry(sil):
    """the entry sum as the device takes it: exp(-klm) times exp(m - vec) in float64 (what underflows, underflows)"""
    def f(vec, klm, axis):
        r = _lin(vec, klm, axis, sil)
        if r is None:
            return np.full(klm.shape[1 - axis], INF)
        m, a, Lk = r
        with np.errstate(under="ignore", divide="ignore"):
            X = Lk @ a
            return np.where(X > 0, m - np.log(np.where(X > 0, X, 1.0)), INF)
    return f


def lin_entry_mean(sil):
    def f(vec, vals, klm, axis):
        r = _lin(vec, klm, axis, sil)
        if r is None:
            return np.full(klm.shape[1 - axis], INF), np.zeros(klm.shape[1 - axis])
        m, a, Lk = r
        with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
            X, XA = Lk @ a, Lk @ (a * np.where(np.isfinite(vec), vals, 0.0))
            return np.where(X > 0, m - np.log(np.where(X > 0, X, 1.0)), INF), np.where(X > 0, XA / np.where(X > 0, X, 1.0), 0.0)
    return f


# ---- references: per utterance, once, shared ---------------------------------------------------------------------------------------------
_DT = {"float64": np.float64, "longdouble": LD}


def sampled(case):
    return tuple(range(len(case.lens))) if case.sample is None else case.sample


def _entry(case, variant, mean, seen=None):
    """variant: cut (the yardstick and its float64 run) | lin (float64 only) | plain | cut650 | cut790"""
    sil = LEXICA[case.lex].sil
    if variant == "plain":
        return None
    if variant == "lin":
        return (lin_entry_mean if mean else lin_entry)(sil)
    cut = {"cut": CUT, "cut650": -BAND[1], "cut790": -BAND[0]}[variant]
    return (cut_entry_mean if mean else cut_entry)(sil, cut, seen)


def yardstick(case):
    return "plain" if case.plain else "cut"


@functools.lru_cache(maxsize=None)
def free_reference(case, dtype_name, variant):
    """{u: (F, word posteriors [T, W], occupancies [T, S])} of the free network on the sanitised table"""
    if case.base:
        r = free_reference(root(case), dtype_name, variant)
        return {u: r[u] for u in range(len(case.lens))}
    nt, S, dt = net(case.lex), LEXICA[case.lex].S, _DT[dtype_name]
    out = {}
    for u in sampled(case):
        with np.errstate(all="ignore"):
            kF, G = R.gammas(rows(case, u), nt, lm(case), tdp32(case), case.kappa, _entry(case, variant, False), dt)
        p, occ = R.collect(G, nt.word, nt.W), R.collect(G, nt.state, S)
        p.setflags(write=False)
        occ.setflags(write=False)
        out[u] = (kF / dt(case.kappa), p, occ)
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(case, dtype_name):
    """{u: (F, occupancies [T, S])} of the transcripts' chains (log space throughout, on the device too)"""
    if case.base:
        r = chain_reference(root(case), dtype_name)
        return {u: r[u] for u in range(len(case.lens))}
    out = {}
    for u in sampled(case):
        with np.errstate(all="ignore"):
            F, occ = BM.chain_occupancies(rows(case, u), net(case.lex), lm(case), tdp32(case), transcripts(case)[u], case.kappa,
                                          dtype=_DT[dtype_name])
        occ.setflags(write=False)
        out[u] = (F, occ)
    return out


@functools.lru_cache(maxsize=None)
def smbr_reference(case, dtype_name, variant):
    """{u: (F, Abar, gamma [T, S])} of the accuracy recursion"""
    if case.base:
        r = smbr_reference(root(case), dtype_name, variant)
        return {u: r[u] for u in range(len(case.lens))}
    off = frame_off(case)
    out = {}
    for u in sampled(case):
        with np.errstate(all="ignore"):
            F, A, g = BS.smbr(rows(case, u), net(case.lex), lm(case), tdp32(case), labels(case)[int(off[u]):int(off[u + 1])], case.kappa,
                              dtype=_DT[dtype_name], entry_sum=_entry(case, variant, True))
        g.setflags(write=False)
        out[u] = (F, A, g)
    return out


def exponents(case):
    """{"band": terms of any entry sum of the case with an exponent inside BAND, "dropped": those below it}, forward and backward, of
    the float64 run cut at 790 (which keeps every term above the band: none it would meet is hidden by an earlier drop)"""
    seen = {"band": 0, "dropped": 0}
    entry = cut_entry(LEXICA[case.lex].sil, -BAND[0], seen)
    for u in range(len(case.lens)):
        with np.errstate(all="ignore"):
            R.gammas(rows(case, u), net(case.lex), lm(case), tdp32(case), case.kappa, entry)
    return seen


def restatements(case, kind, u):
    """the float64 runs the rule measures the number format with, for utterance u: [(F, weights)] (smbr: [(F, Abar, gamma)])"""
    if kind == "chain":
        return [chain_reference(case, "float64")[u]]
    vs = (yardstick(case), "lin")
    if kind == "smbr":
        return [smbr_reference(case, "float64", v)[u] for v in vs]
    i = 1 if kind == "post" else 2
    return [(r[0], r[i]) for r in (free_reference(case, "float64", v)[u] for v in vs)]


def reference(case, kind, u):
    """the longdouble yardstick for utterance u: (F, weights) (smbr: (F, Abar, gamma))"""
    if kind == "chain":
        return chain_reference(case, "longdouble")[u]
    if kind == "smbr":
        return smbr_reference(case, "longdouble", yardstick(case))[u]
    r = free_reference(case, "longdouble", yardstick(case))[u]
    return r[0], r[1 if kind == "post" else 2]


# ---- the rule for the suites on fixed tolerances (test_gpu_bigram_posteriors.py, test_gpu_bigram_mmi.py, test_gpu_bigram_smbr.py) ----------
def rule(fixed, v64s, v80, tag=None):
    """netfb_cases.tighter with the float64 distance the larger of several restatements': value by value the rule's bound against the
    longdouble run where it is tighter than the fixed one for every restatement, +inf where it is not (there the fixed bound against
    the float64 run, which those suites go on asserting, stays what holds)"""
    return np.max(np.stack([np.asarray(nc.tighter(fixed, v, v80, tag and f"{tag} ({i})"), dtype=np.float64) for i, v in enumerate(v64s)]), axis=0)


def measured(run, r64, entry, fixed, tag=None):
    """For one utterance of those suites: run(dtype=, entry_sum=) is its restatement -> (F, weights) or (F, Abar, gamma), r64 what it
    gave in float64, entry the linear-domain entry of its network (None: a chain, which has no product), fixed the suite's bounds in
    the order of the outputs.  -> (the longdouble run, [rule(...) per output]); an utterance without a path or without frames gets
    bounds of 0 (the suites compare its F exactly)"""
    with np.errstate(all="ignore"):
        r80 = run(dtype=LD)
        rs = [r64] + ([run(entry_sum=entry)] if entry is not None else [])
    if not np.isfinite(r80[0]) or np.asarray(r80[-1]).shape[0] == 0:
        return r80, [np.zeros(np.shape(v)) for v in r80]
    return r80, [rule(f, [r[i] for r in rs], r80[i], tag and f"{tag} output {i}") for i, f in enumerate(fixed)]


# ---- the launch plan at SRGPU_SCORE_CHUNK_MB=1 SRGPU_FB_MB=1, restated (make_chunks, srplan::linear_cost, srplan::launch_groups) ------------
def plan(case, mult, chunk_mb=1, fb_mb=1):
    """-> [chunk: [(u0, u1) launch groups]] of the free network's pass at multiplicity mult (1: posteriors and occupancies, 2: accuracies)"""
    S, nt = LEXICA[case.lex].S, net(case.lex)
    ld = (S + 7) // 8 * 8
    Kp = (nt.W + 63) // 64 * 64
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
    per_utt = mult * (24 * Kp + 16 * nt.P + 8)
    cost = [mult * 8 * nt.P * off[i] + i * per_utt for i in range(U + 1)]
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


# ---- the calls (the only part that touches the GPU) -----------------------------------------------------------------------------------------
def open_model(S):
    return nc.open_model(S)


def open_net(m, case):
    word_off, mixtures, sil = lexicon(case.lex)
    return m.bigram(word_off, mixtures, sil, lm(case), tdp32(case))


def run(m, case, kind, floor=0.0, max_items=None, bg=None, kappa=None, tab=None):
    """kind post -> (F, count, word, weight); occ / chain -> (F, count, state, weight); smbr -> (F, Abar, count, state, weight): the
    hook on the case's table, dense (max_items = the words, or the model's states) unless told otherwise"""
    off = frame_off(case)
    own = bg is None
    bg = open_net(m, case) if own else bg
    kappa = case.kappa if kappa is None else kappa
    tab = table(case) if tab is None else tab
    corpus = m.upload(np.zeros((int(off[-1]), MODEL_DIM), np.float32), off)
    try:
        if kind == "post":
            return corpus.bigram_word_posteriors_scores(bg, tab, kappa, floor, max_items or net(case.lex).W)
        K = max_items or LEXICA[case.lex].S
        if kind == "smbr":
            return corpus.bigram_accuracies_scores(bg, labels(case), tab, kappa, floor, K)
        trans = [list(t) for t in transcripts(case)] if kind == "chain" else None
        return corpus.bigram_occupancies_scores(bg, tab, kappa, trans, floor, K)
    finally:
        corpus.close()
        if own:
            bg.close()


def run_in_child(case, kinds, path, chunk_mb=1, fb_mb=1):
    """the case's calls in a child process under SRGPU_SCORE_CHUNK_MB / SRGPU_FB_MB (read when a model is made) -> {kind: outputs}"""
    import os
    import subprocess
    import sys

    top = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SRGPU_SCORE_CHUNK_MB=str(chunk_mb), SRGPU_FB_MB=str(fb_mb))
    r = subprocess.run([sys.executable, "-m", "tests.bigram_fb_cases", case.name, str(path)] + list(kinds), cwd=top, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(str(path)) as z:
        return {k: tuple(z[f"{k}{i}"] for i in range(5 if k == "smbr" else 4)) for k in kinds}


if __name__ == "__main__":  # run_in_child's child: case, out.npz, kinds
    import sys

    c = by_name(sys.argv[1])
    with open_model(LEXICA[c.lex].S) as model:
        out = {f"{k}{i}": a for k in sys.argv[3:] for i, a in enumerate(run(model, c, k))}
    np.savez(sys.argv[2], **out)
