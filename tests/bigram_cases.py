"""Cases for the bigram search kernels (viterbi_bigram.hip) run alone on score tables the test makes up
(sr_recognize_bigram_corpus_scores): lexica with the kernel route each must get, LM tables, score tables, batches, the oracle's answers
and the conditions that keep a case from passing vacuously.  No GPU and no pytest in here: tests/test_bigram_cases_cpu.py checks every
case's conditions and route, tests/test_gpu_bigram_scores.py runs the kernels on them.

Why tables: see tests/search_cases.py.  Here every number that enters a path sum is dyadic in the `dyadic` kinds -- score tables and LM
tables hold multiples of 0.25, the transition and exit penalties are multiples of 0.5, beams multiples of 0.125 -- so sums below 2^13 are
exact in float and equal sums are equal bits: ties between word ends, hypotheses exactly ON best + beam, word ends exactly on the bound
of the recombination's skip test.  The search casts a double score to float; the `real` tables hold doubles that are not floats, so the
rounding of that cast is compared too.

Words draw their states from a pool of 12 (the silence word takes states 0 .. its length - 1), so a table is a few columns wide;
`model_states` widens the model (and the table) where a case is about the row length: the register layout copies a row to the LDS in
1 KiB pieces dealt to 16 waves.

The route rules are restated here in Python (route()); tests/test_bigram_route_cpu.py holds the restatement against the function the
launch switches on (speechrecognition_amd/csrc/bigram_route.h) compiled alone."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import search_cases as sc

FLT_MAX = float(np.finfo(np.float32).max)
POOL = 12
TDP = np.array([[3.0, 0.0, 30.0, 1.0], [2.0, 0.0, 40.0, 1.5]], np.float32)
SIL_TDP = np.array([[3.0, 0.0, 30.0, 5.0], [1.0, 7.0, 3.0, 2.0]], np.float32)  # tests/test_bigram.py: the silence's own forward / skip
TIE_TDP = np.array([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 0.0]], np.float32)  # every transition alike, for words and for silence
MODEL_DIM = sc.MODEL_DIM
model_file = sc.model_file
KINDS = sc.KINDS + ("neginf", "const")


# ---- the route rules, restated ------------------------------------------------------------------------------------------------------
LDS_BYTES = 160 * 1024


def _up(x, a):
    return (x + a - 1) // a * a


def lds_small(W):
    """entries 16 W, staging 3 x 256 words, scan and reduction scratch 33 words, two active lists 8 W, flags 2 W, 64"""
    return 26 * W + 3268


def lds_dense(W, P2):
    return 8 * P2 + lds_small(W)


def lds_row_off(W):
    return _up(_up(lds_small(W), 16) + 8 * W, 1024)


def lds_regs(W, ld):
    return lds_row_off(W) + _up(8 * ld, 1024)


def gs_lds(W, entries_global):
    return _up(lds_small(W) - (16 * W if entries_global else 0), 16) + 8 * W


def dense_fit(W):
    """the most positions whose dense image fits the LDS beside W words' lists"""
    return (LDS_BYTES - lds_small(W)) // 8


def ld_fit(W):
    """the longest score row (doubles) the register layout takes at W words"""
    return (LDS_BYTES - lds_row_off(W)) // 1024 * 128


def staging_capacity(W):
    """word ends one pass of the recombination stages: 256, or min(W / 3, 1024) where that is more"""
    return min(4 * W // 12, 1024) if 4 * W // 12 > 256 else 256


def route(W, P2, ld, max_slot_states, silence_states, row4_mask, dense=False, glob=False):
    """-> the text of sr_bigram_route"""
    if W < 1 or W > 8192 or P2 < 2 * W or (dense and glob):
        return "none"
    rows = -(-W // 1024)
    kw = 1 if rows <= 1 else 2 if rows <= 2 else 4 if rows <= 4 else 8
    if not glob:
        if not dense and max_slot_states <= 4 and silence_states == 1 and W <= 3072 and lds_regs(W, ld) <= LDS_BYTES:
            every = (1 << rows) - 1
            mask = 0 if max_slot_states <= 3 else (row4_mask & every) or every
            return f"registers {rows} rows4 {bin(mask)}"
        if lds_dense(W, P2) <= LDS_BYTES:
            pr = -(-P2 // 1024)
            return f"lds {kw} x {4 if pr <= 4 else 12 if pr <= 12 else 20}"
        if dense:
            return "none"
    return f"global {kw} entries {'global' if gs_lds(W, False) > LDS_BYTES else 'lds'}"


# every instantiation the launcher has: 14 of the register layout, 8 of the dense LDS layout, 5 of the global-states layout
ROUTES = tuple([f"registers {r} rows4 {bin(m)}" for r in (1, 2, 3) for m in range(1 << r) if r > 1 or m < 2]
               + [f"lds {kw} x {kp}" for kw, kp in ((1, 4), (1, 12), (1, 20), (2, 4), (2, 12), (2, 20), (4, 12), (4, 20))]
               + [f"global {kw} entries lds" for kw in (1, 2, 4, 8)] + ["global 8 entries global"])


# ---- lexica -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lex:
    """A named lexicon and the exact route text it must get with no flag, with dense_states and with global_states."""
    name: str
    W: int
    lens: tuple               # (lo, hi): word lengths drawn from lo .. hi
    route: str
    route_dense: str
    route_global: str
    sil_states: int = 1
    sil_idx: int = 0
    four: tuple = ()          # words of exactly four states (register lexica: they set the row mask)
    p2: int = None            # the exact number of positions (words and silence copies), by stretching or shrinking the words
    model_states: int = 16
    seed: int = 0
    n_long: int = 2
    frames: tuple = (30, 60)
    beams: tuple = (12.0, 6.0)  # acoustic, LM
    tie_tdp: bool = False

    @property
    def tdp(self):
        return TIE_TDP if self.tie_tdp else SIL_TDP if self.sil_states > 1 else TDP

    def route_for(self, flags):
        return {"": self.route, "dense": self.route_dense, "global": self.route_global}[flags]


LEXICA = {}


def _add(name, W, lens, route_, route_dense, route_global, **kw):
    LEXICA[name] = Lex(name, W, lens, route_, route_dense, route_global, **kw)


def _bits(mask):
    return bin(mask)


# register layout: words of one to three states, four-state words at the edges of the 1024-word slot rows where the mask allows it
#   W 40: row 0;  W 1100: rows 0, 1 (words 1023 | 1024, 1099);  W 2100: rows 0, 1, 2 (1023 | 1024, 2047 | 2048, 2099)
_EDGES = {40: ((5, 39),), 1100: ((1023,), (1024, 1099)), 2100: ((1023,), (1024, 2047), (2048, 2099))}
for _W, _rows, _kw in ((40, 1, 1), (1100, 2, 2), (2100, 3, 4)):
    for _m in range(1 << _rows):
        _four = tuple(w for r in range(_rows) if (_m >> r) & 1 for w in _EDGES[_W][r])
        # (silence copies of one state: P2 = the words' states + W <= 4 W: 4 or 12 positions a thread)
        _add(f"r{_W}m{_m}", _W, (1, 3), f"registers {_rows} rows4 {_bits(_m)}", f"lds {_kw} x {12 if _W == 2100 else 4}",
             f"global {_kw} entries lds", four=_four, sil_idx=0 if _m % 2 == 0 else 7, seed=10 * _rows + _m,
             beams={40: (12.0, 6.0), 1100: (8.0, 4.0), 2100: (6.0, 3.0)}[_W])
# every word of one state: every word ends in every frame, and the book of an utterance is exactly full at max_word_ends = W
_add("r40one", 40, (1, 1), "registers 1 rows4 0b0", "lds 1 x 4", "global 1 entries lds", seed=5)
# everything alike: with TIE_TDP, a flat LM and a constant table a word and its silence copy end in the same frame at the same score, and
# so do all words of a length; list order alone decides
_add("r40tie", 40, (1, 3), "registers 1 rows4 0b1", "lds 1 x 4", "global 1 entries lds", four=(5, 39), seed=6, tie_tdp=True, beams=(3.0, 2.0))
_add("r1100tie", 1100, (1, 3), "registers 2 rows4 0b11", "lds 2 x 4", "global 2 entries lds", four=(1023, 1024, 1099), sil_idx=7, seed=7,
     tie_tdp=True, beams=(3.0, 2.0))
_add("l300tie", 300, (1, 6), "lds 1 x 4", "lds 1 x 4", "global 1 entries lds", sil_states=2, sil_idx=3, seed=8, tie_tdp=True, beams=(3.0, 2.0))
# the row DMA of the register layout: 128 bytes (a tail alone), 2 048 (two pieces, no tail), 2 KiB + 384, more than 16 KiB (wave 0 and 1
# take two pieces), the longest row that fits beside 2 100 words' lists (87 KiB) and 8 doubles more, which leaves the layout
_add("r40row2048", 40, (1, 3), "registers 1 rows4 0b1", "lds 1 x 4", "global 1 entries lds", four=(5, 39), model_states=256, seed=11)
_add("r1100row2432", 1100, (1, 3), "registers 2 rows4 0b10", "lds 2 x 4", "global 2 entries lds", four=(1024, 1099), model_states=304, seed=22,
     beams=(8.0, 4.0))
_add("r40row18k", 40, (1, 3), "registers 1 rows4 0b0", "lds 1 x 4", "global 1 entries lds", model_states=2304 + 5, seed=12)
_add("r2100rowfit", 2100, (1, 3), "registers 3 rows4 0b100", "lds 4 x 12", "global 4 entries lds", four=(2048, 2099), model_states=ld_fit(2100),
     seed=34, beams=(6.0, 3.0))
_add("r2100rowover", 2100, (1, 3), "lds 4 x 12", "lds 4 x 12", "global 4 entries lds", four=(2048, 2099), model_states=ld_fit(2100) + 1, seed=34,
     beams=(6.0, 3.0))
# dense LDS layout: the eight (KW, KP); P2 exactly 4 096 | 4 097 and 12 288 | 12 289; the most positions that fit at W and one more.
# Silence words of 2 and 3 states with SIL_TDP's own silence penalties (what the register layout refuses), or words beyond four states.
_add("l1p4096", 300, (2, 9), "lds 1 x 4", "lds 1 x 4", "global 1 entries lds", sil_states=2, p2=4096, seed=41, beams=(24.0, 8.0))
_add("l1p4097", 300, (2, 9), "lds 1 x 12", "lds 1 x 12", "global 1 entries lds", sil_states=2, p2=4097, sil_idx=3, seed=42, beams=(24.0, 8.0))
_add("l1p12288", 600, (5, 20), "lds 1 x 12", "lds 1 x 12", "global 1 entries lds", sil_states=3, p2=12288, seed=43, beams=(40.0, 10.0))
_add("l1p12289", 600, (5, 20), "lds 1 x 20", "lds 1 x 20", "global 1 entries lds", sil_states=3, p2=12289, seed=44, beams=(40.0, 10.0))
_add("l1fit", 500, (20, 40), "lds 1 x 20", "lds 1 x 20", "global 1 entries lds", p2=dense_fit(500), seed=45, frames=(50, 70), beams=(60.0, 12.0))
_add("l1over", 500, (20, 40), "global 1 entries lds", "none", "global 1 entries lds", p2=dense_fit(500) + 1, seed=45, frames=(50, 70), beams=(60.0, 12.0))
_add("l2p4096", 1100, (1, 2), "lds 2 x 4", "lds 2 x 4", "global 2 entries lds", sil_states=2, p2=4096, seed=46, beams=(8.0, 4.0))
_add("l2p4097", 1100, (1, 2), "lds 2 x 12", "lds 2 x 12", "global 2 entries lds", sil_states=2, p2=4097, seed=47, beams=(8.0, 4.0))
_add("l2p12288", 1500, (2, 8), "lds 2 x 12", "lds 2 x 12", "global 2 entries lds", sil_states=3, p2=12288, seed=48, beams=(16.0, 6.0))
_add("l2p12289", 1500, (2, 8), "lds 2 x 20", "lds 2 x 20", "global 2 entries lds", sil_states=3, p2=12289, sil_idx=9, seed=49, beams=(16.0, 6.0))
_add("l4p12288", 2100, (2, 5), "lds 4 x 12", "lds 4 x 12", "global 4 entries lds", sil_states=2, p2=12288, seed=50, beams=(8.0, 4.0))
_add("l4p12289", 2100, (2, 5), "lds 4 x 20", "lds 4 x 20", "global 4 entries lds", sil_states=2, p2=12289, seed=51, beams=(8.0, 4.0))
_add("l4fit", 2100, (3, 7), "lds 4 x 20", "lds 4 x 20", "global 4 entries lds", p2=dense_fit(2100), seed=52, beams=(8.0, 4.0))
_add("l4over", 2100, (3, 7), "global 4 entries lds", "none", "global 4 entries lds", p2=dense_fit(2100) + 1, seed=52, beams=(8.0, 4.0))
# global states: beyond 4 096 words (KW 8), the entries in device memory too from 4 723 words on; long words at a small W; a silence
# of three states.  The oracle costs W x (word ends) a frame: 20 frames or fewer, beams on.
_add("g4200", 4200, (1, 3), "global 8 entries lds", "none", "global 8 entries lds", sil_states=3, seed=61, frames=(18, 22), beams=(6.0, 3.0))
_add("g4722", 4722, (1, 3), "global 8 entries lds", "none", "global 8 entries lds", seed=62, frames=(18, 22), beams=(5.0, 2.5))
_add("g4723", 4723, (1, 3), "global 8 entries global", "none", "global 8 entries global", seed=62, frames=(18, 22), beams=(5.0, 2.5))
_add("g8192", 8192, (1, 3), "global 8 entries global", "none", "global 8 entries global", sil_idx=8191, seed=63, frames=(6, 8), beams=(3.0, 1.5))
_add("glong", 800, (18, 24), "global 1 entries lds", "none", "global 1 entries lds", seed=64, frames=(50, 70), beams=(40.0, 10.0))
# the persistent grid of the global-states layout: W 60, several hundred utterances (tests/test_gpu_bigram_scores.py)
_add("g60", 60, (2, 9), "lds 1 x 4", "lds 1 x 4", "global 1 entries lds", seed=65)


@functools.lru_cache(maxsize=None)
def lexicon(name):
    """-> (word_off u32[W + 1], mixtures u16[], lengths i64[W])"""
    spec = LEXICA[name]
    rng = np.random.default_rng(5000 + spec.seed)
    W = spec.W
    n = rng.integers(spec.lens[0], spec.lens[1] + 1, size=W)
    n[list(spec.four)] = 4
    n[spec.sil_idx] = spec.sil_states
    if spec.p2 is not None:
        free = np.array([w for w in range(W) if w != spec.sil_idx and w not in spec.four])
        q, r = divmod(spec.p2 - W * spec.sil_states - int(n.sum()), len(free))
        n[free] += q
        n[free[:r]] += 1
        assert n.min() >= 1 and int(n.sum()) + W * spec.sil_states == spec.p2
    word_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    mixtures = rng.integers(spec.sil_states, POOL, size=int(word_off[-1])).astype(np.uint16)
    mixtures[word_off[spec.sil_idx]:word_off[spec.sil_idx + 1]] = np.arange(spec.sil_states)
    for a in (word_off, mixtures, n):
        a.setflags(write=False)
    return word_off, mixtures, n


def shape(name):
    """-> what route() takes: W, P2, ld, the most states of a slot, the silence's states, the mask of rows with a four-state word"""
    spec = LEXICA[name]
    _, _, n = lexicon(name)
    mask = 0
    for w in np.flatnonzero(n >= 4):
        mask |= 1 << (int(w) // 1024)
    return spec.W, int(n.sum()) + spec.W * spec.sil_states, _up(spec.model_states, 8), int(n.max()), spec.sil_states, mask


# ---- LM tables ----------------------------------------------------------------------------------------------------------------------
LM_KINDS = ("dyadic", "flat", "wide", "tight", "tightr", "forbid")


@functools.lru_cache(maxsize=3)
def lm_table(kind, name, beam=0.0):
    """lm[w, h] = the cost of word w after history h, f32 [W, W]; the search reads a history's column over w != silence.
    dyadic: multiples of 0.25 in [0, 3), many equal.  flat: all 1 -- every decision is a tie.  wide: dyadic, and every history's column
    holds a 0 and `beam` (the acoustic beam): with max - min >= beam the skip test of the recombination can drop no word end whose
    score is within the beam of the best.  tight: multiples of 0.5 in [1, 3], every column's minimum exactly 1 and maximum exactly 3 (exact
    in bf16): a word end 2 above the best one sits exactly on the skip test's bound.  tightr: the same with bounds bf16 must round
    (1 + 2^-8 and 3 + 2^-7; every fourth history negative, -3 - 2^-7 and -1 - 2^-8), entries multiples of 2^-8, and history 2's column
    with a NaN.  forbid: dyadic with a quarter of the entries +inf, and history 1's column all NaN."""
    spec = LEXICA[name]
    W, sil = spec.W, spec.sil_idx
    rng = np.random.default_rng(6000 + spec.seed)
    if kind == "flat":
        lm = np.ones((W, W), np.float32)
    elif kind in ("tight", "tightr"):
        lm = (rng.integers(2, 7, size=(W, W), dtype=np.int8) * np.float32(0.5)).astype(np.float32)
        words = np.array([w for w in range(W) if w != sil])
        lo, hi = words[rng.integers(0, len(words), size=W)], words[rng.integers(0, len(words), size=W)]
        hi = np.where(hi == lo, words[(np.searchsorted(words, lo) + 1) % len(words)], hi)
        lm[lo, np.arange(W)] = 1.0
        lm[hi, np.arange(W)] = 3.0
        if kind == "tightr":
            lm += (rng.integers(0, 3, size=(W, W), dtype=np.int8) * np.float32(2.0 ** -8)).astype(np.float32)
            lm[lo, np.arange(W)] = 1.0 + 2.0 ** -8
            lm[hi, np.arange(W)] = 3.0 + 2.0 ** -7
            lm[:, 3::4] *= -1.0
            lm[(sil + 1) % W, 2] = np.nan
    else:
        lm = (rng.integers(0, 12, size=(W, W), dtype=np.int8) * np.float32(0.25)).astype(np.float32)
        if kind == "wide":
            words = np.array([w for w in range(W) if w != sil])
            lo = words[rng.integers(0, len(words), size=W)]
            hi = np.where(lo == words[0], words[1], words[0])
            lm[lo, np.arange(W)] = 0.0
            lm[hi, np.arange(W)] = beam
        elif kind == "forbid":
            lm[rng.random((W, W)) < 0.25] = np.inf
            lm[:, 1] = np.nan
        else:
            assert kind == "dyadic"
    lm.setflags(write=False)
    return lm


# ---- batches and score tables ---------------------------------------------------------------------------------------------------------
def batch_lengths(spec, seed):
    """utterances of 0, 1, 2 and 3 frames among n_long of the lexicon's frame range"""
    rng = np.random.default_rng(3000 + seed)
    lens = [0, 1, 2, 3] + [int(t) for t in rng.integers(spec.frames[0], spec.frames[1] + 1, size=spec.n_long)]
    return [lens[i] for i in rng.permutation(len(lens))]


@functools.lru_cache(maxsize=None)
def _batch(name, kind, seed, lens=None):
    spec = LEXICA[name]
    lens = batch_lengths(spec, seed) if lens is None else list(lens)
    S = spec.model_states
    if kind == "const":  # every cost 1
        table = np.ones((int(sum(lens)), S))
    elif kind == "neginf":  # dyadic with one of the words' states at -inf in every frame
        table = sc.score_table("dyadic", lens, S, seed).copy()
        table[:, POOL - 1] = -np.inf
    else:
        table = sc.score_table(kind, lens, S, seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    table.setflags(write=False)
    off.setflags(write=False)
    return table, off


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    lex: str
    lm: str = "dyadic"
    kind: str = "dyadic"
    flags: tuple = ("",)        # the device runs: "", "dense", "global"
    beams: tuple = None         # (acoustic, LM); None: the lexicon's; FLT_MAX: off
    seed: int = 0
    lens: tuple = None          # None: batch_lengths
    conditions: tuple = ("nontrivial",)

    @property
    def id(self):
        b = "" if self.beams is None else "-b" + "_".join("off" if x >= FLT_MAX else f"{x:g}" for x in self.beams)
        t = "" if self.lens is None else "-t" + "_".join(str(n) for n in self.lens)
        return f"{self.lex}-{self.lm}-{self.kind}{b}{t}" + (f"-s{self.seed}" if self.seed else "")

    @property
    def ac(self):
        return (LEXICA[self.lex].beams if self.beams is None else self.beams)[0]

    @property
    def lmb(self):
        return (LEXICA[self.lex].beams if self.beams is None else self.beams)[1]

    def routes(self):
        return [LEXICA[self.lex].route_for(f) for f in self.flags]


OFF = (FLT_MAX, FLT_MAX)
ALL = ("", "dense", "global")


def _cases():
    out = []
    for name, spec in LEXICA.items():
        if name == "g60":
            continue
        # every lexicon on a dyadic and on a real table, with each flag that names another kernel than no flag does
        flags = ("",) + (("dense",) if spec.route_dense not in ("none", spec.route) else ()) + (("global",) if spec.route_global != spec.route else ())
        for kind in ("dyadic", "real"):
            out.append(Case(name, "dyadic", kind, flags))
    # the table kinds of the zerogram cases and a column of -inf, per layout; beams off and on
    for name in ("r40m1", "l1p4097", "r1100m2"):
        for kind in ("negative", "inf", "nan"):
            out.append(Case(name, "dyadic", kind, ALL))
        for kind in ("inf", "nan"):  # (beams off: under a beam a large finite cost is pruned like +inf)
            out.append(Case(name, "dyadic", kind, ALL, beams=OFF, conditions=("nontrivial", "infnan")))
        out.append(Case(name, "dyadic", "neginf", ALL, beams=OFF, conditions=("nontrivial",)))
        out.append(Case(name, "dyadic", "neginf", ALL, conditions=("all_pruned",)))
    out.append(Case("r40m0", "dyadic", "dyadic", ALL, beams=OFF))
    # LM kinds.  flat: every decision a tie; forbid: +inf entries and a NaN column
    for name in ("r40m1", "r1100m1", "l1p4096", "r2100m5"):
        out.append(Case(name, "flat", "dyadic", ALL, conditions=("nontrivial", "ties")))
        out.append(Case(name, "forbid", "dyadic", ALL))
    out.append(Case("r40m0", "flat", "dyadic", ALL, beams=OFF, conditions=("nontrivial", "ties")))
    for name in ("r40tie", "r1100tie", "l300tie"):  # a word and its silence copy tie, whole words tie
        out.append(Case(name, "flat", "const", ALL, conditions=("ties",)))
        out.append(Case(name, "flat", "const", ALL, beams=OFF, conditions=("ties",)))
        out.append(Case(name, "dyadic", "dyadic", ALL, beams=(6.0, 3.0), conditions=("nontrivial", "ties")))
    out.append(Case("g4723", "flat", "dyadic", ("",), conditions=("nontrivial", "ties")))
    # hypotheses exactly on best + beam, for either beam
    for name, b1, b2 in (("r40m1", (4.0, 2.0), (6.0, 2.0)), ("l2p4096", (8.0, 2.0), (12.0, 6.0)), ("r1100m3", (4.0, 2.0), (6.0, 2.0)),
                         ("r2100m6", (4.0, 2.0), (5.0, 2.0))):
        out.append(Case(name, "dyadic", "dyadic", ALL, beams=b1, conditions=("nontrivial", "beam_edge")))
        out.append(Case(name, "flat", "negative", ALL, beams=b2, conditions=("nontrivial", "beam_edge", "ties")))
    # a word end exactly on the skip test's bound: float bounds (LDS, global) and bf16 bounds (registers)
    for name in ("r40m1", "r1100m2"):
        out.append(Case(name, "tight", "dyadic", ALL, conditions=("nontrivial", "skip_bound")))
        out.append(Case(name, "tightr", "dyadic", ALL, conditions=("nontrivial", "skip_bound_bf16")))
    # more surviving word ends than one pass of the staging buffer, nothing skipped
    for name, beam in (("r1100m0", 16.0), ("l2p4096", 16.0), ("r2100m0", 12.0)):
        out.append(Case(name, "wide", "dyadic", ALL, beams=(beam, FLT_MAX), lens=(0, 3, 12), conditions=("nontrivial", "staging")))
    # the book: one utterance, exactly full at max_word_ends = k (r40one: every word ends in every frame) and an ordinary one
    out.append(Case("r40one", "dyadic", "dyadic", ALL, beams=OFF, lens=(25,), conditions=("nontrivial", "book", "book_exact")))
    out.append(Case("r40m1", "dyadic", "dyadic", ALL, lens=(40,), conditions=("nontrivial", "book")))
    out.append(Case("l1p4097", "dyadic", "real", ALL, lens=(40,), conditions=("nontrivial", "book")))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()
# case id -> the seed of its batch and table where seed 0 does not meet the case's conditions
SEEDS = {}


def case(id_):
    return next(c for c in CASES if c.id == id_)


def batch(case):
    """-> (table [F, model_states] f64, frame_off u64[U + 1]); built once per case and never written to"""
    return _batch(case.lex, case.kind, SEEDS.get(case.id, case.seed), case.lens)


def decode(name, lm, rows, ac, lmb):
    """the oracle on one utterance -> (words, scores, times, stats)"""
    from oracle import pyoracle

    spec = LEXICA[name]
    word_off, mixtures, _ = lexicon(name)
    if len(rows) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(10, np.uint64)
    return pyoracle.bigram_decode(rows, word_off, mixtures, spec.sil_idx, lm, spec.tdp, float(ac), float(lmb), stats=True)


@functools.lru_cache(maxsize=None)
def _reference(name, lm_kind, kind, seed, lens, ac, lmb, replace=None):
    table, off = _batch(name, kind, seed, lens)
    if replace is not None:
        table = np.where(np.isfinite(table), table, replace)
    lm = lm_table(lm_kind, name, ac if lm_kind == "wide" else 0.0)
    out = []
    for u in range(len(off) - 1):
        res = decode(name, lm, table[int(off[u]):int(off[u + 1])], ac, lmb)
        for a in res:
            a.setflags(write=False)
        out.append(res)
    return tuple(out)


def reference(case, ac=None, lmb=None, replace=None):
    """The oracle's answer per utterance: ((words, scores, times, stats), ...), computed once per (lexicon, LM, table, beams)"""
    return _reference(case.lex, case.lm, case.kind, SEEDS.get(case.id, case.seed), case.lens, case.ac if ac is None else ac,
                      case.lmb if lmb is None else lmb, replace)


# ---- conditions, from the oracle alone --------------------------------------------------------------------------------------------
def _long(case):
    _, off = batch(case)
    return [u for u in range(len(off) - 1) if int(off[u + 1]) - int(off[u]) > 3]


def _stats(case, **kw):
    return np.array([[int(x) for x in r[3]] for r in reference(case, **kw)], dtype=np.uint64)


def nontrivial(case):
    """every utterance longer than 3 frames gets an answer that names a word other than silence"""
    sil = LEXICA[case.lex].sil_idx
    ref = reference(case)
    return all(bool(np.any(ref[u][0] != sil)) for u in _long(case))


def all_pruned(case):
    """(-inf with a beam on: best + beam is -inf and nothing is below it) every answer is empty"""
    return all(len(r[0]) == 0 for r in reference(case))


def ties(case):
    """some frame's merged list holds two word ends of equal score"""
    return int(_stats(case)[:, 5].sum()) > 0


# beams move by 2^-10: every sum of a dyadic case is a multiple of 2^-3 below 2^13, so best + (beam +- 2^-10) is exact and nothing but a
# hypothesis exactly on the limit can change sides.  (One ulp of the beam itself is less than half an ulp of best + beam as soon as best
# exceeds the beam, and the sum would round back.)  The limit is exclusive (score < best + beam), so the hypotheses ON it are out: raising a
# beam by the step lets them in and changes the statistics, lowering it by the step changes nothing -- with <= it would be the other way
# round.
BEAM_STEP = 2.0 ** -10


def beam_edge(case):
    """for either beam some hypothesis has score == best + beam exactly: raising the beam by 2^-10 changes stats[0..2], lowering it by
    2^-10 does not"""
    at = _stats(case)
    if int(at[:, 7].sum()) == 0:
        return False
    up = [_stats(case, ac=case.ac + BEAM_STEP), _stats(case, lmb=case.lmb + BEAM_STEP)]
    down = [_stats(case, ac=case.ac - BEAM_STEP), _stats(case, lmb=case.lmb - BEAM_STEP)]
    return all(not np.array_equal(at[:, :3], m[:, :3]) for m in up) and all(np.array_equal(at[:, :3], m[:, :3]) for m in down)


def skip_bound(case):
    """some word end sits exactly on the skip test's bound, with the float bounds and with the bf16 bounds"""
    st = _stats(case)
    return int(st[:, 8].sum()) > 0 and int(st[:, 9].sum()) > 0


def skip_bound_bf16(case):
    """... with the bf16 bounds, where bf16 must round them"""
    lm = lm_table(case.lm, case.lex)
    rounds = np.any((lm.view(np.uint32) & 0xFFFF) != 0)
    return bool(rounds) and int(_stats(case)[:, 9].sum()) > 0


def staging(case):
    """some frame's merged list is longer than one pass of the staging buffer; every history's LM column spans the acoustic beam and
    the list's scores lie within it, so the skip test drops none"""
    spec = LEXICA[case.lex]
    lm = lm_table(case.lm, case.lex, case.ac)
    words = np.arange(spec.W) != spec.sil_idx
    span = lm[words].max(axis=0) - lm[words].min(axis=0)
    st = _stats(case)
    u = int(np.argmax(st[:, 4]))
    spread = float(np.array([st[u, 6]], np.uint64).astype(np.uint32).view(np.float32)[0])
    return int(st[u, 4]) > staging_capacity(spec.W) and bool(np.all(span >= case.ac)) and spread < case.ac


def book_k(case):
    """one utterance: the smallest max_word_ends whose book (2 + min(max_word_ends, W) T entries) holds the 2 + stats[0] the search writes"""
    _, off = batch(case)
    assert len(off) == 2
    T = int(off[1])
    return -(-int(_stats(case)[0, 0]) // T), T


def book(case):
    k, T = book_k(case)
    return 2 <= k <= LEXICA[case.lex].W


def book_exact(case):
    """the book is exactly full at k"""
    k, T = book_k(case)
    return int(_stats(case)[0, 0]) == k * T


def infnan(case):
    """the search reads such entries: with every +inf / NaN replaced by a large finite cost the oracle's statistics differ (beams
    off: under a beam the large cost is pruned as +inf is)"""
    table, _ = batch(case)
    return bool(np.any(~np.isfinite(table[:, :POOL]))) and not np.array_equal(_stats(case)[:, :4], _stats(case, replace=1024.0)[:, :4])


CONDITIONS = {"nontrivial": nontrivial, "all_pruned": all_pruned, "ties": ties, "beam_edge": beam_edge, "skip_bound": skip_bound,
              "skip_bound_bf16": skip_bound_bf16, "staging": staging, "book": book, "book_exact": book_exact, "infnan": infnan}


def counts(case):
    """does the case count towards its routes' coverage: not every long utterance's answer empty or all silence"""
    sil = LEXICA[case.lex].sil_idx
    ref = reference(case)
    return any(bool(np.any(ref[u][0] != sil)) for u in _long(case))
