"""Cases for the zerogram search kernels run alone on score tables the test makes up (sr_recognize_corpus_scores): lexica, tables,
batches, the oracle's answers and the conditions that keep a case from passing vacuously.  No GPU and no pytest in here:
tests/test_search_cases_cpu.py checks every case's conditions, tests/test_gpu_search_scores.py runs the kernels on them.

Why tables and not features: through a mixture model a test cannot place an exact tie, a hypothesis exactly on the beam limit, a
+inf or a NaN where the search will read it.  Here the table is the input.  `dyadic` tables hold multiples of 0.25; with the
transition penalties (3, 0, 30), the word penalty 1 and beams that are multiples of 0.125 every path sum is exact in binary, so
equal sums are equal bits: ties between words and positions are dense, and hypotheses sit exactly on best + beam.

Lexica draw their words' states from a small shared pool (state 0 is the silence state), so a lexicon of thousands of words needs a
table only a few columns wide; the model behind it (one density per state, dimension 2) only gives sr_lexicon_create and the oracle
something to attach to -- its scores are never used.  `model_states` widens the model (and the table) beyond the pool where a case is
about the row length (the word-per-lane kernel keeps two score rows in the LDS)."""
from __future__ import annotations

import atexit
import functools
import os
import shutil
import tempfile
from dataclasses import dataclass

import numpy as np

from speechrecognition_amd import synth

TDP = (3.0, 0.0, 30.0)
PENALTY = 1.0
KINDS = ("dyadic", "negative", "inf", "nan", "real")
DYADIC_KINDS = ("dyadic", "negative", "inf", "nan")
FLAG_SLOW, FLAG_REPLAY, FLAG_CORRUPT = 1, 2, 4  # traceback.h: kFlagSlowPath, kFlagReplay, kFlagCorrupt


# ---- lexica -----------------------------------------------------------------------------------------------------------------------
def _assemble(words, sil_idx):
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.uint32)
    aut = np.concatenate([np.asarray(w, dtype=np.uint16) for w in words]).astype(np.uint16)
    return synth.ExplicitLexicon(off, aut, sil_idx)


def word_lexicon(n_plain, L, n_general=0, clones=0.0, sil_idx=0, sil_len=1, pool=12, seed=0):
    """A lexicon for the word-per-lane kernel (every word at most four positions): silence (state 0, sil_len positions) at index
    sil_idx, n_plain words of L positions over states 1 .. pool - 1 -- the share `clones` of them copies of an earlier plain word --
    and n_general words the kernel's general code takes: another length of 2 .. 4, a first state equal to the silence state, or
    the silence state further in.  A silence word of 2 or 3 positions is a general word itself; a one-position word (state 1)
    joins it then, so that the group of single words is never empty and the words-per-lane rule sees the same counts."""
    rng = np.random.default_rng(1000 + seed)
    plain = []
    for _ in range(n_plain):
        if plain and rng.random() < clones:
            plain.append(plain[int(rng.integers(0, len(plain)))])
        else:
            plain.append([int(s) for s in rng.integers(1, pool, size=L)])
    general = []
    for g in range(n_general):
        k = g % 3
        if k == 0:
            n = [n for n in (2, 3, 4) if n != L][int(rng.integers(0, 2))]
            general.append([int(s) for s in rng.integers(1, pool, size=n)])
        elif k == 1:
            general.append([0] + [int(s) for s in rng.integers(1, pool, size=int(rng.integers(1, 4)))])
        else:
            w = [int(s) for s in rng.integers(1, pool, size=int(rng.integers(2, 5)))]
            w[int(rng.integers(1, len(w)))] = 0
            general.append(w)
    words = plain + general
    if sil_len > 1:
        words.append([1])
    order = rng.permutation(len(words))
    words = [words[i] for i in order]
    sil_idx = min(sil_idx, len(words))
    words.insert(sil_idx, [0] + [int(s) for s in rng.integers(1, pool, size=sil_len - 1)])
    return _assemble(words, sil_idx)


def ragged_lexicon(n_positions, lengths, clones=0.0, sil_idx=0, pool=12, seed=0):
    """A lexicon for the slot-per-lane and the replay kernels: words whose lengths are drawn from `lengths` (1 .. 40 positions) until
    they have n_positions positions together with the one-position silence; now and then a clone or a word that starts in the silence
    state."""
    rng = np.random.default_rng(2000 + seed)
    words, total = [], 1
    while total < n_positions:
        n = min(int(rng.choice(lengths)), n_positions - total)
        if words and rng.random() < clones:
            w = words[int(rng.integers(0, len(words)))]
            if len(w) > n_positions - total:
                continue
        else:
            w = [int(s) for s in rng.integers(1, pool, size=n)]
            if n > 1 and rng.random() < 0.05:
                w[0] = 0
        words.append(w)
        total += len(w)
    if max(len(w) for w in words) < 2:  # sr_lexicon_create: some word with two or more positions
        words[-1] = words[-1] + [1]
    sil_idx = min(sil_idx, len(words))
    words.insert(sil_idx, [0])
    return _assemble(words, sil_idx)


SHORT = (1, 2, 2, 3, 3, 4)
MIXED = (1, 2, 3, 3, 4, 7, 13, 40)


@dataclass(frozen=True)
class Lex:
    """A named lexicon: how it is built, the model it attaches to, and the search route sr_lexicon_describe must report for it."""
    name: str
    build: tuple          # ("word" | "ragged", kwargs as a sorted tuple of pairs)
    describe: str         # the exact text, or for "slots" / "big" the prefix before the position count
    model_states: int = 16
    n_long: int = 3       # utterances of 40 .. 70 frames in a batch (beside those of 0, 1, 2, 3 frames)
    beam: float = 4.0
    neg_fits: bool = True  # (word-per-lane route) the NEG variant's word-end arrays fit the LDS beside the two score rows


def _lex(name, kind, describe, model_states=16, n_long=3, beam=4.0, neg_fits=True, **kw):
    return Lex(name, (kind, tuple(sorted(kw.items()))), describe, model_states, n_long, beam, neg_fits)


# The word-per-lane grid.  build_word_net (viterbi_words.hip) fills groups of 64 lane slots: g_plain = ceil(plain / 64), one group of
# single words (silence, one position), g_gen = ceil(general / 64) waves of their own; NW is the smallest of 1, 2, 3 with
# ceil((g_plain + 1) / NW) + g_gen <= 8 waves (else the smallest with <= 16), NT = 64 * that.
#   100 plain:  g_plain  2 -> NW 1: 3 waves (192)          ; with 20 general: 3 + 1 = 4 waves (256)
#   460 plain:  g_plain  8 -> NW 1: 9 > 8, NW 2: 5 (320)   ; with 20 general: 10 > 8, 5 + 1 = 6 (384)
#   970 plain:  g_plain 16 -> NW 2: 9 > 8, NW 3: 6 (384)   ; with 20 general: NW 2: 9 + 1 > 8, NW 3: 6 + 1 = 7 (448)
_GRID = {1: (100, 192, 256), 2: (460, 320, 384), 3: (970, 384, 448)}
LEXICA = {}
for _nw, (_n, _nt, _ntg) in _GRID.items():
    for _L in (2, 3, 4):
        _long, _beam = (3, 4.0) if _nw == 1 else (2, 3.0)
        LEXICA[f"w{_nw}l{_L}"] = _lex(f"w{_nw}l{_L}", "word", f"words {_nw} x {_nt} plain {_L}", n_long=_long, beam=_beam, n_plain=_n, L=_L,
                                    sil_idx=0 if _L == 3 else 7, seed=10 * _nw + _L)
        # (the general lexica of plain length 3 have a two-position silence word, a general word itself)
        LEXICA[f"w{_nw}l{_L}g"] = _lex(f"w{_nw}l{_L}g", "word", f"words {_nw} x {_ntg} plain {_L} general", n_long=_long, beam=_beam, n_plain=_n,
                                     L=_L, n_general=20, sil_idx=5, sil_len=2 if _L == 3 else 1, seed=100 + 10 * _nw + _L)
# NT > 512: the NEG/1024 build, and the fast build with more than 8 waves
#   1600 plain: g_plain 25, 26 groups: NW 1..3 need 26, 13, 9 > 8 waves; <= 16: NW 2 -> 13 waves (832)
#   2200 plain: g_plain 35, 36 groups: 36, 18 > 16, NW 3 -> 12 waves (768)
#   300 plain + 400 general: 5 + 1 groups and 7 waves of general words: 13, 10, 9 > 8; NW 1 -> 13 waves (832)
LEXICA["w2wide"] = _lex("w2wide", "word", "words 2 x 832 plain 3", n_long=2, beam=3.0, n_plain=1600, L=3, seed=31)
LEXICA["w3wide"] = _lex("w3wide", "word", "words 3 x 768 plain 2", n_long=2, beam=2.5, n_plain=2200, L=2, seed=32)
LEXICA["w1wide"] = _lex("w1wide", "word", "words 1 x 832 plain 3 general", n_long=2, beam=3.0, n_plain=300, L=3, n_general=400, sil_idx=3, seed=33)
# LDS limits.  words_smem (viterbi_words.hip) = 1024 + 2 * roundup(ld * 8 + 16, 1024) [+ 2 * roundup(n_words * 8, 1024) for the NEG
# variant], ld = n_states rounded up to 8, against 160 KB = 163 840:
#   10 104 states: ld 10 104, rows 2 * 80 896 -> 162 816 <= 163 840: the word-per-lane kernel applies; its NEG variant needs
#                  2 * 1 024 more for 101 words -> 164 864: does not fit, the fast build runs and flags what it cannot do
#   10 105 states: ld 10 112, 80 912 rounds up to 81 920 -> 164 864: the kernel does not apply, the slot-per-lane kernel runs
LEXICA["w1edge"] = _lex("w1edge", "word", "words 1 x 192 plain 3", model_states=10104, neg_fits=False, n_long=2, n_plain=100, L=3, seed=41)
LEXICA["w1over"] = _lex("w1over", "word", "slots (", model_states=10105, n_long=2, n_plain=100, L=3, seed=41)
# clone lexica: ties between whole words, which the hypothesis order decides
LEXICA["w1clone"] = _lex("w1clone", "word", "words 1 x 192 plain 3", n_plain=100, L=3, clones=0.3, pool=9, seed=51)
LEXICA["w2clone"] = _lex("w2clone", "word", "words 2 x 384 plain 3 general", n_long=2, beam=3.0, n_plain=460, L=3, n_general=20, clones=0.3, seed=52)
# the slot-per-lane kernel and the LDS replay: positions P in each range of launch_decode_lds (viterbi_decode.hip): <= 64 (64 x 1),
# <= 256 (64 x 4), <= 1024 (256 x 4), <= 2048 (256 x 8), <= 4096 (512 x 8), <= 8192 (1024 x 8); type padding (build_fast_net) adds at
# most 63 positions per slot type, so 7 000 stays within the 8 192 the LDS holds
for _i, _p in enumerate((60, 250, 1000, 2000, 4000, 7000)):
    LEXICA[f"p{_p}"] = _lex(f"p{_p}", "ragged", "slots (", n_long=3 if _p <= 1000 else 2, beam=4.0 if _p <= 1000 else 3.0, n_positions=_p,
                           lengths=MIXED, clones=0.1, sil_idx=_i, seed=60 + _i)
for _i, _p in enumerate((40, 200, 900)):  # short words only: beside the word-per-lane kernel by default
    LEXICA[f"s{_p}"] = _lex(f"s{_p}", "ragged", "words ", n_positions=_p, lengths=SHORT, clones=0.2, sil_idx=2 * _i, pool=9, seed=70 + _i)
LEXICA["pclone"] = _lex("pclone", "ragged", "slots (", n_positions=500, lengths=(2, 3, 3, 4, 7), clones=0.4, pool=9, seed=81)
# more than 8 192 positions: the hypotheses in device memory
LEXICA["big4"] = _lex("big4", "word", "words 3 x 768 plain 4 (replay: big, 8401 positions)", n_long=2, beam=3.0, n_plain=2100, L=4, seed=91)
LEXICA["biglong"] = _lex("biglong", "ragged", "big (", n_long=2, beam=3.0, n_positions=9000, lengths=MIXED, clones=0.1, sil_idx=4, seed=92)

P_RANGES = {"p60": (1, 64), "p250": (65, 256), "p1000": (257, 1024), "p2000": (1025, 2048), "p4000": (2049, 4096), "p7000": (4097, 8192),
            "s40": (1, 64), "s200": (65, 256), "s900": (257, 1024), "pclone": (257, 1024), "biglong": (8193, 65534), "big4": (8193, 65534)}


@functools.lru_cache(maxsize=None)
def lexicon(name):
    kind, kw = LEXICA[name].build
    lex = (word_lexicon if kind == "word" else ragged_lexicon)(**dict(kw))
    lex.word_off.setflags(write=False)
    lex.automaton.setflags(write=False)
    return lex


def clone_words(lex):
    """-> bool[W]: the word has the state sequence of another word"""
    seen = {}
    for w in range(lex.n_words):
        seen.setdefault(bytes(lex.automaton[lex.word_off[w]:lex.word_off[w + 1]]), []).append(w)
    out = np.zeros(lex.n_words, dtype=bool)
    for ws in seen.values():
        if len(ws) > 1:
            out[ws] = True
    return out


# ---- the tiny model ---------------------------------------------------------------------------------------------------------------
_TMP = None


@functools.lru_cache(maxsize=None)
def model_file(n_states):
    """path of a MIXSET file: n_states states of one density each, dimension 2"""
    global _TMP
    if _TMP is None:
        _TMP = tempfile.mkdtemp(prefix="search_cases_")
        atexit.register(shutil.rmtree, _TMP, ignore_errors=True)
    path = os.path.join(_TMP, f"tiny{n_states}.mix")
    synth.write_mixset(path, synth.make_mixset(n_states, 1, MODEL_DIM, seed=3))
    return path


MODEL_DIM = 2


# ---- batches and tables -------------------------------------------------------------------------------------------------------------
def batch_lengths(n_long, seed):
    """utterances of 0, 1, 2 and 3 frames (the word-per-lane kernel loads two rows ahead: its edge is T <= 3) among n_long of 40 .. 70"""
    rng = np.random.default_rng(3000 + seed)
    lens = [0, 1, 2, 3] + [int(t) for t in rng.integers(40, 71, size=n_long)]
    return [lens[i] for i in rng.permutation(len(lens))]


def score_table(kind, lens, n_states, seed):
    """[sum(lens), n_states] f64.  dyadic: multiples of 0.25 in [0, 6); negative: in [-2, 6); inf: dyadic with about 10 % +inf; nan:
    dyadic with about 2 % NaN; real: uniform doubles in [0, 6).  In the negative and nan kinds the first of the long utterances stays
    plain dyadic: an utterance that no fast kernel may hand to the replay."""
    rng = np.random.default_rng(4000 + seed)
    F = int(sum(lens))
    if kind == "real":
        return rng.uniform(0.0, 6.0, size=(F, n_states))
    t = rng.integers(0, 24, size=(F, n_states)).astype(np.float64) * 0.25
    if kind == "negative":
        alt = rng.integers(-8, 24, size=(F, n_states)).astype(np.float64) * 0.25
    elif kind == "inf":
        alt = np.where(rng.random((F, n_states)) < 0.10, np.inf, t)
    elif kind == "nan":
        alt = np.where(rng.random((F, n_states)) < 0.02, np.nan, t)
    else:
        assert kind == "dyadic"
        return t
    if kind in ("negative", "nan"):
        off = np.concatenate([[0], np.cumsum(lens)])
        u = next(i for i, n in enumerate(lens) if n > 3)
        alt[off[u]:off[u + 1]] = t[off[u]:off[u + 1]]
    return alt


def clean_utterances(table, off):
    """-> bool[U]: the utterance's rows hold no negative and no NaN value (no fast kernel may flag it for the replay)"""
    return np.array([not np.any((r < 0) | np.isnan(r)) for r in (table[int(off[u]):int(off[u + 1])] for u in range(len(off) - 1))])


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    lex: str
    kind: str
    seed: int = 0
    beam: float = None          # None: the lexicon's
    conditions: tuple = ("nontrivial",)
    # the device runs: (exact_negative, general_kernel, slot_kernel)
    runs: tuple = ((0, False, False), (1, False, False))
    handoff: bool = False       # at exact_negative 0: some utterance is flagged for the replay and some is not

    @property
    def id(self):
        return f"{self.lex}-{self.kind}" + (f"-b{self.am_threshold:g}" if self.beam is not None else "")

    @property
    def am_threshold(self):
        return self.beam if self.beam is not None else LEXICA[self.lex].beam


WORDS_FIRST, WORDS_NEG = (0, False, False), (1, False, False)
SLOTS, SLOTS_NEG = (0, False, True), (1, False, True)
REPLAY = (0, True, False)


def _cases():
    out = []
    grid = [f"w{nw}l{L}{g}" for nw in (1, 2, 3) for L in (2, 3, 4) for g in ("", "g")]
    for i, name in enumerate(grid):  # every (NW, L, GEN) at exact_negative 0 and 1; `real` for a sample
        for kind in DYADIC_KINDS + (("real",) if i % 4 == 0 else ()):
            handoff = kind in ("negative", "nan")  # ... which also run the slot-per-lane kernel first
            out.append(Case(name, kind, runs=(WORDS_FIRST, WORDS_NEG) + ((SLOTS,) if handoff else ()), handoff=handoff))
    for name in ("w1wide", "w2wide", "w3wide"):
        for kind in DYADIC_KINDS:
            out.append(Case(name, kind, handoff=kind in ("negative", "nan")))
    # the NEG arrays do not fit: at exact_negative 1 the fast build runs and the flagged utterances take the replay; and the first
    # row length at which the kernel does not apply at all
    for name in ("w1edge", "w1over"):
        for kind in DYADIC_KINDS:
            out.append(Case(name, kind, runs=(WORDS_FIRST, WORDS_NEG, SLOTS), handoff=kind in ("negative", "nan")))
    # slot-per-lane first, and the LDS replay alone on every utterance
    for name in ("p60", "p250", "p1000", "p2000", "p4000", "p7000", "s40", "s200", "s900"):
        for kind in DYADIC_KINDS + (("real",) if name in ("p250", "s900") else ()):
            out.append(Case(name, kind, runs=(SLOTS, SLOTS_NEG, REPLAY), handoff=kind in ("negative", "nan")))
    for kind in DYADIC_KINDS:
        out.append(Case("big4", kind, runs=(WORDS_FIRST, WORDS_NEG, REPLAY), handoff=kind in ("negative", "nan")))
        out.append(Case("biglong", kind, runs=((0, False, False), REPLAY)))
    # ties between clones, and the beam limit itself, per first kernel
    every = (WORDS_FIRST, WORDS_NEG, SLOTS, REPLAY)
    edge = ("nontrivial", "beam_edge_decides", "no_word_end_frames")
    for kind in DYADIC_KINDS:
        handoff = kind in ("negative", "nan")
        out.append(Case("w1clone", kind, conditions=("nontrivial", "ties_decide"), runs=every, handoff=handoff))
        out.append(Case("w2clone", kind, conditions=("nontrivial", "ties_decide"), runs=every, handoff=handoff))
        out.append(Case("pclone", kind, conditions=("nontrivial", "ties_decide"), runs=(SLOTS, SLOTS_NEG, REPLAY), handoff=handoff))
        out.append(Case("w1clone", kind, beam=3.5, conditions=edge, runs=every, handoff=handoff))
        out.append(Case("pclone", kind, beam=3.5, conditions=edge, runs=(SLOTS, SLOTS_NEG, REPLAY), handoff=handoff))
    return out


# case id -> the seed of its batch and table where seed 0 does not meet the case's conditions (p60: the 60 positions hold few words,
# and the traceback must name three)
SEEDS = {"p60-dyadic": 1, "p60-negative": 1, "p60-nan": 1, "pclone-dyadic-b3.5": 1, "pclone-negative-b3.5": 1}
CASES = _cases()


def batch(case):
    """-> (table [F, model_states] f64, frame_off u64[U + 1]); built once per case and never written to"""
    return _batch(case.lex, case.kind, SEEDS.get(case.id, case.seed))


@functools.lru_cache(maxsize=None)
def _batch(lex, kind, seed):
    spec = LEXICA[lex]
    lens = batch_lengths(spec.n_long, seed)
    table = score_table(kind, lens, spec.model_states, seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    table.setflags(write=False)
    off.setflags(write=False)
    return table, off


@functools.lru_cache(maxsize=None)
def _reference(lex, kind, seed, beam):
    from oracle import pyoracle

    spec = LEXICA[lex]
    table, off = _batch(lex, kind, seed)
    orc = pyoracle.Oracle(model_file(spec.model_states), MODEL_DIM, lexicon(lex), tdp=TDP, am_threshold=beam, word_penalty=PENALTY)
    out = []
    for u in range(len(off) - 1):
        rows = table[int(off[u]):int(off[u + 1])]
        words, tb = orc.decode(np.zeros((len(rows), MODEL_DIM), np.float32), dense=rows if len(rows) else None, traceback=True)
        for a in (words,) + tb:
            a.setflags(write=False)
        out.append((words, tb))
    orc.close()
    return tuple(out)


def reference(case, beam=None):
    """The oracle's answer per utterance: ((words, (tb_score, tb_word, tb_bkp)), ...), computed once and shared"""
    return _reference(case.lex, case.kind, SEEDS.get(case.id, case.seed), case.am_threshold if beam is None else beam)


def same_traceback(a, b):
    """tb_word and tb_bkp equal, tb_score equal bit for bit -- but that positions where both hold a NaN count as equal"""
    (sa, wa, ba), (sb, wb, bb) = a, b
    if not (np.array_equal(wa, wb) and np.array_equal(ba, bb)):
        return False
    both_nan = np.isnan(sa) & np.isnan(sb)
    return bool(np.all((sa.view(np.uint64) == sb.view(np.uint64)) | both_nan))


# ---- conditions, from the oracle alone --------------------------------------------------------------------------------------------
def _long(case):
    _, off = batch(case)
    return [u for u in range(len(off) - 1) if int(off[u + 1]) - int(off[u]) > 3]


def nontrivial(case):
    """at least half of the utterances longer than 3 frames get words; their tracebacks name at least 3 distinct words"""
    ref = reference(case)
    long = _long(case)
    named = set()
    for u in long:
        s, w, _ = ref[u][1]
        named.update(int(x) for x in w[1:][np.isfinite(s[1:])])
    return 2 * sum(len(ref[u][0]) > 0 for u in long) >= len(long) and len(named) >= 3


def ties_decide(case):
    """in at least half of the utterances longer than 3 frames a recognised word has a clone: the index order decided it"""
    ref = reference(case)
    clones = clone_words(lexicon(case.lex))
    long = _long(case)
    return 2 * sum(bool(np.any(clones[ref[u][0]])) for u in long) >= len(long)


def beam_edge_decides(case):
    """for some utterance the traceback at the case's beam differs from that at beam - 0.125 or beam + 0.125: hypotheses exactly on
    the limit exist and matter"""
    at = reference(case)
    return any(not same_traceback(at[u][1], other[u][1])
               for d in (-0.125, 0.125) for other in (reference(case, case.am_threshold + d),) for u in range(len(at)))


def no_word_end_frames(case):
    """some frame's traceback entry has no surviving word end"""
    return any(bool(np.any(np.isinf(tb[0][1:]))) for _, tb in reference(case))


CONDITIONS = {"nontrivial": nontrivial, "ties_decide": ties_decide, "beam_edge_decides": beam_edge_decides,
              "no_word_end_frames": no_word_end_frames}
