"""Cases for the forced aligners and the Baum-Welch pass run alone on score tables the test makes up (sr_align_corpus_scores,
sr_state_posteriors_corpus_scores): batches of (positions, frames), automata, tables, the references' answers and the conditions that
keep a case from passing vacuously.  No GPU and no pytest in here: tests/test_align_cases_cpu.py checks every case's conditions,
tests/test_gpu_align_scores.py and tests/test_gpu_fb_scores.py run the kernels on them.

Why tables and not features: through a mixture model a test cannot place a tie between loop, forward and skip, a +inf cell, a frame
that kills every path, a beam that ends below the last position, costs of 1e6 or a posterior exactly on the floor.  Here the table
is the input.  `dyadic` tables hold multiples of 0.25 up to 4 and go with the penalties (0.5, 0, 0.75): every path sum is exact in
binary, so equal sums are equal bits and ties are dense.

One tiny model (40 states of one density, dimension 2) gives the handles something to attach to; only its number of states
matters.  State 0 is the silence state of every call; an automaton holds it only where a case places it."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from tests import fb_reference as fbr
from tests import search_cases as sc

N_STATES = 40
SIL = 0
MODEL_DIM = sc.MODEL_DIM
INF = math.inf

TDP = (3.0, 0.0, 30.0)
TDP_DYADIC = (0.5, 0.0, 0.75)
TDP_NO_SKIP = (3.0, 0.0, INF)
TDP_FORWARD_ONLY = (INF, 0.0, INF)  # one position a frame (any jump out of silence costs `forward`): a path needs N = T
TDP_ZERO = (0.0, 0.0, 0.0)


def model_file():
    return sc.model_file(N_STATES)


# ---- batches: the (positions N, frames T) of a call's utterances -----------------------------------------------------------------
def _ragged70():
    rng = np.random.default_rng(7070)
    out = []
    for _ in range(70):
        T = int(rng.integers(1, 41))
        out.append((int(rng.integers(1, T + 1)), T))
    return tuple(out)


def _chunky():
    """16 utterances of 250 .. 300 frames: some 4 400 frames, more than the 3 276 a 1 MiB score chunk of this model holds (two chunks,
    the second at a frame base other than 0), and trellises of 0.1 .. 0.6 MiB each (several launch groups at SRGPU_FB_MB=1)"""
    rng = np.random.default_rng(1616)
    return tuple((int(rng.integers(60, 258)), int(rng.integers(250, 301))) for _ in range(16))


BATCHES = {
    "tiny": ((1, 1), (1, 5), (2, 2)),
    "tiny_wide": ((3, 2), (1, 1), (2, 2)),      # N > T: not for the full aligner
    "onepath": ((5, 3),),                       # N = 2 T - 1: one path, all skips
    "b64": ((64, 70),),                         # the forward-backward's one-wave block
    "b65": ((65, 70),),                         # ... and the first length that takes 256 threads
    "b64_65": ((64, 70), (65, 70)),
    "b257": ((257, 300),),                      # more positions than threads
    "b600": ((600, 301),),                      # N = 2 T - 2
    "ragged70": _ragged70(),
    "chunky": _chunky(),
    "five": ((20, 31), (33, 40), (25, 38), (12, 12), (30, 33)),
    "exact_fit": ((30, 30), (12, 20), (40, 40), (1, 1)),  # N = T: the paths TDP_FORWARD_ONLY leaves
    "floor": ((2, 3), (3, 4)),
}


def kinds_of(batch):
    """which passes take the batch: the full aligner needs N <= T, the forward-backward N <= 2 T - 1"""
    shapes = BATCHES[batch]
    return (("full",) if all(n <= t for n, t in shapes) else ()) + ("pruned",) + (("fb",) if all(n <= 2 * t - 1 for n, t in shapes) else ())


@dataclass(frozen=True)
class Case:
    batch: str
    table: str                  # dyadic | random | signed | inf_band | inf_frame | nan | neginf | zeros
    scale: float = 1.0          # random: uniform in [0, scale) (the penalties scaled alike: the same problem in other units) ...
    offset: float = 0.0         # ... plus offset
    tdp: tuple = TDP
    sil: str = None             # None (absent) | first | middle | last: where every automaton holds the silence state
    thresholds: tuple = ()      # the pruned aligner's runs
    seed: int = 0
    conditions: tuple = ()      # names in CONDITIONS, beside those every case gets
    only: tuple = None          # the passes, where fewer than kinds_of(batch)

    @property
    def id(self):
        parts = [self.batch, self.table]
        if self.table == "random" and (self.scale != 1.0 or self.offset):
            parts.append(f"x{self.scale:g}" + (f"+{self.offset:g}" if self.offset else ""))
        if self.tdp == TDP_NO_SKIP:
            parts.append("noskip")
        if self.tdp == TDP_FORWARD_ONLY:
            parts.append("fwdonly")
        if self.sil:
            parts.append("sil_" + self.sil)
        return "-".join(parts)

    @property
    def kinds(self):
        k = kinds_of(self.batch)
        return tuple(x for x in k if self.only is None or x in self.only)


HOSTILE_UTT = 2   # the utterance of `five` (and of ragged70's inf_frame) that gets the NaN, the -inf, the frame of +inf


def _cases():
    out = []
    dy = dict(table="dyadic", tdp=TDP_DYADIC, thresholds=(0.0, 0.25, INF))
    for b in ("tiny", "tiny_wide", "onepath", "b64", "b65", "b64_65", "b257", "b600", "ragged70", "five"):
        out.append(Case(b, **dy, conditions=("ties",) if b in ("b64_65", "b257", "ragged70", "five") else ()))
        out.append(Case(b, "random", thresholds=(0.0, 2.0, INF)))
    for b in ("b64_65", "ragged70"):
        for scale in (1e-3, 1e3, 1e6):
            out.append(Case(b, "random", scale=scale, tdp=tuple(x * scale for x in TDP), thresholds=(0.0, 2.0 * scale, INF)))
        out.append(Case(b, "random", offset=1e8, thresholds=(0.0, 2.0, INF)))
        out.append(Case(b, "signed", thresholds=(0.0, 60.0, INF)))
        out.append(Case(b, "inf_band", thresholds=(0.0, 2.0, INF)))
        out.append(Case(b, "random", tdp=TDP_NO_SKIP, thresholds=(2.0,)))
        for sil in ("first", "middle", "last"):
            out.append(Case(b, "dyadic", tdp=TDP_DYADIC, sil=sil, thresholds=(0.25,)))
            out.append(Case(b, "random", sil=sil, thresholds=(2.0,)))
    out.append(Case("b257", "random", scale=1e6, tdp=tuple(x * 1e6 for x in TDP), thresholds=(2e6,)))
    out.append(Case("exact_fit", "random", tdp=TDP_FORWARD_ONLY, thresholds=(2.0, INF)))
    out.append(Case("exact_fit", "dyadic", tdp=TDP_FORWARD_ONLY, sil="middle", thresholds=(0.25,)))
    for b in ("five", "ragged70"):
        out.append(Case(b, "inf_frame", thresholds=(2.0, INF), conditions=("no_path",)))
    out.append(Case("five", "nan", thresholds=(2.0, INF)))
    out.append(Case("five", "neginf", thresholds=(2.0, INF)))
    # the beam ends below the last position: 600 positions in 301 frames take a skip in all frames but one, and the cheap ways on do not
    out.append(Case("b600", "random", seed=1, thresholds=(0.0, 2.0), conditions=("ends_below",), only=("pruned",)))
    out.append(Case("b600", "dyadic", tdp=TDP_DYADIC, seed=1, thresholds=(0.25,), conditions=("ends_below",), only=("pruned",)))
    out.append(Case("floor", "zeros", tdp=TDP_ZERO, conditions=("half",), only=("fb",)))
    out.append(Case("chunky", "random", thresholds=(2.0,)))
    out.append(Case("chunky", "dyadic", tdp=TDP_DYADIC, thresholds=(0.25,)))
    ids = [c.id + f"-s{c.seed}" for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()


def case_id(c):
    return c.id + (f"-s{c.seed}" if c.seed else "")


# ---- automata and tables -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def automata(batch, sil=None, seed=0):
    """One automaton per utterance over states 1 .. 39: even utterances of at most 39 positions hold distinct states (the posteriors of
    their mixtures are those of their positions), the others draw theirs from a few states, or -- longer ones -- from all (a mixture's
    posterior is a sum over positions).  sil: the silence state at the first, the middle or the last position of every one."""
    rng = np.random.default_rng(5000 + seed)
    out = []
    for i, (N, _) in enumerate(BATCHES[batch]):
        if N <= 39 and i % 2 == 0:
            ref = rng.permutation(np.arange(1, N_STATES))[:N]
        elif N <= 39:
            ref = rng.integers(1, 7, size=N)
        else:
            ref = rng.integers(1, N_STATES, size=N)
        ref = ref.astype(np.uint16)
        if sil:
            ref[{"first": 0, "middle": N // 2, "last": N - 1}[sil]] = SIL
        ref.setflags(write=False)
        out.append(ref)
    return tuple(out)


def frame_off(batch):
    return np.concatenate([[0], np.cumsum([t for _, t in BATCHES[batch]])]).astype(np.uint64)


def batch(case):
    """-> (table [F, 40] f64, frame_off u64[U + 1], automata); built once per case and never written to"""
    return _batch(case.batch, case.table, case.scale, case.offset, case.tdp, case.sil, case.seed)


@functools.lru_cache(maxsize=None)
def _batch(name, kind, scale, offset, tdp, sil, seed):
    rng = np.random.default_rng(6000 + seed)
    off = frame_off(name)
    auts = automata(name, sil, seed)
    F = int(off[-1])
    if kind == "dyadic":
        t = rng.integers(0, 17, size=(F, N_STATES)).astype(np.float64) * 0.25
    elif kind == "signed":
        t = rng.uniform(-50.0, 50.0, size=(F, N_STATES))
    elif kind == "zeros":
        t = np.zeros((F, N_STATES))
    else:
        t = rng.uniform(0.0, 1.0, size=(F, N_STATES)) * scale + offset
    if kind == "inf_band":  # the state of every automaton's middle position, for the frames of the utterance's second quarter
        for u, ref in enumerate(auts):
            f0, T = int(off[u]), int(off[u + 1]) - int(off[u])
            t[f0 + T // 4:f0 + T // 2 + 1, ref[len(ref) // 2]] = INF
    elif kind == "inf_frame":  # no path through the utterance
        f0, T = int(off[HOSTILE_UTT]), int(off[HOSTILE_UTT + 1]) - int(off[HOSTILE_UTT])
        t[f0 + T // 2] = INF
    elif kind in ("nan", "neginf"):  # on the utterance's best path, half way
        f0, T = int(off[HOSTILE_UTT]), int(off[HOSTILE_UTT + 1]) - int(off[HOSTILE_UTT])
        states, _ = fbr.viterbi(t[f0:f0 + T], auts[HOSTILE_UTT], tdp, SIL)
        t[f0 + T // 2, states[T // 2]] = np.nan if kind == "nan" else -INF
    t.setflags(write=False)
    off.setflags(write=False)
    return t, off, auts


def rows(case, u):
    t, off, _ = batch(case)
    return t[int(off[u]):int(off[u + 1])]


# ---- references ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import pyoracle
    from speechrecognition_amd import synth

    lex = synth.ExplicitLexicon(np.array([0, 1, 3], np.uint32), np.array([0, 1, 2], np.uint16), 0)  # (only the model is used)
    return pyoracle, pyoracle.Oracle(model_file(), MODEL_DIM, lex)


def oracle_align(table_rows, ref, tdp, threshold=None):
    """Oracle.align_full (threshold None) / align_pruned on the rows of one utterance -> (states u16[T], cost)"""
    pyoracle, orc = _oracle()
    orc._tdp = pyoracle._Tdp(tdp[0], tdp[1], tdp[2], SIL)
    feats = np.zeros((len(table_rows), MODEL_DIM), np.float32)
    if threshold is None:
        return orc.align_full(feats, ref, dense=table_rows)
    return orc.align_pruned(feats, ref, threshold, dense=table_rows)


@functools.lru_cache(maxsize=None)
def align_reference(case, threshold):
    """per utterance (states, cost) of the oracle on the case's table; threshold None: the full aligner"""
    _, _, auts = batch(case)
    out = []
    for u, ref in enumerate(auts):
        states, cost = oracle_align(rows(case, u), ref, case.tdp, threshold)
        states.setflags(write=False)
        out.append((states, float(cost)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fb_reference(case, dtype_name):
    """per utterance (F, mixtures ascending, [T, M] posteriors) of tests/fb_reference.py in float64 or longdouble"""
    dtype = {"float64": np.float64, "longdouble": np.longdouble}[dtype_name]
    _, _, auts = batch(case)
    out = []
    for u, ref in enumerate(auts):
        with np.errstate(all="ignore"):
            F, g = fbr.posteriors(rows(case, u), ref, case.tdp, SIL, dtype=dtype)
        mix, gm = fbr.mixture_posteriors(g, ref)
        gm.setflags(write=False)
        out.append((F, mix, gm))
    return tuple(out)


def same_cost(a, b):
    """equal as uint64; both NaN counts as equal"""
    a, b = np.float64(a), np.float64(b)
    return bool(a.view(np.uint64) == b.view(np.uint64)) or bool(np.isnan(a) and np.isnan(b))


# ---- conditions, from the references alone -------------------------------------------------------------------------------------------
def tie_fraction(case):
    """share of the full aligner's cells (inside the window, finite) whose best candidate has an equal among loop, forward, skip"""
    _, _, auts = batch(case)
    tied = cells = 0
    for u, ref in enumerate(auts):
        A, _ = fbr.forward(rows(case, u), ref, case.tdp, SIL, "min")
        c = fbr._jump_costs(ref, case.tdp, SIL)
        for t in range(1, A.shape[0]):
            cand = np.stack([fbr._shift(A[t - 1] + c[j], j) for j in range(3)])
            best = cand.min(axis=0)
            ok = np.isfinite(best)
            tied += int(np.sum((np.sum(cand == best, axis=0) >= 2) & ok))
            cells += int(np.sum(ok))
    return tied / max(cells, 1)


def pruned_stats(table_rows, ref, tdp, threshold):
    """The pruned aligner restated for counting -> (nodes created, nodes pruned, highest position alive at the end, its cost)"""
    ref = np.asarray(ref, dtype=np.int64)
    E = np.asarray(table_rows)[:, ref]
    T, N = E.shape
    c = np.empty((3, N))
    for j in range(3):
        c[j] = tdp[j]
    c[:, ref == SIL] = tdp[1]  # keyed on the DESTINATION
    alive = np.zeros(N, bool)
    alive[0] = True
    cost = np.full(N, INF)
    cost[0] = E[0, 0]
    created = killed = 0
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            new, have = np.full(N, INF), np.zeros(N, bool)
            for j in (2, 1, 0):  # sources in ascending position
                src = np.zeros(N, bool)
                src[j:] = alive[:N - j] if j else alive
                n = fbr._shift(cost, j) + c[j] + E[t]
                first, better = src & ~have, src & have & (new > n)
                new[first | better] = n[first | better]
                have |= src
            vals = new[have & ~np.isnan(new)]
            best = vals.min() if len(vals) else INF
            kill = have & (new > best + threshold)
            created += int(have.sum())
            killed += int(kill.sum())
            alive, cost = have & ~kill, new
    hi = int(np.flatnonzero(alive)[-1])
    return created, killed, hi, float(cost[hi])


def prune_share(case, threshold):
    _, _, auts = batch(case)
    created = killed = 0
    for u, ref in enumerate(auts):
        c, k, _, _ = pruned_stats(rows(case, u), ref, case.tdp, threshold)
        created, killed = created + c, killed + k
    return killed / max(created, 1)


def ties(case):
    return tie_fraction(case) >= 0.05


def no_path(case):
    """the hostile utterance has F = +inf (and its Viterbi cost with it), its neighbours a finite one"""
    _, _, auts = batch(case)
    A = [fbr.forward(rows(case, u), auts[u], case.tdp, SIL, "min")[0][-1, -1] for u in (HOSTILE_UTT - 1, HOSTILE_UTT, HOSTILE_UTT + 1)]
    return bool(np.isfinite(A[0]) and A[1] == INF and np.isfinite(A[2]))


def ends_below(case):
    """at every threshold of the case some utterance's beam ends below its last position"""
    _, _, auts = batch(case)
    return all(any(pruned_stats(rows(case, u), ref, case.tdp, thr)[2] < len(ref) - 1 for u, ref in enumerate(auts)) for thr in case.thresholds)


def half(case):
    """the symmetric case: two paths of equal cost, so the middle frame's two posteriors are exactly 0.5"""
    _, g = fbr.posteriors(rows(case, 0), batch(case)[2][0], case.tdp, SIL)
    return bool(np.array_equal(g[1], [0.5, 0.5]))


CONDITIONS = {"ties": ties, "no_path": no_path, "ends_below": ends_below, "half": half}


def pruning_runs():
    """(case, threshold) of every run in which the beam is at work: a finite threshold"""
    return [(c, thr) for c in CASES if "pruned" in c.kinds for thr in c.thresholds if math.isfinite(thr)]
