"""The FP64 refinement alone (sr_refine_masks) on masks the prefilter never writes.

In a scoring call the refinement sees the prefilter's masks only: one candidate for ~96 % of the pairs on the suite's models, and at
the suite's small shapes one main-pass iteration per workgroup, so that no list ever carries entries over.  A candidate that is not the
minimum is invisible in the scores whether it is evaluated twice or never.  Here the kernel gets mask arrays of every kind -- walking
single bits, all ones, exactly two and three candidates, random, empty, per-chunk patterns -- and has to return, bit for bit, the
minimum of density_scores (tests/prefilter_reference.py: density_score_sse's operation order, checked against the oracle's
score_matrix on this very model) over the set bits, and to have evaluated every candidate exactly once (refined_densities == the
number of set bits that are densities).  (i) every instantiation at one-iteration shapes; (ii) shapes taken from sr_refine_geometry at
which every workgroup runs three main-pass iterations, with masks laid out by (wave, iteration, lane) so that the lists hold
63 + 64 = 127 entries, fill in mid-run, stay at exactly 64, loop over 31 candidates at level 2, and -- on the deferred routes -- fill a
segment in iteration 1 and leave the drain kernel more than one batch."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import prefilter_reference as PR

pytestmark = pytest.mark.gpu

ROUTES = {"default": {}, "cap3": {"SRGPU_DEFER_CAP": "3"}, "cap70": {"SRGPU_DEFER_CAP": "70"}, "mb0": {"SRGPU_DEFER_MB": "0"}}
_models = {}


def _model(tmp_path_factory, oracle_lib, D, sizes, n_unique, seed):
    """-> (tables as capi.Model.from_tables takes them, unique frames [U, D], their density scores [U, C]).  The tables are the oracle's
    own (MixtureModel::finalize of a synthetic mixset), so that density_scores can be held against Oracle.score_matrix: a mismatch
    there is an error of the reference, not of the kernel, and ends the test as an error."""
    key = (D, tuple(sizes), n_unique, seed)
    if key not in _models:
        spec = synth.make_mixset(len(sizes), sizes, D, seed=seed)
        mp = str(tmp_path_factory.mktemp("refine") / f"m{D}_{max(sizes)}.mix")
        synth.write_mixset(mp, spec)
        o = oracle_lib.Oracle(mp, D, synth.make_lexicon(2, 1, 1))
        tb = o.tables()
        C = len(tb["mix_mean"])
        if not (np.array_equal(tb["mix_mean"], np.arange(C)) and np.array_equal(tb["mix_var"], np.arange(C))):
            raise RuntimeError("the synthetic mixset ties nothing: one mean and one variance row per density")
        tables = (tb["mix_off"], tb["means"], tb["vars_inv"], tb["norm"], tb["logw"])
        rng = np.random.default_rng(seed + 1)
        uniq = (rng.standard_normal((n_unique, D)) * rng.choice([0.3, 1.0, 2.5], size=(n_unique, 1))).astype(np.float32)
        uniq[3, D // 2] = np.nan
        uniq[n_unique - 2, 0] = np.nan
        ds = PR.density_scores(tables, uniq)
        mine, theirs = PR.state_minimum(tb["mix_off"], ds), o.score_matrix(uniq, 16)
        o.close()
        same = np.array_equal(mine.view(np.uint64), theirs.view(np.uint64))
        print(f"D={D} largest mixture {max(sizes)}: density_scores' minima equal Oracle.score_matrix bit for bit on {n_unique} frames: {same}")
        if not same:
            raise RuntimeError("the reference is wrong: density_scores' state minima differ from Oracle.score_matrix")
        _models[key] = (tables, uniq, ds)
    return _models[key]


def _sizes(rng, S, largest):
    """one state of the largest mixture, one of a single density, one of three, the others of 2 .. 5: the reference stays cheap"""
    sizes = [int(v) for v in rng.integers(2, 6, S)]
    sizes[int(S // 2)], sizes[1], sizes[S - 1] = largest, 1, 3
    return sizes


def _set(masks, ps, frames, words):
    masks[ps >> 2, frames, ps & 3] = words


def _cyclic(dens_off, masks, s, start, k):
    """state s: frame t gets the k[t] densities start[t], start[t] + 1, ... (cyclic) as candidates, across the state's chunks"""
    Cs, _, _ = PR.pseudo_states(dens_off)
    nd = int(dens_off[s + 1] - dens_off[s])
    k = np.minimum(k, nd)
    words = np.zeros((len(start), Cs), np.uint32)
    for i in range(int(k.max())):
        d = (start + i) % nd
        on = i < k
        np.bitwise_or.at(words, (np.flatnonzero(on), d[on] >> 5), (np.uint32(1) << (d[on] & 31).astype(np.uint32)))
    for c in range(Cs):
        _set(masks, s * Cs + c, slice(None), words[:, c])


def _run(m, dens_off, ds, feats, rows, masks, name):
    """the hook twice (equal bytes), against the reference (equal bits), and the evaluation count"""
    want, n_bits, complete = PR.masked_minimum(dens_off, ds, masks, rows)
    m.profile(True)
    got = m.refine_masks(feats, masks)
    n_eval = m.profile_read()["refined_densities"]
    m.profile(False)
    again = m.refine_masks(feats, masks)
    assert got.tobytes() == again.tobytes(), f"{name}: two runs differ"
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (f"{name}: {len(bad)} of {got.size} entries differ, first (frame, state) {bad[0]}: {got[tuple(bad[0])]!r} "
                           f"against {want[tuple(bad[0])]!r}")
    print(f"{name}: {got.size} pairs, {n_bits} candidates, {n_eval} evaluated" + ("" if complete else " (some pairs without a candidate)"))
    if complete:
        assert n_eval == n_bits, f"{name}: {n_eval} evaluations for {n_bits} candidates"
    else:
        assert n_eval >= n_bits, f"{name}: {n_eval} evaluations for {n_bits} candidates"  # (a pair without one still costs the main pass one)


# ---- (i) every instantiation, one main-pass iteration --------------------------------------------------------------------------------
SMALL = [(9, 8, "default"), (13, 16, "default"), (25, 16, "default"), (26, 32, "default"), (39, 8, "default"), (39, 32, "default"),
         (39, 64, "default"), (39, 64, "cap3"), (39, 64, "mb0"), (39, 128, "default"), (25, 160, "default"), (45, 32, "default"),
         (47, 64, "default"), (50, 32, "default"), (62, 100, "default")]


def _families(rng, dens_off, ds_rows, T, spw):
    """name -> masks [groups][T][4]"""
    Cs, PS, cnt = PR.pseudo_states(dens_off)
    S, G = len(dens_off) - 1, (PS + 3) // 4
    t = np.arange(T)
    unit = min(Cs, 4)  # chunks the kernel takes a first candidate from: the state's, or one half's (Cs = 8)
    # The kernel evaluates slot 31 where a mask is empty and drops the result; in the last panel of a workgroup whose panels have fewer
    # than 32 slots that read would leave the workgroup's LDS image.  The prefilter never writes an empty mask; here they stay off that panel.
    narrow = int(np.max(np.diff(dens_off))) <= 16
    out = {}

    def blank():
        return np.zeros((G, T, 4), np.uint32)

    def keep_nonempty(masks):
        for ps in range(PS):
            if narrow and ps % spw == spw - 1 and cnt[ps]:
                w = masks[ps >> 2, :, ps & 3]
                empty = (w & np.uint32((1 << int(cnt[ps])) - 1)) == 0
                w[empty] |= np.uint32(1) << ((t[empty] + ps) % cnt[ps]).astype(np.uint32)
        return masks

    walk = blank()
    for ps in range(PS):
        if cnt[ps]:
            _set(walk, ps, slice(None), np.uint32(1) << ((t + ps) % cnt[ps]).astype(np.uint32))
    out["one walking bit"] = walk
    out["all ones"] = np.full((G, T, 4), 0xFFFFFFFF, np.uint32)
    for k in (2, 3):
        mk = blank()
        for s in range(S):
            _cyclic(dens_off, mk, s, (5 * t + s) % int(dens_off[s + 1] - dens_off[s]), np.full(T, k))
        out[f"exactly {k} candidates"] = mk
    for p in (0.05, 0.5):
        bits = rng.random((G, T, 4, 32)) < p
        out[f"random bits, p = {p}"] = keep_nonempty((bits * (np.uint32(1) << np.arange(32, dtype=np.uint32))).sum(-1).astype(np.uint32))
    holes = walk.copy()
    holes[rng.random((G, T, 4)) < 0.15] = 0
    out["walking bit with empty masks"] = keep_nonempty(holes)
    if Cs > 1:
        last = blank()
        for u in range(PS // unit):  # candidates only in the last chunk that has densities
            chunks = [ps for ps in range(u * unit, (u + 1) * unit) if cnt[ps]]
            if chunks:
                ps = chunks[-1]
                w = (rng.random((T, 32)) < 0.3) * (np.uint32(1) << np.arange(32, dtype=np.uint32))
                _set(last, ps, slice(None), w.sum(-1).astype(np.uint32) | (np.uint32(1) << ((t + ps) % cnt[ps]).astype(np.uint32)))
        out["candidates in the last chunk only"] = last
    if Cs == 8:
        alt = walk.copy()
        for s in range(S):
            lo, hi = int(dens_off[s]), int(dens_off[s + 1])
            if hi - lo <= 128:
                continue
            sc = np.where(np.isnan(ds_rows[:, lo:hi]), np.inf, ds_rows[:, lo:hi])
            first = t % 2 == 0  # the half that gets its smallest density; the other half gets its largest
            d0 = np.where(first, np.argmin(sc[:, :128], 1), np.argmax(sc[:, :128], 1))
            d1 = 128 + np.where(first, np.argmax(sc[:, 128:], 1), np.argmin(sc[:, 128:], 1))
            for c in range(8):
                w = np.zeros(T, np.uint32)
                for d in (d0, d1):
                    on = (d >> 5) == c
                    w[on] |= np.uint32(1) << (d[on] & 31).astype(np.uint32)
                _set(alt, s * 8 + c, slice(None), w)
            best = np.where(sc[t, d0] <= sc[t, d1], 0, 1)
            assert np.mean(best == np.where(first, 0, 1)) > 0.9, "the minimum alternates between the halves"
        out["the minimum alternately in either half"] = alt
    return out


@pytest.mark.parametrize("D, largest, route", SMALL, ids=[f"{d}-{m}-{r}" for d, m, r in SMALL])
def test_every_instantiation(tmp_path_factory, oracle_lib, monkeypatch, D, largest, route):
    rng = np.random.default_rng(100 * D + largest)
    S = 13 + (D + largest) % 9
    tables, uniq, ds = _model(tmp_path_factory, oracle_lib, D, _sizes(rng, S, largest), 997, 31 * D + largest)
    for k in ("SRGPU_DEFER_CAP", "SRGPU_DEFER_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    with capi.Model.from_tables(*tables) as m:  # (the knobs are read when the model is created)
        threads, spw, _, chunks = m.refine_geometry(1)
        T = threads + 37
        threads, spw, fps, chunks = m.refine_geometry(T)
        assert chunks == PR.pseudo_states(tables[0])[0] and fps <= threads, (threads, spw, fps, chunks)
        rows = np.arange(T) % len(uniq)  # both NaN frames are among them
        feats = uniq[rows]
        with pytest.raises(capi.SrError):  # a mask array of another size than groups x frames x 4 is refused on the host
            m.refine_masks(feats, np.zeros(((PR.pseudo_states(tables[0])[1] + 3) // 4 + 1, T, 4), np.uint32))
        for name, masks in _families(rng, tables[0], ds[rows], T, spw).items():
            _run(m, tables[0], ds, feats, rows, masks, f"D={D} M<={largest} {route}: {name}")


# ---- (ii) lists that carry over: three main-pass iterations per workgroup ---------------------------------------------------------------
LARGE = [(39, 32, "default"), (9, 8, "default"), (39, 64, "default"), (39, 64, "cap3"), (39, 64, "cap70"), (39, 64, "mb0"), (45, 32, "default"),
         (62, 32, "default")]


@pytest.mark.parametrize("D, largest, route", LARGE, ids=[f"{d}-{m}-{r}" for d, m, r in LARGE])
def test_lists_that_carry_over(tmp_path_factory, oracle_lib, monkeypatch, D, largest, route):
    rng = np.random.default_rng(7 * D + largest)
    # states with a part to play: `big` every candidate in every lane and iteration; the others by (wave, iteration, lane), see below
    sizes = [4, 1, 5, 2, largest, 3, 3, 4] + [1, 2] * 4
    second, third, sixty_four, big, fills, two_batches = 0, 2, 3, 4, 5, 6
    tables, uniq, ds = _model(tmp_path_factory, oracle_lib, D, sizes, 4099, 17 * D + largest)
    dens_off = tables[0]
    for k in ("SRGPU_DEFER_CAP", "SRGPU_DEFER_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    with capi.Model.from_tables(*tables) as m:
        threads, spw, fps0, chunks = m.refine_geometry(1 << 24)
        splits = -(-(1 << 24) // fps0)  # of a long launch: as many as the launcher ever cuts for this model
        fps = 2 * threads + 64          # two full passes of the threads and wave 0 once more
        T = splits * fps
        assert m.refine_geometry(T) == (threads, spw, fps, chunks)
        n_it = [-(-(min(T, (y + 1) * fps) - y * fps) // threads) for y in range(splits)]
        assert min(n_it) >= 3, n_it
        print(f"D={D} M<={largest} {route}: {threads} threads, {spw} pseudo-states and {fps} frames per workgroup, {splits} splits, {T} frames, "
              f"{T * len(sizes)} pairs, {min(n_it)} iterations")
        t = np.arange(T)
        r = t % fps
        it, wave, lane = r // threads, (r % threads) // 64, r % 64
        Cs, PS, cnt = PR.pseudo_states(dens_off)
        masks = np.zeros(((PS + 3) // 4, T, 4), np.uint32)
        for ps in range(PS):  # everybody else: one walking bit per pseudo-state
            if cnt[ps]:
                _set(masks, ps, slice(None), np.uint32(1) << ((t + ps) % cnt[ps]).astype(np.uint32))
        w0 = wave == 0
        # wave 0's list of `second`: 63 pending after iteration 0, 63 + 64 = 127 in iteration 1 (a batch of 64 leaves 63), 64 at the end
        k = 1 + (w0 & (((it == 0) & (lane < 63)) | (it == 1) | ((it == 2) & (lane == 0))))
        _cyclic(dens_off, masks, second, t % sizes[second], k)
        # the same at level 2 in wave 0's list of `third`: iteration 0 lists 64 pairs, 63 with a third candidate: the level-1 batch leaves 63
        # at level 2; iteration 1 lists 64 with three: 63 + 64 = 127 there; one more pair in the last iteration
        k = 1 + np.where(w0 & (it == 0), np.where(lane < 63, 2, 1), np.where(w0 & ((it == 1) | (lane == 0)), 2, 0))
        _cyclic(dens_off, masks, third, t % sizes[third], k)
        # every lane of every wave lists a pair in every iteration: the list is at exactly 64 each time
        _cyclic(dens_off, masks, sixty_four, t % sizes[sixty_four], np.full(T, 2))
        # every candidate everywhere: every list full every time, level 2 loops over up to 31 candidates
        _cyclic(dens_off, masks, big, np.zeros(T, np.int64), np.full(T, largest))
        # deferred routes: 2 + 2 entries -- a segment of 3 fills in iteration 1; 40 + 30 = 70 entries -- a segment of 70 is full after
        # iteration 1, is worked off in two batches, and iteration 2's 64 are evaluated on the spot
        _cyclic(dens_off, masks, fills, t % sizes[fills], 1 + ((lane < 2) & (it < 2)) + ((lane == 0) & (it == 2)))
        _cyclic(dens_off, masks, two_batches, t % sizes[two_batches], 1 + np.where(it == 0, lane < 40, np.where(it == 1, lane < 30, True)) * 2)
        rows = t % len(uniq)  # a prime period: a pair evaluated with another frame's features (64 or `threads` frames off) shows
        _run(m, dens_off, ds, uniq[rows], rows, masks, f"D={D} M<={largest} {route}")
