"""The head of the refinement's main-pass iteration: 64-frame blocks handed out to the waves, every mask quad requested with the
features.

Through sr_refine_masks on shapes taken from sr_refine_geometry, against the CPU oracle's score table bit for bit: every mask holds the
density the oracle's minimum comes from plus none, one or two others, so that what the kernel has to store IS Oracle.score_matrix's
entry -- and the minimum is the first, the second or the third candidate by (wave, iteration, lane), so that a candidate that is
dropped, taken from another frame's quad or evaluated with another frame's features shows.  refined_densities must equal the number of
candidates.  Which wave takes which block is up to the hardware: the scores and the count may not depend on it, and every launch
runs twice.  (A phase offset between the waves of a SIMD was measured and not kept -- profiles/refine_iteration_head.txt -- so there
is no knob for it to test.)

Frames per workgroup (T threads): T - 1 (the last block one frame short), T (full blocks only), T + 1 (a last block of one frame: 63
shadow lanes), 2 T + 1 (every wave more than one block, lists carried over); and one launch the launcher cuts into two frame splits,
the second one frame shorter.  16 states x 32 densities at dimension 39 (768 threads, 8 states = two mask quads per
workgroup); 2 T + 1 once more at dimension 50 (512 threads, one quad)."""
import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import prefilter_reference as PR

pytestmark = pytest.mark.gpu

S, M, U = 16, 32, 4099  # states, densities per state, unique frames (a prime period: features 64 or T frames off are another row)
_models, _cases = {}, {}


def _model(tmp_path_factory, oracle_lib, D):
    """-> (tables for capi.Model.from_tables, unique frames [U, D], the oracle's score table [U, S], the density of each minimum [U, S])"""
    if D not in _models:
        spec = synth.make_mixset(S, [M] * S, D, seed=41 + D)
        mp = str(tmp_path_factory.mktemp("head") / f"m{D}.mix")
        synth.write_mixset(mp, spec)
        o = oracle_lib.Oracle(mp, D, synth.make_lexicon(2, 1, 1))
        tb = o.tables()
        tables = (tb["mix_off"], tb["means"], tb["vars_inv"], tb["norm"], tb["logw"])
        rng = np.random.default_rng(D)
        uniq = (rng.standard_normal((U, D)) * rng.choice([0.3, 1.0, 2.5], size=(U, 1))).astype(np.float32)
        uniq[5, D // 2] = np.nan  # the oracle keeps the seed 1e10 there
        table = o.score_matrix(uniq, 16)
        o.close()
        assert np.array_equal(np.diff(tables[0]), np.full(S, M))
        # which density the minimum is: from density_score_sse's operation order in numpy, held against the oracle's table bit for bit
        ds = PR.density_scores(tables, uniq)
        if not np.array_equal(PR.state_minimum(tables[0], ds).view(np.uint64), table.view(np.uint64)):
            raise RuntimeError("the reference is wrong: density_scores' state minima differ from Oracle.score_matrix")
        arg = np.argmin(np.where(np.isnan(ds), np.inf, ds).reshape(U, S, M), axis=2)
        _models[D] = (tables, uniq, table, arg, ds)
    return _models[D]


def _masks(arg_rows, threads, fps):
    """[4 groups][T][4]: state s of frame t gets k = 1, 2 or 3 candidates by the frame's place in its workgroup's range -- (wave, iteration,
    lane) of a fixed share per wave, tests/test_gpu_refine_masks.py's coordinates -- and s, the oracle's minimum the p-th of them in bit
    order, p by (lane, iteration, s) as far as densities 0 .. 31 leave room below and above it"""
    T = len(arg_rows)
    r = np.arange(T) % fps
    it, wave, lane = r // threads, (r % threads) // 64, r % 64
    masks = np.zeros((S // 4, T, 4), np.uint32)
    n_bits = 0
    for s in range(S):
        a = arg_rows[:, s].astype(np.int64)
        k = 1 + (lane + 5 * wave + 7 * it + s) % 3
        p = (lane + it + s) % k
        p = np.maximum(np.minimum(p, a), k - 1 - (M - 1 - a))  # p below, k - 1 - p above
        w = np.uint32(1) << a.astype(np.uint32)
        for i in (1, 2):
            w |= np.where(i <= p, np.uint32(1) << np.maximum(a - i, 0).astype(np.uint32), np.uint32(0))
            w |= np.where(i <= k - 1 - p, np.uint32(1) << np.minimum(a + i, M - 1).astype(np.uint32), np.uint32(0))
        assert np.array_equal(np.unpackbits(w.view(np.uint8)).reshape(T, 32).sum(1), k)
        masks[s >> 2, :, s & 3] = w
        n_bits += int(k.sum())
    return masks, n_bits


def _case(tmp_path_factory, oracle_lib, m, D, shape):
    """-> (features, masks, the oracle's table for these frames, candidates) of a launch whose workgroups get `shape` frames each"""
    tables, uniq, table, arg, ds = _model(tmp_path_factory, oracle_lib, D)
    if (D, shape) not in _cases:
        threads, spw, fps0, chunks = m.refine_geometry(1 << 24)
        assert chunks == 1 and threads == (768 if D <= 46 else 512), (threads, chunks)
        splits = -(-(1 << 24) // fps0)  # of a long launch: as many as the launcher ever cuts for this model
        if shape == "two splits":
            T = threads + 101
            fps = -(-T // 2)
            assert T - fps == fps - 1  # the second split is one frame short
        else:
            fps = {"T-1": threads - 1, "T": threads, "T+1": threads + 1, "2T+1": 2 * threads + 1}[shape]
            T = splits * fps
        assert m.refine_geometry(T) == (threads, spw, fps, 1), (m.refine_geometry(T), threads, spw, fps)
        rows = np.arange(T) % U
        masks, n_bits = _masks(arg[rows], threads, fps)
        # the test's own masks: the minimum over their bits is the oracle's entry (every mask holds the density it comes from)
        want, n_ref, complete = PR.masked_minimum(tables[0], ds, masks, rows)
        assert complete and n_ref == n_bits and np.array_equal(want.view(np.uint64), table[rows].view(np.uint64))
        print(f"D={D} {shape}: {threads} threads, {fps} frames per workgroup, {T} frames, {n_bits} candidates for {T * S} pairs")
        _cases[(D, shape)] = (uniq[rows], masks, table[rows], n_bits)
    return _cases[(D, shape)]


CASES = [(39, "T-1"), (39, "T"), (39, "T+1"), (39, "2T+1"), (39, "two splits"), (50, "2T+1")]


@pytest.mark.parametrize("D, shape", CASES, ids=[f"{d}-{s.replace(' ', '_')}" for d, s in CASES])
def test_scores_are_the_oracles_whichever_wave_takes_a_block(tmp_path_factory, oracle_lib, D, shape):
    tables = _model(tmp_path_factory, oracle_lib, D)[0]
    with capi.Model.from_tables(*tables) as m:
        feats, masks, want, n_bits = _case(tmp_path_factory, oracle_lib, m, D, shape)
        for run in range(2):
            m.profile(True)
            got = m.refine_masks(feats, masks)
            n_eval = m.profile_read()["refined_densities"]
            m.profile(False)
            bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
            assert bad.size == 0, (f"D={D} {shape} run {run}: {len(bad)} of {got.size} entries differ from the oracle's, first (frame, state) "
                                   f"{bad[0]}: {got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}")
            assert n_eval == n_bits, f"D={D} {shape} run {run}: {n_eval} evaluations for {n_bits} candidates"
