"""The device's candidate masks against the documented limit (tests/prefilter_reference.py: reference_limits, check_masks).

Every other test of the prefilter compares the final scores with the oracle, or the two routes' masks with each other; both routes
share one epilogue and one table of limits, and on a model whose states are all drawn alike a limit read from the wrong state slot, or
one a few times too small or too large, changes no score (tests/test_prefilter_masks_reference_cpu.py shows it on the emulation).  Here
the masks of sr_prefilter_masks are held against 2 eps = limD |b^ - b| + lim1 |b| + lim0 computed in numpy from the model's tables: on a
model whose four state slots per group have limits about 100x apart and whose even states are ladders of copies 1e-4 .. 1e2 apart, no
candidate lies beyond twice the limit, no copy within half of it is dropped, the exact minimum is always in, padding is never set.
(Found when this was first run: the state slots beyond the last pseudo-state came out 0xFFFFFFFF for every frame -- all their rows
+inf, and inf <= inf + limit.  The refinement never read them; pack_prefilter now packs such a slot so that its word is 0.)"""
import numpy as np
import pytest

from speechrecognition_amd import capi
from tests import prefilter_reference as PR

pytestmark = pytest.mark.gpu

STAGED, STATIONARY = 0, 1
T = 400


def _case(M, D, n_frames=T, S=18):
    rng = np.random.default_rng(1000 * M + D + 7 * n_frames)
    tables, ladder = PR.heterogeneous_model(rng, M, D, S)
    feats = PR.reference_frames(rng, D, n_frames, tables[1][0])
    ref = PR.reference_limits(*tables, feats)
    share = PR.decided_share(ref, ladder)  # from the reference alone: before any device mask is looked at
    print(f"D={D} M={M} T={n_frames} S={S}: {ref.Cs} chunk(s) per state, decided share of ladder entries {share:.3f}")
    return tables, ladder, feats, ref, share


def _check(tables, ladder, feats, ref, D):
    with capi.Model.from_tables(*tables) as m:
        routes = [("staged", STAGED)] + ([("stationary", STATIONARY)] if D <= 46 else [])
        got = {}
        for name, route in routes:
            masks = m.prefilter_masks(feats, route)
            assert masks.shape == (ref.groups, feats.shape[0], 4), (name, masks.shape)
            try:
                PR.check_masks(masks, ref, ladder)
            except AssertionError as e:
                raise AssertionError(f"route {name}, dimension {D}: {e}") from None
            got[name] = masks
        if len(got) == 2:
            bad = np.argwhere(got["staged"] != got["stationary"])
            assert bad.size == 0, f"dimension {D}: {len(bad)} mask words differ between the routes, first (group, frame, slot) {bad[0]}"


CASES = ([(M, D) for D in (9, 14, 15, 30, 31, 39, 46, 47, 62) for M in (8, 32)]  # K = 2D + 3 = 31 / 33, 63 / 65, 95 / 97, 127; routes 46 / 47
         + [(M, D) for D in (39, 50) for M in (40, 64, 100)]                     # 2 and 4 chunks per state, a ragged last chunk
         + [(160, 25)])                                                          # two halves of four chunks


@pytest.mark.parametrize("M, D", CASES)
def test_masks_lie_inside_the_documented_limit(M, D):
    tables, ladder, feats, ref, share = _case(M, D)
    assert share >= 0.85, "a model that decides so little is a bad model, not a pass"
    _check(tables, ladder, feats, ref, D)


@pytest.mark.parametrize("n_frames", [1, 17, "range + 1"])
def test_frame_counts(n_frames):
    """one frame, a ragged tile, and one frame more than a frame range of the stationary route (6 states: the reference stays small)"""
    D, M = 39, 8
    S = 18
    if n_frames == "range + 1":
        n_frames, S = capi.prefilter_range_frames() + 1, 6
    tables, ladder, feats, ref, share = _case(M, D, n_frames, S)
    assert share >= 0.85
    _check(tables, ladder, feats, ref, D)
