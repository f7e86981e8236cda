"""check_masks (tests/prefilter_reference.py) has teeth: on the heterogeneous model -- four state slots per group with limits far
apart, every other state a ladder of copies from 1e-4 to 1e2 apart -- the masks of the fp16 emulation with the documented limit pass,
and a limit read from the neighbouring slot, 2.5 times too large or 2.5 times too small is caught.  And the reason the checker exists:
with the limit a quarter of what it should be, or read from the wrong slot, every exact arg-min is still in its mask on this model, so
a comparison of final scores with the oracle sees nothing."""
import numpy as np
import pytest

from tests import prefilter_reference as PR

M, T = 8, 400


@pytest.fixture(scope="module", params=[9, 39, 62])
def case(request):
    D = request.param
    rng = np.random.default_rng(1000 + D)
    tables, ladder = PR.heterogeneous_model(rng, M, D)
    feats = PR.reference_frames(rng, D, T, tables[1][0])
    ref = PR.reference_limits(*tables, feats)
    return D, ref, ladder


def swapped(L):
    """the limit of the neighbouring state slot of the group (si ^ 1)"""
    return L[:, np.arange(L.shape[1]) ^ 1]


def test_the_model_decides_most_ladder_entries_and_spreads_the_limits(case):
    D, ref, ladder = case
    share = PR.decided_share(ref, ladder)
    t = 300  # a plain frame
    print(f"D={D}: decided share of ladder entries {share:.3f}; limits of group 0's slots at frame {t}: {ref.L[t, :4]}")
    assert share >= 0.85
    assert np.all(ref.residual_form)
    assert ref.L[t, 0] > 50 * ref.L[t, 3]


def test_emulated_masks_pass(case):
    D, ref, ladder = case
    assert PR.check_masks(PR.emulated_masks(ref), ref, ladder) >= 0.85


@pytest.mark.parametrize("name, mutate", [("slots swapped", swapped), ("limit x 2.5", lambda L: L * 2.5), ("limit / 2.5", lambda L: L / 2.5)])
def test_a_wrong_limit_is_caught(case, name, mutate):
    D, ref, ladder = case
    with pytest.raises(AssertionError, match=r"rule \([cd]\)") as e:
        PR.check_masks(PR.emulated_masks(ref, mutate), ref, ladder)
    n = int(str(e.value).rsplit("(", 1)[1].split()[0])
    print(f"D={D}, {name}: {e.value}")
    assert n > 100, "each of these mutations moves hundreds of entries on this model"


@pytest.mark.parametrize("name, mutate", [("limit / 4", lambda L: L / 4), ("slots swapped", swapped)])
def test_score_parity_cannot_see_it(case, name, mutate):
    """every exact arg-min stays a candidate under the wrong limit: the final scores would equal the oracle's"""
    D, ref, ladder = case
    bits = PR.mask_bits(PR.emulated_masks(ref, mutate), ref)
    gap = PR._gaps(ref)
    frames = np.flatnonzero(ref.ok)
    assert np.all(bits[frames][gap[frames] == 0.0])


def test_poison_padding_and_out_of_range_frames_are_caught(case):
    D, ref, ladder = case
    good = PR.emulated_masks(ref)
    bad = good.copy(); bad[1, 7, 2] = PR.POISON
    with pytest.raises(AssertionError, match=r"rule \(a\)"):
        PR.check_masks(bad, ref, ladder)
    bad = good.copy(); bad[0, 300, 1] |= 1 << M  # a bit beyond the state's eight densities
    with pytest.raises(AssertionError, match=r"rule \(e\)"):
        PR.check_masks(bad, ref, ladder)
    bad = good.copy(); bad[ref.groups - 1, 300, 3] = 1  # 18 pseudo-states: slots 2 and 3 of the last group hold none
    with pytest.raises(AssertionError, match=r"rule \(e\)"):
        PR.check_masks(bad, ref, ladder)
    bad = good.copy(); bad[2, 0, 0] &= ~np.uint32(2)  # frame 0 holds a NaN
    with pytest.raises(AssertionError, match=r"rule \(f\)"):
        PR.check_masks(bad, ref, ladder)
    t = int(np.flatnonzero(ref.ok)[-1])
    best = int(np.argmin(ref.exact[t, :M]))
    bad = good.copy(); bad[0, t, 0] &= ~np.uint32(1 << best)
    with pytest.raises(AssertionError, match=r"rule \(b\)"):
        PR.check_masks(bad, ref, ladder)
