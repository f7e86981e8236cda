"""MAP adaptation on the device (sr_map_statistics_corpus, sr_map_statistics_bw_corpus, sr_model_map_adapt) against the numpy
restatement (tests/map_reference.py: the documented order of summation bit for bit, and sums in longdouble), against the EM statistics
the library already forms, and end to end.

The statistics bound, per entry and element, where the weights are soft: (n_pairs + C_TERM) 2^-52 sum |gamma x_i|.  This is
tests/test_gpu_mllr.py's count: 2 u per pair (a product and an addition), 8 u for the device's memberships (its exp within 2 ulp,
numpy's within 1, the normalising sum inherits those, a division, the product with the posterior), at most 3 u for the segments'
partials here.  C_TERM = 16 covers it and was fixed before the first run.  With max_approx every weight is 1 and the reference replays
the order of summation: bit for bit."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from speechrecognition_amd import capi, synth
from tests import fmllr_reference as F
from tests import map_reference as R
from tests.test_gpu_mllr import make_case, open_model, shifted_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
C_TERM = 16
TDP = (3.0, 0.0, 30.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def planted_states(auts, off):
    """make_case's own alignment, on the CPU: frame t of an utterance of T frames and N automaton states takes state t N // T"""
    out = []
    for u, a in enumerate(auts):
        T, N = int(off[u + 1] - off[u]), len(a)
        out.append(a[np.minimum(np.arange(T) * N // T, N - 1)])
    return np.concatenate(out).astype(np.uint16)


def check_exact(got, ref, label):
    ent_off, dens, occ, x = got
    assert np.array_equal(ent_off, ref["ent_off"]), label
    assert np.array_equal(dens, ref["dens"]), label
    assert np.array_equal(bits(occ), bits(ref["occ"])), label
    assert np.array_equal(bits(x), bits(ref["x"])), label


def check_bound(got, ref, label):
    ent_off, dens, occ, x = got
    assert np.array_equal(ent_off, ref["ent_off"]), label
    assert np.array_equal(dens, ref["dens"]), label
    f = ((ref["n_pairs"] + C_TERM) * EPS).astype(np.longdouble)
    err_o, lim_o = np.abs(occ - ref["occ_ld"]), f * ref["occ_ld"]
    err_x, lim_x = np.abs(x - ref["x_ld"]), f[:, None] * ref["x_abs"]
    worst = max(float((err_o / lim_o).max()), float((err_x / np.where(lim_x > 0, lim_x, 1)).max()))
    print(f"{label}: worst |gpu - ref| / bound = {worst:.3f}, {len(dens)} entries, up to {int(ref['n_pairs'].max())} pairs")
    assert (err_o <= lim_o).all() and (err_x <= lim_x).all(), (label, worst)


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", [(2, False), (13, True), (39, False), (70, False)])   # 70: more dimensions than a wave has lanes
def test_alignment_statistics_against_the_reference(D, tied, max_approx):
    model, feats, off, auts, spk, S, tied, _ = make_case(D, 500 + D, tied=tied)
    states = planted_states(auts, off)
    pairs = F.alignment_pairs(feats, model, states, max_approx)
    ref = R.entries(feats, pairs, off, spk, S)
    assert ref["ent_off"][2] == ref["ent_off"][3] and len(ref["dens"]) > 3   # speaker 2 has no utterance
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        got = corpus.map_statistics(states, spk, S, max_approx)
        again = corpus.map_statistics(states, spk, S, max_approx)
        corpus.close()
    if max_approx:
        check_exact(got, ref, f"align D={D}")
        frames = np.zeros(S)
        for u in range(len(spk)):
            frames[spk[u]] += int(off[u + 1] - off[u])
        o = got[0].astype(np.int64)
        assert [got[2][o[s]:o[s + 1]].sum() for s in range(S)] == frames.tolist()
    else:
        check_bound(got, ref, f"align soft D={D} tied={tied}")
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes(), "two identical calls differ"


@pytest.mark.parametrize("max_approx", [True, False])
@pytest.mark.parametrize("D,tied", [(13, True), (70, False)])
def test_posterior_statistics_against_the_reference(D, tied, max_approx):
    model, feats, off, auts, spk, S, tied, _ = make_case(D, 600 + D, n_utts=24, tied=tied, lens=(20, 50))
    with open_model(model, max_approx, tied) as m:
        corpus = m.upload(feats, off)
        cost, count, state, weight = corpus.state_posteriors(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, 64)
        bw_cost, got = corpus.map_statistics_bw(auts, TDP, 0, spk, S, capi.GMM_DEFAULT, 0.0, max_approx)
        bw_cost2, again = corpus.map_statistics_bw(auts, TDP, 0, spk, S, capi.GMM_DEFAULT, 0.0, max_approx)
        corpus.close()
    assert int(count.max()) < 64   # no item lost
    assert np.array_equal(bits(cost), bits(bw_cost)) and np.array_equal(bits(cost), bits(bw_cost2))
    pairs = F.posterior_pairs(feats, model, count, state, weight, max_approx)
    check_bound(got, R.entries(feats, pairs, off, spk, S), f"posterior D={D} tied={tied} max_approx={max_approx}")
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes(), "two identical calls differ"


@pytest.mark.parametrize("max_approx", [True, False])
def test_one_speaker_equals_the_em_statistics(max_approx):
    """one speaker, an untied model, no entry beyond one segment: x and occ are sr_accumulate_corpus' / sr_baum_welch_corpus' mean_acc
    and mean_w rows bit for bit -- the same pairs in the same order; the soft weights make that sensitive to the order"""
    D = 13
    model, feats, off, auts, _, _, _, _ = make_case(D, 77, n_utts=5)
    assert len(feats) <= R.SEG   # so every entry holds at most one segment (a density takes at most one pair per frame)
    spk = np.zeros(len(auts), np.uint32)
    states = planted_states(auts, off)
    reached = {d for _, d, _ in F.alignment_pairs(feats, model, states, max_approx)}
    assert 10 < len(reached) < int(model[0][-1])   # some density has no entry
    with open_model(model, max_approx, False) as m:
        corpus = m.upload(feats, off)
        ma, mw, _, _ = corpus.accumulate(states, first_pass=False, max_approx=max_approx)
        ent_off, dens, occ, x = corpus.map_statistics(states, spk, 1, max_approx)
        cost, (bma, bmw, _, _) = corpus.baum_welch(auts, TDP, 0, capi.GMM_DEFAULT, 0.0, False, max_approx)
        cost2, (boff, bdens, bocc, bx) = corpus.map_statistics_bw(auts, TDP, 0, spk, 1, capi.GMM_DEFAULT, 0.0, max_approx)
        corpus.close()
    for label, (a, w), (d, o, xx) in (("alignment", (ma, mw), (dens, occ, x)), ("posteriors", (bma, bmw), (bdens, bocc, bx))):
        assert len(d) > 10 and (np.diff(d.astype(np.int64)) > 0).all(), label
        assert np.array_equal(bits(xx), bits(a[d])), label
        assert np.array_equal(bits(o), bits(w[d])), label
        rest = np.setdiff1d(np.arange(len(w)), d)
        assert not w[rest].any(), label
    assert ent_off.tolist() == [0, len(dens)] and boff.tolist() == [0, len(bdens)] and set(dens.tolist()) == reached
    assert np.array_equal(bits(cost), bits(cost2))
    if not max_approx:
        assert (occ != np.round(occ)).any()   # soft weights


def long_case():
    """2 mixtures x 1 density, D = 3; speakers 0, 1, 2 hold 2500, 1024 and 1025 frames of mixture 0 -- three segments, exactly one, and a
    second segment of one pair -- and a few frames of mixture 1; their utterances interleaved"""
    D = 3
    rng = np.random.default_rng(12)
    model = F.random_model(rng, 2, 1, D, ragged=False)
    lens = {0: [900, 800, 805], 1: [500, 529], 2: [1025, 4]}      # per speaker; the frames of mixture 1 end its last utterance
    tail = {0: 5, 1: 5, 2: 4}
    order = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (0, 2)]
    T, spk, states = [], [], []
    for s, i in order:
        n = lens[s][i]
        st = np.zeros(n, np.uint16)
        if i == len(lens[s]) - 1:
            st[n - tail[s]:] = 1
        T.append(n); spk.append(s); states.append(st)
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.uint64)
    states = np.concatenate(states)
    feats = (rng.normal(size=(int(off[-1]), D)) * 2.0 ** rng.integers(-20, 21, size=(int(off[-1]), D))).astype(np.float32)
    return model, feats, off, np.array(spk, np.uint32), states


def test_long_entries_follow_the_segmented_order():
    model, feats, off, spk, states = long_case()
    pairs = [(t, int(s), 1.0) for t, s in enumerate(states)]
    ref = R.entries(feats, pairs, off, spk, 3)
    assert ref["dens"].tolist() == [0, 1, 0, 1, 0, 1] and ref["n_pairs"].tolist() == [2500, 5, 1024, 5, 1025, 4]
    single = R.entries(feats, pairs, off, spk, 3, seg=None)
    assert (bits(ref["x"][0]) != bits(single["x"][0])).any()   # the order shows in speaker 0's sums: checked before any device run
    assert np.array_equal(bits(ref["x"][2]), bits(single["x"][2]))
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        got = corpus.map_statistics(states, spk, 3, True)
        again = corpus.map_statistics(states, spk, 3, True)
        corpus.close()
    check_exact(got, ref, "long entries")
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def small_case(D=5, seed=9):
    model, feats, off, auts, spk, S, _, _ = make_case(D, seed, n_utts=6, lens=(10, 20))
    return model, feats, off, auts, spk, S, planted_states(auts, off)


def test_the_sizing_protocol():
    model, feats, off, auts, spk, S, states = small_case()
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    D = 5
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        call = lambda cap, o, d, oc, x: L.sr_map_statistics_corpus(m.h, corpus.h, P(states), P(spk), S, 1, cap, P(o), d, oc, x)  # noqa: E731
        sized = np.full(S + 1, 99, np.uint64)
        assert call(0, sized, None, None, None) == 0
        n = int(sized[-1])
        assert sized[0] == 0 and n > 2 and (np.diff(sized.astype(np.int64)) >= 0).all()
        # one too small: SR_EINVAL, the arrays untouched, the offsets still there
        dens, occ, x = np.full(n, 7, np.uint32), np.full(n, -3.0), np.full((n, D), -3.0)
        o2 = np.full(S + 1, 99, np.uint64)
        assert call(n - 1, o2, P(dens), P(occ), P(x)) == -1
        assert b"capacity" in L.sr_last_error()
        assert np.array_equal(o2, sized) and (dens == 7).all() and (occ == -3.0).all() and (x == -3.0).all()
        o3 = np.full(S + 1, 99, np.uint64)
        assert call(n, o3, P(dens), P(occ), P(x)) == 0
        assert np.array_equal(o3, sized) and (occ > 0).all() and (dens < m.n_densities).all()
        want = corpus.map_statistics(states, spk, S, True)
        assert np.array_equal(dens, want[1]) and np.array_equal(bits(occ), bits(want[2])) and np.array_equal(bits(x), bits(want[3]))
        assert n <= len(feats)   # with max_approx and an alignment, total_frames always suffices
        corpus.close()


def test_statistics_errors_are_refused_before_any_launch():
    model, feats, off, auts, spk, S, states = small_case()
    L = capi.lib()
    P = lambda a: a.ctypes.data  # noqa: E731
    D = 5
    with capi.Model.from_tables(*model, max_approx=True) as m, capi.Model.from_tables(*model, max_approx=True) as other:
        corpus = m.upload(feats, off)
        n = len(feats)
        eo, dens, occ, x = np.zeros(S + 1, np.uint64), np.zeros(n, np.uint32), np.zeros(n), np.zeros((n, D))
        call = lambda mh, ch, sp, ns, o, d, oc, xx, st=states: L.sr_map_statistics_corpus(mh, ch, P(st), P(sp), ns, 1, n, o, d, oc, xx)  # noqa: E731
        assert call(m.h, corpus.h, spk, S, P(eo), P(dens), P(occ), P(x)) == 0
        dens[:] = 0; occ[:] = 0; x[:] = 0
        bad_spk = spk.copy()
        bad_spk[2] = S
        assert call(None, corpus.h, spk, S, P(eo), P(dens), P(occ), P(x)) == -1
        assert call(m.h, None, spk, S, P(eo), P(dens), P(occ), P(x)) == -1
        assert call(other.h, corpus.h, spk, S, P(eo), P(dens), P(occ), P(x)) == -1      # a corpus of another model
        assert call(m.h, corpus.h, spk, S, None, P(dens), P(occ), P(x)) == -1
        assert call(m.h, corpus.h, spk, S, P(eo), None, P(occ), P(x)) == -1               # a partial set of arrays
        assert call(m.h, corpus.h, spk, S, P(eo), P(dens), None, P(x)) == -1
        assert call(m.h, corpus.h, spk, S, P(eo), P(dens), P(occ), None) == -1
        assert call(m.h, corpus.h, spk, S, P(eo), None, None, P(x)) == -1
        assert call(m.h, corpus.h, spk, 0, P(eo), P(dens), P(occ), P(x)) == -1
        assert call(m.h, corpus.h, bad_spk, S, P(eo), P(dens), P(occ), P(x)) == -1
        assert call(m.h, corpus.h, spk, 2 ** 32 // m.n_densities + 1, P(eo), P(dens), P(occ), P(x)) == -4
        assert b"keys" in L.sr_last_error()
        bad_states = states.copy()
        bad_states[0] = 60000
        assert call(m.h, corpus.h, spk, S, P(eo), P(dens), P(occ), P(x), bad_states) == -1   # sr_accumulate_corpus' errors
        t3 = (C.c_double * 3)(*TDP)
        flat, aoff = corpus._aut(auts)
        cost = np.zeros(len(auts))
        bw = lambda sp, ns, o, d, floor=0.0, c=cost: L.sr_map_statistics_bw_corpus(  # noqa: E731
            m.h, corpus.h, P(flat), P(aoff), C.byref(t3), 0, capi.GMM_DEFAULT, floor, P(sp), ns, 1, None if c is None else P(c), n, o, d,
            P(occ), P(x))
        assert bw(bad_spk, S, P(eo), P(dens)) == -1 and bw(spk, 0, P(eo), P(dens)) == -1
        assert bw(spk, S, None, P(dens)) == -1 and bw(spk, S, P(eo), None) == -1
        assert bw(spk, 2 ** 32 // m.n_densities + 1, P(eo), P(dens)) == -4
        assert bw(spk, S, P(eo), P(dens), -1.0) == -1 and bw(spk, S, P(eo), P(dens), 0.0, None) == -1   # sr_baum_welch_corpus' errors
        assert not dens.any() and not occ.any() and not x.any()
        corpus.close()


def random_entries(rng, n_dens, D, keep=0.6):
    sel = rng.uniform(size=n_dens) < keep
    sel[0] = True
    dens = np.flatnonzero(sel).astype(np.uint32)
    occ = rng.uniform(0.2, 40.0, size=len(dens))
    x = (rng.normal(0.0, 2.0, size=(len(dens), D)) + rng.normal(size=(len(dens), 1))) * occ[:, None]
    return dens, occ, x


@pytest.mark.parametrize("D,shared", [(2, False), (39, False), (70, False), (13, True)])
def test_map_adapt_is_the_documented_loop(D, shared):
    model, feats, off, auts, spk, S, _, _ = make_case(D, 700 + D, n_utts=4)
    dens_off, means, inv_vars, norm, logw = model
    n = int(dens_off[-1])
    dens_mean = np.arange(n, dtype=np.uint32)
    if shared:   # densities 2k and 2k + 1 share a mean row (and hold one mean), across mixtures too
        dens_mean = (dens_mean // 2).astype(np.uint32)
        means = means[dens_mean * 2].copy()
        model = (dens_off, means, inv_vars, norm, logw)
    rng = np.random.default_rng(D)
    dens, occ, x = random_entries(rng, n, D)
    if shared:
        assert (np.bincount(dens_mean[dens]) > 1).any()   # a row with two entries
    tau, tau_w = 12.5, 7.0
    want_means = R.map_means(means, dens_mean, dens, occ, x, tau)
    want_logw = R.map_weights(dens_off, logw, dens, occ, tau_w)
    free = ~np.isin(dens_mean, dens_mean[dens])
    assert free.any() and np.array_equal(bits(want_means[free]), bits(means[free]))
    with capi.Model.from_tables(*model, max_approx=True) as m:
        if shared:
            dv = np.arange(n, dtype=np.uint32)
            capi._check(capi.lib().sr_model_set_tying(m.h, int(dens_mean.max()) + 1, n, dens_mean.ctypes.data, dv.ctypes.data))
        t0 = m.tables()
        with m.map_adapt(dens, occ, x, tau) as a, m.map_adapt(dens, occ, x, tau, tau_w) as aw, m.map_adapt(dens[:0], occ[:0], x[:0], tau, tau_w) as e:
            ta, tw, te = a.tables(), aw.tables(), e.tables()
            assert np.array_equal(bits(ta[0]), bits(want_means)) and np.array_equal(bits(tw[0]), bits(want_means))
            assert not np.array_equal(ta[0], t0[0])
            for k in (1, 2):
                assert np.array_equal(bits(ta[k]), bits(t0[k])) and np.array_equal(bits(tw[k]), bits(t0[k]))
            assert np.array_equal(bits(ta[3]), bits(t0[3]))
            assert np.array_equal(bits(tw[3]), bits(want_logw)) and not np.array_equal(tw[3], t0[3])
            for x0, x1 in zip(t0, te):   # no entry: every table is the prior's
                assert np.array_equal(bits(x0), bits(x1))
            for mm in (a, aw, e):
                for p, q in zip(m.topology(), mm.topology()):
                    assert np.array_equal(p, q)
                assert m.tying_info() == mm.tying_info()
            # the adapted model scores like a model created from the reference's tables: its packed tables were built
            kernels = (capi.GMM_EXACT, capi.GMM_PREFILTER, capi.GMM_MFMA) if D == 39 else (capi.GMM_EXACT,)
            with capi.Model.from_tables(dens_off, want_means, inv_vars, norm, want_logw, max_approx=True) as b:
                ca, cb, c0, ce = aw.upload(feats, off), b.upload(feats, off), m.upload(feats, off), e.upload(feats, off)
                for kernel in kernels:
                    sa, sb = ca.score(kernel), cb.score(kernel)
                    assert np.array_equal(bits(sa), bits(sb)), kernel
                    s0 = c0.score(kernel)
                    assert np.array_equal(bits(s0), bits(ce.score(kernel))), kernel
                    assert not np.array_equal(sa, s0)
                for c in (ca, cb, c0, ce):
                    c.close()


def test_tau_zero_is_the_ml_mean():
    """tau = 0, one speaker, an untied model: on the occupied rows the means are sr_model_create_from_accumulated's (POOL_NONE): both are
    mean_acc / mean_w"""
    D = 13
    model, feats, off, auts, _, _, _, _ = make_case(D, 78, n_utts=5)
    assert len(feats) <= R.SEG
    spk = np.zeros(len(auts), np.uint32)
    states = planted_states(auts, off)
    reached = sorted({d for _, d, _ in F.alignment_pairs(feats, model, states, True)})
    assert 10 < len(reached) < int(model[0][-1])   # some density has no entry
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        ent_off, dens, occ, x = corpus.map_statistics(states, spk, 1, True)
        corpus.accumulate_on_device(states, first_pass=False, max_approx=True)
        with corpus.next_model(capi.POOL_NONE, True) as ml, m.map_adapt(dens, occ, x, 0.0) as a:
            got, want, prior = a.tables()[0], ml.tables()[0], m.tables()[0]
        corpus.close()
    assert dens.tolist() == reached
    assert np.array_equal(bits(got[dens]), bits(want[dens]))
    rest = np.setdiff1d(np.arange(len(prior)), dens)
    assert np.array_equal(bits(got[rest]), bits(prior[rest]))


@pytest.mark.parametrize("tau", [0.0, 10.0])
def test_adapted_models_lower_the_cost_of_the_alignment(tau):
    """Under a fixed alignment and the arg-min statistics, a speaker's cost under its own adapted model falls strictly: with the arg-min
    densities held, the cost is convex in every mean with its minimum at the ML mean, and the MAP mean lies between the prior and the
    ML mean (tau = 0: at it); re-picking the arg-min under the adapted model can only lower the cost further."""
    model, feats, off, auts, spk, S, _, planted = shifted_case()
    states = planted.astype(np.uint16)
    o = off.astype(np.int64)
    with capi.Model.from_tables(*model, max_approx=True) as m:
        corpus = m.upload(feats, off)
        ent_off, dens, occ, x = corpus.map_statistics(states, spk, S + 1, True)   # speaker S has no data
        corpus.close()
        e = ent_off.astype(np.int64)
        assert e[S] == e[S + 1] and (np.diff(e[: S + 1]) > 0).all()

        def own(s):
            us = np.flatnonzero(spk == s)
            f = np.concatenate([feats[o[u]:o[u + 1]] for u in us])
            st = np.concatenate([states[o[u]:o[u + 1]] for u in us])
            po = np.concatenate([[0], np.cumsum([o[u + 1] - o[u] for u in us])]).astype(np.uint64)
            return f, st, po

        for s in range(S + 1):
            f, st, po = own(min(s, S - 1))
            sl = slice(e[s], e[s + 1])
            with m.map_adapt(dens[sl], occ[sl], x[sl], tau) as adapted:
                c0, c1 = m.upload(f, po), adapted.upload(f, po)
                before, after = c0.path_scores(st), c1.path_scores(st)
                c0.close()
                c1.close()
            if s < S:
                print(f"tau {tau} speaker {s}: cost {before.sum():.3f} -> {after.sum():.3f}")
                assert after.sum() < before.sum()
            else:
                assert np.array_equal(bits(before), bits(after))


def test_cpp_helper_adapts_a_corpus(tmp_path):
    """sr::MapAdaptation through tests/cpp/map_mirror_driver: the same statistics and adapted tables, bit for bit, as the calls made here"""
    D = 13
    lex = synth.make_lexicon(6, 3, 1)
    spec = synth.make_mixset(lex.n_states, 3, D, seed=41)
    mp = os.path.join(str(tmp_path), "a.mix")
    synth.write_mixset(mp, spec)
    feats, off = synth.make_batch(6, 60, 90, D, seed=42)
    spk = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint32)
    word_off, automaton, sil = lex.flatten()
    rng = np.random.default_rng(5)
    orths = [rng.integers(1, 6, size=3).astype(np.uint32) for _ in range(6)]
    orths = [np.where(o == lex.silence_idx, (lex.silence_idx + 1) % 6, o).astype(np.uint32) for o in orths]
    tau, tau_w = 8.0, 3.0
    blob = struct.pack("<I", len(lex.word_states))
    for n, r in zip(lex.word_states, lex.word_reps):
        blob += struct.pack("<HH", int(n), int(r))
    blob += struct.pack("<Iddddd", lex.silence_idx, *TDP, tau, tau_w) + struct.pack("<I", 6)
    o = off.astype(np.int64)
    for u in range(6):
        blob += struct.pack("<II", int(spk[u]), len(orths[u])) + orths[u].tobytes()
        blob += struct.pack("<I", int(o[u + 1] - o[u])) + feats[o[u]:o[u + 1]].tobytes()
    case = tmp_path / "case.bin"
    case.write_bytes(blob)
    drv = str(tmp_path / "map_mirror_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_mirror_driver.cpp"), "-o", drv,
                           "-L" + os.path.join(ROOT, "speechrecognition_amd"), "-lsrgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "speechrecognition_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([drv, mp, str(D), str(case)], text=True).splitlines()
    assert not out[0].startswith("error"), out[0]
    lines = {}
    for ln in out:
        w = ln.split()
        key = w[0] if w[0] in ("off", "dens", "occ", "x") else w[0] + w[1]
        lines[key] = w[1:] if w[0] in ("off", "dens", "occ", "x") else w[2:]
    hexes = lambda v: np.array([int(t, 16) for t in v], dtype=np.uint64)  # noqa: E731
    auts = []
    for u in range(6):
        a = [sil]
        for w in orths[u]:
            a += list(automaton[word_off[w]:word_off[w + 1]]) + [sil]
        auts.append(np.asarray(a, dtype=np.uint16))
    with capi.Model.from_mixset(mp, D) as m:
        corpus = m.upload(feats, off)
        states, _ = corpus.align(auts, TDP, sil, capi.GMM_DEFAULT)
        ent_off, dens, occ, x = corpus.map_statistics(states, spk, 2, True)
        corpus.close()
        assert [int(v) for v in lines["off"]] == ent_off.tolist() and [int(v) for v in lines["dens"]] == dens.tolist()
        assert np.array_equal(hexes(lines["occ"]), bits(occ)) and np.array_equal(hexes(lines["x"]), bits(x).reshape(-1))
        e = ent_off.astype(np.int64)
        for s in range(2):
            sl = slice(e[s], e[s + 1])
            with m.map_adapt(dens[sl], occ[sl], x[sl], tau, tau_w) as a:
                t = a.tables()
            assert np.array_equal(hexes(lines[f"means{s}"]), bits(t[0]).reshape(-1))
            assert np.array_equal(hexes(lines[f"logw{s}"]), bits(t[3]))
